"""Regridding on the GPU (cra5_regrid_f32 / ops.regrid, VAEformer regrid=, cra5_api regrid=): every value against the
sequential float64 numpy loop of tests/regrid_helpers.py, bit for bit."""
import numpy as np
import pytest
import torch

import regrid_helpers as rh
from regrid_helpers import ref_regrid, same_bits
from time_stats_helpers import ref_time_stats
from cra5_amd import metrics, ops, subset, synth
from cra5_amd._lib import Cra5Error
from cra5_amd.api import cra5_api
from cra5_amd.regrid import Grid, tile_table
from cra5_amd.vaeformer import VAEformer

pytestmark = pytest.mark.gpu

H, W = 721, 1440
GRIDS = [(13, 24), (25, 40), (7, 1440)]
METHODS = ("bilinear", "conservative")


def _source(full, plan):
    """The plan's source box cut out of the global field (columns wrap)."""
    sr0, sr1, sc0, snc = plan["src_box"]
    return np.ascontiguousarray(full[:, sr0:sr1][:, :, (sc0 + np.arange(snc)) % full.shape[2]])


def _targets(Hg, Wg):
    """Coarser, equal-size offset and finer than the source; both row orders; across 0 deg; regional; one point;
    irregular latitudes; on (7, 1440) a 24-tap column window and more columns than one tile holds."""
    dlat, dlon = 180.0 / (Hg - 1), 360.0 / Wg
    slat, slon = rh.source_lat(Hg), rh.source_lon(Wg)
    out = []
    for m in METHODS:
        out += [("coarse south-to-north", Grid.equiangular(4, max(6, Wg // 20), method=m)),
                ("offset", Grid(slat[:-1] - 0.3 * dlat, slon + 0.4 * dlon, m)),
                ("offset south-to-north", Grid((slat[:-1] - 0.3 * dlat)[::-1].copy(), slon[:min(Wg, 300)] + 0.4 * dlon, m)),
                ("fine across 0", Grid(40.0 - np.arange(11) * (dlat / 2.5), -2.2 * dlon + np.arange(13) * (dlon / 2.5), m)),
                ("regional across 0", Grid([50.0, 20.0, -10.0], (-7.48 + 4.4 * np.arange(4)) * dlon, m)),
                ("gaussian", Grid.gaussian(6, max(10, Wg // 18), method=m))]
    out += [("one point", Grid([12.3], [45.6])),
            ("one cell", Grid([12.3], [45.6], "conservative", lat_bnds=[[20.0, 5.0]], lon_bnds=[[40.0, 50.0]])),
            ("poles on the lattice", Grid.equiangular(Hg, Wg // 2, poles=True))]
    if (Hg, Wg) == (7, 1440):
        lon = 3.125 + 6.0 * np.arange(60)                 # cells of 24 source columns, edge on edge
        out.append(("24 taps", Grid([60.0, 0.0, -60.0], lon, "conservative", lon_bnds=np.stack([lon - 3.0, lon + 3.0], axis=1))))
    return out


def _run(full, plan, dev, chan_map=None, off_src=0, off_dst=0):
    C = full.shape[0]
    t = ops.regrid_tables(plan, dev)
    src = _source(full, plan)
    sbuf = torch.full((src.size + 4,), -3.0, device=dev)
    sbuf[off_src:off_src + src.size].copy_(torch.from_numpy(src).reshape(-1))
    xs = sbuf[off_src:off_src + src.size].view(src.shape)
    Co = C if chan_map is None else len(chan_map)
    n = Co * plan["Ho"] * plan["Wo"]
    dbuf = torch.full((n + 12,), -7.0, device=dev)
    lo = 4 + off_dst                       # guard words in front; `out` starts 4 * off_dst bytes past a 16-byte boundary
    out = dbuf[lo:lo + n].view(Co, plan["Ho"], plan["Wo"])
    assert sbuf.data_ptr() % 16 == 0 and dbuf.data_ptr() % 16 == 0
    assert xs.data_ptr() % 16 == 4 * off_src and out.data_ptr() % 16 == 4 * off_dst
    cm = None if chan_map is None else torch.tensor(chan_map, device=dev, dtype=torch.int32)
    got = ops.regrid(xs, t, out=out, chan_map=cm)
    assert got is out
    assert (dbuf[:lo] == -7.0).all() and (dbuf[lo + n:] == -7.0).all()      # nothing written around the result
    return out.cpu().numpy()


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("C", [1, 3])
def test_kernel_equals_the_sequential_float64_loop(dev, grid, C):
    Hg, Wg = grid
    n_cases = single = taps24 = tiles = 0
    for physical in (True, False):                      # zero-mean data: cancellation shows a wrong summation order
        full = rh.field(C, Hg, Wg, seed=Hg + C, physical=physical)
        for name, g in _targets(Hg, Wg):
            plan = g.plan(Hg, Wg)
            ref, _ = ref_regrid(full, plan)
            got = _run(full, plan, dev)
            assert np.array_equal(got, ref, equal_nan=True) and same_bits(got, ref), (grid, C, physical, name, g.method)
            assert same_bits(_run(full, plan, dev), got), name                          # two runs: identical bits
            n_cases += 1
            single += ref.shape[1:] == (1, 1)
            taps24 += int(plan["ctap"].max()) == 24
            tiles += len(tile_table(plan)[0]) > 1
    assert n_cases >= 20 and single >= 2
    if grid == (7, 1440):
        assert taps24 >= 2 and tiles >= 2


def test_kernel_chan_map_alignment_nonfinite_and_sub_block(dev):
    Hg, Wg = 25, 40
    dlat, dlon = 180.0 / (Hg - 1), 360.0 / Wg
    full = rh.field(5, Hg, Wg, seed=9)
    cons = Grid.equiangular(8, 12, method="conservative").plan(Hg, Wg)
    # chan_map: a reordered variable subset of the full source, no gather
    assert same_bits(_run(full, cons, dev, chan_map=[4, 0, 2]), ref_regrid(full, cons, chans=[4, 0, 2])[0])
    # source and destination 4 and 12 bytes off a 16-byte boundary, on a regional source box
    reg = Grid(40.0 - np.arange(11) * 3.1, -20.0 + np.arange(13) * 3.7, "conservative").plan(Hg, Wg)
    assert reg["src_box"][3] < Wg
    for plan in (reg, cons):
        ref = ref_regrid(full, plan)[0]
        for off_src, off_dst in ((1, 3), (3, 1), (1, 1), (3, 3)):
            assert same_bits(_run(full, plan, dev, off_src=off_src, off_dst=off_dst), ref), (off_src, off_dst)
    # NaN / +inf / -inf appear in exactly the windows that hold them: bilinear 0.3 rows south, 0.4 columns east of the
    # lattice - output (i, j) reads rows i, i + 1 and columns j, j + 1
    off = Grid(rh.source_lat(Hg)[:-1] - 0.3 * dlat, rh.source_lon(Wg) + 0.4 * dlon).plan(Hg, Wg)
    bad = full.copy()
    bad[1, 10, 6] = np.nan
    bad[3, 14, 0] = np.inf                              # column 0: read by outputs 39 (across the east edge) and 0
    bad[0, 0, 2] = -np.inf
    for plan in (off, cons):
        ref = ref_regrid(bad, plan)[0]
        got = _run(bad, plan, dev)
        assert np.array_equal(got, ref, equal_nan=True)
        assert np.isfinite(got[2]).all() and np.isfinite(got[4]).all()
    got = _run(bad, off, dev)
    assert np.isnan(got[1]).sum() == 4 and np.isnan(got[1, 9:11, 5:7]).all()
    assert np.isposinf(got[3]).sum() == 4 and np.isposinf(got[3, 13:15][:, [39, 0]]).all()
    assert np.isneginf(got[0]).sum() == 2 and np.isneginf(got[0, 0, 1:3]).all()
    # a sub-grid's result is the sub-block of the whole target grid's, as bit patterns
    for m in METHODS:
        whole = Grid(80.0 - np.arange(30) * 5.3, -100.0 + np.arange(50) * 6.1, m)
        glob = _run(full, whole.plan(Hg, Wg), dev)
        for (a, b, c, d) in [(0, 30, 10, 50), (3, 17, 0, 20), (29, 30, 49, 50), (5, 6, 7, 40)]:
            sub = Grid(whole.lat[a:b], whole.lon[c:d], m, lat_bnds=whole.lat_bnds[a:b], lon_bnds=whole.lon_bnds[c:d])
            got = _run(full, sub.plan(Hg, Wg), dev)
            assert np.array_equal(got.view(np.int32), glob[:, a:b, c:d].view(np.int32)), (m, a, b, c, d)


def _launch_rows(C_out, n_tiles, Ho):
    """(rows_per_block, n_chunks) of a launch: the launcher's rule - at least 4096 blocks, at most one chunk per row."""
    chunks = max(1, min(Ho, -(-4096 // (C_out * n_tiles))))
    rpb = -(-Ho // chunks)
    return rpb, -(-Ho // rpb)


WALK_LAT, WALK_LON = 88.0 - 8.0 * np.arange(22), 2.0 + 12.0 * np.arange(30)
# (target grid, C_out, Ho, rows per block, chunks)
WALKS = {"bilinear": (Grid(WALK_LAT, WALK_LON, "bilinear"), 1024, 22, 6, 4),
         "bilinear south-to-north": (Grid(WALK_LAT[::-1].copy(), WALK_LON, "bilinear"), 1024, 22, 6, 4),     # through `order`
         "conservative south-to-north": (Grid(WALK_LAT[::-1].copy(), WALK_LON, "conservative"), 1024, 22, 6, 4),   # 3 x 3 taps
         "5 x 5 taps": (Grid.equiangular(6, 12, method="conservative"), 2048, 6, 3, 2)}       # windows sharing edge rows


def test_kernel_walks_runs_of_rows_per_block(dev):
    """A long chan_map over a 3-channel source: C_out * tiles is large enough that one block walks several target rows -
    the two kept inner, the look-ahead load, `order`, the chunk boundary where a shared row is staged again."""
    Hg, Wg = 25, 40
    full = rh.field(3, Hg, Wg, seed=21)
    got = {}
    for name, (g, C_out, Ho, rpb, chunks) in WALKS.items():
        plan = g.plan(Hg, Wg)
        cmap = ((np.arange(C_out) * 7 + 1) % 3).tolist()
        assert plan["Ho"] == Ho and len(tile_table(plan)[0]) == 1
        assert _launch_rows(C_out, 1, Ho) == (rpb, chunks) and rpb > 1 and _launch_rows(3, 1, Ho) == (1, Ho)
        got[name] = _run(full, plan, dev, chan_map=cmap)
        assert same_bits(got[name], ref_regrid(full, plan)[0][cmap]), name
        # the plain 3-channel source walks one row per block: the multi-row walk against the single-row walk
        assert same_bits(got[name], _run(full, plan, dev)[cmap]), name
    assert int(WALKS["conservative south-to-north"][0].plan(Hg, Wg)["ntap"].max()) == 3
    assert int(WALKS["5 x 5 taps"][0].plan(Hg, Wg)["ntap"].max()) == 5
    assert same_bits(got["bilinear south-to-north"], got["bilinear"][:, ::-1])


def test_ops_argument_checks(dev):
    Hg, Wg = 13, 24
    full = rh.field(2, Hg, Wg, seed=1)
    plan = Grid([50.0, 20.0], [100.0, 130.0, 170.0], "conservative").plan(Hg, Wg)
    t = ops.regrid_tables(plan, dev)
    x = torch.from_numpy(_source(full, plan)).to(dev)
    assert same_bits(ops.regrid(x, t).cpu().numpy(), ref_regrid(full, plan)[0])
    with pytest.raises(ValueError, match="source box"):
        ops.regrid(x[:, :, :-1].contiguous(), t)
    with pytest.raises(TypeError):
        ops.regrid(x.double(), t)
    with pytest.raises(ValueError, match="source box"):
        ops.regrid(x.transpose(1, 2), t)
    with pytest.raises(ValueError, match="out must be"):
        ops.regrid(x, t, out=torch.empty((2, 3, 3), device=dev))
    with pytest.raises(ValueError, match="chan_map"):
        ops.regrid(x, t, chan_map=torch.tensor([0], device=dev))                    # int64
    with pytest.raises(ValueError, match="regrid_tables"):
        ops.regrid(x, plan)                                                         # host tables
    with pytest.raises(ValueError, match="do not belong"):
        ops.regrid(x, dict(t, Ho=3))
    with pytest.raises(RuntimeError):
        ops.regrid(x.cpu(), t)
    # the launcher's own checks (CRA5_ERR_ARG = -7), before any launch
    sr0, sr1, sc0, snc = plan["src_box"]
    for key, val in (("tile_cols", 257), ("tile_cols", 0), ("max_span", 7937), ("max_span", 2 * Wg + 1), ("grid", (sr1 - 1, Wg)),
                     ("grid", (Hg, snc)), ("src_box", (sr0, sr1, Wg, snc)), ("src_box", (-1, sr1 - sr0 - 1, sc0, snc))):
        with pytest.raises(Cra5Error) as e:
            ops.regrid(x, dict(t, **{key: val}))
        assert e.value.status == -7, (key, val)
    # a mapped channel outside the source gives NaN, nothing is read
    got = ops.regrid(x, t, chan_map=torch.tensor([1, 2], device=dev, dtype=torch.int32))
    assert torch.isnan(got[1]).all() and same_bits(got[0].cpu().numpy(), ref_regrid(full, plan)[0][1])


def test_a_tap_outside_the_source_gives_nan_and_is_not_read(dev):
    """The source is a view inside a larger allocation filled with a finite sentinel: a kernel that followed a bad table
    entry would read the sentinel - inside allocated memory - and return a finite value."""
    Hg, Wg = 25, 40
    full = rh.field(2, Hg, Wg, seed=6)
    plan = Grid(40.0 - np.arange(6) * 4.0, 30.0 + np.arange(7) * 5.0, "conservative").plan(Hg, Wg)
    sr0, sr1, sc0, snc = plan["src_box"]
    assert sr0 > 1 and sr1 < Hg - 1 and snc < Wg
    src = _source(full, plan)
    pad = 4 * src[0].size
    buf = torch.full((src.size + 2 * pad,), 12345.0, device=dev)
    x = buf[pad:pad + src.size].view(src.shape)
    x.copy_(torch.from_numpy(src))
    ref = ref_regrid(full, plan)[0]
    t = ops.regrid_tables(plan, dev)
    assert same_bits(ops.regrid(x, t).cpu().numpy(), ref)

    def run(key, edit, **other):
        a = np.array(plan[key] if key in plan else t[key].cpu().numpy())
        edit(a)
        out = torch.full(ref.shape, -5.0, device=dev)
        return ops.regrid(x, dict(t, **{key: torch.from_numpy(a).to(dev)}, **other), out=out).cpu().numpy()

    def only(got, rows=None, cols=None):
        bad = np.zeros(ref.shape, dtype=bool)
        if rows is not None:
            bad[:, rows] = True
        if cols is not None:
            bad[:, :, cols] = True
        assert np.isnan(got[bad]).all() and np.array_equal(got[~bad].view(np.int32), ref[~bad].view(np.int32))

    first, last = int(np.argmin(plan["row0"])), int(np.argmax(plan["row0"] + plan["ntap"]))
    only(run("row0", lambda a: a.__setitem__(first, sr0 - 1)), rows=[first])            # a window that starts above the box
    only(run("row0", lambda a: a.__setitem__(last, a[last] + 1)), rows=[last])          # ... that ends below it
    only(run("row0", lambda a: a.__setitem__(2, Hg + 5)), rows=[2])                     # ... outside the grid
    only(run("ntap", lambda a: a.__setitem__(1, 0)), rows=[1])                          # an empty window
    only(run("col0", lambda a: a.__setitem__(0, (sc0 - 1) % Wg)), cols=[0])             # west of the tile's span
    only(run("col0", lambda a: a.__setitem__(6, a[6] + 1)), cols=[6])                   # east of it
    only(run("ctap", lambda a: a.__setitem__(3, 65)), cols=[3])
    got = run("order", lambda a: a.__setitem__(4, -1))                                  # an entry that names no row: skipped
    assert (got[:, 4] == -5.0).all() and np.array_equal(np.delete(got, 4, axis=1).view(np.int32), np.delete(ref, 4, axis=1).view(np.int32))
    assert len(t["tiles"]) == 1
    # a span that leaves the source (the launch's own budget allows it), and one beyond the budget
    assert np.isnan(run("tiles", lambda a: a.__setitem__((0, 3), snc + 1), max_span=snc + 1)).all()
    assert np.isnan(run("tiles", lambda a: a.__setitem__((0, 3), snc + 1))).all()
    assert (run("tiles", lambda a: a.__setitem__((0, 1), 8)) == -5.0).all()            # more columns than the target has
    assert (buf[:pad] == 12345.0).all() and (buf[pad + src.size:] == 12345.0).all()


# ---- the model ---------------------------------------------------------------------------------------------------------


def _yhat(latent, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.round(2.0 * torch.randn(1, latent, 72, 144, generator=g)) + torch.randn(1, latent, 72, 144, generator=g)


def _thin(dev, mod=None):
    net = VAEformer(0, **synth.thin_model_kwargs())
    synth.load_synthetic(net, seed=7)
    if mod is not None:
        with torch.no_grad():
            mod(net)
    return net.to(dev)


@pytest.fixture(scope="module")
def thin(dev):
    return _thin(dev)


@pytest.fixture(scope="module")
def latent(dev):
    return _yhat(16, seed=11).to(dev)


WB32 = Grid.equiangular(32, 64, method="conservative")                  # WeatherBench 5.625 deg, south to north: 23 taps
WB128 = Grid.equiangular(128, 256)
BOX01 = Grid.regular(0.1, 0.1, region=(40, 44, -3, 5))                  # finer than the source, across 0 deg
GAUSS = Grid.gaussian(48, 96, method="conservative")
MODEL_GRIDS = [WB32, WB128, BOX01, GAUSS, Grid.regular(1.0, 1.0, method="conservative")]
MODEL_CHANS = [None, [6], [5, 1, 3]]


@pytest.mark.parametrize("engine", ["default", "f32"])
def test_regridded_decode_equals_the_helper_on_the_full_decode(thin, latent, dev, engine):
    keep = thin.gemm_mode
    try:
        if engine == "f32":
            thin.gemm_mode = "f32"
        mean = torch.linspace(-1, 1, 8, device=dev)
        std = torch.linspace(0.5, 2, 8, device=dev)
        full_n = thin.decode_latent(latent)[0].cpu().numpy()
        full_d = thin._decode_guarded(latent[0], mean=mean, std=std).cpu().numpy()
        for n, g in enumerate(MODEL_GRIDS):
            chans = MODEL_CHANS[n % 3]
            plan = g.plan(H, W)
            if n % 2 == 0:
                c_, _, _, _, p_ = thin._selection_args(chans, regrid=g)
                assert p_ is plan
                got = thin._decode_guarded(latent[0], mean=mean, std=std, channels=c_, regrid=p_)
                ref = ref_regrid(full_d, plan, chans)[0]
            else:
                got = thin.decode_latent(latent, channels=chans, regrid=g if n % 4 == 1 else plan)[0]
                ref = ref_regrid(full_n, plan, chans)[0]
            assert same_bits(got.cpu().numpy(), ref), (engine, g, chans)
            # the un-embed ran on the source box only
            sb = plan["src_box"]
            shape = thin._tls.bufs["dev"]["ue_regrid_src"][0][0]
            assert shape == (8 if chans is None else len(chans), sb[1] - sb[0], sb[3]), (g, shape)
        assert BOX01.plan(H, W)["src_box"] == (184, 201, 1428, 33)
        # a plain decode afterwards is unchanged
        assert same_bits(thin.decode_latent(latent)[0].cpu().numpy(), full_n)
        assert thin.range_fallbacks == [0, 0]
    finally:
        thin.gemm_mode = keep


def test_regrid_onto_the_stride_and_coarsen_grids(thin, latent):
    full = thin.decode_latent(latent)[0].cpu().numpy()
    g = subset.grid_box((-90, 90, 0, 360), stride=6)
    got = thin.decode_latent(latent, regrid=Grid(g["lat"], g["lon"]))[0].cpu().numpy()
    assert same_bits(got, thin.decode_latent(latent, step=6)[0].cpu().numpy()) and same_bits(got, full[:, ::6, ::6])
    # conservative onto coarsen=6's own cells: the same real number by two float64 routes, each rounded to fp32 once
    c = subset.grid_box((-90, 90, 0, 360), coarsen=6)
    cons = Grid(c["lat"], c["lon"], "conservative", c["lat_bnds"], c["lon_bnds"])
    plan = cons.plan(H, W)
    a = thin.decode_latent(latent, regrid=cons)[0].cpu().numpy().astype(np.float64)
    b = thin.decode_latent(latent, coarsen=6)[0].cpu().numpy()
    ulp = np.maximum(np.spacing(np.abs(b)), np.spacing(np.abs(a.astype(np.float32)))).astype(np.float64)
    bound = (plan["ntap"][None, :, None] + plan["ctap"][None, None, :] + 3) * 2.0 ** -52 * rh.abs_regrid(full, plan)
    diff = np.abs(a - b.astype(np.float64))
    print("regrid vs coarsen=6: max |diff| / ulp =", float((diff / ulp).max()), " points that differ:", int((diff > 0).sum()))
    assert (diff <= np.maximum(ulp, bound)).all()


def test_regrid_argument_errors(thin, latent):
    for kw, name in ((dict(box=(0, 100, 0, 100)), "box"), (dict(step=6), "step"), (dict(coarsen=6), "coarsen")):
        with pytest.raises(ValueError, match=f"regrid and {name}"):
            thin.decode_latent(latent, regrid=WB128, **kw)
    for bad in ((32, 64), "wb32", 6, WB128.plan(13, 24)):
        with pytest.raises(ValueError, match="regrid"):
            thin.decode_latent(latent, regrid=bad)
    with pytest.raises(ValueError, match="latent"):
        thin.decompress([[b""], [b""]], (18, 36), return_format="latent", regrid=WB128)
    with pytest.raises(ValueError, match="regrid_frame"):
        thin.regrid_frame(torch.zeros(8, 10, 10, device=latent.device), WB128)


def _mod_gs(net):      # outlier hidden units in a g_s MLP (tests/test_strided_decode_gpu.py)
    net.g_s.blocks[2].mlp.fc1.weight[:4] *= 3e5
    net.g_s.blocks[2].mlp.fc1.bias[:4] *= 3e5
    net.g_s.blocks[2].mlp.fc2.weight[:, :4] /= 3e5


def test_range_guard_reruns_a_poisoned_regridded_decode(dev, latent):
    net = _thin(dev, _mod_gs)
    ref = _thin(dev, _mod_gs)
    ref.gemm_mode, ref.attn_mode = "f32", "f32"
    full = ref.decode_latent(latent)[0].cpu().numpy()
    assert ref.range_fallbacks == [0, 0]
    for chans, g in [([6, 2], BOX01), (None, WB32)]:
        with pytest.warns(RuntimeWarning, match="exact-f32"):
            got = net.decode_latent(latent, channels=chans, regrid=g)[0]
        assert torch.isfinite(got).all()
        assert same_bits(got.cpu().numpy(), ref_regrid(full, g.plan(H, W), chans)[0]), (chans, g)
    assert net.range_fallbacks == [0, 2]


# ---- the API -----------------------------------------------------------------------------------------------------------


def _api(net, dev, tmp_path):
    api = cra5_api(local_root=str(tmp_path), device="cuda", weights=net)
    api._mean_flat = torch.linspace(-1, 1, 8, device=dev)
    api._std_flat = torch.linspace(0.5, 2, 8, device=dev)
    api.mean, api.std = api._mean_flat.view(8, 1, 1), api._std_flat.view(8, 1, 1)
    return api


@pytest.fixture(scope="module")
def files(thin, dev, tmp_path_factory):
    root = tmp_path_factory.mktemp("regrid")
    api = _api(thin, dev, root)
    frames = [(synth.synth_frame(8, seed=s) * api.std.cpu() + api.mean.cpu()).numpy() for s in (3, 4, 5)]
    stamps = [f"2024-06-01T{6 * h:02d}:00:00" for h in range(3)]
    api.encode_era5_batch(stamps, data=frames, save_root=str(root / "CRA5"), workers=2)
    fulls = [api.decode_from_bin(ts, to_host=True)["x_hat"].reshape(8, H, W) for ts in stamps]
    return api, stamps, frames, fulls, [ref_regrid(f, WB32.plan(H, W))[0] for f in fulls]


META = {"x_hat", "decoding_time", "variables", "lat", "lon", "regrid", "lat_bnds", "lon_bnds"}


def test_api_decode_from_bin_regrid(files):
    api, stamps, _, fulls, refs = files
    d = api.decode_from_bin(stamps[0], regrid=WB32, to_host=True)
    assert set(d) == META and d["regrid"] == "conservative"
    assert d["x_hat"].shape == (8, 32, 64) and same_bits(d["x_hat"], refs[0])
    assert np.array_equal(d["lat"], WB32.lat) and d["lat"][0] == -87.1875 and np.array_equal(d["lon"], WB32.lon)
    assert d["lat_bnds"].shape == (32, 2) and d["lat_bnds"][0].tolist() == [-84.375, -90.0] and d["lon_bnds"][1].tolist() == [5.625, 11.25]
    # variables, on the device, normalised; the latent route; out=
    names = ["z_850", "z_1000", "z_925"]
    chans = [api.vname_to_channels[v] for v in names]
    dn = api.decode_from_bin(stamps[1], variables=names, regrid=BOX01)
    assert dn["variables"] == names and dn["regrid"] == "bilinear" and np.array_equal(dn["lat"], BOX01.lat)
    assert same_bits(dn["x_hat"].reshape(3, 40, 80).cpu().numpy(), ref_regrid(fulls[1], BOX01.plan(H, W), chans)[0])
    full_n = api.decode_from_bin(stamps[1], return_format="normalized", to_host=True)["x_hat"].reshape(8, H, W)
    xr = api.latent_to_reconstruction(api.bin_to_latent(time_stamp=stamps[1]), variables=names[:1], regrid=WB128)
    assert xr.shape == (1, 1, 128, 256) and same_bits(xr[0].cpu().numpy(), ref_regrid(full_n, WB128.plan(H, W), chans[:1])[0])
    out = np.empty((8, 32, 64), dtype=np.float32)
    assert api.decode_from_bin(stamps[0], regrid=WB32, out=out)["x_hat"] is out and same_bits(out, refs[0])
    with pytest.raises(ValueError, match="out"):
        api.decode_from_bin(stamps[0], regrid=WB32, out=np.empty((8, H, W), dtype=np.float32))
    assert set(api.decode_from_bin(stamps[0])) == {"x_hat", "decoding_time"}


def test_api_exclusions(files):
    api, stamps, frames, _, _ = files
    for kw, msg in ((dict(region=(35, 72, -25, 45)), "regrid and region"), (dict(stride=6), "regrid and stride"),
                    (dict(coarsen=6), "regrid and coarsen"), (dict(return_format="latent"), "latent"),
                    (dict(residual=True), "residual= with regrid=")):
        with pytest.raises(ValueError, match=msg):
            api.decode_from_bin(stamps[0], regrid=WB32, **kw)
    for call in (api.decode_batch, api.aggregate_batch, api.decode_to_nc):
        with pytest.raises(ValueError, match="regrid and stride"):
            call(stamps, regrid=WB32, stride=6)
        with pytest.raises(ValueError, match="residual= with regrid="):
            call(stamps, regrid=WB32, residual=True)
    with pytest.raises(ValueError, match="regrid and region"):
        api.latent_to_reconstruction(None, regrid=WB32, region=(0, 10, 0, 10))
    with pytest.raises(ValueError, match="regrid and coarsen"):
        api.evaluate_batch(stamps[:1], data=frames[:1], regrid=WB32, coarsen=6)
    with pytest.raises(ValueError, match="max_error with regrid="):
        api.evaluate_batch(stamps[:1], data=frames[:1], regrid=WB32, max_error=1.0)
    with pytest.raises(ValueError, match="close"):                         # a regional target has no latitude circles
        api.evaluate_batch(stamps[:1], data=frames[:1], regrid=BOX01, spectrum=True)
    with pytest.raises(ValueError, match="width 14"):                      # closes the circle, but 14 = 2 * 7
        api.evaluate_batch(stamps[:1], data=frames[:1], regrid=Grid.equiangular(4, 14), spectrum=True)
    with pytest.raises(ValueError, match="regrid must be"):
        api.decode_batch(stamps, regrid=(32, 64))


def test_api_decode_batch_regrid(files):
    import pack_helpers as ph
    from cra5_amd import pack
    api, stamps, _, _, refs = files
    out = np.empty((3, 8, 32, 64), dtype=np.float32)
    api.decode_batch(stamps, out=out, workers=3, regrid=WB32)
    seen = {}
    api.decode_batch(stamps, workers=1, regrid=WB32, sink=lambda i, fr: seen.__setitem__(i, (fr.shape, fr.copy())))
    fresh = api.decode_batch(stamps, workers=2, regrid=WB32.plan(H, W))
    packed = api.decode_batch(stamps, workers=2, regrid=WB32, pack="int16")
    for i in range(3):
        assert same_bits(out[i], refs[i]) and seen[i][0] == (8, 32, 64) and same_bits(seen[i][1], refs[i]) and same_bits(fresh[i], refs[i])
        rq, scale, offset, vmin, vmax, nonfinite, saturated = ph.ref_pack(refs[i])
        it = packed[i]
        assert it["q"].dtype == np.int16 and np.array_equal(it["q"], rq)
        assert np.array_equal(it["scale_factor"], scale) and np.array_equal(it["add_offset"], offset)
        assert np.array_equal(pack.unpack(it["q"], it["scale_factor"], it["add_offset"]), ph.unpack(rq, scale, offset))
    with pytest.raises(ValueError, match="out"):       # the source grid's shape
        api.decode_batch(stamps, out=np.empty((3, 8, H, W), dtype=np.float32), regrid=WB32)


def test_api_aggregate_batch_regrid(files):
    api, stamps, _, _, refs = files
    res = api.aggregate_batch(stamps, stats=("mean", "max"), regrid=WB32, workers=3)
    assert res["n"] == 3 and res["regrid"] == "conservative" and res["mean"].shape == (8, 32, 64)
    assert np.array_equal(res["lat"], WB32.lat) and np.array_equal(res["lon_bnds"], WB32.lon_bnds) and res["lat_bnds"].shape == (32, 2)
    ref = ref_time_stats(refs)
    assert same_bits(res["mean"], ref["mean"]) and same_bits(res["max"], ref["max"])


def test_api_evaluate_batch_regrid(files, dev):
    api, stamps, frames, fulls, refs = files
    paths = [f"{api.local_root}/CRA5/{ts[:4]}/{ts}.bin" for ts in stamps]
    plan = WB32.plan(H, W)
    reps = api.evaluate_batch(stamps[:2], data=frames[:2], bins=paths[:2], workers=2, regrid=WB32)
    for i, rep in enumerate(reps):
        truth = ref_regrid(frames[i], plan)[0]
        t_dev = api.net.regrid_frame(torch.from_numpy(frames[i]).to(dev), WB32)
        assert same_bits(t_dev.cpu().numpy(), truth)
        same = metrics.reconstruction_error(torch.from_numpy(refs[i]).to(dev), torch.from_numpy(truth).to(dev),
                                            lat_weights=plan["area_weights"])
        for key in ("mse", "rmse", "wrmse", "bias", "mae", "max_abs", "nonfinite"):
            assert np.array_equal(rep[key], same[key], equal_nan=True), key
        assert not np.array_equal(rep["wrmse"], rep["rmse"])
        assert rep["regrid"] == "conservative" and np.array_equal(rep["lat"], WB32.lat) and np.array_equal(rep["lon"], WB32.lon)
        assert np.array_equal(rep["lat_bnds"], WB32.lat_bnds) and np.array_equal(rep["lon_bnds"], WB32.lon_bnds)
        assert rep["compression_ratio"] == 8 * H * W * 4 / rep["bin_bytes"]
    assert abs(plan["area_weights"].mean() - 1.0) < 1e-15 and plan["area_weights"][0] < 0.1
    # a regional truth goes through the crop of its source box; the spectrum of a target that closes the circle
    t_box = api.net.regrid_frame(torch.from_numpy(frames[0]).to(dev), BOX01)
    assert same_bits(t_box.cpu().numpy(), ref_regrid(frames[0], BOX01.plan(H, W))[0])
    spec = api.evaluate_batch(stamps[:1], data=frames[:1], bins=paths[:1], workers=1, regrid=WB32, spectrum=True)[0]
    assert spec["power_truth"].shape == (8, 33) and np.array_equal(spec["rmse"], reps[0]["rmse"])
    assert "regrid" not in api.evaluate_batch(stamps[:1], data=frames[:1], bins=paths[:1], workers=1)[0]


def test_api_decode_to_nc_regrid(files, tmp_path):
    from scipy.io import netcdf_file
    api, stamps, _, _, refs = files
    res = api.decode_to_nc(stamps[:1], save_root=str(tmp_path), variables=["z_850", "z_1000"], regrid=WB32, workers=1)
    path = f"{tmp_path}/ERA5/2024/{stamps[0]}_pressure.nc"
    assert res[0]["files"] == [path]
    f = netcdf_file(path, "r", mmap=False, maskandscale=True)
    assert f.variables["z"].shape == (1, 2, 32, 64)
    assert np.array_equal(f.variables["latitude"][:], WB32.lat.astype(np.float32))
    assert np.array_equal(f.variables["longitude"][:], WB32.lon.astype(np.float32))
    chans = [api.vname_to_channels[v] for v in ("z_850", "z_1000")]
    z = np.ma.filled(f.variables["z"][:], np.nan)[0]
    want = refs[0][chans].astype(np.float64)
    assert np.abs(z - want).max() <= (want.max() - want.min()) / 65534 * 0.51 + 1e-9 * np.abs(want).max()
    f.close()
