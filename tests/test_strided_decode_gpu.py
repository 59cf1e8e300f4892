"""Thinned (strided) decode on the GPU (VAEformer.decode_latent / decompress with step, cra5_api stride=): the result is
the slice full[channels][:, kept_rows][:, :, kept_cols] of a full decode of the same latent, bit for bit, under every
engine and precision the full decode supports; the two new kernels (cra5_gather_token_lattice,
cra5_strided_scatter_f32) equal their numpy restatement."""
import warnings

import numpy as np
import pytest
import torch

from cra5_amd import ops, subset, synth
from cra5_amd.api import cra5_api
from cra5_amd.vaeformer import VAEformer

pytestmark = pytest.mark.gpu

H, W = 721, 1440


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


def _slice(full, chans, box, stride):
    """full [C, H, W] -> full[chans][:, kept rows][:, :, kept columns]: the rows r of the box with r % s_lat == 0, the
    columns c of the box (eastward, wrapping at W) with c % s_lon == 0; stride None: every row / column of the box."""
    x = full if chans is None else full[list(chans)]
    r0, r1, c0, nc = box if box is not None else (0, full.shape[-2], 0, full.shape[-1])
    sy, sx = stride if stride is not None else (1, 1)
    rows = [r for r in range(r0, r1) if r % sy == 0]
    cols = [(c0 + k) % full.shape[-1] for k in range(nc) if ((c0 + k) % full.shape[-1]) % sx == 0]
    return x.index_select(1, torch.tensor(rows, device=full.device)).index_select(
        2, torch.tensor(cols, device=full.device)).contiguous()


def _same_bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    return tuple(a.shape) == tuple(b.shape) and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.fixture(scope="module")
def thin(dev):
    return _thin(dev)


@pytest.fixture(scope="module")
def latent(dev):
    return _yhat(16, seed=11).to(dev)


# ---- the two new kernels against numpy -------------------------------------------------------------------------------


def test_gather_token_lattice_matches_numpy(dev):
    g = torch.Generator().manual_seed(0)
    Hp, Wp, K = 7, 12, 36
    src = torch.randn(Hp * Wp, K, generator=g)
    s = src.numpy().reshape(Hp, Wp, K)
    cases = [(1, 2, 3, 7, 3, 4), (0, 1, 7, 0, 1, 12), (6, 5, 1, 11, 7, 1), (2, 3, 2, 10, 4, 3), (0, 6, 2, 5, 6, 2),
             (3, 1, 4, 9, 1, 6)]
    for ti0, ti_step, n_ti, tj0, tj_step, n_tj in cases:
        out = ops.gather_token_rows(src.to(dev), torch.full((n_ti * n_tj, K), -7.0, device=dev), Hp, Wp, ti0, n_ti, tj0,
                                    n_tj, ti_step=ti_step, tj_step=tj_step)
        ref = s[[ti0 + i * ti_step for i in range(n_ti)]][:, [(tj0 + j * tj_step) % Wp for j in range(n_tj)]]
        assert np.array_equal(out.cpu().numpy(), ref.reshape(-1, K)), (ti0, ti_step, n_ti, tj0, tj_step, n_tj)
    # steps of 1 are cra5_gather_token_rows
    a = ops.gather_token_rows(src.to(dev), torch.empty(3 * 5, K, device=dev), Hp, Wp, 2, 3, 9, 5)
    b = ops.gather_token_rows(src.to(dev), torch.empty(3 * 5, K, device=dev), Hp, Wp, 2, 3, 9, 5, ti_step=1, tj_step=1)
    assert torch.equal(a, b)
    # split-f16 rows (and plain rows) are copied verbatim, layout flag and scale included, into a slice of a workspace
    sm = ops.split_f16(src.to(dev), "auto")
    for plain in (False, True):
        m = sm.plain_copy() if plain else sm
        if plain:   # a plain row living in a split-layout buffer, as the LayerNorm writes it
            buf = ops.SplitMat.empty(Hp * Wp, K, dev, zero=True)
            buf.data[:, :m.Kp].copy_(m.data)
            m = ops.SplitMat(buf.data, Hp * Wp, K, m.Kp, m.scale_inv, plain=True)
        ws = ops.SplitMat.empty(20, K, dev, zero=True)
        dst = ops.SplitMat(ws.data[4:4 + 2 * 3], 6, K, ws.Kp)
        out = ops.gather_token_rows(m, dst, Hp, Wp, 1, 2, 8, 3, ti_step=4, tj_step=3)
        assert out.plain == plain and out.scale_inv == m.scale_inv
        idx = [t * Wp + (8 + 3 * j) % Wp for t in (1, 5) for j in range(3)]
        n = m.Kp if plain else 2 * m.Kp
        assert torch.equal(ws.data[4:10, :n], m.data[idx, :n])
        assert not ws.data[:4].any() and not ws.data[10:].any()        # nothing outside the slice
    with pytest.raises(Exception, match="cra5_gather_token_lattice"):
        ops.gather_token_rows(src.to(dev), torch.empty(2 * 3, K, device=dev), Hp, Wp, 0, 2, 0, 3, ti_step=7, tj_step=1)


def _scatter_ref(tb, g, C, Ho, Wo, mean=None, std=None):
    """numpy restatement of cra5_strided_scatter_f32."""
    rows, cols, cls, n_cc = tb["rows"], tb["cols"], tb["cls"], tb["n_cc"]
    cc, tj, kx = cols[:, 0], cols[:, 1], cols[:, 2]
    out = np.empty((C, Ho, Wo), dtype=np.float32)
    for c in range(C):
        for i in range(Ho):
            acc = None
            for rc, ti, ky in (rows[i, :3], rows[i, 3:]):
                if rc < 0:
                    continue
                k = cls[rc * n_cc + cc]
                v = g[k[:, 0] + (ti * k[:, 2] + tj) * k[:, 1] + c * k[:, 4] + ky * k[:, 3] + kx]
                acc = v if acc is None else acc + v
            out[c, i] = acc if mean is None else acc * std[c] + mean[c]
    return out


# (kh, kw, sh, sw, Hp, Wp) small un-embed geometries with kh = sh + 1, kw = sw; box; stride
SCATTER_CASES = [
    ((3, 2, 2, 2, 5, 7), None, (2, 2)),               # H = 11, W = 14: one class, odd output width (7)
    ((3, 2, 2, 2, 5, 7), None, (4, 1)),               # two row classes with a single tap each
    ((3, 2, 2, 2, 5, 7), None, (3, 7)),               # three row classes; one column kept per 7
    ((3, 2, 2, 2, 5, 7), (1, 2, 3, 5), (1, 1)),       # a box inside one patch row: no seam at all
    ((3, 2, 2, 2, 5, 7), (3, 9, 11, 9), (2, 2)),      # seams at both ends, columns wrap
    ((11, 10, 10, 10, 3, 6), None, (6, 4)),           # the ERA5 patch on a small grid: 3 x 2 classes
    ((11, 10, 10, 10, 3, 6), (9, 22, 55, 11), (5, 3)),
    ((4, 3, 3, 3, 6, 5), None, (1, 5)),               # every row, every 5th column: W = 15
]


@pytest.mark.parametrize("geo, box, stride", SCATTER_CASES)
def test_strided_scatter_matches_numpy(dev, geo, box, stride):
    kh, kw, sh, sw, Hp, Wp = geo
    Hi, Wi = sh * (Hp - 1) + kh, sw * Wp
    C = 3
    plan = subset.stride_plan(box, stride, Hi, Wi, kh, kw, sh, sw, C=C)
    tb = subset.scatter_tables(plan, C)
    rng = np.random.default_rng(1)
    # integer-valued data and statistics: x * std + mean is exact, fused or not
    g = rng.integers(-99, 100, size=tb["elems"]).astype(np.float32)
    mean = np.array([3.0, -20.0, 0.0], dtype=np.float32)
    std = np.array([2.0, 1.0, -8.0], dtype=np.float32)
    t = {k: torch.from_numpy(tb[k]).to(dev) for k in ("rows", "cols", "cls")}
    for m, s in ((None, None), (mean, std)):
        base = torch.full((C * plan["Ho"] * plan["Wo"] + 2,), -7.0, device=dev)
        out = base[1:-1].view(C, plan["Ho"], plan["Wo"])             # at 4-byte, not 16-byte, alignment
        ops.strided_scatter(torch.from_numpy(g).to(dev), t["rows"], t["cols"], t["cls"], tb["n_cc"], C,
                            mean=None if m is None else torch.from_numpy(m).to(dev),
                            std=None if s is None else torch.from_numpy(s).to(dev), out=out)
        ref = _scatter_ref(tb, g, C, plan["Ho"], plan["Wo"], m, s)
        assert np.array_equal(out.cpu().numpy(), ref)
        assert float(base[0]) == -7.0 and float(base[-1]) == -7.0    # nothing written around the image
    # the numpy restatement itself: the tables assemble the slice of the overlap-add image
    Y = rng.integers(-50, 51, size=(Hp, Wp, C, kh, kw)).astype(np.float32)
    full = np.zeros((C, Hi, Wi), dtype=np.float32)
    for ti in range(Hp):
        for tj in range(Wp):
            full[:, sh * ti:sh * ti + kh, sw * tj:sw * tj + kw] += Y[ti, tj]
    g2 = np.zeros(tb["elems"], dtype=np.float32)
    for i, j, off, M, N in tb["gemms"]:
        rc, cc = plan["row_classes"][i], plan["col_classes"][j]
        tis = [rc["t0"] + k * rc["step"] for k in range(rc["n"])]
        tjs = [(cc["t0"] + k * cc["step"]) % Wp for k in range(cc["n"])]
        g2[off:off + M * N] = Y[np.ix_(tis, tjs, range(C), rc["taps"], cc["taps"])].reshape(-1)
    got = ops.strided_scatter(torch.from_numpy(g2).to(dev), t["rows"], t["cols"], t["cls"], tb["n_cc"], C)
    assert np.array_equal(got.cpu().numpy(), full[:, plan["rows"]][:, :, plan["cols"]])


def test_strided_scatter_refuses_foreign_tables(dev):
    """Tables that do not belong to the workspace write NaN into the point and read nothing out of bounds."""
    plan = subset.stride_plan(None, (2, 2), 11, 14, 3, 2, 2, 2, C=1)
    tb = subset.scatter_tables(plan, 1)
    t = {k: torch.from_numpy(tb[k]).to(dev) for k in ("rows", "cols", "cls")}
    g = torch.ones(tb["elems"], device=dev)
    assert torch.isfinite(ops.strided_scatter(g, t["rows"], t["cols"], t["cls"], tb["n_cc"], 1)).all()
    out = ops.strided_scatter(g[:8], t["rows"], t["cols"], t["cls"], tb["n_cc"], 1)       # a workspace too small
    assert torch.isnan(out).any() and tuple(out.shape) == (1, plan["Ho"], plan["Wo"])
    bad = t["cols"].clone()
    bad[0, 0] = 5                                                                          # a class that does not exist
    out = ops.strided_scatter(g, t["rows"], bad, t["cls"], tb["n_cc"], 1)
    assert torch.isnan(out[:, :, 0]).all() and torch.isfinite(out[:, :, 1:]).all()
    with pytest.raises(ValueError, match="strided_scatter"):
        ops.strided_scatter(g, t["rows"].long(), t["cols"], t["cls"], tb["n_cc"], 1)


# ---- bit identity with the slice of a full decode --------------------------------------------------------------------

STRIDES = [(2, 2), (4, 4), (5, 5), (6, 6), (10, 10), (6, 4), (7, 6), (1, 6), (6, 1)]
CHANNELS = [None, [0], [7], [0, 7], [5, 1, 3], list(range(8))]
BOXES = [
    (30, 31, 100, 50),       # a single seam row
    (30, 41, 0, 40),         # both edges on seam rows
    (0, 5, 0, 40),           # row 0 (the grid's top edge)
    (715, 721, 200, 33),     # row 720 (the bottom edge)
    (360, 361, 720, 1),      # a single kept point
    (72, 221, 1340, 281),    # across 0 deg (Europe: 35-72 N, -25-45 E)
    (123, 456, 1437, 7),     # odd offsets across 0 deg
    (200, 260, 1, 1440),     # the full circle off a patch boundary
    (0, 721, 720, 1440),     # the whole globe centred on Greenwich
    None,                    # the whole globe
]
ENGINES = {
    "default": {},
    "f32": dict(gemm_mode="f32"),
    "unfused": dict(fused_unembed=False),
    "f16": dict(precision="f16"),
    "f16_unfused": dict(precision="f16", fused_unembed=False),
    "f16_split": dict(precision="f16", f16_layout="split"),
    "f16_split_unfused": dict(precision="f16", f16_layout="split", fused_unembed=False),
}


def _keeps(box, stride):
    try:
        subset.kept_points(box if box is not None else (0, H, 0, W), stride, W)
        return True
    except ValueError:
        return False


def _cases():
    """(channels, box, stride, de-normalised): every stride over the globe and over every box that holds a kept point,
    the channel selections rotating through the boxes; every channel selection at every stride on one box."""
    out, k = [], 0
    for st in STRIDES:
        for box in BOXES:
            if not _keeps(box, st):
                continue
            out.append((CHANNELS[k % len(CHANNELS)], box, st, k % 3 == 0))
            k += 1
        for ch in CHANNELS:
            out.append((ch, BOXES[5], st, k % 2 == 0))
            k += 1
    return out


def test_case_list_leaves_nothing_out():
    cases = _cases()
    assert {c[2] for c in cases} == set(STRIDES)
    for st in STRIDES:
        boxes = {c[1] for c in cases if c[2] == st}
        assert None in boxes and BOXES[5] in boxes and BOXES[7] in boxes and BOXES[8] in boxes
        assert len(boxes) >= 7                      # (a few boxes hold no kept point at a few strides: that is refused)
        assert {tuple(c[0]) if c[0] else None for c in cases if c[2] == st and c[1] == BOXES[5]} == \
               {tuple(c) if c else None for c in CHANNELS}
    for box in BOXES:                               # every box is decoded at some stride, in both output forms
        assert {c[3] for c in cases if c[1] == box} == {True, False}


@pytest.mark.parametrize("engine", list(ENGINES))
def test_thinned_equals_slice_of_full_decode(thin, latent, dev, engine):
    keep = (thin.precision, thin.gemm_mode, thin.fused_unembed, thin.f16_layout)
    try:
        for k, v in ENGINES[engine].items():
            setattr(thin, k, v)
        mean = torch.linspace(-1, 1, 8, device=dev)
        std = torch.linspace(0.5, 2, 8, device=dev)
        full_n = thin.decode_latent(latent)[0]
        full_d = thin._decode_guarded(latent[0], mean=mean, std=std)
        for chans, box, st, denorm in _cases():
            if denorm:
                ch, bx = thin._subset_args(chans, box)
                got = thin._decode_guarded(latent[0], mean=mean, std=std, channels=ch, box=bx, step=thin._step_arg(st, bx))
            else:
                got = thin.decode_latent(latent, channels=chans, box=box, step=st)[0]
            assert _same_bits(got, _slice(full_d if denorm else full_n, chans, box, st)), (engine, chans, box, st, denorm)
        # an int is the pair; 1 / (1, 1) / None are the unthinned path
        assert _same_bits(thin.decode_latent(latent, step=6)[0], _slice(full_n, None, None, (6, 6)))
        assert _same_bits(thin.decode_latent(latent, step=1)[0], full_n)
        assert _same_bits(thin.decode_latent(latent, channels=[2], box=BOXES[6], step=(1, 1))[0],
                          _slice(full_n, [2], BOXES[6], None))
        assert thin.range_fallbacks == [0, 0]
    finally:
        thin.precision, thin.gemm_mode, thin.fused_unembed, thin.f16_layout = keep


def test_no_stride_after_strides_and_alternating_strides(thin, latent, dev):
    """Workspaces are not shared wrongly (a full / subset decode after thinned ones is unchanged) and the cache keys
    are complete (alternating strides, channels and boxes on one thread, more request shapes than the cache holds)."""
    full = thin.decode_latent(latent)[0].clone()
    reqs = [(None, None, (6, 6)), ([5, 1, 3], None, (6, 6)), (None, None, (4, 4)), ([5, 1, 3], BOXES[5], (6, 4)),
            (None, None, None), ([3, 1, 5], None, (6, 6)), (None, BOXES[5], (6, 4)), ([5, 1, 3], BOXES[5], None),
            (None, None, (2, 2)), (None, None, (6, 6)), ([5, 1, 3], BOXES[6], (6, 4)), (None, None, (10, 10)),
            ([0], None, (5, 5)), ([7], BOXES[7], (1, 6)), (None, None, (7, 6)), (None, None, (6, 1))]
    for rnd in range(2):
        for chans, box, st in reqs:
            got = thin.decode_latent(latent, channels=chans, box=box, step=st)[0]
            assert _same_bits(got, _slice(full, chans, box, st)), (rnd, chans, box, st)
            assert len(thin._sub_cache) <= VAEformer.SUBSET_CACHE
    assert _same_bits(thin.decode_latent(latent, step=None)[0], full)


def test_step_argument_errors(thin, latent):
    for bad in (0, -1, (2, 0), 2.5, "2", (2, 2, 2), True):
        with pytest.raises(ValueError, match="stride"):
            thin.decode_latent(latent, step=bad)
    with pytest.raises(ValueError, match=r"1440 % s_lon \(7\)"):
        thin.decode_latent(latent, step=7)
    with pytest.raises(ValueError, match="no row"):
        thin.decode_latent(latent, box=(1, 5, 0, 40), step=6)
    with pytest.raises(ValueError, match="no column"):
        thin.decode_latent(latent, box=(0, 10, 1, 5), step=6)


# ---- range guard ------------------------------------------------------------------------------------------------------


def _mod_gs(net):      # outlier hidden units in a g_s MLP (tests/test_model_gpu.py, range guard on the decode side)
    net.g_s.blocks[2].mlp.fc1.weight[:4] *= 3e5
    net.g_s.blocks[2].mlp.fc1.bias[:4] *= 3e5
    net.g_s.blocks[2].mlp.fc2.weight[:, :4] /= 3e5


def test_range_guard_reruns_a_poisoned_thinned_decode(dev, latent):
    net = _thin(dev, _mod_gs)
    ref = _thin(dev, _mod_gs)
    ref.gemm_mode, ref.attn_mode = "f32", "f32"
    full = ref.decode_latent(latent)[0]
    assert ref.range_fallbacks == [0, 0]
    for chans, box, st in [([6, 2], (72, 221, 1340, 281), (6, 4)), (None, None, (6, 6)), (None, (360, 361, 720, 1), (10, 10))]:
        with pytest.warns(RuntimeWarning, match="exact-f32"):
            got = net.decode_latent(latent, channels=chans, box=box, step=st)[0]
        assert _same_bits(got, _slice(full, chans, box, st)), (chans, box, st)
    assert net.range_fallbacks == [0, 3]


def test_thinned_decode_itself_is_probed(thin, latent, dev):
    """A non-finite std of a kept channel poisons only the thinned result (the residual stream is finite): the probe of
    the result catches it - the re-run gives the same, and the decode is an error; the same std on a channel that is
    not kept is no error."""
    mean = torch.zeros(8, device=dev)
    std = torch.ones(8, device=dev)
    std[5] = float("nan")
    before = list(thin.range_fallbacks)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        with pytest.raises(FloatingPointError, match="exact-f32 engines too"):
            thin._decode_guarded(latent[0], mean=mean, std=std, channels=(1, 5), step=(6, 6))
        with pytest.raises(FloatingPointError, match="exact-f32 engines too"):
            thin._decode_guarded(latent[0], mean=mean, std=std, step=(10, 10))
    thin.range_fallbacks[:] = before
    ok = thin._decode_guarded(latent[0], mean=mean, std=std, channels=(1, 4), step=(6, 6))
    assert torch.isfinite(ok).all() and tuple(ok.shape) == (2, 121, 240)


# ---- API (thin model) --------------------------------------------------------------------------------------------------


def _api(net, dev, tmp_path, C=8):
    api = cra5_api(local_root=str(tmp_path), device="cuda", weights=net)
    if C != 268:                                               # (268-channel stats do not fit the 8-channel thin model)
        api._mean_flat = torch.linspace(-1, 1, C, device=dev)
        api._std_flat = torch.linspace(0.5, 2, C, device=dev)
        api.mean, api.std = api._mean_flat.view(C, 1, 1), api._std_flat.view(C, 1, 1)
    return api


def test_api_decode_from_bin_stride(thin, dev, tmp_path):
    api = _api(thin, dev, tmp_path)
    frame = synth.synth_frame(8, seed=3) * api.std.cpu() + api.mean.cpu()
    ts = "2024-06-01T00:00:00"
    api.encode_era5_as_bin(ts, save_root=str(tmp_path / "CRA5"), data=frame)
    full = api.decode_from_bin(ts)
    fx = full["x_hat"].reshape(8, H, W)
    assert set(full) == {"x_hat", "decoding_time"}
    for same in (1, (1, 1), None):                             # "no stride": today's result, today's dict
        d1 = api.decode_from_bin(ts, stride=same)
        assert set(d1) == {"x_hat", "decoding_time"} and _same_bits(d1["x_hat"], full["x_hat"])
    # the 1.5 degree grid
    d = api.decode_from_bin(ts, stride=6)
    g = cra5_api.grid_box((-90, 90, 0, 360), stride=6)
    assert set(d) == {"x_hat", "decoding_time", "variables", "lat", "lon"}
    assert tuple(d["x_hat"].shape[-3:]) == (8, 121, 240) and _same_bits(d["x_hat"].reshape(8, 121, 240), _slice(fx, None, None, (6, 6)))
    assert np.array_equal(d["lat"], g["lat"]) and np.array_equal(d["lon"], g["lon"]) and d["lat"][1] == 88.5
    assert d["variables"] == [api.channels_to_vname[c] for c in range(8)]
    # with variables and a region, to the host
    names = ["z_850", "z_1000", "z_925"]
    chans = [api.vname_to_channels[v] for v in names]
    region = (35, 72, -25, 45)
    g = cra5_api.grid_box(region, stride=(6, 4))
    d = api.decode_from_bin(ts, variables=names, region=region, stride=(6, 4), to_host=True)
    assert d["variables"] == names and isinstance(d["x_hat"], np.ndarray)
    assert np.array_equal(d["lat"], g["lat"]) and np.array_equal(d["lon"], g["lon"])
    assert d["lat"][0] == 72.0 and d["lat"][-1] == 36.0 and d["lon"][0] == 335.0 and d["lon"][-1] == 45.0
    ref = _slice(fx, chans, g["box"], (6, 4)).cpu().numpy()
    assert d["x_hat"].shape == (3, 25, 71) == (3, len(g["lat"]), len(g["lon"]))
    assert np.array_equal(d["x_hat"].view(np.int32), ref.view(np.int32))
    # out= is checked against the thinned shape
    out = np.empty((3, 25, 71), dtype=np.float32)
    d = api.decode_from_bin(ts, variables=names, region=region, stride=(6, 4), out=out)
    assert d["x_hat"] is out and np.array_equal(out.view(np.int32), ref.view(np.int32))
    with pytest.raises(ValueError, match="out"):
        api.decode_from_bin(ts, variables=names, region=region, stride=(6, 4), out=np.empty((3, 149, 281), dtype=np.float32))
    with pytest.raises(ValueError, match="out"):
        api.decode_from_bin(ts, stride=6, out=np.empty((8, H, W), dtype=np.float32))
    # normalised, region only, and the latent route
    full_n = api.decode_from_bin(ts, return_format="normalized")["x_hat"]
    dn = api.decode_from_bin(ts, return_format="normalized", region=(-10.3, 20.1, 350.2, 9.9), stride=(5, 2))
    gb = cra5_api.grid_box((-10.3, 20.1, 350.2, 9.9), stride=(5, 2))
    assert _same_bits(dn["x_hat"][0], _slice(full_n[0], None, gb["box"], (5, 2))) and np.array_equal(dn["lon"], gb["lon"])
    xr = api.latent_to_reconstruction(api.bin_to_latent(time_stamp=ts), variables=names[:1], stride=10)
    assert xr.shape == (1, 1, 73, 144) and _same_bits(xr[0], _slice(full_n[0], chans[:1], None, (10, 10)))
    with pytest.raises(ValueError, match="latent"):
        api.decode_from_bin(ts, return_format="latent", stride=6)
    with pytest.raises(ValueError, match=r"1440 % s_lon \(7\)"):
        api.decode_from_bin(ts, stride=7)
    with pytest.raises(ValueError, match="stride"):
        api.decode_from_bin(ts, stride=0)
    with pytest.raises(ValueError, match="no row"):
        api.decode_from_bin(ts, region=(89.0, 89.75, 0, 10), stride=6)
    with pytest.raises(ValueError, match="latent"):
        thin.decompress([[b""], [b""]], (18, 36), return_format="latent", step=6)


def test_api_decode_batch_stride(thin, dev, tmp_path):
    api = _api(thin, dev, tmp_path)
    frames = [(synth.synth_frame(8, seed=s) * api.std.cpu() + api.mean.cpu()).numpy() for s in (3, 4, 5)]
    stamps = [f"2024-06-01T{h:02d}:00:00" for h in range(3)]
    api.encode_era5_batch(stamps, data=frames, save_root=str(tmp_path / "CRA5"), workers=3)
    names, region, st = ["z_825", "z_975"], (-10.3, 20.1, 350.2, 9.9), (4, 6)
    g = cra5_api.grid_box(region, stride=st)
    chans = [api.vname_to_channels[v] for v in names]
    shape = (2, len(g["lat"]), len(g["lon"]))
    out = np.empty((3,) + shape, dtype=np.float32)
    rec = api.decode_batch(stamps, out=out, workers=3, variables=names, region=region, stride=st)
    seen, glob = {}, {}
    api.decode_batch(stamps, workers=2, variables=names, region=region, stride=st,
                     sink=lambda i, fr: seen.__setitem__(i, (fr.shape, fr.copy())))
    api.decode_batch(stamps, workers=3, stride=6, return_format="normalized",
                     sink=lambda i, fr: glob.__setitem__(i, (fr.shape, fr.copy())))
    for i, ts in enumerate(stamps):
        full = api.decode_from_bin(ts)["x_hat"].reshape(8, H, W)
        ref = _slice(full, chans, g["box"], st).cpu().numpy()
        assert np.array_equal(out[i].view(np.int32), ref.view(np.int32)) and rec[i] is not None
        assert seen[i][0] == shape and np.array_equal(seen[i][1].view(np.int32), ref.view(np.int32))
        full_n = api.decode_from_bin(ts, return_format="normalized")["x_hat"].reshape(8, H, W)
        assert glob[i][0] == (8, 121, 240)
        assert np.array_equal(glob[i][1].view(np.int32), _slice(full_n, None, None, (6, 6)).cpu().numpy().view(np.int32))
    with pytest.raises(ValueError, match="out"):       # the unthinned subset's shape
        api.decode_batch(stamps, out=np.empty((3, 2, 123, 80), dtype=np.float32), variables=names, region=region, stride=st)
    with pytest.raises(ValueError, match="out"):
        api.decode_batch(stamps, out=np.empty((3, 8, H, W), dtype=np.float32), stride=6)
    # stride=1 is a plain decode_batch
    out_full = np.empty((3, 8, H, W), dtype=np.float32)
    api.decode_batch(stamps, out=out_full, workers=3, stride=1)
    assert np.array_equal(out_full[1].view(np.int32), api.decode_from_bin(stamps[1])["x_hat"].reshape(8, H, W).cpu().numpy().view(np.int32))


# ---- the 268 model ----------------------------------------------------------------------------------------------------


def test_stride_6_on_the_268_model(dev, tmp_path):
    net = VAEformer(268)
    synth.load_synthetic(net, seed=0)
    net = net.to(dev)
    api = _api(net, dev, tmp_path, C=268)
    y = _yhat(256, seed=5).to(dev)
    full = net._decode_guarded(y[0], mean=api._mean_flat, std=api._std_flat)
    got = net._decode_guarded(y[0], mean=api._mean_flat, std=api._std_flat, step=(6, 6))
    assert tuple(got.shape) == (268, 121, 240) and _same_bits(got, _slice(full, None, None, (6, 6)))
    # (2, 2) and (4, 4) on 268 channels: class GEMMs of 10368 x 8040 and 2592 x 2412, the big-tile instantiations
    for st, shape in (((2, 2), (268, 361, 720)), ((4, 4), (268, 181, 360))):
        got = net._decode_guarded(y[0], mean=api._mean_flat, std=api._std_flat, step=st)
        assert tuple(got.shape) == shape and _same_bits(got, _slice(full, None, None, st)), st
    del full, got
    # through the files: decode_batch(stride=6, sink=...) delivers [268, 121, 240] arrays, the slice of decode_from_bin
    frame = (synth.synth_frame(268, seed=1) * api.std.cpu() + api.mean.cpu()).numpy()
    stamps = ["2024-06-01T00:00:00", "2024-06-01T06:00:00"]
    api.encode_era5_batch(stamps, data=[frame, frame], save_root=str(tmp_path / "CRA5"), workers=2)
    seen = {}
    api.decode_batch(stamps, workers=2, stride=6, sink=lambda i, fr: seen.__setitem__(i, (fr.shape, fr.dtype, fr.copy())))
    ref = _slice(api.decode_from_bin(stamps[0])["x_hat"].reshape(268, H, W), None, None, (6, 6)).cpu().numpy()
    for i in range(2):
        assert seen[i][0] == (268, 121, 240) and seen[i][1] == np.float32
        assert np.array_equal(seen[i][2].view(np.int32), ref.view(np.int32))
