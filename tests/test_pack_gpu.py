"""Packed int16 output on the GPU (cra5_pack_range_f32 / cra5_pack_i16_f32, ops.pack_range / ops.pack_i16, cra5_api pack= and
decode_to_nc): every code against the plain numpy float64 definition of tests/pack_helpers.py, bit for bit."""
import numpy as np
import pytest
import torch

import coarsen_helpers as ch
import pack_helpers as ph
from cra5_amd import ops, pack, synth
from cra5_amd._lib import lib
from cra5_amd.api import cra5_api
from cra5_amd.vaeformer import VAEformer

pytestmark = pytest.mark.gpu

H, W = 721, 1440
SHAPES = [(3, 7, 13), (1, 1, 1), (2, 70, 1440), (5, 25, 40)]
NF = len(ops.PACK_FIELDS)


def _same_values(a, b):
    """== as values: NaN equals NaN, the sign of a zero may differ."""
    return np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True)


def _run(x, fixed, dev, off_src=0, off_dst=0):
    """Range + pack of the host frame x through views `off_src` floats / `off_dst` int16 past aligned buffers, guard
    words round the codes and the table -> (q, table) on the host."""
    C, n = x.shape[0], x.size
    sbuf = torch.full((n + 8,), -3.0, device=dev)
    sbuf[off_src:off_src + n].copy_(torch.from_numpy(x).reshape(-1))
    xs = sbuf[off_src:off_src + n].view(x.shape)
    qbuf = torch.full((n + 24,), 0x5a5a, device=dev, dtype=torch.int16)
    lo = 8 + off_dst
    q = qbuf[lo:lo + n].view(x.shape)
    tbuf = torch.full((C * NF + 8,), -7.0, device=dev, dtype=torch.float64)
    table = tbuf[4:4 + C * NF].view(C, NF)
    assert sbuf.data_ptr() % 16 == 0 and qbuf.data_ptr() % 16 == 0
    assert xs.data_ptr() % 16 == 4 * off_src and q.data_ptr() % 16 == 2 * off_dst
    fx = None if fixed is None else torch.from_numpy(fixed).to(dev)
    assert ops.pack_range(xs, fx, out=table) is table
    assert ops.pack_i16(xs, table, out=q) is q
    assert (qbuf[:lo] == 0x5a5a).all() and (qbuf[lo + n:] == 0x5a5a).all()          # nothing written round the codes
    assert (tbuf[:4] == -7.0).all() and (tbuf[4 + C * NF:] == -7.0).all()            # ... nor round the table
    assert (sbuf[:off_src] == -3.0).all() and (sbuf[off_src + n:] == -3.0).all()
    return q.cpu().numpy(), table.cpu().numpy()


def _assert_matches(got, ref, fixed, what):
    q, table = got
    rq, scale, offset, vmin, vmax, nonfinite, saturated = ref
    assert np.array_equal(q, rq), (what, int((q != rq).sum()))
    st = pack.frame_stats(table, fixed)
    assert _same_values(st["vmin"], vmin) and _same_values(st["vmax"], vmax), what
    assert st["vmin"].dtype == np.float32 and _same_values(table[:, 0], vmin)          # exact fp32 values
    assert _same_values(st["scale_factor"], scale) and _same_values(st["add_offset"], offset), what
    assert np.array_equal(st["nonfinite"], nonfinite) and np.array_equal(st["saturated"], saturated), what


@pytest.mark.parametrize("shape", SHAPES)
def test_kernels_equal_the_definition_on_every_input(dev, shape):
    """(3, 7, 13): odd planes, every plane at another phase, less than one block's span; (2, 70, 1440): several bands per
    channel - the reduction across bands runs; and the two in between."""
    inputs = ph.pack_inputs(shape)
    assert len(inputs) >= 12
    for name, (x, fixed) in inputs.items():
        ref = ph.ref_pack(x, fixed)
        got = _run(x, fixed, dev)
        _assert_matches(got, ref, fixed, (shape, name))
        again = _run(x, fixed, dev)
        assert got[0].tobytes() == again[0].tobytes() and got[1].tobytes() == again[1].tobytes(), (shape, name)
    assert shape[1] * shape[2] <= 24576 or lib().cra5_pack_range_slab_bytes(shape[0], shape[1] * shape[2]) > 16 * shape[0]


@pytest.mark.parametrize("offs", [(1, 3), (3, 1), (1, 1), (2, 2)])
def test_misaligned_views_and_guard_words(dev, offs):
    for shape in SHAPES:
        inputs = ph.pack_inputs(shape)
        for name in ("physical", "sprinkled", "ties_recip", "outside_fixed"):
            x, fixed = inputs[name]
            _assert_matches(_run(x, fixed, dev, *offs), ph.ref_pack(x, fixed), fixed, (shape, name, offs))


def test_pack_frame_and_unpack_bound(dev):
    x, fixed = ph.pack_inputs((5, 25, 40))["outside_fixed"]
    res = pack.pack_frame(torch.from_numpy(x).to(dev)[None], fixed)
    ref = ph.ref_pack(x, fixed)
    assert res["q"].dtype == torch.int16 and res["q"].is_cuda and tuple(res["q"].shape) == x.shape
    assert np.array_equal(res["q"].cpu().numpy(), ref[0]) and np.array_equal(res["saturated"], ref[6]) and res["saturated"].any()
    assert set(res) == {"q", "scale_factor", "add_offset", "vmin", "vmax", "nonfinite", "saturated", "fill_value"}
    back = pack.unpack(res["q"], res["scale_factor"], res["add_offset"])
    c = 1                                              # the per-frame channel of the table: every point inside its range
    err = np.abs(back[c] - x[c].astype(np.float64)).max()
    assert err <= ph.bound(res["scale_factor"][c], float(res["vmin"][c]), float(res["vmax"][c]))
    with pytest.raises(ValueError, match="lo < hi"):
        pack.pack_frame(torch.from_numpy(x).to(dev), np.tile([1.0, 1.0], (5, 1)))


def test_ops_argument_checks(dev):
    x = torch.randn(3, 7, 13, device=dev)
    table = ops.pack_range(x)
    assert tuple(table.shape) == (3, NF) and table.dtype == torch.float64 and ops.PACK_FIELDS[3:] == ("scale", "offset")
    for fn, args in ((ops.pack_range, ()), (ops.pack_i16, (table,))):
        name = fn.__name__
        with pytest.raises(TypeError, match=name):
            fn(x.cpu(), *args)
        with pytest.raises(TypeError, match=name):
            fn(x.double(), *args)
        with pytest.raises(TypeError, match=name):
            fn(x.transpose(1, 2), *args)
        with pytest.raises(ValueError, match=name):
            fn(x[0], *args)
    with pytest.raises(ValueError, match="pack_range: fixed"):
        ops.pack_range(x, torch.zeros(2, 2, device=dev, dtype=torch.float64))
    with pytest.raises(TypeError, match="pack_range: fixed"):
        ops.pack_range(x, torch.zeros(3, 2, device=dev))
    with pytest.raises(ValueError, match="pack_range: out"):
        ops.pack_range(x, out=torch.zeros(3, 6, device=dev, dtype=torch.float64))
    with pytest.raises(ValueError, match="pack_i16: table"):
        ops.pack_i16(x, table[:2].contiguous())
    with pytest.raises(TypeError, match="pack_i16: table"):
        ops.pack_i16(x, table.float())
    with pytest.raises(ValueError, match="pack_i16: out"):
        ops.pack_i16(x, table, out=torch.zeros(3, 13, 7, device=dev, dtype=torch.int16))
    with pytest.raises(TypeError, match="pack_i16: out"):
        ops.pack_i16(x, table, out=torch.zeros(3, 7, 13, device=dev, dtype=torch.int32))
    # the launchers' own checks (CRA5_ERR_ARG = -7), before any device work
    L, p = lib(), x.data_ptr()
    assert L.cra5_pack_range_slab_bytes(0, 5) == 0 and L.cra5_pack_range_slab_bytes(1, 0) == 0
    assert L.cra5_pack_range_slab_bytes(1, 1 << 31) == 0 and L.cra5_pack_range_slab_bytes(3, 91) == 3 * 16
    slab = torch.empty(16, device=dev, dtype=torch.float64)
    q = torch.empty(3, 7, 13, device=dev, dtype=torch.int16)
    for C, plane, xs, sl, nb, o in ((0, 91, p, slab.data_ptr(), 128, table.data_ptr()), (3, 0, p, slab.data_ptr(), 128, table.data_ptr()),
                                    (3, 1 << 31, p, slab.data_ptr(), 1 << 40, table.data_ptr()), (3, 91, None, slab.data_ptr(), 128, table.data_ptr()),
                                    (3, 91, p, None, 128, table.data_ptr()), (3, 91, p, slab.data_ptr(), 128, None),
                                    (3, 91, p, slab.data_ptr(), 47, table.data_ptr())):
        assert L.cra5_pack_range_f32(xs, C, plane, None, sl, nb, o, None) == -7, (C, plane, nb)
    for C, plane, xs, t, qq in ((0, 91, p, table.data_ptr(), q.data_ptr()), (3, 0, p, table.data_ptr(), q.data_ptr()),
                                (3, 1 << 31, p, table.data_ptr(), q.data_ptr()), (3, 91, None, table.data_ptr(), q.data_ptr()),
                                (3, 91, p, None, q.data_ptr()), (3, 91, p, table.data_ptr(), None)):
        assert L.cra5_pack_i16_f32(xs, C, plane, t, qq, None) == -7, (C, plane)


# ---- the API on the thin model -----------------------------------------------------------------------------------------


def _api(net, dev, root):
    api = cra5_api(local_root=str(root), device="cuda", weights=net)
    api._mean_flat = torch.linspace(-1, 1, 8, device=dev)
    api._std_flat = torch.linspace(0.5, 2, 8, device=dev)
    api.mean, api.std = api._mean_flat.view(8, 1, 1), api._std_flat.view(8, 1, 1)
    return api


@pytest.fixture(scope="module")
def files(dev, tmp_path_factory):
    """Three synthetic 8-channel frames encoded once (the first with a residual sidecar), their plain full decodes and the
    definition's packing of those."""
    root = tmp_path_factory.mktemp("pack")
    net = VAEformer(0, **synth.thin_model_kwargs())
    synth.load_synthetic(net, seed=7)
    api = _api(net.to(dev), dev, root)
    frames = [(synth.synth_frame(8, seed=s) * api.std.cpu() + api.mean.cpu()).numpy() for s in (3, 4, 5)]
    stamps = [f"2024-06-01T{6 * h:02d}:00:00" for h in range(3)]
    api.encode_era5_batch(stamps, data=frames, save_root=str(root / "CRA5"), workers=2)
    fulls = [api.decode_from_bin(ts, to_host=True)["x_hat"].reshape(8, H, W) for ts in stamps]
    return api, stamps, frames, fulls, [ph.ref_pack(f) for f in fulls]


STAT_KEYS = {"scale_factor", "add_offset", "fill_value", "vmin", "vmax", "nonfinite", "saturated"}


def _assert_item(item, q, ref, what=None):
    rq, scale, offset, vmin, vmax, nonfinite, saturated = ref
    assert q.dtype == np.int16 and np.array_equal(q, rq), what
    assert _same_values(item["scale_factor"], scale) and _same_values(item["add_offset"], offset), what
    assert item["scale_factor"].dtype == item["add_offset"].dtype == np.float64 and item["fill_value"] == -32768
    assert item["vmin"].dtype == np.float32 and _same_values(item["vmin"], vmin) and _same_values(item["vmax"], vmax)
    assert item["nonfinite"].dtype == np.int64 and np.array_equal(item["nonfinite"], nonfinite)
    assert item["saturated"].dtype == bool and np.array_equal(item["saturated"], saturated)


def test_api_decode_from_bin_pack(files):
    api, stamps, _, fulls, refs = files
    d = api.decode_from_bin(stamps[0], pack="int16", to_host=True)
    assert set(d) == {"x_hat", "decoding_time"} | STAT_KEYS and isinstance(d["x_hat"], np.ndarray)
    _assert_item(d, d["x_hat"], refs[0])
    dd = api.decode_from_bin(stamps[0], pack=True)              # on the device by default
    assert isinstance(dd["x_hat"], torch.Tensor) and dd["x_hat"].is_cuda and dd["x_hat"].dtype == torch.int16
    assert np.array_equal(dd["x_hat"].cpu().numpy(), refs[0][0])
    out = np.empty((8, H, W), dtype=np.int16)
    assert api.decode_from_bin(stamps[0], pack="int16", out=out)["x_hat"] is out and np.array_equal(out, refs[0][0])
    # subsets: the packing of the respective plain subset decode
    names = ["z_850", "z_1000", "z_925"]
    for kw in (dict(variables=names, region=(35, 72, -25, 45)), dict(stride=6), dict(coarsen=6)):
        plain = api.decode_from_bin(stamps[1], to_host=True, **kw)
        got = api.decode_from_bin(stamps[1], pack="int16", to_host=True, **kw)
        sub = plain["x_hat"].reshape(plain["x_hat"].shape[-3:])
        assert got["x_hat"].shape == sub.shape and got["variables"] == plain["variables"]
        _assert_item(got, got["x_hat"], ph.ref_pack(sub), kw)
    assert got["coarsen"] == (6, 6) and np.array_equal(got["x_hat"], ph.ref_pack(ch.ref_coarsen(fulls[1], (6, 6)))[0])
    # a fixed range: the region's codes are the slice of the globe's; per frame they are not
    fixed = {"z": (-3.0, 2.5)}                                 # (the thin model's eight channels are levels of z)
    g = cra5_api.grid_box((35, 72, -25, 45))
    r0, r1, c0, nc = g["box"]
    cols = (c0 + np.arange(nc)) % W
    chans = [api.vname_to_channels[v] for v in names]
    globe = api.decode_from_bin(stamps[1], pack=fixed, to_host=True)
    part = api.decode_from_bin(stamps[1], pack=fixed, to_host=True, variables=names, region=(35, 72, -25, 45))
    assert np.array_equal(part["x_hat"], globe["x_hat"][chans, r0:r1][:, :, cols])
    assert np.array_equal(part["scale_factor"], globe["scale_factor"][chans]) and globe["saturated"].any()
    fx = pack.resolve_ranges(fixed, [api.channels_to_vname[c] for c in range(8)])
    _assert_item(globe, globe["x_hat"], ph.ref_pack(fulls[1], fx))
    per_frame = api.decode_from_bin(stamps[1], pack="int16", to_host=True, variables=names, region=(35, 72, -25, 45))
    assert not np.array_equal(per_frame["x_hat"], refs[1][0][chans, r0:r1][:, :, cols])
    # errors
    for fmt in ("normalized", "latent"):
        with pytest.raises(ValueError, match="pack"):
            api.decode_from_bin(stamps[0], pack="int16", return_format=fmt)
    with pytest.raises(ValueError, match="int16"):
        api.decode_from_bin(stamps[0], pack="int16", out=np.empty((8, H, W), dtype=np.float32))
    with pytest.raises(ValueError, match="unknown variable"):
        api.decode_from_bin(stamps[0], pack={"sst": (0, 1)})


def test_api_decode_batch_pack(files):
    api, stamps, _, _, refs = files
    out = np.empty((3, 8, H, W), dtype=np.int16)
    items = api.decode_batch(stamps, out=out, workers=4, pack="int16")
    seen = {}

    def sink(i, item):
        assert set(item) == {"q"} | STAT_KEYS and item["q"].shape == (8, H, W) and item["q"].dtype == np.int16
        seen[i] = dict(item, q=item["q"].copy())
        return i
    assert api.decode_batch(stamps, workers=1, pack="int16", sink=sink) == [0, 1, 2]
    fresh1 = api.decode_batch(stamps, workers=1, pack=True)
    fresh4 = api.decode_batch(stamps, workers=4, pack="int16")
    for i in range(3):
        assert items[i]["q"].base is out or np.shares_memory(items[i]["q"], out[i])
        _assert_item(items[i], out[i], refs[i])
        for it in (seen[i], fresh1[i], fresh4[i]):
            _assert_item(it, it["q"], refs[i])
    for bad in (np.empty((3, 8, H, W), dtype=np.float32), np.empty((3, 8, 121, 240), dtype=np.int16)):
        with pytest.raises(ValueError, match="out"):
            api.decode_batch(stamps, out=bad, pack="int16")
    with pytest.raises(ValueError, match="out"):            # ... and the unpacked call still wants float32
        api.decode_batch(stamps, out=out)
    for fmt in ("normalized", "latent"):
        with pytest.raises(ValueError):
            api.decode_batch(stamps, pack="int16", return_format=fmt)
    with pytest.raises(ValueError, match="pack must be"):
        api.decode_batch(stamps, pack="int8")


def test_api_residual_then_pack(files, tmp_path):
    api, stamps, frames, fulls, _ = files
    corr = (1, 5)                                              # two channels corrected to twice their rmse
    rmse = [float(np.sqrt(np.mean((fulls[2][c].astype(np.float64) - frames[2][c]) ** 2))) for c in corr]
    enc = api.encode_era5_as_bin(stamps[2], save_root=str(tmp_path), data=frames[2],
                                 max_error={api.channels_to_vname[c]: 2.0 * r for c, r in zip(corr, rmse)})
    assert enc["residual"]["records"] > 0
    corrected = api.decode_from_bin(custom_path=enc["save_path"], residual=True, to_host=True)["x_hat"].reshape(8, H, W)
    ref = ph.ref_pack(corrected)
    got = api.decode_from_bin(custom_path=enc["save_path"], residual=True, pack="int16", to_host=True)
    _assert_item(got, got["x_hat"], ref)
    item = api.decode_batch(paths=[enc["save_path"]], residual=True, pack="int16", workers=1)[0]
    _assert_item(item, item["q"], ref)
    # the truth is within the sidecar's tolerance plus the packing bound of the unpacked codes
    tol = enc["residual"]["tol"].astype(np.float64)
    back = pack.unpack(item["q"], item["scale_factor"], item["add_offset"])
    bound = tol + np.array([ph.bound(item["scale_factor"][c], float(item["vmin"][c]), float(item["vmax"][c])) for c in range(8)])
    # (fp32 rounding of the corrected value itself: half an ulp of the largest magnitude)
    slack = np.abs(corrected).reshape(8, -1).max(1) * 2.0 ** -23
    worst = np.abs(back - frames[2].astype(np.float64)).reshape(8, -1).max(1)
    assert (worst[list(corr)] <= (bound + slack)[list(corr)]).all(), (worst, bound)
    assert not np.array_equal(corrected, fulls[2])


def test_api_decode_to_nc(files, tmp_path):
    from scipy.io import netcdf_file
    api, stamps, _, fulls, _ = files
    names = ["z_850", "z_1000", "z_925"]
    region = (35, 72, -25, 45)
    res = api.decode_to_nc(stamps[:2], save_root=str(tmp_path), variables=names, region=region, workers=2)
    g = cra5_api.grid_box(region)
    r0, r1, c0, nc = g["box"]
    cols = (c0 + np.arange(nc)) % W
    chans = [api.vname_to_channels[v] for v in names]
    for i, r in enumerate(res):
        path = f"{tmp_path}/ERA5/2024/{stamps[i]}_pressure.nc"
        assert r["time_stamp"] == stamps[i] and r["files"] == [path] and r["bytes"] > 3 * (r1 - r0) * nc * 2
        sub = np.ascontiguousarray(fulls[i][chans, r0:r1][:, :, cols])
        shared = np.tile([float(sub.min()), float(sub.max())], (3, 1))
        rq, scale, offset, *_ = ph.ref_pack(sub, shared)
        f = netcdf_file(path, "r", mmap=False, maskandscale=False)
        z = f.variables["z"]
        assert z.dimensions == ("time", "level", "latitude", "longitude") and z.shape == (1, 3, r1 - r0, nc)
        assert np.asarray(z.scale_factor).shape == () and float(z.scale_factor) == scale[0] and float(z.add_offset) == offset[0]
        assert np.array_equal(z[:][0], rq)
        unpacked = z[:][0].astype(np.float64) * float(z.scale_factor) + float(z.add_offset)
        assert np.array_equal(unpacked, ph.unpack(rq, scale, offset))
        assert f.variables["level"][:].tolist() == [850.0, 1000.0, 925.0]
        assert np.array_equal(f.variables["latitude"][:], g["lat"].astype(np.float32))
        assert np.array_equal(f.variables["longitude"][:], g["lon"].astype(np.float32))
        assert f.variables["time"][:].tolist() == [pack.hours_since_1900(stamps[i])]
        f.close()
        f = netcdf_file(path, "r", mmap=False, maskandscale=True)
        assert np.array_equal(np.ma.filled(f.variables["z"][:], np.nan)[0], ph.unpack(rq, scale, offset))
        f.close()
    assert sorted(p.name for p in (tmp_path / "ERA5" / "2024").iterdir()) == [f"{ts}_pressure.nc" for ts in stamps[:2]]
    with pytest.raises(ValueError, match="variable name"):
        api.decode_to_nc(stamps[:1], save_root=str(tmp_path), variables=names, pack={"z_850": (0, 1)})
    with pytest.raises(ValueError, match="time_stamps"):
        api.decode_to_nc(paths=["x.bin"], save_root=str(tmp_path))
