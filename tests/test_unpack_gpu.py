"""Packed int16 input on the GPU (cra5_unpack_i16_f32, ops.unpack_i16, PackedFrame through the cra5_api encode entry points and
ingest=): every value against the numpy definition of tests/unpack_helpers.py bit for bit, every .bin byte for byte."""
import os

import numpy as np
import pytest
import torch

import pack_helpers as ph
import unpack_helpers as uh
from cra5_amd import ops, pack, synth
from cra5_amd._lib import lib
from cra5_amd.api import cra5_api
from cra5_amd.vaeformer import VAEformer

pytestmark = pytest.mark.gpu

H, W = 721, 1440
NF = len(ops.UNPACK_FIELDS)
GUARD = -7.0


def _run(q, table, dev, swapped=False, off_src=0, off_dst=0):
    """ops.unpack_i16 of the codes q (values) through views `off_src` codes / `off_dst` floats past 16-byte aligned
    buffers, guard words round x -> x on the host.  swapped: the device sees every code's two bytes exchanged."""
    C, n = q.shape[0], q.size
    raw = q.byteswap() if swapped else q
    qbuf = torch.full((n + 16,), 0x5a5a, device=dev, dtype=torch.int16)
    qbuf[off_src:off_src + n].copy_(torch.from_numpy(np.ascontiguousarray(raw)).reshape(-1))
    qs = qbuf[off_src:off_src + n].view(q.shape)
    xbuf = torch.full((n + 24,), GUARD, device=dev)
    lo = 8 + off_dst
    x = xbuf[lo:lo + n].view(q.shape)
    tbuf = torch.full((C * NF + 8,), GUARD, device=dev, dtype=torch.float64)
    tbuf[4:4 + C * NF].copy_(torch.from_numpy(table).reshape(-1))
    t = tbuf[4:4 + C * NF].view(C, NF)
    assert qbuf.data_ptr() % 16 == 0 and xbuf.data_ptr() % 16 == 0
    assert qs.data_ptr() % 16 == (2 * off_src) % 16 and x.data_ptr() % 16 == 4 * off_dst
    q_before, t_before = qbuf.clone(), tbuf.clone()
    assert ops.unpack_i16(qs, t, swapped=swapped, out=x) is x
    assert (xbuf[:lo] == GUARD).all() and (xbuf[lo + n:] == GUARD).all()            # nothing written round x
    assert torch.equal(qbuf, q_before)                                                # the codes are only read
    assert torch.equal(tbuf.view(torch.int64), t_before.view(torch.int64))            # ... and the table (NaN fill included)
    return x.cpu().numpy()


def _plane_shapes(shape):
    """The cases of one shape: every named input on it; fma_ties at its own channel count on the first and last planes."""
    inputs = uh.unpack_inputs(shape)
    if shape not in (uh.SHAPES[0], uh.SHAPES[-1]):
        del inputs["fma_ties"]
    return inputs


@pytest.mark.parametrize("shape", uh.SHAPES + [uh.FULL_SHAPE])
def test_kernel_equals_the_definition_on_every_input(dev, shape):
    """(3, 7, 13): odd planes, every plane at another phase; (2, 35, 1440): several chunks per plane; FULL_SHAPE: every
    code value in every channel."""
    inputs = _plane_shapes(shape)
    assert set(inputs) >= {"random", "tp_like", "no_fill"}
    for name, (q, table) in inputs.items():
        ref = uh.bits(uh.ref_unpack(q, table))
        for swapped in (False, True):
            got = _run(q, table, dev, swapped)
            bad = uh.bits(got) != ref
            assert not bad.any(), (shape, name, swapped, int(bad.sum()), got[bad][:4], ref[bad][:4])
            again = _run(q, table, dev, swapped)
            assert got.tobytes() == again.tobytes(), (shape, name, swapped)
    if shape == uh.SHAPES[-1]:
        assert shape[1] * shape[2] // 4 > 3 * 4096          # (a chunk is 4096 groups of four values: four chunks per plane)


@pytest.mark.parametrize("off_src", [1, 3, 5, 7])
def test_misaligned_views_and_guard_words(dev, off_src):
    for shape in uh.SHAPES:
        inputs = _plane_shapes(shape)
        for off_dst in (1, 2, 3):
            for name, (q, table) in inputs.items():
                swapped = (off_src + off_dst) % 2 == 0
                got = _run(q, table, dev, swapped, off_src, off_dst)
                assert np.array_equal(uh.bits(got), uh.bits(uh.ref_unpack(q, table))), (shape, name, off_src, off_dst)


def test_ops_argument_checks(dev):
    q = torch.zeros(3, 7, 13, device=dev, dtype=torch.int16)
    table = torch.zeros(3, NF, device=dev, dtype=torch.float64)
    assert ops.UNPACK_FIELDS == ("scale", "offset", "fill", "mul")
    x = ops.unpack_i16(q, table)
    assert x.dtype == torch.float32 and x.shape == q.shape and x.is_cuda
    for bad in (q.cpu(), q.int(), q.float(), q.transpose(1, 2), q.cpu().numpy()):
        with pytest.raises(TypeError, match="unpack_i16"):
            ops.unpack_i16(bad, table)
    for bad in (q[0], q[:, :0]):
        with pytest.raises(ValueError, match="unpack_i16"):
            ops.unpack_i16(bad.contiguous(), table)
    with pytest.raises(ValueError, match="unpack_i16: table"):
        ops.unpack_i16(q, table[:2].contiguous())
    with pytest.raises(ValueError, match="unpack_i16: table"):
        ops.unpack_i16(q, torch.zeros(3, 5, device=dev, dtype=torch.float64))
    with pytest.raises(TypeError, match="unpack_i16: table"):
        ops.unpack_i16(q, table.float())
    with pytest.raises(TypeError, match="unpack_i16: table"):
        ops.unpack_i16(q, table.cpu())
    with pytest.raises(ValueError, match="unpack_i16: out"):
        ops.unpack_i16(q, table, out=torch.zeros(3, 13, 7, device=dev))
    with pytest.raises(TypeError, match="unpack_i16: out"):
        ops.unpack_i16(q, table, out=torch.zeros(3, 7, 13, device=dev, dtype=torch.float64))
    with pytest.raises(TypeError, match="unpack_i16: out"):
        ops.unpack_i16(q, table, out=torch.zeros(3, 7, 13))
    # the launcher's own checks (CRA5_ERR_ARG = -7), before any device work
    L, qp, tp, xp = lib(), q.data_ptr(), table.data_ptr(), x.data_ptr()
    for args in ((None, 3, 91, tp, 0, xp), (qp, 3, 91, None, 0, xp), (qp, 3, 91, tp, 0, None), (qp, 0, 91, tp, 0, xp),
                 (qp, 3, 0, tp, 0, xp), (qp, 3, 1 << 31, tp, 0, xp), (qp, 3, 91, tp, 2, xp), (qp + 1, 3, 91, tp, 0, xp),
                 (qp, 3, 91, tp + 4, 0, xp), (qp, 3, 91, tp, 0, xp + 2)):
        assert L.cra5_unpack_i16_f32(*args, None) == -7, args


def test_inverse_of_the_output_path(dev):
    """pack_range + pack_i16, then unpack_i16 with FILL = -32768: fl32 of pack.unpack of the codes, NaN exactly where x was
    not finite."""
    for shape in ((5, 25, 40), (2, 35, 1440)):
        for name in ("physical", "sprinkled", "extremes", "outside_fixed"):
            x, fixed = ph.pack_inputs(shape)[name]
            xd = torch.from_numpy(x).to(dev)
            t5 = ops.pack_range(xd, None if fixed is None else torch.from_numpy(fixed).to(dev))
            q = ops.pack_i16(xd, t5)
            t4 = torch.stack([t5[:, 3], t5[:, 4], torch.full_like(t5[:, 0], -32768.0), torch.ones_like(t5[:, 0])], 1).contiguous()
            got = ops.unpack_i16(q, t4).cpu().numpy()
            st = pack.frame_stats(t5.cpu().numpy())
            with np.errstate(over="ignore"):
                want = pack.unpack(q, st["scale_factor"], st["add_offset"]).astype(np.float32)
            assert np.array_equal(uh.bits(got), uh.bits(want)), (shape, name)
            assert np.array_equal(np.isnan(got), ~ph.finite_mask(x)), (shape, name)
            f = pack.PackedFrame(q.cpu().numpy(), st["scale_factor"], st["add_offset"])
            assert np.array_equal(uh.bits(pack.unpack_f32(f)), uh.bits(got))


# ---- the API on the thin model -----------------------------------------------------------------------------------------


def _api(net, dev, root):
    api = cra5_api(local_root=str(root), device="cuda", weights=net)
    api._mean_flat = torch.linspace(-1, 1, 8, device=dev)
    api._std_flat = torch.linspace(0.5, 2, 8, device=dev)
    api.mean, api.std = api._mean_flat.view(8, 1, 1), api._std_flat.view(8, 1, 1)
    return api


TS = "2024-06-01T06:00:00"


@pytest.fixture(scope="module")
def packed(dev, tmp_path_factory):
    """One synthetic 8-channel frame encoded and decoded packed: pf is that decode as a PackedFrame, xf its host unpacking,
    ref the .bin of xf through the float32 route."""
    root = tmp_path_factory.mktemp("unpack")
    net = VAEformer(0, **synth.thin_model_kwargs())
    synth.load_synthetic(net, seed=7)
    api = _api(net.to(dev), dev, root)
    frame = (synth.synth_frame(8, seed=3) * api.std.cpu() + api.mean.cpu()).numpy()
    api.encode_era5_batch([TS], data=[frame], save_root=str(root / "CRA5"), workers=1)
    pf = pack.PackedFrame.from_decode(api.decode_from_bin(TS, pack="int16", to_host=True))
    xf = pack.unpack_f32(pf)
    assert pf.shape == (8, H, W) and np.isfinite(xf).all()
    enc = api.encode_era5_batch([TS], data=[xf], save_root=str(root / "f32"), workers=1)[0]
    return api, root, pf, xf, open(enc["save_path"], "rb").read()


def _bin(enc):
    return open(enc["save_path"], "rb").read()


def test_api_encode_is_byte_identical(packed):
    api, root, pf, xf, ref = packed
    assert len(ref) > 1000
    assert _bin(api.encode_era5_batch([TS], data=[pf], save_root=str(root / "i16"), workers=1)[0]) == ref
    assert _bin(api.encode_era5_batch([TS, TS], data=[pf, xf], save_root=str(root / "i16b"), workers=2)[0]) == ref
    assert _bin(api.encode_era5_as_bin(TS, save_root=str(root / "i16c"), data=pf)) == ref
    big = pf.byteswapped()
    assert big.swapped != pf.swapped and big.blocks[0].tobytes() != pf.blocks[0].tobytes()
    assert _bin(api.encode_era5_as_bin(TS, save_root=str(root / "i16d"), data=big)) == ref
    assert _bin(api.encode_era5_batch([TS], data=[big], save_root=str(root / "i16e"), workers=1)[0]) == ref
    # the same frame as blocks
    blocks = pack.PackedFrame([pf.blocks[0][:3].copy(), pf.blocks[0][3:4].copy(), pf.blocks[0][4:].copy()], pf.scale_factor,
                              pf.add_offset, pf.fill, pf.multiplier)
    assert _bin(api.encode_era5_as_bin(TS, save_root=str(root / "i16f"), data=blocks)) == ref
    y = api.encode_to_latent(TS, data=pf).clone()
    assert torch.equal(y, api.encode_to_latent(TS, data=xf))


def test_api_staged_frame_is_the_definition(packed):
    api, _, pf, xf, _ = packed
    x = api._stage_packed(pf)
    torch.cuda.synchronize()
    assert x.dtype == torch.float32 and tuple(x.shape) == (8, H, W)
    assert np.array_equal(uh.bits(x.cpu().numpy()), uh.bits(xf))


def test_api_roundtrip_and_evaluate_are_identical(packed):
    api, root, pf, xf, ref = packed
    a = api.roundtrip_batch([TS], data=[pf], save_root=str(root / "rt_i16"), workers=1)
    b = api.roundtrip_batch([TS], data=[xf], save_root=str(root / "rt_f32"), workers=1)
    assert _bin(a[0][0]) == _bin(b[0][0]) == ref and a[0][1].tobytes() == b[0][1].tobytes()
    ra = api.evaluate_batch([TS], data=[pf], workers=1, quantiles=(0.5, 0.99))[0]
    rb = api.evaluate_batch([TS], data=[xf], workers=1, quantiles=(0.5, 0.99))[0]
    assert set(ra) == set(rb) and "rmse" in ra
    for k in ra:
        if isinstance(ra[k], np.ndarray):
            assert ra[k].dtype == rb[k].dtype and ra[k].tobytes() == rb[k].tobytes(), k
        else:
            assert ra[k] == rb[k], k
    # an existing .bin against a packed truth
    path = str(root / "f32" / "2024" / f"{TS}.bin")
    rc = api.evaluate_batch([TS], data=[pf], bins=[path], workers=1)[0]
    rd = api.evaluate_batch([TS], data=[xf], bins=[path], workers=1)[0]
    assert rc["rmse"].tobytes() == rd["rmse"].tobytes() and rc["bias"].tobytes() == rd["bias"].tobytes()


def test_api_fill_code_is_a_non_finite_input(packed):
    api, root, pf, _, _ = packed
    q = pf.blocks[0].copy()
    q[5, 360, 700] = -32768
    bad = pack.PackedFrame(q, pf.scale_factor, pf.add_offset)
    with pytest.raises(ValueError, match="NaN / inf"):
        api.encode_era5_as_bin(TS, save_root=str(root / "bad"), data=bad)
    with pytest.raises(ValueError, match="NaN / inf"):
        api.encode_era5_batch([TS], data=[bad], save_root=str(root / "bad"), workers=1)
    # without a fill code the same codes are numbers
    fine = pack.PackedFrame(q, pf.scale_factor, pf.add_offset, None)
    assert len(_bin(api.encode_era5_as_bin(TS, save_root=str(root / "fine"), data=fine))) > 1000


def test_api_residual_sidecar_is_byte_identical(packed):
    api, root, pf, xf, ref = packed
    a = api.encode_era5_batch([TS], data=[pf], save_root=str(root / "res_i16"), workers=1, max_error=0.05, max_fraction=1.0)[0]
    b = api.encode_era5_batch([TS], data=[xf], save_root=str(root / "res_f32"), workers=1, max_error=0.05, max_fraction=1.0)[0]
    assert _bin(a) == _bin(b) == ref
    ra, rb = open(a["residual"]["path"], "rb").read(), open(b["residual"]["path"], "rb").read()
    assert a["residual"]["records"] > 0 and len(ra) > 100 and ra == rb
    c = api.encode_era5_as_bin(TS, save_root=str(root / "res_i16b"), data=pf, max_error=0.05, max_fraction=1.0)
    assert open(c["residual"]["path"], "rb").read() == rb


def _write_float_pressure(path, levels, lat, lon, values):
    from scipy.io import netcdf_file
    f = netcdf_file(path, "w", version=2)
    for name, n in (("time", 1), ("level", len(levels)), ("latitude", len(lat)), ("longitude", len(lon))):
        f.createDimension(name, n)
    v = f.createVariable("level", "f4", ("level",))
    v[:] = np.asarray(levels, dtype=np.float32)
    v = f.createVariable("z", "f4", ("time", "level", "latitude", "longitude"))
    v[:] = values[None]
    f.close()


def test_api_ingest_from_files(packed, dev):
    """The thin model's eight channels are the first eight levels of z: decode_to_nc writes them, and the encode reads them
    back packed, on the host, or whichever fits."""
    from scipy.io import netcdf_file
    shared, root, pf, xf, _ = packed
    api = _api(shared.net, dev, root / "nc")
    api.vnames = dict(pressure=["z"], single=[])
    api.pressure_level = list(api.pressure_level[:8])
    assert [api.channels_to_vname[c] for c in range(8)] == [f"z_{int(v)}" for v in api.pressure_level]
    bin_path = str(root / "CRA5" / "2024" / f"{TS}.bin")
    stamps = [TS, "2024-06-01T12:00:00"]
    files = api.decode_to_nc(stamps, paths=[bin_path, bin_path], workers=2)
    folder = f"{api.local_root}/ERA5/2024"
    assert files[0]["files"] == [f"{folder}/{TS}_pressure.nc"]
    for ts in stamps + ["2024-06-02T00:00:00"]:           # (the host reader opens the single-level file too)
        f = netcdf_file(f"{folder}/{ts}_single.nc", "w", version=2)
        f.createDimension("time", 1)
        f.close()
    host = api.encode_era5_batch(stamps, save_root=str(root / "nc_host"), workers=2)
    assert [_bin(e) for e in host] == [_bin(e) for e in api.encode_era5_batch(stamps, save_root=str(root / "nc_def"),
                                                                            workers=2, ingest="host")]
    got = api.encode_era5_batch(stamps, save_root=str(root / "nc_packed"), workers=2, ingest="packed")
    assert [_bin(e) for e in got] == [_bin(e) for e in host] and len(_bin(host[0])) > 1000
    assert _bin(api.encode_era5_as_bin(TS, save_root=str(root / "nc_packed1"), ingest="packed")) == _bin(host[0])
    auto = api.encode_era5_batch(stamps, save_root=str(root / "nc_auto"), workers=2, ingest="auto")
    assert [_bin(e) for e in auto] == [_bin(e) for e in host]
    rp = api.evaluate_batch(stamps[:1], workers=1, ingest="packed")[0]
    rh = api.evaluate_batch(stamps[:1], workers=1)[0]
    assert rp["rmse"].tobytes() == rh["rmse"].tobytes()
    # a float variable: "auto" is the host route, "packed" names the file
    ts = "2024-06-02T00:00:00"
    lat, lon = np.linspace(90, -90, H), np.arange(W) * 0.25
    _write_float_pressure(f"{folder}/{ts}_pressure.nc", api.pressure_level, lat, lon, xf)
    h = api.encode_era5_batch([ts], save_root=str(root / "fl_host"), workers=1, ingest="host")[0]
    a = api.encode_era5_batch([ts], save_root=str(root / "fl_auto"), workers=1, ingest="auto")[0]
    assert _bin(a) == _bin(h)
    with pytest.raises(ValueError, match=f"{ts}_pressure.nc"):
        api.encode_era5_batch([ts], save_root=str(root / "fl_packed"), workers=1, ingest="packed")
    with pytest.raises(ValueError, match="ingest"):
        api.encode_era5_batch([ts], ingest="int16")
    assert os.path.exists(f"{folder}/{ts}_pressure.nc")
