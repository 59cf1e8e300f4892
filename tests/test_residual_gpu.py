"""Residual layer on the GPU: the quantise / apply / gather kernels against the numpy reference bit for bit, and the
error-bounded encode / decode / aggregate / evaluate of cra5_api with the thin 8-channel model."""
import os

import numpy as np
import pytest
import torch

import residual_helpers as rh
from time_stats_helpers import ref_time_stats
from cra5_amd import _lib, ops, residual, synth
from cra5_amd.api import cra5_api
from cra5_amd.residual import ResidualBudgetError, ResidualFormatError, ResidualMismatchError
from cra5_amd.subset import kept_points
from cra5_amd.vaeformer import VAEformer

pytestmark = pytest.mark.gpu

PAD = 8                              # guard words on each side of an output


def _placed(a, dev, off_words):
    """The float32 array on the device, `off_words` * 4 bytes past a 16-byte boundary."""
    buf = torch.empty(a.size + 8, device=dev, dtype=torch.float32)
    assert buf.data_ptr() % 16 == 0
    t = buf[off_words:off_words + a.size].view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.data_ptr() % 16 == (4 * off_words) % 16 and t.is_contiguous()
    return t


def _guarded(n, dtype, dev):
    """-> (whole buffer, the n-element middle): PAD guard elements on each side, every byte of the buffer 0x5A."""
    whole = torch.empty(n + 2 * PAD, device=dev, dtype=dtype)
    whole.view(torch.uint8).fill_(0x5A)
    return whole, whole[PAD:PAD + n]


def _guards_intact(whole, n):
    b = whole.view(torch.uint8).cpu().numpy().reshape(len(whole), -1)
    return bool((b[:PAD] == 0x5A).all() and (b[PAD + n:] == 0x5A).all())


def _quantize_raw(x, xh, tol, dev):
    """The three C entry points on caller-owned, guarded buffers -> (idx, q, eidx, ebits, per_channel) as numpy."""
    L = _lib.lib()
    C, H, W = x.shape
    S = L.cra5_residual_spans(C, H, W)
    assert S == C * -(-H * W // ops.RESIDUAL_SPAN)
    tol_d = torch.from_numpy(tol).to(dev)
    st = ops._stream()
    cw, counts = _guarded(2 * S, torch.int32, dev)
    ow, offs = _guarded(2 * (S + 1), torch.int32, dev)
    hw, chan = _guarded(2 * C, torch.int64, dev)
    _lib.check(L.cra5_residual_count_f32(x.data_ptr(), xh.data_ptr(), tol_d.data_ptr(), C, H, W, counts.data_ptr(), st), "count")
    _lib.check(L.cra5_residual_scan(counts.data_ptr(), C, H, W, offs.data_ptr(), chan.data_ptr(), st), "scan")
    per = chan.cpu().numpy().reshape(C, 2)
    n, m = (int(v) for v in per.sum(axis=0))
    offs_h = offs.cpu().numpy().view(np.uint32).reshape(S + 1, 2)
    cnt_h = counts.cpu().numpy().view(np.uint32).reshape(S, 2).astype(np.int64)
    assert offs_h[-1].tolist() == [n, m]
    assert np.array_equal(offs_h[:-1].astype(np.int64), np.cumsum(cnt_h, axis=0) - cnt_h)
    iw, idx = _guarded(n, torch.int32, dev)
    qw, q = _guarded(n, torch.int16, dev)
    ew, eidx = _guarded(m, torch.int32, dev)
    bw, ebits = _guarded(m, torch.int32, dev)
    _lib.check(L.cra5_residual_emit_f32(x.data_ptr(), xh.data_ptr(), tol_d.data_ptr(), C, H, W, offs.data_ptr(),
                                        idx.data_ptr() if n else None, q.data_ptr() if n else None, n,
                                        eidx.data_ptr() if m else None, ebits.data_ptr() if m else None, m, st), "emit")
    torch.cuda.synchronize()
    for whole, k in ((cw, 2 * S), (ow, 2 * (S + 1)), (hw, 2 * C), (iw, n), (qw, n), (ew, m), (bw, m)):
        assert _guards_intact(whole, k)
    return (idx.cpu().numpy().view(np.uint32), q.cpu().numpy(), eidx.cpu().numpy().view(np.uint32),
            ebits.cpu().numpy().view(np.uint32), per)


def _assert_equal(got, ref):
    for name, g, r in zip(("idx", "q", "eidx", "ebits", "per_channel"), got, ref):
        assert g.dtype == r.dtype and g.shape == r.shape and np.array_equal(g, r), name


# ---- quantise ------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("placement", [(0, 0), (1, 3)], ids=["aligned", "off4_off12"])
@pytest.mark.parametrize("tol", list(rh.TOLS))
@pytest.mark.parametrize("kind", ["offset", "zero"])
@pytest.mark.parametrize("shape", rh.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_quantize_equals_the_reference(dev, shape, kind, tol, placement):
    seed = 100 * rh.SHAPES.index(shape) + 10 * list(rh.TOLS).index(tol) + (kind == "zero")
    x, xh, t = rh.inject(*rh.field(shape, kind, rh.TOLS[tol], seed))
    ref = rh.ref_quantize(x, xh, t)
    got = _quantize_raw(_placed(x, dev, placement[0]), _placed(xh, dev, placement[1]), t, dev)
    _assert_equal(got, ref)
    assert ref[4][:, 1].sum() >= 5          # the injected escapes went through the kernel
    if shape[0] >= 3:
        assert got[4][1].tolist() == [0, 0]     # x_hat == x over a whole channel


def test_quantize_every_point_a_record_and_none_at_all(dev):
    rng = np.random.default_rng(1)
    shape = (2, 9, 1440)
    x = rng.integers(-1000, 1000, size=shape).astype(np.float32)
    t = np.array([1.0, 1.0], dtype=np.float32)
    xh = x + np.float32(4.0)
    got = _quantize_raw(_placed(x, dev, 0), _placed(xh, dev, 0), t, dev)
    _assert_equal(got, rh.ref_quantize(x, xh, t))
    assert got[4].tolist() == [[9 * 1440, 0]] * 2 and (got[1] == -2).all()
    assert np.array_equal(got[0], np.arange(x.size, dtype=np.uint32))
    # no record, no escape: n == m == 0, the emit pass launches nothing and takes NULL arrays
    got = _quantize_raw(_placed(x, dev, 1), _placed(x.copy(), dev, 1), t, dev)
    assert all(len(a) == 0 for a in got[:4]) and got[4].tolist() == [[0, 0]] * 2
    # every channel uncorrected
    inf = np.full(2, np.inf, dtype=np.float32)
    assert _quantize_raw(_placed(x, dev, 0), _placed(xh, dev, 0), inf, dev)[4].tolist() == [[0, 0]] * 2
    # every point an escape
    nan = np.full(shape, np.nan, dtype=np.float32)
    got = _quantize_raw(_placed(x, dev, 0), _placed(nan, dev, 0), t, dev)
    _assert_equal(got, rh.ref_quantize(x, nan, t))
    assert got[4].tolist() == [[0, 9 * 1440]] * 2


def test_ops_residual_quantize_and_argument_checks(dev):
    x, xh, t = rh.inject(*rh.field((5, 33, 250), "offset", 8 * rh.ULP, 9))
    xd, hd = torch.from_numpy(x).to(dev), torch.from_numpy(xh).to(dev)
    idx, q, eidx, ebits, per = ops.residual_quantize(xd, hd, t)
    assert (idx.dtype, q.dtype, eidx.dtype, ebits.dtype) == (torch.int32, torch.int16, torch.int32, torch.int32)
    got = (idx.cpu().numpy().view(np.uint32), q.cpu().numpy(), eidx.cpu().numpy().view(np.uint32),
           ebits.cpu().numpy().view(np.uint32), per)
    _assert_equal(got, rh.ref_quantize(x, xh, t))
    again = ops.residual_quantize(xd, hd, torch.from_numpy(t))
    assert all(torch.equal(a, b) for a, b in zip(again[:4], (idx, q, eidx, ebits)))
    with pytest.raises(ValueError, match="one shape"):
        ops.residual_quantize(xd, hd[:4].contiguous(), t)
    with pytest.raises(TypeError, match="x_hat must be a contiguous"):
        ops.residual_quantize(xd, hd.transpose(1, 2), t)
    with pytest.raises(TypeError, match="x must be a contiguous"):
        ops.residual_quantize(xd.double(), hd, t)
    with pytest.raises(ValueError, match=r"tol must be \[5\]"):
        ops.residual_quantize(xd, hd, t[:4])
    with pytest.raises(ValueError, match=r"tol\[2\]"):
        ops.residual_quantize(xd, hd, [1.0, 1.0, -1.0, 1.0, 1.0])
    out = hd.clone()
    step = torch.from_numpy(np.float32(2) * t).to(dev)
    with pytest.raises(ValueError, match="records must be"):
        ops.residual_apply(out, (idx, q), step, (5, 33, 250))
    with pytest.raises(TypeError, match="records.q"):
        ops.residual_apply(out, (idx, q.int(), eidx, ebits), step, (5, 33, 250))
    with pytest.raises(ValueError, match="step must be"):
        ops.residual_apply(out, (idx, q, eidx, ebits), step[:4].contiguous(), (5, 33, 250))
    with pytest.raises(ValueError, match="pass chan_lut"):
        ops.residual_apply(out[:3].contiguous(), (idx, q, eidx, ebits), step, (5, 33, 250))
    with pytest.raises(ValueError, match="keep 17 rows"):
        ops.residual_apply(out, (idx, q, eidx, ebits), step, (5, 33, 250), stride=(2, 1))
    with pytest.raises(ValueError, match="stride"):
        ops.residual_apply(out, (idx, q, eidx, ebits), step, (5, 33, 250), stride=(1, 3))
    with pytest.raises(ValueError, match="box"):
        ops.residual_apply(out, (idx, q, eidx, ebits), step, (5, 33, 250), box=(0, 34, 0, 250))
    with pytest.raises(TypeError, match="chan_lut"):
        ops.residual_apply(out, (idx, q, eidx, ebits), step, (5, 33, 250), chan_lut=torch.arange(5, device=dev))
    assert torch.equal(out.view(torch.int32), hd.view(torch.int32))      # nothing was applied (bits: x_hat holds a NaN)


# ---- apply ---------------------------------------------------------------------------------------------------------------

GRID = (5, 25, 48)
GEOMETRIES = {
    "globe": dict(),
    "across_0deg": dict(box=(5, 19, 40, 17)),
    "north_pole": dict(box=(0, 4, 10, 20)),
    "south_pole": dict(box=(20, 25, 0, 48)),
    "stride_2_3": dict(stride=(2, 3)),
    "stride_6_6": dict(stride=(6, 6)),
    "stride_in_box_across_0deg": dict(box=(3, 22, 41, 30), stride=(2, 3)),
    "channels_reordered": dict(channels=[3, 0, 2]),                     # corrected channel 1 left out, 4 is +inf
    "channels_box_stride": dict(channels=[2, 1], box=(1, 24, 44, 11), stride=(3, 2)),
    "single_point": None,                                               # a record of channel 1, chosen in the test
}


@pytest.fixture(scope="module")
def apply_case():
    x, xh, t = rh.field(GRID, "offset", 1.3 * rh.ULP, 21)
    noisy = xh[1].copy()
    rh.inject(x, xh, t)
    xh[1] = noisy                      # (inject leaves channel 1 without records; the subsets below need some)
    t[2] = np.float32(100.0)
    xh[2] = x[2] + np.float32(300.0) * np.random.default_rng(2).standard_normal(GRID[1:]).astype(np.float32)
    idx, q, eidx, ebits, per = rh.ref_quantize(x, xh, t)
    assert per[:4, 0].min() > 0 and per[0, 1] > 5 and per[3, 1] > 0 and per[4].tolist() == [0, 0]
    full = rh.ref_apply(xh, GRID, t, idx, q, eidx, ebits)
    assert rh.guarantee_holds(x, full, t)
    return x, xh, t, (idx, q, eidx, ebits), full


def _slice(full, channels=None, box=None, stride=None):
    C, H, W = GRID
    rows, cols = kept_points(box or (0, H, 0, W), stride or (1, 1), W)
    chans = list(range(C)) if channels is None else channels
    return np.ascontiguousarray(full[chans][:, rows][:, :, cols])


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_apply_equals_the_reference_and_the_slice_of_the_full_frame(dev, apply_case, name):
    x, xh, t, rec, full = apply_case
    g = GEOMETRIES[name]
    if name == "single_point":
        i = int(rec[0][rec[0] // (GRID[1] * GRID[2]) == 1][3])
        g = dict(channels=[1], box=(i // GRID[2] % GRID[1], i // GRID[2] % GRID[1] + 1, i % GRID[2], 1))
    plain = _slice(xh, **g)
    ref = rh.ref_apply(plain, GRID, t, *rec, **g)
    assert rh.same_bits(ref, _slice(full, **g))            # the reference itself: subset of corrected == corrected subset
    whole, flat = _guarded(plain.size, torch.float32, dev)
    out = flat.view(plain.shape)
    out.copy_(torch.from_numpy(plain))
    lut = None
    if g.get("channels") is not None:
        lut = np.full(GRID[0], -1, dtype=np.int32)
        lut[g["channels"]] = np.arange(len(g["channels"]))
        lut = torch.from_numpy(lut).to(dev)
    rec_d = tuple(torch.from_numpy(a.view(np.int16 if a.dtype.itemsize == 2 else np.int32)).to(dev) for a in rec)
    step = torch.from_numpy(np.float32(2) * t).to(dev)
    # the witness gather runs on the UNCORRECTED output
    first = _slice(np.arange(xh.size).reshape(GRID), **g).reshape(-1)[:1]
    widx = np.unique(np.concatenate([residual.witness_indices(*GRID)[::7], rec[0][:50], rec[2][:20], first])).astype(np.uint32)
    got = ops.residual_gather(out, torch.from_numpy(widx.view(np.int32)).to(dev), GRID, lut, g.get("box"), g.get("stride"))
    got = got.cpu().numpy()
    where = {int(v): k for k, v in enumerate(_slice(np.arange(xh.size).reshape(GRID), **g).reshape(-1))}
    for k, i in enumerate(widx):      # global index -> position in the subset, through kept_points
        if int(i) in where:
            assert got[k, 0] == 1 and got[k].view(np.uint32)[1] == plain.reshape(-1).view(np.uint32)[where[int(i)]]
        else:
            assert got[k].tolist() == [0, 0]
    assert 0 < sum(int(i) in where for i in widx)
    ops.residual_apply(out, rec_d, step, GRID, lut, g.get("box"), g.get("stride"))
    res = out.cpu().numpy()
    assert rh.same_bits(res, ref)
    assert _guards_intact(whole, plain.size)
    # untouched elements keep their bits; touched ones satisfy the guarantee
    touched = np.zeros(xh.size, dtype=bool)
    touched[rec[0]] = touched[rec[2]] = True
    keep = ~_slice(touched.reshape(GRID), **g)
    assert rh.same_bits(res[keep], plain[keep]) and (~keep).any()
    chans = g.get("channels") or list(range(GRID[0]))
    assert rh.guarantee_holds(_slice(x, **g), res, t[chans])


def test_apply_with_empty_records(dev, apply_case):
    _, xh, t, rec, _ = apply_case
    out = torch.from_numpy(xh).to(dev)
    empty = (torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.int16, device=dev),
             torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.int32, device=dev))
    ops.residual_apply(out, empty, torch.from_numpy(np.float32(2) * t).to(dev), GRID)
    assert rh.same_bits(out.cpu().numpy(), xh)
    assert ops.residual_gather(out, empty[0], GRID).shape == (0, 2)


# ---- the API: thin 8-channel model, two frames -----------------------------------------------------------------------------

H, W = 721, 1440
CORRECTED = (1, 5)


def _api(net, dev, tmp_path):
    api = cra5_api(local_root=str(tmp_path), device="cuda", weights=net)
    api._mean_flat = torch.linspace(-1, 1, 8, device=dev)
    api._std_flat = torch.linspace(0.5, 2, 8, device=dev)
    api.mean, api.std = api._mean_flat.view(8, 1, 1), api._std_flat.view(8, 1, 1)
    return api


@pytest.fixture(scope="module")
def files(dev, tmp_path_factory):
    net = VAEformer(0, **synth.thin_model_kwargs())
    synth.load_synthetic(net, seed=7)
    root = tmp_path_factory.mktemp("residual")
    api = _api(net.to(dev), dev, root)
    frames = [(synth.synth_frame(8, seed=s) * api.std.cpu() + api.mean.cpu()).numpy() for s in (3, 4)]
    stamps = ["2024-06-01T00:00:00", "2024-06-01T06:00:00"]
    plain_rep = api.evaluate_batch(stamps, data=frames, workers=2)
    names = [api.channels_to_vname[c] for c in CORRECTED]
    max_error = {v: 2.0 * float(plain_rep[0]["rmse"][c]) for v, c in zip(names, CORRECTED)}
    tol = residual.resolve_tolerance(max_error, api.vname_to_channels, np.ones(8))
    plain_root, save_root = str(root / "plain"), str(root / "CRA5")
    api.encode_era5_batch(stamps, data=frames, save_root=plain_root, workers=2)
    enc = api.encode_era5_batch(stamps, data=frames, save_root=save_root, workers=2, max_error=max_error)
    fulls = [api.decode_from_bin(ts, to_host=True)["x_hat"].reshape(8, H, W) for ts in stamps]
    corrected = np.empty((2, 8, H, W), dtype=np.float32)
    api.decode_batch(stamps, out=corrected, workers=2, residual=True)
    return dict(api=api, stamps=stamps, frames=frames, plain_rep=plain_rep, names=names, max_error=max_error, tol=tol,
                plain_root=plain_root, save_root=save_root, enc=enc, fulls=fulls, corrected=corrected)


def _bin(f, i, root=None):
    ts = f["stamps"][i]
    return f"{root or f['save_root']}/{ts[:4]}/{ts}.bin"


def test_bin_is_byte_identical_and_the_sidecar_is_reported(files):
    f = files
    for i, enc in enumerate(f["enc"]):
        assert open(_bin(f, i), "rb").read() == open(_bin(f, i, f["plain_root"]), "rb").read()
        r = enc["residual"]
        assert r["path"] == _bin(f, i)[:-4] + ".res" and os.path.getsize(r["path"]) == r["bytes"]
        assert rh.same_bits(r["tol"], f["tol"]) and r["per_channel"].shape == (8, 2)
        side = residual.unpack(open(r["path"], "rb").read())
        assert (len(side["idx"]), len(side["eidx"])) == (r["records"], r["escapes"]) == tuple(r["per_channel"].sum(axis=0))
        off = [c for c in range(8) if c not in CORRECTED]
        assert (r["per_channel"][off] == 0).all() and (r["per_channel"][list(CORRECTED), 0] > 0).all()
        assert 0 < r["records"] + r["escapes"] <= 0.25 * 2 * H * W
        assert rh.same_bits(side["wbits"], f["fulls"][i].reshape(-1).view(np.uint32)[side["widx"]])


def test_single_frame_encode_writes_the_same_files(files, tmp_path):
    f = files
    enc = f["api"].encode_era5_as_bin(f["stamps"][0], save_root=str(tmp_path), data=f["frames"][0], max_error=f["max_error"])
    assert open(enc["save_path"], "rb").read() == open(_bin(f, 0), "rb").read()
    r = enc["residual"]
    assert r["path"] == enc["save_path"][:-4] + ".res"
    assert open(r["path"], "rb").read() == open(f["enc"][0]["residual"]["path"], "rb").read()
    assert (r["records"], r["escapes"]) == (f["enc"][0]["residual"]["records"], f["enc"][0]["residual"]["escapes"])
    with pytest.raises(ValueError, match="sidecar"):
        f["api"].encode_era5_as_bin(f["stamps"][0], save_root=str(tmp_path), data=f["frames"][0], max_error=0.1,
                                    return_format="latent")


def test_decode_batch_equals_the_reference_on_the_plain_decode(files):
    f = files
    for i in range(2):
        side = residual.unpack(open(f["enc"][i]["residual"]["path"], "rb").read())
        ref = rh.ref_quantize(f["frames"][i], f["fulls"][i], f["tol"])
        for k, r in zip(("idx", "q", "eidx", "ebits"), ref):
            assert rh.same_bits(side[k], r), k
        assert rh.same_bits(f["corrected"][i], rh.ref_apply(f["fulls"][i], (8, H, W), f["tol"], *ref[:4]))
        assert rh.guarantee_holds(f["frames"][i], f["corrected"][i], f["tol"])
        d = np.abs(f["frames"][i].astype(np.float64) - f["corrected"][i].astype(np.float64))
        for c in CORRECTED:
            assert d[c].max() <= float(f["tol"][c])
    one = f["api"].decode_from_bin(f["stamps"][1], to_host=True, residual=True)["x_hat"]
    assert rh.same_bits(one.reshape(8, H, W), f["corrected"][1])
    dev_out = f["api"].decode_from_bin(f["stamps"][0], residual=f["enc"][0]["residual"]["path"])["x_hat"]
    assert rh.same_bits(dev_out.reshape(8, H, W).cpu().numpy(), f["corrected"][0])


def test_subset_decode_is_the_slice_of_the_corrected_frame(files):
    f, api = files, files["api"]
    variables = [f["names"][1], api.channels_to_vname[2], f["names"][0]]
    chans = [CORRECTED[1], 2, CORRECTED[0]]
    region, stride = (35, 72, -25, 45), (2, 3)
    g = cra5_api.grid_box(region, stride=stride)
    got = api.decode_batch(f["stamps"], workers=2, variables=variables, region=region, stride=stride, residual=True)
    for i in range(2):
        ref = f["corrected"][i][chans][:, g["kept_rows"]][:, :, g["kept_cols"]]
        assert rh.same_bits(got[i], ref)
        assert not rh.same_bits(got[i], f["fulls"][i][chans][:, g["kept_rows"]][:, :, g["kept_cols"]])
    d = api.decode_from_bin(f["stamps"][0], variables=variables[:1], stride=6, to_host=True, residual=True)
    assert rh.same_bits(d["x_hat"], f["corrected"][0][chans[:1], ::6, ::6])


def test_aggregate_batch_over_the_corrected_frames(files):
    f = files
    res = f["api"].aggregate_batch(f["stamps"], stats=("mean", "max"), residual=True, workers=2)
    ref = ref_time_stats([f["corrected"][0], f["corrected"][1]])
    assert res["n"] == 2 and rh.same_bits(res["mean"], ref["mean"]) and rh.same_bits(res["max"], ref["max"])


def test_evaluate_batch_reports_the_bound(files):
    f = files
    reps = f["api"].evaluate_batch(f["stamps"], data=f["frames"], workers=2, max_error=f["max_error"])
    off = [c for c in range(8) if c not in CORRECTED]
    for i, (rep, plain) in enumerate(zip(reps, f["plain_rep"])):
        for c in CORRECTED:
            assert rep["max_abs"][c] <= float(f["tol"][c]) and rep["max_abs"][c] < plain["max_abs"][c]
            assert rep["rmse"][c] < plain["rmse"][c]
        for key in ("rmse", "max_abs", "bias", "mae", "wrmse"):
            assert np.array_equal(rep[key][off], plain[key][off]), key
        r = f["enc"][i]["residual"]
        assert (rep["res_bytes"], rep["records"], rep["escapes"]) == (r["bytes"], r["records"], r["escapes"])
        assert rep["bin_bytes"] == plain["bin_bytes"] and rep["compression_ratio"] == plain["compression_ratio"]
        assert rep["compression_ratio_total"] == 8 * H * W * 4 / (rep["bin_bytes"] + rep["res_bytes"])
        assert "res_bytes" not in plain


def test_altered_witness_and_damaged_payload_are_refused(files, tmp_path):
    f, api = files, files["api"]
    good = f["enc"][0]["residual"]["path"]
    s = residual.unpack(open(good, "rb").read())
    s["wbits"] = s["wbits"].copy()
    s["wbits"][len(s["wbits"]) // 2] ^= 1
    bad = tmp_path / "witness.res"
    bad.write_bytes(residual.pack(s["C"], s["H"], s["W"], s["tol"], s["widx"], s["wbits"], s["idx"], s["q"], s["eidx"],
                                  s["ebits"]))
    out = np.full((1, 8, H, W), -7.0, dtype=np.float32)
    with pytest.raises(ResidualMismatchError, match="not the encoder's"):
        api.decode_batch(f["stamps"][:1], out=out, workers=1, residual=[str(bad)])
    assert (out == -7.0).all()
    # the altered witness lies outside this subset: not checked, the subset decodes
    c_out = int(s["widx"][len(s["widx"]) // 2]) // (H * W)
    keep = [api.channels_to_vname[c] for c in range(8) if c != c_out][:2]
    api.decode_batch(f["stamps"][:1], workers=1, variables=keep, stride=6, residual=[str(bad)])
    blob = bytearray(open(good, "rb").read())
    blob[len(blob) // 2] ^= 0x40
    flipped = tmp_path / "flipped.res"
    flipped.write_bytes(bytes(blob))
    with pytest.raises(ResidualFormatError, match="CRC"):
        api.decode_batch(f["stamps"][:1], out=out, workers=1, residual=[str(flipped)])
    assert (out == -7.0).all()
    with pytest.raises(FileNotFoundError, match="not found"):
        api.decode_batch(f["stamps"][:1], paths=[_bin(f, 0, f["plain_root"])], residual=True)


def test_budget_and_unsupported_combinations(files, tmp_path):
    f, api = files, files["api"]
    tiny = {v: 1e-3 * float(f["plain_rep"][0]["rmse"][c]) for v, c in zip(f["names"], CORRECTED)}
    with pytest.raises(ResidualBudgetError, match="densest channels"):
        api.encode_era5_batch(f["stamps"][:1], data=f["frames"][:1], save_root=str(tmp_path), workers=1, max_error=tiny)
    assert not [p for _, _, fs in os.walk(tmp_path) for p in fs if p.endswith(".res")]
    with pytest.raises(ValueError, match="coarsen"):
        api.decode_batch(f["stamps"], residual=True, coarsen=6)
    with pytest.raises(ValueError, match="normalized"):
        api.decode_batch(f["stamps"], residual=True, return_format="normalized")
    with pytest.raises(ValueError, match="coarsen"):
        api.decode_from_bin(f["stamps"][0], residual=True, coarsen=(6, 6))
    with pytest.raises(ValueError, match="normalized"):
        api.decode_from_bin(f["stamps"][0], residual=True, return_format="normalized")
    with pytest.raises(ValueError):
        api.decode_from_bin(f["stamps"][0], residual=True, return_format="latent")
    with pytest.raises(ValueError, match="coarsen"):
        api.aggregate_batch(f["stamps"], residual=True, coarsen=6)
    with pytest.raises(ValueError, match="coarsen"):
        api.evaluate_batch(f["stamps"], data=f["frames"], max_error=0.1, coarsen=6)
