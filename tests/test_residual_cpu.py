"""Residual layer, host side (no GPU): the numpy reference's guarantee, the sidecar container, the tolerances, the ops'
argument checks."""
import struct
import zlib

import numpy as np
import pytest
import torch

import residual_helpers as rh
from cra5_amd import ops, residual
from cra5_amd.residual import ResidualBudgetError, ResidualFormatError, ResidualMismatchError


def _cases():
    for si, shape in enumerate(rh.SHAPES):
        for kind in ("offset", "zero"):
            for ti, (name, tol) in enumerate(rh.TOLS.items()):
                yield shape, kind, name, tol, 100 * si + 10 * ti + (kind == "zero")


@pytest.mark.parametrize("injected", [False, True])
def test_reference_guarantee_holds_everywhere(injected):
    for shape, kind, name, tol, seed in _cases():
        x, xh, t = rh.field(shape, kind, tol, seed)
        if injected:
            rh.inject(x, xh, t)
        idx, q, eidx, ebits, per = rh.ref_quantize(x, xh, t)
        assert (np.diff(idx.astype(np.int64)) > 0).all() and (np.diff(eidx.astype(np.int64)) > 0).all()
        assert not np.intersect1d(idx, eidx).size and (q != 0).all()
        assert per[:, 0].sum() == len(idx) and per[:, 1].sum() == len(eidx) and (per[~np.isfinite(t)] == 0).all()
        xt = rh.ref_apply(xh, shape, t, idx, q, eidx, ebits)
        # (a NaN truth is an escape: its bits come back)
        assert rh.guarantee_holds(x, xt, t), (shape, kind, name)
        off = ~np.isfinite(t)
        assert rh.same_bits(xt[off], xh[off])
        if injected:
            assert per[0, 1] >= 5        # |q| > 32767 twice, x_hat NaN / inf, the NaN truth
            if shape[0] >= 3:
                assert per[1].tolist() == [0, 0]


def test_escape_path_is_exercised_but_does_not_dominate():
    shape = (2, 64, 256)
    share = {}
    for name, tol in [("0.7ulp", 0.7 * rh.ULP), ("1.3ulp", 1.3 * rh.ULP), ("1000ulp", 1000 * rh.ULP), ("5000ulp", 5000 * rh.ULP)]:
        x, xh, t = rh.field(shape, "offset", tol, seed=5, inf_channel=False)
        idx, q, eidx, ebits, per = rh.ref_quantize(x, xh, t)
        share[name] = (len(eidx) / x.size, len(eidx) / max(1, len(idx) + len(eidx)))
        assert rh.guarantee_holds(x, rh.ref_apply(xh, shape, t, idx, q, eidx, ebits), t)
    assert share["0.7ulp"][0] > 0 and share["1.3ulp"][0] > 0, share
    assert share["1000ulp"][1] <= 0.01 and share["5000ulp"][1] <= 0.01, share


def _sidecar(shape=(3, 5, 37), tol=1.0, seed=3, empty=None):
    x, xh, t = rh.inject(*rh.field(shape, "zero", tol, seed))
    if empty == "records":        # only escapes
        xh = np.where(np.isfinite(t)[:, None, None], np.float32(np.nan), xh).astype(np.float32)
    if empty == "escapes":
        x, xh, t = rh.field(shape, "zero", tol, seed)
    if empty == "both":
        x, xh, t = rh.field(shape, "zero", tol, seed)
        xh = x.copy()
    idx, q, eidx, ebits, per = rh.ref_quantize(x, xh, t)
    widx = residual.witness_indices(*shape)
    wbits = xh.reshape(-1).view(np.uint32)[widx]
    return dict(C=shape[0], H=shape[1], W=shape[2], tol=t, widx=widx, wbits=wbits, idx=idx, q=q, eidx=eidx, ebits=ebits)


def _pack(s):
    return residual.pack(s["C"], s["H"], s["W"], s["tol"], s["widx"], s["wbits"], s["idx"], s["q"], s["eidx"], s["ebits"])


@pytest.mark.parametrize("empty", [None, "records", "escapes", "both"])
def test_pack_unpack_round_trip(empty):
    s = _sidecar(empty=empty)
    assert (len(s["idx"]) == 0) == (empty in ("records", "both")) and (len(s["eidx"]) == 0) == (empty in ("escapes", "both"))
    blob = _pack(s)
    assert blob[:8] == b"CRA5RES1"
    u = residual.unpack(blob)
    assert (u["C"], u["H"], u["W"]) == (3, 5, 37)
    for k in ("tol", "widx", "wbits", "idx", "q", "eidx", "ebits"):
        assert u[k].dtype == s[k].dtype and rh.same_bits(u[k], s[k]), k
    assert len(u["widx"]) == 3 * 5 * 37        # a frame smaller than 1024 points: every point is a witness


def test_witness_indices():
    w = residual.witness_indices(268, 721, 1440)
    N = 268 * 721 * 1440
    assert w.dtype == np.uint32 and len(w) == 1024 and w[0] == 0
    assert w.tolist() == [i * N // 1024 for i in range(1024)]
    assert residual.witness_indices(1, 2, 3).tolist() == [0, 1, 2, 3, 4, 5]


def test_unpack_refuses_damaged_bytes():
    blob = _pack(_sidecar())
    with pytest.raises(ResidualFormatError, match="magic|start with"):
        residual.unpack(b"CRA5RESX" + blob[8:])
    with pytest.raises(ResidualFormatError, match="CRC"):
        residual.unpack(blob[:-9])
    with pytest.raises(ResidualFormatError):
        residual.unpack(blob[:20])
    with pytest.raises(ResidualFormatError):
        residual.unpack(b"")
    for at in (12, len(blob) // 2, len(blob) - 6):
        bad = bytearray(blob)
        bad[at] ^= 0x10
        with pytest.raises(ResidualFormatError, match="CRC"):
            residual.unpack(bytes(bad))

    def recrc(body):
        return body + struct.pack("<I", zlib.crc32(body) & 0xffffffff)
    # a valid CRC over a truncated payload, and over indexes that do not ascend / leave the frame
    with pytest.raises(ResidualFormatError, match="truncated"):
        residual.unpack(recrc(blob[:-40]))
    s = _sidecar()
    with pytest.raises(ValueError, match="ascend"):
        residual.pack(s["C"], s["H"], s["W"], s["tol"], s["widx"], s["wbits"], s["idx"][::-1], s["q"], s["eidx"], s["ebits"])
    body = bytearray(blob[:-4])      # a header that claims a smaller frame than the witnesses and indexes cover
    body[8:8 + residual.HEADER.size] = residual.HEADER.pack(3, 5, 36, len(s["idx"]), len(s["eidx"]), len(s["widx"]))
    with pytest.raises(ResidualFormatError):
        residual.unpack(recrc(bytes(body)))


def test_resolve_tolerance():
    v2c = {"a": 0, "b": 1, "c": 2, "far": 7}
    std = np.array([0.5, 2.0, 3.0], dtype=np.float32)
    t = residual.resolve_tolerance(0.1, v2c, std)
    assert t.dtype == np.float32 and rh.same_bits(t, (0.1 * std.astype(np.float64)).astype(np.float32))
    t = residual.resolve_tolerance({"c": 0.25, "a": 2}, v2c, std)
    assert t.tolist() == [2.0, np.inf, 0.25]
    assert residual.resolve_tolerance(np.float32(1.5), v2c, std).tolist() == [0.75, 3.0, 4.5]
    for bad in (0, -1.0, float("nan"), float("inf"), True, "0.1", {}, {"a": 0.0}, {"a": -1}, {"a": float("inf")},
                {"a": True}, {"a": "1"}, {"zz": 1.0}, {"far": 1.0}, 1e35, {"a": 1e31}, None.__class__, [0.1]):
        with pytest.raises(ValueError):
            residual.resolve_tolerance(bad, v2c, std)


def test_budget_error_names_the_densest_channels():
    per = np.array([[10, 0], [700, 50], [0, 0], [300, 0]])
    tol = np.array([1.0, 1.0, np.inf, 1.0], dtype=np.float32)
    residual.check_budget(per, tol, 1000, 0.5)
    residual.check_budget(per, tol, 1000, None)
    with pytest.raises(ResidualBudgetError, match=r"v1 75\.0 %, v3 30\.0 %, v0 1\.0 %") as e:
        residual.check_budget(per, tol, 1000, 0.25, names=["v0", "v1", "v2", "v3"])
    assert "1060" in str(e.value) and "3000" in str(e.value)


def test_witness_check():
    w = np.array([1, 2, 3], dtype=np.uint32)
    residual.check_witnesses([True, False, True], np.array([1, 9, 3], dtype=np.uint32), w)
    with pytest.raises(ResidualMismatchError, match="not the encoder's"):
        residual.check_witnesses([True, True, True], np.array([1, 9, 3], dtype=np.uint32), w)


def test_sidecar_path():
    assert residual.sidecar_path("/a/2024/2024-06-01T00:00:00.bin") == "/a/2024/2024-06-01T00:00:00.res"
    assert residual.sidecar_path("frame") == "frame.res"


def test_ops_argument_checks_without_gpu():
    x = torch.zeros(2, 3, 4)
    with pytest.raises(TypeError, match="x must be a contiguous fp32 device tensor"):
        ops.residual_quantize(x, x, [1.0, 1.0])
    with pytest.raises(TypeError, match="x must be a torch tensor"):
        ops.residual_quantize(np.zeros((2, 3, 4), dtype=np.float32), x, [1.0, 1.0])
    with pytest.raises(TypeError, match="out must be a contiguous fp32 device tensor"):
        ops.residual_apply(x, (x, x, x, x), x, (2, 3, 4))
    with pytest.raises(TypeError, match="out must be"):
        ops.residual_gather(x, x, (2, 3, 4))
    for bad in ([1.0], [1.0, 0.0], [1.0, -2.0], [1.0, float("nan")], [1.0, 2e30], [[1.0, 1.0]]):
        with pytest.raises(ValueError, match="tol"):
            ops.residual_tolerance(np.array(bad, dtype=np.float32), 2)
    with pytest.raises(TypeError, match="tol"):
        ops.residual_tolerance(np.array([1, 2]), 2)
    t = ops.residual_tolerance([0.5, float("inf")], 2)
    assert t.dtype == np.float32 and t.tolist() == [0.5, np.inf]
    assert ops.RESIDUAL_SPAN == 4096
