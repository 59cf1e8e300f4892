"""The split-f16 reference and reporter of tests/split_helpers.py, checked without a GPU: the reference against float64,
the layout arithmetic of ops.SplitMat against it, and one deliberately wrong store per fault the GPU tests are meant to
catch - each must be reported with the class and the position that names it."""
import numpy as np
import pytest
import torch

import split_helpers as S
from cra5_amd import ops


def _finite():
    v, c = S.split_domain()
    keep = (c & (S.OVERFLOW | S.NONFINITE)) == 0
    return v[keep], c[keep]


def test_domain_holds_every_class():
    v, c = S.split_domain()
    assert 4.4e5 < v.size < 4.7e5 and v.dtype == np.float32
    n_hi, n_lo = S.domain_counts()
    print(f"domain: {v.size} values; the reference stores {n_hi} subnormal hi and {n_lo} subnormal lo halves; per class: "
          + ", ".join(f"{n} {int(((c >> i) & 1).sum())}" for i, n in enumerate(S.CLASSES)))
    # 2 x (1023 subnormal f16 + their midpoints and neighbours) and ~ 10 / 256 of the random patterns; lo: far more
    assert n_hi > 8000 and n_lo > 4 * n_hi
    for i, n in enumerate(S.CLASSES):
        assert int(((c >> i) & 1).sum()) > 0, n
    assert not v.flags.writeable


def test_fp32_residual_is_exact():
    """x - f32(hi) in fp32 equals the float64 difference on the whole finite domain: the two-conversion form and the
    fused multiply-add form of the kernels have one expectation"""
    v, _ = _finite()
    hi, _ = S.split_ref(v)
    d32 = v - hi.astype(np.float32)
    d64 = v.astype(np.float64) - hi.astype(np.float64)
    assert np.array_equal(d32.astype(np.float64), d64)


def test_reconstruction_bounds():
    """hi + lo = x within 2^-22 |x| for |x| >= 2^-3 (two 11-bit halves), within 2^-25 absolutely below (half the
    spacing of the f16 subnormals)"""
    v, _ = _finite()
    hi, lo = S.split_ref(v)
    err = np.abs(hi.astype(np.float64) + lo.astype(np.float64) - v.astype(np.float64))
    big = np.abs(v) >= 2.0 ** -3
    rel, ab = float((err[big] / np.abs(v[big].astype(np.float64))).max()), float(err[~big].max())
    print(f"largest relative error at |x| >= 2^-3: {rel:.3g} (bound {2.0 ** -22:.3g}); largest absolute error below: {ab:.3g} "
          f"(bound {2.0 ** -25:.3g})")
    assert rel <= 2.0 ** -22 and ab <= 2.0 ** -25


def test_ties_go_to_even_and_the_edges_are_ieee():
    h = np.arange(0x7c00, dtype=np.uint16)
    hf = h.view(np.float16).astype(np.float64)
    mid = ((hf[:-1] + hf[1:]) * 0.5).astype(np.float32)
    hi, lo = S.split_ref(mid)
    even = np.where(h[:-1] % 2 == 0, h[:-1], h[1:])
    assert np.array_equal(hi.view(np.uint16), even)
    assert bool((S.classify(mid) & S.TIE).all())
    hi_n, _ = S.split_ref(-mid)
    assert np.array_equal(hi_n.view(np.uint16), even | 0x8000)
    # the residual of a tie is half a spacing of hi: a power of two, stored exactly from 2^-24 on (hi >= 2^-13)
    big = mid >= 2.0 ** -13
    assert np.array_equal((hi.astype(np.float64) + lo.astype(np.float64))[big], mid.astype(np.float64)[big])
    x = np.array([65504.0, 65519.996, 65520.0, -65520.0, 1e5, np.inf, -np.inf, np.nan, 2.0 ** -25,
                  np.nextafter(np.float32(2.0 ** -25), np.float32(1)), 2.0 ** -26, -0.0], dtype=np.float32)
    hi, lo = S.split_ref(x)
    assert [f"{u:#06x}" for u in hi.view(np.uint16)[:7]] == ["0x7bff", "0x7bff", "0x7c00", "0xfc00", "0x7c00", "0x7c00", "0xfc00"]
    assert [f"{u:#06x}" for u in lo.view(np.uint16)[2:5]] == ["0xfc00", "0x7c00", "0xfc00"]
    assert np.isnan(hi[7]) and np.isnan(lo[5]) and np.isnan(lo[6]) and np.isnan(lo[7])
    # 2^-25 is the tie between 0 and the smallest subnormal: to even = 0, and lo rounds the same way
    assert hi.view(np.uint16)[8] == 0 and lo.view(np.uint16)[8] == 0
    assert hi.view(np.uint16)[9] == 1 and hi.view(np.uint16)[10] == 0 and hi.view(np.uint16)[11] == 0x8000
    assert lo.view(np.uint16)[11] == 0          # -0 - (-0) = +0


def test_domain_matrix_covers_every_class_in_every_residue_and_both_end_chunks():
    for rows, K, classes in ((8730, 52, S.ALL_CLASSES), (1, 144, S.FINITE_IN_RANGE), (333, 77, S.ALL_CLASSES),
                             (7, 360, S.FINITE_IN_RANGE), (16, 64, S.ALL_CLASSES)):
        m = S.domain_matrix(rows, K, classes)
        c = S.classify(m)
        assert not (c & ~np.uint8(classes)).any()
        last = (K - 1) // 32
        for i, n in enumerate(S.CLASSES):
            if not classes & (1 << i):
                continue
            has = (c & (1 << i)) != 0
            assert all(has[:, q::4].any() for q in range(4)), (rows, K, n)
            assert has[:, :32].any() and has[:, last * 32:].any(), (rows, K, n)
    assert np.array_equal(S.domain_matrix(40, 52, seed=3), S.domain_matrix(40, 52, seed=3), equal_nan=True)


@pytest.mark.parametrize("K", [52, 64, 77])
def test_splitmat_layout_arithmetic_matches_the_helper(K):
    """a CPU SplitMat holding split_ref's storage: planes() and to_float() return the same halves"""
    x = S.domain_matrix(40, K, S.FINITE_IN_RANGE)
    Kp = (K + 31) // 32 * 32
    raw = S.storage_from_ref(x)
    sm = ops.SplitMat(torch.from_numpy(raw.view(np.int16).copy()), 40, K, Kp)
    hi, lo = S.split_ref(x)
    ph, pl = sm.planes()
    assert np.array_equal(ph.numpy().astype(np.float16).view(np.uint16), hi.view(np.uint16))
    assert np.array_equal(pl.numpy().astype(np.float16).view(np.uint16), lo.view(np.uint16))
    assert np.array_equal(sm.to_float().numpy(), hi.astype(np.float32) + lo.astype(np.float32))
    assert S.compare_planes(sm.data.numpy(), x, K, Kp) == 40 * 2 * Kp
    plain = ops.SplitMat(torch.from_numpy(S.storage_from_ref(x, plain=True).view(np.int16).copy()), 40, K, Kp, plain=True)
    assert np.array_equal(plain.planes()[0].numpy().astype(np.float16).view(np.uint16), hi.view(np.uint16))
    assert np.array_equal(plain.data.numpy()[:, :Kp], sm.plain_copy().data.numpy())
    S.compare_planes(plain.data.numpy(), x, K, Kp, plain=True)
    S.compare_planes(sm.plain_copy().data.numpy(), x, K, Kp, plain=True)          # (pitch Kp: a plain weight copy)


# ------------------------------------------------------------------------------------------------ mutations

ROWS, K, KP = 8730, 52, 64


@pytest.fixture(scope="module")
def stored():
    x = S.domain_matrix(ROWS, K, S.FINITE_IN_RANGE)
    raw = S.storage_from_ref(x)
    assert S.compare_planes(raw, x, K, KP) == raw.size
    return x, raw


def _planes(raw):
    v = raw.reshape(ROWS, KP // 32, 2, 32)
    return v[:, :, 0].reshape(ROWS, KP).copy(), v[:, :, 1].reshape(ROWS, KP).copy()


def _storage(hi_bits, lo_bits):
    raw = np.zeros((ROWS, KP // 32, 2, 32), dtype=np.uint16)
    raw[:, :, 0] = hi_bits.reshape(ROWS, KP // 32, 32)
    raw[:, :, 1] = lo_bits.reshape(ROWS, KP // 32, 32)
    return raw.reshape(ROWS, 2 * KP)


def _trunc_f16(d):
    """f16 of the fp32 array d rounded TOWARD ZERO"""
    r = d.astype(np.float16)
    over = np.abs(r.astype(np.float64)) > np.abs(d.astype(np.float64))
    return np.where(over, np.nextafter(r, np.float16(0)), r).astype(np.float16)


def _report(raw, x, **kw):
    with pytest.raises(S.SplitMismatch) as ei:
        S.compare_planes(raw, x, K, KP, **kw)
    print(str(ei.value))
    return ei.value


def test_reports_a_truncated_lo(stored):
    x, raw = stored
    hi, _ = S.split_ref(x)
    lo_t = _trunc_f16(x - hi.astype(np.float32))
    hb, lb = _planes(raw)
    lb[:, :K] = lo_t.view(np.uint16)
    e = _report(_storage(hb, lb), x)
    # only inexact residuals move: never a tie (its residual is stored exactly), never a hi half, never the padding
    assert e.planes == [0, e.n, 0] and e.n > 10000
    assert e.by_class["tie"] == 0 and e.by_class["zero"] == 0 and e.by_class["padding"] == 0
    assert e.by_class["normal"] > 0 and e.by_class["lo-subnormal"] > 0
    assert min(e.col4) > 0.15 * e.n               # no column pattern: a rounding rule


def test_reports_a_subnormal_hi_read_as_zero(stored):
    """the mix instruction reading a subnormal hi as 0: lo = f16(x) again, the operand is 2 x"""
    x, raw = stored
    hi, _ = S.split_ref(x)
    hb, lb = _planes(raw)
    sub = (hi != 0) & (np.abs(hi.astype(np.float64)) < S.F16_MIN_NORMAL)
    lb[:, :K] = np.where(sub, hi.view(np.uint16), lb[:, :K])
    e = _report(_storage(hb, lb), x)
    assert e.planes == [0, e.n, 0]
    assert e.by_class["hi-subnormal"] == e.n and e.by_class["normal"] == 0 and e.by_class["padding"] == 0
    assert "hi-subnormal: " in str(e)


def test_reports_a_flushed_subnormal_lo(stored):
    x, raw = stored
    hb, lb = _planes(raw)
    sub = ((lb & 0x7c00) == 0) & ((lb & 0x03ff) != 0)
    lb = np.where(sub, lb & 0x8000, lb).astype(np.uint16)
    e = _report(_storage(hb, lb), x)
    assert e.planes == [0, e.n, 0] and e.n == int(sub.sum())
    assert e.by_class["lo-subnormal"] == e.n and e.by_class["normal"] == 0


def test_reports_swapped_pairs(stored):
    """the halves of each (4k, 4k + 1) pair exchanged, as a wrong op_sel would: columns = 0, 1 (mod 4) alone"""
    x, raw = stored
    hb, lb = _planes(raw)
    for p in (hb, lb):
        a, b = p[:, 0::4].copy(), p[:, 1::4].copy()
        p[:, 0::4], p[:, 1::4] = b, a
    e = _report(_storage(hb, lb), x)
    assert e.col4[2] == 0 and e.col4[3] == 0 and e.col4[0] > 0 and e.col4[0] == e.col4[1]
    assert e.planes[0] > 0 and e.planes[1] > 0
    assert sum(1 for n in ("normal", "tie", "hi-subnormal", "lo-subnormal") if e.by_class[n] > 0) == 4   # every class: not arithmetic


def test_reports_a_wrong_tail_column(stored):
    """column 4k + 3 of the last chunk taken from its neighbour: a scalar tail that disagrees with the quad path"""
    x, raw = stored
    hb, lb = _planes(raw)
    for p in (hb, lb):
        p[:, 35:K:4] = p[:, 34:K:4]
    e = _report(_storage(hb, lb), x)
    assert e.col4[:3] == [0, 0, 0] and e.col4[3] == e.n and e.last_chunk == e.n
    assert all(k == 0 for q, k in enumerate(e.col32) if q % 4 != 3)


def test_reports_one_half_in_the_padding(stored):
    x, raw = stored
    bad = raw.copy()
    bad[17, 64 + 32 + 25] = 0x3c00                 # row 17, chunk 1, lo plane, column 32 + 25 = 57 >= K
    e = _report(bad, x)
    assert e.n == 1 and e.by_class["padding"] == 1 and e.planes == [0, 1, 0] and e.last_chunk == 1
    assert "(17, 57, lo, padding, 0x3c00 = 1.0, 0x0000 = 0.0)" in str(e)
    # a plain row: the padding K..Kp is zero, the rest of the 2 * Kp row what the caller filled it with
    pl = S.expected_storage(x, K, KP, plain=True, fill=0x3c00).copy()
    assert S.compare_planes(pl, x, K, KP, plain=True, fill=0x3c00) == pl.size
    pl[3, K + 2] = 0x3c00
    pl[4, KP + 9] = 0
    with pytest.raises(S.SplitMismatch) as ei:
        S.compare_planes(pl, x, K, KP, plain=True, fill=0x3c00)
    assert ei.value.n == 2 and ei.value.planes == [1, 0, 1] and ei.value.by_class["padding"] == 2
    # the reduced-precision GEMM writes no lo plane: it must stay as filled
    hi_only = S.expected_storage(x, K, KP, plain=False, lo_written=False)
    assert not hi_only.reshape(ROWS, KP // 32, 2, 32)[:, :, 1].any()
    with pytest.raises(S.SplitMismatch):
        S.compare_planes(raw, x, K, KP, lo_written=False)


def test_nan_patterns_compare_equal_and_nothing_else_does():
    x = np.array([[np.nan, np.inf, 1.0, -np.inf] * 2], dtype=np.float32)
    raw = S.storage_from_ref(x)
    other = raw.copy()
    other[0, 0] = 0xfe01                            # another NaN pattern in the hi plane
    other[0, 32 + 1] = 0x7e00                       # lo of +inf is NaN: any NaN
    assert S.compare_planes(other, x, 8, 32) == 64
    other[0, 1] = 0xfc00                            # -inf is not +inf
    with pytest.raises(S.SplitMismatch) as ei:
        S.compare_planes(other, x, 8, 32)
    assert ei.value.n == 1 and ei.value.by_class["non-finite"] == 1
