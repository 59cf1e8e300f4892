"""Bit-exact tests of the split-f16 store (csrc/split.h) in every producer kernel: the RAW 16-bit storage a producer
leaves behind - padding included - against tests/split_helpers.split_ref, on a domain that holds every rounding case
(ties, subnormal hi / lo halves, the 65504..65520 edge, overflow, non-finite values).

Where a producer passes chosen values straight through, it is fed split_helpers.domain_matrix / a shuffled image of the
domain; where it computes, the expectation is split_ref of the fp32 output of the SAME call (or, for the epilogue body
that exists without an fp32 output only, of the same operands' launch that has one).  The only leniency anywhere is
NaN == NaN.  Every output buffer is zero-filled first."""
import numpy as np
import pytest
import torch

import split_helpers as S
from cra5_amd import ops
from cra5_amd._lib import check, lib

pytestmark = pytest.mark.gpu

RARE = S.ZERO | S.EDGE          # classes of a handful of values: repeated when an image is filled at random


def _u16(sm):
    return sm.data.cpu().numpy().view(np.uint16)


def _np(t):
    return t.detach().cpu().numpy()


def _same(a, b):
    """numerically equal fp32 arrays (-0 == +0, NaN == NaN)"""
    return np.array_equal(a, b, equal_nan=True)


def _compare(sm, x, label, **kw):
    n = S.compare_planes(_u16(sm), x, sm.K, sm.Kp, plain=sm.plain, label=label, **kw)
    return n


def _require(x, classes, label, chunks=True):
    """every class of `classes` in every column residue mod 4 and in the first and the last 32-column chunk of x"""
    c = S.classify(x)
    last = (x.shape[1] - 1) // 32 * 32
    for i, name in enumerate(S.CLASSES):
        if not classes & (1 << i):
            continue
        has = (c & (1 << i)) != 0
        assert all(has[:, q::4].any() for q in range(4)), f"{label}: class {name} misses a column residue mod 4"
        if chunks:
            assert has[:, :32].any() and has[:, last:].any(), f"{label}: class {name} misses the first or the last chunk"


def _domain_fill(n, classes, seed):
    """n fp32 values: the domain restricted to `classes`, its rare classes repeated 300 times, shuffled, cut / repeated to n"""
    v, c = S.split_domain()
    keep = (c & ~np.uint8(classes)) == 0
    pool = np.concatenate([v[keep], np.tile(v[keep & ((c & RARE) != 0)], 300)])
    rng = np.random.default_rng(seed)
    return np.resize(pool[rng.permutation(pool.size)], n).astype(np.float32)


# ------------------------------------------------------------------------------------------------ cra5_split_f16


@pytest.mark.parametrize("K", [52, 64])
def test_split_rows_kernel(dev, K):
    """the whole domain through split_rows_kernel: scale 1 and 2^-3 (more subnormal halves), a contiguous input and a
    row-strided view"""
    rows = -(-S.split_domain()[0].size // K)
    x = S.domain_matrix(rows, K)
    _require(x, S.ALL_CLASSES, "split_rows input")
    big = torch.zeros(rows, K + 12, device=dev)
    big[:, 3:3 + K] = torch.from_numpy(x).to(dev)
    for xin in (torch.from_numpy(x).to(dev), big[:, 3:3 + K]):
        for scale in (1.0, 0.125):
            sm = ops.SplitMat.empty(rows, K, dev, zero=True)
            ops.split_f16(xin, scale, out=sm)
            with np.errstate(invalid="ignore"):
                want = x * np.float32(scale)
            _compare(sm, want, f"cra5_split_f16 K = {K}, scale {scale}, ldx {xin.stride(0)}")


# ------------------------------------------------------------------------------------------------ LayerNorm


@pytest.mark.parametrize("rows", [7, 33])
@pytest.mark.parametrize("D", [144, 360, 1024, 2048])
def test_layernorm_store(dev, D, rows):
    """gamma = 0, beta = domain: every row is beta (asserted on the fp32 output of the same call); then random gamma /
    beta against the call's own fp32 y.  Split and plain rows; D = 144, 360 have K padding."""
    g = torch.Generator().manual_seed(D + rows)
    x = (torch.randn(rows, D, generator=g) * 2 + 0.3).to(dev)
    beta = S.domain_matrix(1, D, S.FINITE_IN_RANGE, seed=D)
    _require(beta, S.FINITE_IN_RANGE, f"LayerNorm beta D = {D}", chunks=D > 32)
    cases = [("beta route", torch.zeros(D, device=dev), torch.from_numpy(beta[0]).to(dev)),
             ("random", (1 + 0.3 * torch.randn(D, generator=g)).to(dev), (1e-3 * torch.randn(D, generator=g)).to(dev))]
    for name, ga, be in cases:
        for plain in (False, True):
            y = torch.full((rows, D), float("nan"), device=dev)
            sm = ops.SplitMat.empty(rows, D, dev, zero=True)
            ops.layernorm(x, ga, be, 1e-6, out=y, out_split=sm, out_plain=plain)
            yn = _np(y)
            if name == "beta route":
                assert _same(yn, np.broadcast_to(beta, (rows, D))), "gamma = 0 must give rows equal to beta"
            assert sm.plain == plain
            _compare(sm, yn, f"layernorm {name} {rows} x {D}, plain {plain}")
            only = ops.SplitMat.empty(rows, D, dev, zero=True)           # (and the launch without an fp32 output)
            ops.layernorm(x, ga, be, 1e-6, out_split=only, want_f32=False, out_plain=plain)
            assert torch.equal(only.data, sm.data)


# ------------------------------------------------------------------------------------------------ patch gathers


def _im2col_both(x, mean, std, kh, kw, sh, sw, ldk, plain, dev):
    """cra5_im2col_f32 with BOTH output pointers: (fp32 cols [tokens, ldk], the SplitMat of the same call)"""
    C, H, W = x.shape
    Hp, Wp = (H - kh) // sh + 1, (W - kw) // sw + 1
    K = C * kh * kw
    cols = torch.zeros(Hp * Wp, ldk, device=dev)
    sm = ops.SplitMat.empty(Hp * Wp, K, dev, zero=True)
    assert sm.Kp == ldk
    sm.plain = plain
    check(lib().cra5_im2col_f32(x.data_ptr(), None if mean is None else mean.data_ptr(), None if std is None else std.data_ptr(),
                                cols.data_ptr(), sm.data.data_ptr(), C, H, W, kh, kw, sh, sw, Hp, Wp, ldk, int(plain),
                                torch.cuda.current_stream().cuda_stream), "cra5_im2col_f32")
    return cols, sm


def _unfold(img, kh, kw, sh, sw):
    """numpy patch gather: [C, H, W] -> [Hp * Wp, C * kh * kw], column (c * kh + i) * kw + j"""
    C, H, W = img.shape
    Hp, Wp = (H - kh) // sh + 1, (W - kw) // sw + 1
    r = (np.arange(Hp) * sh)[:, None] + np.arange(kh)[None]                    # [Hp, kh]
    c = (np.arange(Wp) * sw)[:, None] + np.arange(kw)[None]                    # [Wp, kw]
    p = img[:, r[:, None, :, None], c[None, :, None, :]]                       # [C, Hp, Wp, kh, kw]
    return np.ascontiguousarray(p.transpose(1, 2, 0, 3, 4)).reshape(Hp * Wp, C * kh * kw)


def _gather_cases(img, dev, classes):
    C = img.shape[0]
    g = torch.Generator().manual_seed(C)
    mean, std = (0.1 * torch.randn(C, generator=g)).to(dev), (1.0 + torch.rand(C, generator=g)).to(dev)
    return [("pass-through", None, None), ("normalised", mean, std)]


def test_im2col_generic_store(dev):
    """3 x 3 patches, stride 2, C = 5, ldk = 64 (19 pad columns): the whole domain passes through unchanged, NaN / inf /
    overflow included; then with mean / std against the fp32 cols of the same call"""
    C, H, W, k, s = 5, 301, 303, 3, 2
    img = _domain_fill(C * H * W, S.ALL_CLASSES, 11).reshape(C, H, W)
    want = _unfold(img, k, k, s, s)
    _require(want, S.ALL_CLASSES, "generic im2col pass-through")
    x = torch.from_numpy(img).to(dev)
    for name, mean, std in _gather_cases(img, dev, S.ALL_CLASSES):
        cols, sm = _im2col_both(x, mean, std, k, k, s, s, 64, False, dev)
        cn = _np(cols)
        assert not cn[:, 45:].any()
        if mean is None:
            assert np.array_equal(cn[:, :45].view(np.uint32), want.view(np.uint32)), "pass-through must copy the bits"
        _compare(sm, cn[:, :45], f"im2col generic {name}")
        only = ops.SplitMat.empty(sm.rows, 45, dev, zero=True)
        ops.im2col(x, k, k, s, s, mean=mean, std=std, out_split=only)
        assert torch.equal(only.data, sm.data)


def test_im2col_generic_plain_store(dev):
    """plain rows of the generic kernel exist at ldk == C kh kw only: C = 32 (K = 288)"""
    C, H, W, k, s = 32, 41, 43, 3, 2
    img = _domain_fill(C * H * W, S.ALL_CLASSES, 12).reshape(C, H, W)
    want = _unfold(img, k, k, s, s)
    _require(want, S.ALL_CLASSES, "generic im2col plain pass-through")
    x = torch.from_numpy(img).to(dev)
    for name, mean, std in _gather_cases(img, dev, S.ALL_CLASSES):
        for plain in (True, False):
            cols, sm = _im2col_both(x, mean, std, k, k, s, s, 288, plain, dev)
            if mean is None:
                assert np.array_equal(_np(cols).view(np.uint32), want.view(np.uint32))
            _compare(sm, _np(cols), f"im2col generic {name}, plain {plain}")


@pytest.mark.parametrize("C", [7, 13])
def test_im2col_tiled_store(dev, C):
    """the LDS-tiled 11 x 10 gather at the smallest grid it takes (2 x 16 tokens): quad body, the scalar tail of the
    ragged last channel tile (110 = 27 * 4 + 2 columns) and the K padding; split and plain rows"""
    H, W, kh, kw, s = 21, 160, 11, 10, 10
    K = C * kh * kw
    Kp = (K + 31) // 32 * 32
    img = _domain_fill(C * H * W, S.ALL_CLASSES, 20 + C).reshape(C, H, W)
    for t in range(2 * 32):       # the last chunk is the scalar tail's two columns: every class there, by hand
        vals = S.class_values(1 << (t % 8))
        img[C - 1, (t // 32) * s + kh - 1, (t // 2 % 16) * s + kw - 2 + t % 2] = vals[(t * 131) % vals.size]
    want = _unfold(img, kh, kw, s, s)
    _require(want, S.ALL_CLASSES, f"tiled im2col C = {C}")
    tail = want[:, K - 2:]                                      # the scalar-tail columns of the last channel
    assert (S.classify(tail) & (S.TIE | S.HI_SUB | S.LO_SUB)).any()
    x = torch.from_numpy(img).to(dev)
    for name, mean, std in _gather_cases(img, dev, S.ALL_CLASSES):
        for plain in (False, True):
            cols, sm = _im2col_both(x, mean, std, kh, kw, s, s, Kp, plain, dev)
            cn = _np(cols)
            assert not cn[:, K:].any()
            if mean is None:
                assert np.array_equal(cn[:, :K].view(np.uint32), want.view(np.uint32))
            _compare(sm, cn[:, :K], f"im2col tiled C = {C} {name}, plain {plain}")
            only = ops.SplitMat.empty(sm.rows, K, dev, zero=True)
            ops.im2col(x, kh, kw, s, s, mean=mean, std=std, out_split=only, out_plain=plain)
            assert torch.equal(only.data, sm.data)


def test_conv_im2col_store(dev):
    """zero-padded 5 x 5 gather, stride 2, on a 3 x 9 x 11 image: pass-through; border taps are +0 in both planes"""
    C, H, W, k, s, p = 3, 9, 11, 5, 2, 2
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    want_all = []
    for seed in range(8):                                       # 8 images of 297 values: every class in every residue
        img = S.domain_matrix(C * H, W, S.FINITE_IN_RANGE, seed=seed).reshape(C, H, W)
        rng = np.random.default_rng(seed)
        for bit in (S.ZERO, S.EDGE):                            # the classes of a handful of values: twelve pixels each
            vals = S.class_values(bit)
            img.reshape(-1)[rng.choice(img.size, 12, replace=False)] = vals[rng.integers(0, vals.size, 12)]
        padded = np.zeros((C, H + 2 * p, W + 2 * p), dtype=np.float32)
        padded[:, p:p + H, p:p + W] = img
        want = _unfold(padded, k, k, s, s)
        assert want.shape == (Ho * Wo, C * k * k)
        sm = ops.SplitMat.empty(Ho * Wo, C * k * k, dev, zero=True)
        xd = torch.from_numpy(img).to(dev)
        check(lib().cra5_conv_im2col_f32(xd.data_ptr(), sm.data.data_ptr(), C, H, W, k, k, s, s, p, p, Ho, Wo, sm.Kp,
                                         torch.cuda.current_stream().cuda_stream), "cra5_conv_im2col_f32")
        _compare(sm, want, f"conv_im2col image {seed}")
        border = _unfold(np.pad(np.ones((C, H, W), np.float32), ((0, 0), (p, p), (p, p))), k, k, s, s) == 0
        assert border.any() and not want.view(np.uint32)[border].any()          # +0 expected there: both planes 0x0000
        want_all.append(want)
    _require(np.concatenate(want_all, 0), S.FINITE_IN_RANGE, "conv_im2col", chunks=False)


# ------------------------------------------------------------------------------------------------ GEMM epilogues

SPLIT_MN = [(256, 256), (10368, 1024), (2048, 4096), (1000, 360), (333, 77), (2048, 1024), (648, 8192), (2100, 2304),
            (4099, 1030), (3000, 2050),          # M, N of test_exact_gpu.SPLIT_SHAPES: the 64 / 128 / 192 / 256-row tiles
            (2100, 2307)]                        # N % 4 != 0 under the 256 x 256 tile ((333, 77), (4099, 1030): the others)
GK = 32


def _gemm_operands(M, N, dev, zero_a):
    g = torch.Generator().manual_seed(M + N)
    a = torch.zeros(M, GK) if zero_a else torch.randn(M, GK, generator=g) * 0.7
    w = torch.randn(N, GK, generator=g) * 0.3
    return ops.split_f16(a.to(dev)), ops.split_f16(w.to(dev), "auto")


def _check_other_body(sm, c, lo_written, label):
    """The straight-line GELU epilogue has no fp32 output, and its GELU is not bit-identical with the generic body's: on
    the MI355X the two differ by an fp32 ulp on ~1.5 % of the elements (measured: 321 320 of 21 233 664 halves at 10368 x
    1024, all but 108 of them lo halves).  So against the generic launch's fp32 output `c` this body's store is held to
    what does not depend on that ulp: the padding is zero; every (hi, lo) is a pair the store can produce, |lo| <= half
    the spacing of hi (a swapped pair or a lo taken from a stale register breaks it); and hi + lo is c within the store's
    own 2^-21 |c| + 2^-24 (hi alone: 2^-11 |c| + 2^-25) plus, for the difference of the two bodies, 2^-20 |c| (a few ulp
    of the result) + 2^-19 (gelu = x / 2 (1 + erf): where 1 + erf cancels, a few ulp OF ONE in it, 2^-23 each, times
    |x| / 2 <= 4 at these operands).  A stale or swapped operand is off by the size of the values themselves."""
    raw = _u16(sm)
    rows, K, Kp = sm.rows, sm.K, sm.Kp
    c64 = c.astype(np.float64)
    if sm.plain:
        assert not raw[:, K:].any(), f"{label}: padding / beyond the plain row"
        hi, lo = raw[:, :K].view(np.float16).astype(np.float64), None
    else:
        v = raw.reshape(rows, Kp // 32, 2, 32)
        hb, lb = v[:, :, 0].reshape(rows, Kp), v[:, :, 1].reshape(rows, Kp)
        assert not hb[:, K:].any() and not lb[:, K:].any(), f"{label}: padding"
        hi = np.ascontiguousarray(hb[:, :K]).view(np.float16).astype(np.float64)
        lo = np.ascontiguousarray(lb[:, :K]).view(np.float16).astype(np.float64)
        if not lo_written:
            assert not lb.any(), f"{label}: the lo plane must stay as filled"
            lo = None
    assert np.isfinite(hi).all() and np.isfinite(c64).all()
    if lo is None:
        err, tol = np.abs(hi - c64), np.abs(c64) * (2.0 ** -11 + 2.0 ** -20) + 2.0 ** -25 + 2.0 ** -19
    else:
        with np.errstate(over="ignore"):
            half = np.spacing(np.abs(hi).astype(np.float16)).astype(np.float64) / 2
        n_bad = int((np.abs(lo) > half).sum())
        assert n_bad == 0, f"{label}: {n_bad} (hi, lo) pairs with |lo| above half the spacing of hi"
        err, tol = np.abs(hi + lo - c64), np.abs(c64) * (2.0 ** -21 + 2.0 ** -20) + 2.0 ** -24 + 2.0 ** -19
    n_bad = int((err > tol).sum())
    assert n_bad == 0, f"{label}: {n_bad} values off the generic body's output, worst {float((err - tol).max()):.3g} over the bound"


def _gemm_check(M, N, dev, sa, sw, label, expect=None, **kw):
    """one operand set through the epilogues that store split values: fp32 + split output together (the generic body),
    the split output alone (the straight-line body on interior tiles, which has no fp32 output: the expectation is the
    first launch's - bit for bit without GELU, _check_other_body with it), and - where `expect` is given - that fp32
    output is the passed-through matrix itself"""
    c = torch.full((M, N), float("nan"), device=dev)
    both = ops.SplitMat.empty(M, N, dev, zero=True)
    ops.gemm_nt_split(sa, sw, out=c, out_split=both, **kw)
    cn = _np(c)
    if expect is not None:
        assert _same(cn, expect), f"{label}: the fp32 output is not the matrix passed through"
    lo = not kw.get("hi_only", False)
    _compare(both, cn, f"{label}, fp32 + split output", lo_written=lo)
    if "res" not in kw or kw["res"] is None:
        alone = ops.SplitMat.empty(M, N, dev, zero=True)
        ops.gemm_nt_split(sa, sw, out_split=alone, want_f32=False, **kw)
        if kw.get("gelu"):
            _check_other_body(alone, cn, lo, f"{label}, split output alone")
        else:
            _compare(alone, cn, f"{label}, split output alone", lo_written=lo)
    return cn


@pytest.mark.parametrize("M,N", SPLIT_MN)
def test_gemm_epilogue_store(dev, M, N):
    """A = 0: gelu(0) + res = res and 0 + bias = bias exactly, so the residual carries the whole domain (NaN, inf and
    overflow included) and the bias its finite part through the interior and the edge body of every tile shape; then
    GELU on ordinary accumulators - a transcendental's result read by the mix instruction"""
    z, sw = _gemm_operands(M, N, dev, zero_a=True)
    res = S.domain_matrix(M, N, S.ALL_CLASSES, seed=M)
    rd = torch.from_numpy(res).to(dev)
    for gelu in (False, True):
        _gemm_check(M, N, dev, z, sw, f"gemm {M}x{N} res route, gelu {gelu}", expect=res, res=rd, gelu=gelu)
    bias = S.domain_matrix(1, N, S.FINITE_IN_RANGE, seed=N)
    _require(bias, S.FINITE_IN_RANGE, "gemm bias", chunks=N - (N - 1) // 32 * 32 >= 6)      # (one row: six classes need six columns)
    bd = torch.from_numpy(bias[0]).to(dev)
    _gemm_check(M, N, dev, z, sw, f"gemm {M}x{N} bias route", expect=np.broadcast_to(bias, (M, N)), bias=bd)
    sa, sw = _gemm_operands(M, N, dev, zero_a=False)
    b = (0.1 * torch.randn(N, generator=torch.Generator().manual_seed(N))).to(dev)
    out = _gemm_check(M, N, dev, sa, sw, f"gemm {M}x{N} gelu on random accumulators", bias=b, gelu=True)
    cls = S.classify(out.ravel()[:400000])
    assert (cls & S.LO_SUB).any() and (cls & S.HI_SUB).any()                # gelu's tail: tiny outputs
    # reduced precision: split rows whose lo plane is not written; plain rows where the wide form runs
    _gemm_check(M, N, dev, sa, sw, f"gemm {M}x{N} hi_only gelu", bias=b, gelu=True, hi_only=True)
    if ops.plain_ok(M, N, 64):
        z64, w64 = ops.split_f16(torch.zeros(M, 64, device=dev)), ops.split_f16(torch.randn(N, 64, device=dev), "auto")
        for kw in (dict(res=rd), dict(bias=b, gelu=True)):
            c = torch.full((M, N), float("nan"), device=dev)
            pl = ops.SplitMat.empty(M, N, dev, zero=True)
            ops.gemm_nt_split(z64, w64, out=c, out_split=pl, hi_only=True, out_plain=True, **kw)
            assert pl.plain
            _compare(pl, _np(c), f"gemm {M}x{N} plain output {sorted(kw)}")
            if "res" not in kw:
                alone = ops.SplitMat.empty(M, N, dev, zero=True)
                ops.gemm_nt_split(z64, w64, out_split=alone, want_f32=False, hi_only=True, out_plain=True, **kw)
                _check_other_body(alone, _np(c), False, f"gemm {M}x{N} plain output alone {sorted(kw)}")


@pytest.mark.parametrize("M,N", [(648, 360), (648, 1080), (100, 77), (648, 270)])
def test_small_gemm_epilogue_store(dev, M, N):
    """cra5_small_gemm_nt_split (scalar store per element, pad columns written by the kernel): the same A = 0 device"""
    z, sw = _gemm_operands(M, N, dev, zero_a=True)
    sa, _ = _gemm_operands(M, N, dev, zero_a=False)
    res = S.domain_matrix(M, N, S.ALL_CLASSES, seed=N)
    bias = S.domain_matrix(1, N, S.FINITE_IN_RANGE, seed=N + 1)
    rd, bd = torch.from_numpy(res).to(dev), torch.from_numpy(bias[0]).to(dev)
    b = (0.1 * torch.randn(N, generator=torch.Generator().manual_seed(N))).to(dev)
    for label, a_, kw, expect in (("res route", z, dict(res=rd), res), ("res route, gelu", z, dict(res=rd, gelu=True), res),
                                  ("bias route", z, dict(bias=bd), np.broadcast_to(bias, (M, N))),
                                  ("gelu on random accumulators", sa, dict(bias=b, gelu=True), None)):
        c = torch.full((M, N), float("nan"), device=dev)
        both = ops.SplitMat.empty(M, N, dev, zero=True)
        ops.small_gemm_nt_split(a_, sw, out=c, out_split=both, **kw)
        cn = _np(c)
        if expect is not None:
            assert _same(cn, expect), label
        _compare(both, cn, f"small gemm {M}x{N} {label}")
        alone = ops.SplitMat.empty(M, N, dev, zero=True)
        ops.small_gemm_nt_split(a_, sw, out_split=alone, want_f32=False, **kw)
        assert torch.equal(alone.data, both.data)


# ------------------------------------------------------------------------------------------------ attention


def _qkv(n, C, seed, dev):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(n, 3 * C, generator=g)
    qkv[:, 2 * C:] *= torch.logspace(-7, 0.5, C)[None]        # v columns from 1e-7 up: outputs down to the subnormal halves
    return qkv.to(dev), (0.1 * torch.randn(3 * C, generator=g)).to(dev)


@pytest.mark.parametrize("hd", [72, 64])
def test_window_attention_f32_store(dev, hd):
    H, W, heads = 18, 36, 2
    qkv, pad = _qkv(H * W, heads * hd, hd, dev)
    for wh, ww in ((H, W),):
        out = torch.full((H * W, heads * hd), float("nan"), device=dev)
        sm = ops.SplitMat.empty(H * W, heads * hd, dev, zero=True)
        ops.window_attention(qkv, pad, heads, H, W, wh, ww, out=out, out_split=sm)
        on = _np(out)
        assert (S.classify(on) & S.HI_SUB).any() and (S.classify(on) & S.LO_SUB).any()
        _compare(sm, on, f"window_attention_f32 hd {hd} window {wh}x{ww}")


@pytest.mark.parametrize("n,heads,hd", [(41, 2, 64), (17, 1, 72)])
def test_hyper_attention_store(dev, n, heads, hd):
    qkv, _ = _qkv(n, heads * hd, n, dev)
    out = torch.full((n, heads * hd), float("nan"), device=dev)
    sm = ops.SplitMat.empty(n, heads * hd, dev, zero=True)
    ops.hyper_attention(qkv, heads, out=out, out_split=sm)
    on = _np(out)
    assert (S.classify(on) & S.LO_SUB).any()
    _compare(sm, on, f"hyper_attention n = {n}, {heads} x {hd}")


def _hi_plane(sm):
    return sm.data.view(sm.rows, sm.Kp // 32, 2, 32)[:, :, 0].reshape(sm.rows, sm.Kp)


def _plain_rows_of(s):
    sm = ops.SplitMat.empty(s.rows, s.K, s.data.device, zero=True)
    sm.data[:, : sm.Kp] = _hi_plane(s)
    sm.plain = True
    return sm


@pytest.mark.parametrize("hi", [0, 1, 3])
@pytest.mark.parametrize("case", ["windowed", "global", "balanced"])
def test_window_attention_split_store(dev, case, hi):
    """cra5_window_attention_split[_ws] against the fp32 out of the same call: the packed store of the main kernel and the
    merge kernel's of the balanced schedule.  hi_only 1 (reduced precision, split rows): the consumers read the hi plane
    alone and the main kernel writes no lo half while the merge kernel does - a lo half is held to be EITHER as zero-filled
    OR split_ref's, nothing else; hi_only 3: plain rows."""
    H, W = 72, 144
    heads, (wh, ww) = (2, (24, 24)) if case == "windowed" else (16, (H, W))
    C = heads * 64
    qkv, pad = _qkv(H * W, C, heads, dev)
    qs, ps = ops.split_f16(qkv), ops.split_f16(pad.reshape(1, -1))
    if hi == 3:
        qs, ps = _plain_rows_of(qs), ps.plain_copy()
    ws = None
    if case == "balanced":
        ok, nb = ops.attention_balanced_plan(H * W, heads)
        assert ok, "no balanced plan on this device"
        ws = torch.zeros(max(nb, 16), dtype=torch.uint8, device=dev)
    out = torch.full((H * W, C), float("nan"), device=dev)
    sm = ops.SplitMat.empty(H * W, C, dev, zero=True)
    ops.window_attention_split(qs, ps, heads, H, W, wh, ww, out=out, out_split=sm, hi_only=bool(hi), workspace=ws,
                               balanced=(case == "balanced") or None)
    on = _np(out)
    assert sm.plain == (hi == 3) and (S.classify(on[:256]) & S.LO_SUB).any()
    label = f"window_attention_split {case}, hi_only {hi}"
    if hi != 1:
        _compare(sm, on, label)
        return
    raw = _u16(sm).copy()
    lo = raw.reshape(sm.rows, sm.Kp // 32, 2, 32)[:, :, 1]
    want_lo = S.expected_storage(on, sm.K, sm.Kp, False).reshape(sm.rows, sm.Kp // 32, 2, 32)[:, :, 1]
    untouched = lo == 0
    lo[untouched] = want_lo[untouched]
    S.compare_planes(raw, on, sm.K, sm.Kp, label=label)


# ------------------------------------------------------------------------------------------------ one store everywhere


def test_four_routes_store_identical_bits(dev):
    """the same fp32 matrix through cra5_split_f16, the LayerNorm beta route (one row per call), the generic im2col
    pass-through (1 x 1 patches) and the GEMM residual route: four bit-identical SplitMats"""
    M, N = 64, 360
    x = S.domain_matrix(M, N, S.FINITE_IN_RANGE, seed=99)
    x = np.where(x == 0, np.float32(0), x)                     # (-0 + 0 = +0 in the routes that add: keep zeros positive)
    xd = torch.from_numpy(x).to(dev)
    a = ops.SplitMat.empty(M, N, dev, zero=True)
    ops.split_f16(xd, out=a)
    _compare(a, x, "four routes: cra5_split_f16")
    b = ops.SplitMat.empty(M, N, dev, zero=True)
    rows_in = torch.randn(1, N, device=dev)
    zero = torch.zeros(N, device=dev)
    for r in range(M):
        one = ops.SplitMat(b.data[r:r + 1], 1, N, b.Kp)
        ops.layernorm(rows_in, zero, xd[r].contiguous(), 1e-6, out_split=one, want_f32=False)
    c = ops.SplitMat.empty(M, N, dev, zero=True)
    ops.im2col(xd.t().contiguous().view(N, 8, 8), 1, 1, 1, 1, out_split=c)          # token (i, j) = row 8 i + j, K = channels
    z, sw = ops.split_f16(torch.zeros(M, GK, device=dev)), ops.split_f16(torch.ones(N, GK, device=dev), "auto")
    d = ops.SplitMat.empty(M, N, dev, zero=True)
    ops.gemm_nt_split(z, sw, res=xd, out_split=d)
    for name, other in (("layernorm beta route", b), ("im2col pass-through", c), ("gemm res route", d)):
        _compare(other, x, f"four routes: {name}")
        assert torch.equal(other.data, a.data), name
