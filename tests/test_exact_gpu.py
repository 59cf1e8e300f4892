"""Exact-arithmetic tests of the matrix-core engines, per element (inputs and expectations: tests/exact_helpers.py).

GEMM family: operands on a grid where every product and every partial sum of every order is an exact fp32 number, so
the fp32 outputs are compared BIT FOR BIT with the three-product model hi.hi + hi.lo + lo.hi (hi.hi alone in the
reduced-precision mode) evaluated in float64 from the planes the kernels really read - whatever the tile shape, k-step
width, split-K or MFMA reduction order.  Attention: a uniform pattern that counts keys (pad tokens included) and a
permutation pattern that pins every (query, key) pairing; bounds derived next to each check, observed maxima printed.
A failure says where: tile row / column for the four tilings, or (window, head, query tile, key)."""
import numpy as np
import pytest
import torch

import exact_helpers as X
from cra5_amd import ops

pytestmark = pytest.mark.gpu


def _density(K):
    """share of non-zero operand elements that keeps sum_k |term| under 2^24 granules (asserted per case, not assumed)"""
    return 1.0 if K <= 1024 else 0.75 if K <= 4096 else 0.5 if K <= 8704 else 0.1


def _split_operands(M, N, K, dev, seed, lo=True):
    """A [M, K], W [N, K] on the exact grid, split on the device; the planes READ BACK from the SplitMats, checked."""
    a = X.grid_matrix(M, K, _density(K), seed, lo_shift=12).to(dev)
    w = X.grid_matrix(N, K, _density(K), seed + 1, lo_shift=12).to(dev)
    if not lo:
        a, w = torch.round(a), torch.round(w)
    sa, sw = ops.split_f16(a), ops.split_f16(w, "auto")
    pa, pw = sa.planes(), sw.planes()
    X.check_planes(a, pa[0], pa[1], 1.0, "A")
    X.check_planes(w, pw[0], pw[1], sw.scale_inv, "W")
    return a, w, sa, sw, pa, pw


def _epilogue_operands(M, N, dev, seed):
    return X.grid_vector(N, seed + 2).to(dev), X.grid_matrix(M, N, 1.0, seed + 3, lo_shift=12).to(dev)


def _hi_plane(sm):
    return sm.data.view(sm.rows, sm.Kp // 32, 2, 32)[:, :, 0].reshape(sm.rows, sm.Kp)


_plain_rows_of = X.plain_rows_of


def _check_split_output(out_s, e, label):
    """the split output holds 22 bits, the exact result may need 24"""
    err = float((out_s.to_float().double() - e).abs().max())
    assert err <= 2 ** -21 * float(e.abs().max()) + 2 ** -24, (label, err)


# ------------------------------------------------------------------------------------------------ exact-f32 GEMM


@pytest.mark.parametrize("M,N,K", [(128, 128, 32), (256, 384, 64), (648, 360, 360), (1000, 1080, 360), (10368, 1024, 1024),
                                   (333, 77, 52), (2048, 4096, 1024), (70, 8192, 360)])
def test_gemm_f32_exact(dev, M, N, K):
    """cra5_gemm_nt_f32 on the grid p + q 2^-6 (products: multiples of 2^-12, all four of them - this engine drops
    nothing): no epilogue, bias, bias + residual - zero differing elements."""
    a = X.grid_matrix(M, K, 1.0, 5 * M + N + K, lo_shift=6).to(dev)
    w = X.grid_matrix(N, K, 1.0, 5 * M + N + K + 1, lo_shift=6).to(dev)
    b, r = _epilogue_operands(M, N, dev, M + N + K)
    for epi in ("none", "bias", "bias_res"):
        e, g, worst = X.product_expectation(a, w, bias=b if epi != "none" else None, res=r if epi == "bias_res" else None)
        out = ops.gemm_nt(a, w, bias=b if epi != "none" else None, res=r if epi == "bias_res" else None)
        X.assert_exact(out, e, g, f"gemm_nt_f32 {M}x{N}x{K} {epi}")
    print(f"gemm_nt_f32 {M}x{N}x{K}: 0 differing elements (max sum |term| {worst:.3g} granules of {g!r})")


def test_gemm_f32_exact_strided_and_inplace_residual(dev):
    big = X.grid_matrix(300, 512, 1.0, 31, lo_shift=6).to(dev)
    a = big[:, 128:384]                                                  # lda = 512, K = 256
    w = X.grid_matrix(96, 256, 1.0, 32, lo_shift=6).to(dev)
    x = X.grid_matrix(300, 96, 1.0, 33, lo_shift=12).to(dev)
    e, g, _ = X.product_expectation(a.contiguous(), w, res=x)
    ops.gemm_nt(a, w, res=x, out=x)                                      # the residual aliases C
    X.assert_exact(x, e, g, "gemm_nt_f32 strided A, in-place residual")


# ------------------------------------------------------------------------------------------------ split-f16 GEMM

SPLIT_SHAPES = [(256, 256, 64), (10368, 1024, 1024), (2048, 4096, 1024), (1000, 360, 360), (333, 77, 52),
                (10368, 1024, 4096), (2048, 1024, 29480), (648, 8192, 360),
                # 1 / 2 / 3 / 5 k-steps of the big-tile main loop, ragged last tile rows / columns, both big tiles
                (2100, 2304, 32), (2100, 2304, 64), (4099, 1030, 96), (3000, 2050, 160)]


@pytest.mark.parametrize("M,N,K", SPLIT_SHAPES)
def test_gemm_split_three_product_model_exact(dev, M, N, K):
    """cra5_gemm_nt_split: no epilogue; bias + residual with the fp32 and the split output together; the residual
    aliasing C.  K = 29 480: the chained form (fp32 output only) AND the one-launch long-K form (split output)."""
    a, w, sa, sw, pa, pw = _split_operands(M, N, K, dev, 3 * M + N + K)
    b, r = _epilogue_operands(M, N, dev, M + N + K)
    e0, g, worst = X.three_product_expectation(pa, pw, sw.scale_inv)
    assert g == 2.0 ** -12
    X.assert_exact(ops.gemm_nt_split(sa, sw), e0, g, f"gemm_nt_split {M}x{N}x{K}, no epilogue")
    e1, g, worst = X.three_product_expectation(pa, pw, sw.scale_inv, bias=b, res=r)
    out_s = ops.SplitMat.empty(M, N, dev, zero=True)
    out = ops.gemm_nt_split(sa, sw, bias=b, res=r, out_split=out_s)
    X.assert_exact(out, e1, g, f"gemm_nt_split {M}x{N}x{K}, bias + res, fp32 + split output")
    _check_split_output(out_s, e1, (M, N, K))
    x = r.clone()
    ops.gemm_nt_split(sa, sw, bias=b, res=x, out=x)
    X.assert_exact(x, e1, g, f"gemm_nt_split {M}x{N}x{K}, bias + in-place residual")
    print(f"gemm_nt_split {M}x{N}x{K}: 0 differing elements in 3 launches (max sum |term| {worst:.3g} granules of {g!r})")


@pytest.mark.parametrize("M,N,K", [(256, 256, 64), (2100, 2304, 64), (10368, 1024, 64)])
def test_gemm_split_output_bit_exact_when_it_fits(dev, M, N, K):
    """lo planes zero, K = 64, integer bias: every output is an integer of <= 8 bits - the split output is bit-exact too"""
    a, w, sa, sw, pa, pw = _split_operands(M, N, K, dev, M + N, lo=False)
    assert float(pa[1].abs().max()) == 0.0 and float(pw[1].abs().max()) == 0.0
    b = torch.round(X.grid_vector(N, 5)).to(dev)
    e, g, _ = X.three_product_expectation(pa, pw, sw.scale_inv, bias=b)
    out_s = ops.SplitMat.empty(M, N, dev, zero=True)
    out = ops.gemm_nt_split(sa, sw, bias=b, out_split=out_s)
    X.assert_exact(out, e, g, f"gemm_nt_split {M}x{N}x{K} integers")
    X.assert_exact(out_s.to_float(), e, g, f"gemm_nt_split {M}x{N}x{K} integers, split output")


@pytest.mark.parametrize("M,N,K", [(256, 256, 64), (2048, 4096, 1024), (10368, 1024, 1024), (648, 360, 360), (2048, 2048, 96),
                                   (1100, 2304, 160), (2048, 1024, 8192 + 64 * 5), (1536, 1024, 29480)])
def test_gemm_hi_only_exact(dev, M, N, K):
    """CRA5_GEMM_HI_ONLY: the hi.hi sum alone, exactly - the lo planes are non-zero, so the mode reads none of them.
    Where the wide form runs: plain A / W / output rows too."""
    a, w, sa, sw, pa, pw = _split_operands(M, N, K, dev, M + 2 * N + K)
    assert float(pa[1].abs().max()) > 0 and float(pw[1].abs().max()) > 0
    b, r = _epilogue_operands(M, N, dev, M + N + K)
    e, g, worst = X.three_product_expectation(pa, pw, sw.scale_inv, hi_only=True, bias=b, res=r)
    assert g == 1.0 / 4096            # (the bias / residual granule; the hi.hi products are integers)
    X.assert_exact(ops.gemm_nt_split(sa, sw, bias=b, res=r, hi_only=True), e, g, f"gemm hi_only {M}x{N}x{K}")
    if ops.plain_ok(M, N, sa.Kp) and sa.Kp <= 8192:
        ppa, ppw = _plain_rows_of(sa), sw.plain_copy()
        for A_, W_ in ((ppa, ppw), (sa, ppw), (ppa, sw)):
            got_s = ops.SplitMat.empty(M, N, dev, zero=True)
            out = ops.gemm_nt_split(A_, W_, bias=b, res=r, hi_only=True, out_split=got_s, out_plain=True)
            X.assert_exact(out, e, g, f"gemm hi_only {M}x{N}x{K} plain A {A_.plain} / W {W_.plain}")
            # a plain output row holds f16(value): round-to-nearest of an exactly known number
            X.assert_exact(got_s.to_float(), e.float().half().double(), g, f"gemm hi_only {M}x{N}x{K} plain output")
    print(f"gemm hi_only {M}x{N}x{K}: 0 differing elements (max sum |term| {worst:.3g} granules)")


def test_gemm_wide_k_slice_equals_the_big_launch(dev):
    """CRA5_GEMM_WIDE_K on a 256 x 256 corner of a big problem: the big launch's slice - exactly, and both the exact
    hi.hi sum (on these inputs the order cannot matter: any difference is an indexing bug)."""
    M, N, K = 2048, 2048, 1024
    a, w, sa, sw, pa, pw = _split_operands(M, N, K, dev, 77)
    e, g, _ = X.three_product_expectation(pa, pw, sw.scale_inv, hi_only=True)
    big = ops.gemm_nt_split(sa, sw, hi_only=True)
    X.assert_exact(big, e, g, "gemm hi_only 2048x2048x1024")
    sa_c = ops.split_f16(a[300:556].contiguous())
    sw_c = ops.split_f16(w[1500:1756].contiguous(), sw.scale_inv ** -1)
    for A_, W_ in ((sa_c, sw_c), (_plain_rows_of(sa_c), sw_c.plain_copy())):
        corner = ops.gemm_nt_split(A_, W_, hi_only=True, wide_k=True)
        X.assert_exact(corner, e[300:556, 1500:1756], g, "gemm hi_only wide_k 256x256 corner")
        assert torch.equal(corner, big[300:556, 1500:1756])


@pytest.mark.parametrize("K", [64, 96])
@pytest.mark.parametrize("M,N", [(1920, 2176), (2048, 2048)])      # 255 and 256 128 x 128 tiles
def test_launcher_accepts_what_the_form_query_accepts(dev, M, N, K):
    """Plain operands in the reduced-precision mode, with and without CRA5_GEMM_WIDE_K, on both sides of the tile-count
    and Kp % 64 thresholds: where ops.gemm_form (cra5_gemm_split_form) refuses, the launcher raises CRA5_ERR_ARG and
    writes nothing; where it accepts, the launch is the exact hi.hi sum."""
    from cra5_amd._lib import Cra5Error
    a, w, sa, sw, pa, pw = _split_operands(M, N, K, dev, M + N + K)
    e, g, _ = X.three_product_expectation(pa, pw, sw.scale_inv, hi_only=True)
    ppa, ppw = _plain_rows_of(sa), sw.plain_copy()
    for wide in (False, True):
        flags = ops.GEMM_HI_ONLY | ops.GEMM_A_PLAIN | ops.GEMM_W_PLAIN | (ops.GEMM_WIDE_K if wide else 0)
        form = ops.gemm_form(M, N, sa.Kp, flags, True, False)
        # plain rows need 64-wide k-steps: Kp % 64 == 0 and (>= 256 tiles or the forced wide form)
        assert (form >= 0) == (sa.Kp % 64 == 0 and (wide or (M, N) == (2048, 2048))), (M, N, K, wide, form)
        out = torch.full((M, N), float("nan"), device=dev)
        if form < 0:
            assert form == ops.ERR_ARG
            with pytest.raises(Cra5Error) as ei:
                ops.gemm_nt_split(ppa, ppw, out=out, hi_only=True, wide_k=wide)
            assert ei.value.status == ops.ERR_ARG
            torch.cuda.synchronize()
            assert bool(torch.isnan(out).all()), (M, N, K, wide)
        else:
            assert form & ops.FORM_K64 and form & ops.FORM_PLAIN and not form & ops.FORM_CHAINED
            assert form & ops.FORM_TILE == 256          # M >= 1024, N >= 2048: the 256-row tile, forced wide or not
            timer, ops.TIMER = ops.TIMER, ops.KernelTimer()
            try:
                ops.gemm_nt_split(ppa, ppw, out=out, hi_only=True, wide_k=wide)
                booked = ops.TIMER.summary()
            finally:
                ops.TIMER = timer
            X.assert_exact(out, e, g, f"gemm hi_only plain {M}x{N}x{K} wide_k={wide}")
            # the timer books a launch by the kernel it runs: 255 tiles with CRA5_GEMM_WIDE_K is a big-tile launch
            assert list(booked) == ["gemm_nt_split"] and booked["gemm_nt_split"]["launches"] == 1


# ------------------------------------------------------------------------------------------------ small-M GEMM


@pytest.mark.parametrize("M,N,K", [(648, 1080, 360), (648, 360, 360), (648, 1440, 360), (648, 360, 1440), (648, 360, 4096),
                                   (648, 256, 360), (648, 256, 256), (162, 432, 144), (648, 8192, 360), (100, 77, 52),
                                   (2000, 3000, 96)])
def test_small_gemm_split_exact(dev, M, N, K):
    """cra5_small_gemm_nt_split, every dispatch branch (1 / 4 / 8-way in-block split-K, 32 / 64 / 128-column wave
    tiles): the split-K partial sums are exact like every other order; pad columns of the split output zero."""
    a, w, sa, sw, pa, pw = _split_operands(M, N, K, dev, M + 5 * N + K)
    b, r = _epilogue_operands(M, N, dev, M + N + K)
    e0, g, _ = X.three_product_expectation(pa, pw, sw.scale_inv)
    X.assert_exact(ops.small_gemm_nt_split(sa, sw), e0, g, f"small gemm {M}x{N}x{K}, no epilogue")
    e1, g, worst = X.three_product_expectation(pa, pw, sw.scale_inv, bias=b, res=r)
    out_s = ops.SplitMat.empty(M, N, dev)
    out_s.data.fill_(0x7e00)                                            # f16 NaN pattern: the kernel writes the pad
    out = ops.small_gemm_nt_split(sa, sw, bias=b, res=r, out_split=out_s)
    X.assert_exact(out, e1, g, f"small gemm {M}x{N}x{K}, bias + res")
    _check_split_output(out_s, e1, (M, N, K))
    if out_s.Kp > N:
        raw = out_s.data.view(torch.float16).view(M, out_s.Kp // 32, 2, 32)
        assert float(raw.permute(0, 1, 3, 2).reshape(M, out_s.Kp, 2)[:, N:, :].float().abs().max()) == 0.0
    print(f"small gemm {M}x{N}x{K}: 0 differing elements (max sum |term| {worst:.3g} granules)")


def test_small_gemm_unembed_store_exact(dev):
    """the '(p1 p2 c)' un-embed store fused into the small GEMM: every pixel of the [512, 72, 144] image, bit for bit"""
    Hz, Wz, p, cout, d = 18, 36, 4, 512, 360
    a, w, sa, sw, pa, pw = _split_operands(Hz * Wz, p * p * cout, d, dev, 91)          # w rows in (c, p1, p2) order
    e, g, _ = X.three_product_expectation(pa, pw, sw.scale_inv)
    exp = e.view(Hz, Wz, cout, p, p).permute(2, 0, 3, 1, 4).reshape(cout * Hz * p, Wz * p)
    img = torch.full((cout, Hz * p, Wz * p), float("nan"), device=dev)
    ops.small_gemm_nt_split(sa, sw, out=img, unembed=(Hz, Wz, p, p))
    X.assert_exact(img.view(cout * Hz * p, Wz * p), exp, g, "small gemm un-embed store", gemm_tiles=False,
                   locate=lambda r, c, _=None: f"channel {r // (Hz * p)}, token ({r % (Hz * p) // p}, {c // p})")


# ------------------------------------------------------------------------------------------------ fused un-embed


@pytest.mark.parametrize("C,K,hi", [(8, 128, False), (159, 1024, False), (268, 1024, False), (8, 1024, True)])
def test_fused_unembed_exact(dev, C, K, hi):
    """cra5_gemm_nt_split_unembed on the 72 x 144 grid: the exact overlap-add of the three-product model, de-normalised
    with std a power of two and mean an integer (exact), every pixel - rows 0, 10 t and 720 included."""
    H, W, kh, kw, Hp, Wp = 721, 1440, 11, 10, 72, 144
    a, w, sa, sw, pa, pw = _split_operands(Hp * Wp, C * kh * kw, K, dev, 7 * C + K)
    e, g, worst = X.three_product_expectation(pa, pw, sw.scale_inv, hi_only=hi)
    mean = (torch.arange(C) % 7 - 3).float().to(dev)
    std = (2.0 ** (torch.arange(C) % 3)).float().to(dev)
    nb = ops.unembed_side_bytes(C, H, W, kh, kw, 10, 10)
    where = lambda r, c, _=None: f"channel {r // H}, image row {r % H} (token row {r % H // 10}), token column {c // 10}"
    for m_, s_ in ((None, None), (mean, std)):
        exp = X.unembed_expectation(e, C, Hp, Wp, kh, kw, mean=m_, std=s_)
        side = torch.full((nb // 4,), float("nan"), device=dev)
        out = torch.full((C, H, W), float("nan"), device=dev)
        ops.gemm_unembed(sa, sw, C, H, W, kh, kw, 10, 10, side, mean=m_, std=s_, out=out, hi_only=hi)
        X.assert_exact(out.view(C * H, W), exp.view(C * H, W), g, f"fused un-embed C = {C}, K = {K}, hi_only {hi}, "
                       f"de-normalised {m_ is not None}", locate=where, gemm_tiles=False)
    print(f"fused un-embed C = {C}, K = {K}: 0 differing pixels of {C * H * W} (max sum |term| {worst:.3g} granules)")


# ------------------------------------------------------------------------------------------------ attention

WINDOWED = [(72, 144, (24, 24)), (72, 144, (12, 48)), (72, 144, (48, 12)),      # none / none / bottom padding (production)
            (72, 100, (24, 24)), (70, 140, (24, 24))]                            # right padding only / both sides
HYPER = [(648, 5, 72), (100, 3, 72), (41, 2, 64), (17, 1, 72)]


def _run_split(qkv, pad, heads, H, W, wh, ww, dev, hi, balanced=False):
    """cra5_window_attention_split[_ws]: hi 0 (fp32-accurate), 1 (reduced precision, split rows), 3 (plain rows)"""
    N, C = H * W, qkv.shape[1] // 3
    qs, ps = ops.split_f16(qkv.to(dev)), ops.split_f16(pad.reshape(1, -1).to(dev))
    if hi == 3:
        qs, ps = _plain_rows_of(qs), ps.plain_copy()
    ws = None
    if balanced:
        ok, nb = ops.attention_balanced_plan(N, heads)
        if not ok:
            pytest.skip("no balanced plan on this device")
        ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=dev).fill_(0xFF)
    out = torch.full((N, C), float("nan"), device=dev)
    out_s = ops.SplitMat.empty(N, C, dev, zero=True)
    ops.window_attention_split(qs, ps, heads, H, W, wh, ww, out=out, out_split=out_s, hi_only=bool(hi), workspace=ws,
                               balanced=balanced or None)
    return out, out_s.to_float()


def _run_f32(qkv, pad, heads, H, W, wh, ww, dev):
    N, C = H * W, qkv.shape[1] // 3
    out = torch.full((N, C), float("nan"), device=dev)
    out_s = ops.SplitMat.empty(N, C, dev, zero=True)
    ops.window_attention(qkv.to(dev), pad.to(dev), heads, H, W, wh, ww, out=out, out_split=out_s)
    return out, out_s.to_float()


def _run_hyper(qkv, heads, dev):
    n, C = qkv.shape[0], qkv.shape[1] // 3
    out = torch.full((n, C), float("nan"), device=dev)
    out_s = ops.SplitMat.empty(n, C, dev, zero=True)
    ops.hyper_attention(qkv.to(dev), heads, out=out, out_split=out_s)
    return out, out_s.to_float()


def _ulp_tol(exp, n):
    return torch.from_numpy(np.spacing(np.abs(exp.float().cpu().numpy()))).double().to(exp.device) * n


def _check_uniform(out, out_s, exp, wins, heads, hd, hi, label):
    """Every p is 1, O an exact integer sum, l the token count: one reciprocal (1 ulp), one multiply, on the balanced
    path one multiply-add per merged key range -> <= 4 ulp of the expected fp32 value, in every mode.  The split output
    adds its 22-bit store (2^-21 relative + 2^-24); the reduced-precision modes store the f16 hi plane only (2^-10)."""
    exp = exp.to(out.device)
    loc = X.attention_locator(wins, heads, hd)
    X.assert_exact(out, exp, 1.0 / wins.L, label + " fp32 out", tol=_ulp_tol(exp, 4), locate=loc, gemm_tiles=False)
    tol_s = exp.abs() * 2.0 ** -10 if hi else _ulp_tol(exp, 4) + exp.abs() * 2.0 ** -21 + 2.0 ** -24
    X.assert_exact(out_s, exp, 1.0 / wins.L, label + " split out", tol=tol_s, locate=loc, gemm_tiles=False)
    print(f"{label}: max {float(X.ulps(out, exp).max()):.2f} ulp (bound 4)")


def _check_permutation(out, out_s, exp, wins, heads, hd, info, mode, label):
    """out_i = the v row of the one key that matches query i (the others hold < 2^-25 of l).  Exact-f32 kernels: 4 ulp.
    Split kernels: p goes through a 22-bit hi / lo pair -> 2^-21 relative.  Reduced precision: p and the reference point
    are f16 -> 2^-10 relative (v itself is exact in f16)."""
    exp = exp.to(out.device)
    loc = X.attention_locator(wins, heads, hd, info)
    tol = {"f32": _ulp_tol(exp, 4), "split": exp.abs() * 2.0 ** -21, "hi": exp.abs() * 2.0 ** -10}[mode]
    X.assert_exact(out, exp, 1.0, label + " fp32 out", tol=tol, locate=loc, gemm_tiles=False)
    tol_s = exp.abs() * 2.0 ** -10 if mode == "hi" else tol + exp.abs() * 2.0 ** -21 + 2.0 ** -24
    X.assert_exact(out_s, exp, 1.0, label + " split out", tol=tol_s, locate=loc, gemm_tiles=False)
    rel = float(((out.double() - exp).abs() / exp.abs()).max())
    print(f"{label}: max relative error {rel:.3g} = 2^{np.log2(max(rel, 1e-300)):.1f}, max {float(X.ulps(out, exp).max()):.2f} ulp; "
          f"u drawn {info['draws']} time(s), score gap {info['gap_log2']:.1f} log2 units")


@pytest.mark.parametrize("H,W,ws", WINDOWED + [(72, 144, None)])
def test_window_attention_f32_exact_patterns(dev, H, W, ws):
    heads, hd = 2, 64
    wh, ww = ws or (H, W)
    qkv, pad, exp, wins = X.uniform_case(H, W, wh, ww, heads, hd, seed=H + W + wh)
    out, out_s = _run_f32(qkv, pad, heads, H, W, wh, ww, dev)
    _check_uniform(out, out_s, exp, wins, heads, hd, 0, f"uniform, window_attention_f32 {H}x{W} {ws}")
    qkv, pad, exp, wins, info = X.permutation_case(H, W, wh, ww, heads, hd, seed=H + W + wh, device=dev)
    out, out_s = _run_f32(qkv, pad, heads, H, W, wh, ww, dev)
    _check_permutation(out, out_s, exp, wins, heads, hd, info, "f32", f"permutation, window_attention_f32 {H}x{W} {ws}")


def test_window_attention_f32_exact_patterns_hd72_ragged(dev):
    """648 keys: the ragged last key tile of the exact-f32 kernel (keys past the window masked, not counted)"""
    H, W, heads, hd = 18, 36, 2, 72
    qkv, pad, exp, wins = X.uniform_case(H, W, H, W, heads, hd, seed=1)
    out, out_s = _run_f32(qkv, pad, heads, H, W, H, W, dev)
    _check_uniform(out, out_s, exp, wins, heads, hd, 0, "uniform, window_attention_f32 18x36 hd 72")
    qkv, pad, exp, wins, info = X.permutation_case(H, W, H, W, heads, hd, seed=1, device=dev)
    out, out_s = _run_f32(qkv, pad, heads, H, W, H, W, dev)
    _check_permutation(out, out_s, exp, wins, heads, hd, info, "f32", "permutation, window_attention_f32 18x36 hd 72")


@pytest.mark.parametrize("hi", [0, 1, 3])
@pytest.mark.parametrize("H,W,ws", WINDOWED)
def test_window_attention_split_exact_patterns(dev, H, W, ws, hi):
    heads, hd = 2, 64
    wh, ww = ws
    qkv, pad, exp, wins = X.uniform_case(H, W, wh, ww, heads, hd, seed=H + W + wh)
    out, out_s = _run_split(qkv, pad, heads, H, W, wh, ww, dev, hi)
    _check_uniform(out, out_s, exp, wins, heads, hd, hi, f"uniform, window_attention_split hi_only {hi} {H}x{W} {ws}")
    qkv, pad, exp, wins, info = X.permutation_case(H, W, wh, ww, heads, hd, seed=H + W + wh, device=dev)
    out, out_s = _run_split(qkv, pad, heads, H, W, wh, ww, dev, hi)
    _check_permutation(out, out_s, exp, wins, heads, hd, info, "hi" if hi else "split",
                       f"permutation, window_attention_split hi_only {hi} {H}x{W} {ws}")


_GLOBAL_CASE = {}


@pytest.mark.parametrize("hi", [0, 1, 3])
@pytest.mark.parametrize("balanced", [False, True])
def test_global_attention_split_exact_patterns(dev, hi, balanced):
    """the whole 72 x 144 grid as one window, 16 heads (the model's shape): the plain launch and the balanced one, whose
    key-split tokens are merged from 2-3 key ranges"""
    H, W, heads, hd = 72, 144, 16, 64
    qkv, pad, exp, wins = X.uniform_case(H, W, H, W, heads, hd, seed=7)
    out, out_s = _run_split(qkv, pad, heads, H, W, H, W, dev, hi, balanced)
    _check_uniform(out, out_s, exp, wins, heads, hd, hi, f"uniform, global attention hi_only {hi} balanced {balanced}")
    if "perm" not in _GLOBAL_CASE:                       # (one draw of u for the six launches: 16 heads x 10 368^2 scores)
        _GLOBAL_CASE["perm"] = X.permutation_case(H, W, H, W, heads, hd, seed=7, device=dev)
    qkv, pad, exp, wins, info = _GLOBAL_CASE["perm"]
    out, out_s = _run_split(qkv, pad, heads, H, W, H, W, dev, hi, balanced)
    _check_permutation(out, out_s, exp, wins, heads, hd, info, "hi" if hi else "split",
                       f"permutation, global attention hi_only {hi} balanced {balanced}")


@pytest.mark.parametrize("n,heads,hd", HYPER)
def test_hyper_attention_exact_patterns(dev, n, heads, hd):
    """cra5_hyper_attention_f32: keys split over the 4 waves of a block and merged through LDS; ragged query / key tiles"""
    qkv, pad, exp, wins = X.uniform_case(1, n, 1, n, heads, hd, seed=n)
    out, out_s = _run_hyper(qkv, heads, dev)
    _check_uniform(out, out_s, exp, wins, heads, hd, 0, f"uniform, hyper_attention n = {n}, {heads} x {hd}")
    qkv, pad, exp, wins, info = X.permutation_case(1, n, 1, n, heads, hd, seed=n, device=dev)
    out, out_s = _run_hyper(qkv, heads, dev)
    _check_permutation(out, out_s, exp, wins, heads, hd, info, "f32", f"permutation, hyper_attention n = {n}, {heads} x {hd}")
