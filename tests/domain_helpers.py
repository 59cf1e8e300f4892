"""Per-element forward-error bounds for the GELU epilogues, LayerNorm, the GaussianConditional likelihood and the
finiteness probe: input builders, float64 references, the bounds B, and fp32 host restatements of the documented
formulas (with the wrong variants a bound has to catch) - shared by tests/test_domain_gpu.py (the kernels) and
tests/test_domain_inputs_cpu.py (the bounds themselves: sound and sensitive).

Every reference is a float64 evaluation from the exact fp32 inputs the kernel saw; every assertion is
|got - ref64| <= B per element.  The constants of each B are operation counts derived in the docstring of its
function (u = 2^-24, the fp32 unit roundoff; a correctly rounded operation has relative error <= u, a 1-ulp device
function <= 2 u), then doubled: the host restatement (exact 1/x, exp2, libm erfc) has to stay within B / 2, the
device's rcp / exp2 / erfcf differ from the host's by about an ulp each.  No constant comes from a run of a kernel.

The restatements use numpy float32 arithmetic (every operation rounded once); fma(a, b, c) is a float64 product
(exact) plus c rounded to float64 and then to fp32 - a double rounding that differs from a true fma on about one
operand in 2^29, by half an ulp.  Nothing here calls a product kernel."""
import math

import numpy as np
import torch

U = 2.0 ** -24
FLT_MIN = 2.0 ** -126
FLT_TRUE_MIN = 2.0 ** -149
F32 = np.float32
SQRT1_2 = 0.70710678118654752440


def f32(x):
    return np.asarray(x, dtype=np.float32)


def fma32(a, b, c):
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def erfc64(t):
    """float64 erfc of a numpy array (std::erfc through torch: relative accuracy in the tail)"""
    return torch.special.erfc(torch.from_numpy(np.ascontiguousarray(t, dtype=np.float64))).numpy()


def Phi64(a):
    return 0.5 * erfc64(-np.asarray(a, np.float64) * math.sqrt(0.5))


def ratio(err, B):
    """|err| / B per element with 0 / 0 = 0 (an exact result under a zero bound) and x / 0 = inf"""
    err, B = np.asarray(err, np.float64), np.asarray(B, np.float64)
    with np.errstate(all="ignore"):
        return np.where(err == 0, 0.0, err / B)


# ------------------------------------------------------------------------------------------------ GELU

GELU_E_FIT = 8.3e-9          # documented |erfc error| of the degree-7 fit (csrc/gemm_split_f16.hip)
GELU_COEF = (0.03080804832279682, -0.3524225652217865, 1.0205539464950562, -0.7088391780853271, 0.6733116507530212,
             0.0958886444568634, 0.2406993806362152)
GELU_VARIANTS = ("coef_0.6733", "sqrt_half_0.70710", "log2e_1.44269", "branch_swapped", "half_dropped", "one_minus_both")
GELU_CA, GELU_CB = 2 * 25, 36


def gelu_dense_vectors(M, N):
    """(a [M], b [N]) of the dense grid: a steps by 3 * 2^-5 from -9 (period 384: up to 27 - 3/32), b by 3 * 2^-13
    (period 256).  a has <= 11 significant bits above 2^-5 and is exact in the split store; every a + b is a multiple of
    2^-13 below 32: exact in fp32.  Rows 0..191 x columns 0..255 are one point every 3 * 2^-13 = 3.7e-4 over [-9, 9)."""
    a = -9.0 + (np.arange(M) % 384) * (3.0 / 32)
    b = (np.arange(N) % 256) * (3.0 / 8192)
    return f32(a), f32(b)


def gelu_point_list(f16_range=False, nonfinite=True):
    """The bias values of the second grid: log-spaced +-2^e (1 + j/8), e = -40..16; the far negative tail -9 .. -14.5
    in steps of 1/16 (v_exp_f32 underflows from about -13.2 on); +-0, +-FLT_TRUE_MIN, +-65504, +-1e30; NaN, +inf, -inf.
    f16_range: only |x| <= 65504 (a route whose only output is the split store; beyond it the store poisons)."""
    e = np.arange(-40, 17, dtype=np.float64)[:, None]
    mag = (2.0 ** e * (1 + np.arange(8) / 8.0)[None, :]).reshape(-1)
    tail = -9.0 - np.arange(89) / 16.0
    special = np.array([0.0, -0.0, FLT_TRUE_MIN, -FLT_TRUE_MIN, 65504.0, -65504.0, 1e30, -1e30])
    pts = f32(np.concatenate([mag, -mag, tail, special]))
    if f16_range:
        pts = pts[np.abs(pts) <= 65504.0]
    if nonfinite:
        pts = np.concatenate([pts, f32([np.nan, np.inf, -np.inf])])
    return pts


GELU_POINT_ROWS = f32([0.0, 1.0, -1.0, -12.0])     # a of the second grid, cycled over the rows: x = fl32(a + point)


def gelu_ref64(x):
    """x * 0.5 erfc(-x / sqrt 2) in float64 from fp32 x (numpy)"""
    x = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        return x * 0.5 * erfc64(-x * math.sqrt(0.5))


def gelu_bound(x, ref):
    """B(x) = |x| (E_fit/2 + [x >= 0] 2^-24 + c(t) u h(x)) + 2 u |ref| + 2^-126,  t = |x|/sqrt 2, h = erfc(t)/2,
    c(t) = 50 + 36 t^2.

    The kernel computes H ~ h as 0.5 p(k) k exp2(-t^2 log2 e), k = rcp(1 + 0.4 t), and returns x H (x < 0) or
    x (1 - H).  Relative error of H, in units of u:
      exp2 argument: t = fl(|x| fl(1/sqrt 2)) 2 u; t t 2 * 2 + 1; times fl(log2 e) 1 + 1: 7 u relative on an argument of
        size t^2 log2 e, i.e. 7 t^2 u relative on the power - the t^2 part of c;
      the power itself (1 ulp device function) 2;
      k: t 2 and fl(0.4) 1, both scaled by 0.4 t k = 1 - k, the fma 1, rcp (1 ulp) 2: 3 (1 - k) + 3, times the
        sensitivity S = |d ln(k p(k)) / d ln k| (2.82 at t = 0, from erfcx'(0) = -2/sqrt pi, falling towards 1): the
        product peaks at 8.75 (t = 0.51): 9;
      Horner: (sum |coefficient| k^i + sum |partial result|) / p(k) <= 11.6: 12;
      the two products by k and by the power: 2.
    25 + 7 t^2, doubled (module docstring): 50 + 14 t^2.  (test_domain_inputs_cpu.py evaluates S and the Horner
    condition in float64.)  The t^2 coefficient is then WIDENED to 36, for soundness and for no other reason: between
    x = -4 and -3 the fit's own error - deterministic, the same on every machine - reaches 7.3e-9 of the documented
    8.3e-9, the restatement's error there is 0.61 of the E_fit term alone, and c(t) u h has to carry the rest of the
    factor 2.  Around H: the fit itself, E_fit / 2 absolute on H (the documented figure holds for t >= 0.88; below it the
    fit is off by up to 7.3e-8, at t = 0, which the c(t) u h term - 1.5e-6 there - covers 20 times over);
    fl(1 - H), half an ulp of a number in [1/2, 1] = 2^-25, on the x >= 0 side only; the final product, u |ref|; both
    doubled.  Underflow: v_exp_f32 returns no subnormal, so a power below 2^-126 is lost; it carries
    |x| 0.5 p k < 0.03 * 14.5 < 1 there: 2^-126 absolute, which also covers the rounding of a subnormal product.
    Non-finite x: NaN (not compared)."""
    x = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        t = np.abs(x) * math.sqrt(0.5)
        h = 0.5 * erfc64(t)
        c = GELU_CA + GELU_CB * t * t
        ch = np.where(h > 0, c * h, 0.0)              # (t^2 overflows for no fp32 x; 0 * big stays 0)
        return np.abs(x) * (GELU_E_FIT / 2 + (x >= 0) * 2.0 ** -24 + ch * U) + 2 * U * np.abs(ref) + FLT_MIN


def gelu_split_store_term(ref):
    """what the split store adds when the output is read back from (hi, lo): 22 bits kept, plus half an f16 subnormal"""
    return 2.0 ** -21 * np.abs(ref) + 2.0 ** -24


def gelu_restated(x, variant=None):
    """gelu_erf of csrc/gemm_split_f16.hip and csrc/hyper.hip, operation by operation in fp32 (exact 1/x and exp2 in
    place of v_rcp_f32 / v_exp_f32); `variant`: one of GELU_VARIANTS, the wrong forms the bound has to catch."""
    assert variant is None or variant in GELU_VARIANTS
    x = f32(x)
    c0 = F32(0.70710) if variant == "sqrt_half_0.70710" else F32(SQRT1_2)
    l2 = F32(1.44269) if variant == "log2e_1.44269" else F32(1.4426950408889634)
    coef = [F32(c) for c in GELU_COEF]
    if variant == "coef_0.6733":
        coef[4] = F32(0.6733)
    with np.errstate(all="ignore"):
        t = np.abs(x) * c0
        k = (F32(1.0) / fma32(F32(0.4), t, F32(1.0))).astype(np.float32)
        p = np.full_like(t, coef[0])
        for c in coef[1:]:
            p = fma32(p, k, c)
        arg = -(t * t) * l2
        e = np.exp2(arg.astype(np.float64)).astype(np.float32)
        half_erfc = p * k * e if variant == "half_dropped" else F32(0.5) * p * k * e
        pos = (x >= 0)
        if variant == "branch_swapped":
            pos = ~pos
        phi = F32(1.0) - half_erfc
        if variant != "one_minus_both":
            phi = np.where(pos, phi, half_erfc)
        return (x * phi).astype(np.float32)


GELU_F32_CE = 12


def gelu_f32_bound(x, ref):
    """The exact-f32 engine (csrc/gemm_f32.hip) computes 0.5 x (1 + erff(x / sqrt 2)): its own form,
        B(x) = 12 u |x| + 2 u |ref| + 2^-126.
    Absolute error of (1 + erf), in u (an ulp of a number in [1/2, 1) is u): the argument fl(x fl(1/sqrt 2)) is off by
    2 u relative, worth 2 z erf'(z) <= 0.97 -> 1; erff allowed 4 ulp -> 4; the addition, half an ulp of a number below 2
    -> 1 (it is the cancellation in 1 + erf that leaves an ABSOLUTE error); together 6, times |x| / 2; the products
    0.5 x (exact) and x (...): u |ref|.  3 u |x| + u |ref|, doubled (module docstring): 6 u |x| + 2 u |ref|.  The
    |x| coefficient is then WIDENED to 12 for the soundness witness alone: torch's fp32 CPU GELU evaluates erf with a
    vectorised polynomial of about 5 u absolute error (8.5e-7 on the output at x = -2.96) and has to fit into B / 2.
    There is NO relative accuracy in the negative tail: below x = -5.4, 1 + erff is 0 or an ulp of 1 and the whole of
    ref (|x| h(x) < u |x|) is error - this bound allows that, the polynomial engines' bound does not."""
    x = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        return GELU_F32_CE * U * np.abs(x) + 2 * U * np.abs(ref) + FLT_MIN


def gelu_f32_restated(x):
    x = f32(x)
    with np.errstate(all="ignore"):
        z = torch.from_numpy(np.ascontiguousarray(x * F32(SQRT1_2)))
        return (F32(0.5) * x * (F32(1.0) + torch.erf(z).numpy())).astype(np.float32)


def gelu_exact_expectations(x, out, label, saturates=True):
    """The properties that hold bit for bit (numpy fp32 arrays of one shape): x >= 9 -> out == x; gelu(+-0) is a zero;
    the sign; NaN / +inf / -inf -> non-finite (-inf -> NaN)."""
    x, out = f32(x), f32(out)
    big = x >= 9.0
    if saturates:
        assert np.array_equal(out[big & np.isfinite(x)], x[big & np.isfinite(x)]), f"{label}: x >= 9 must return x"
    assert np.all(out[x == 0] == 0), f"{label}: gelu(+-0) must be a zero"
    fin = np.isfinite(x)
    assert np.all(out[fin & (x < 0)] <= 0), f"{label}: a positive output for a negative x"
    assert np.all(out[fin & (x > 0)] >= 0), f"{label}: a negative output for a positive x"
    assert not np.any(np.isfinite(out[~fin])), f"{label}: a non-finite accumulator came out finite"
    assert np.all(np.isnan(out[np.isneginf(x)])), f"{label}: gelu(-inf) must be NaN"
    assert np.all(np.isfinite(out[fin])), f"{label}: a finite x gave a non-finite output"


# ------------------------------------------------------------------------------------------------ LayerNorm

LN_DIMS = (4, 144, 256, 260, 360, 512, 516, 1024, 1028, 2048)
LN_EPS = float(np.float32(1e-6))        # what the kernel receives: the fp32 rounding of 1e-6
LN_VARIANTS = ("one_pass_variance", "divide_by_D_minus_1", "eps_outside_sqrt", "tail_in_variance", "mean_over_padded_width")
LN_CLASSES = ("randn*3+1.5", "randn+1e3", "randn+1e4", "randn*1e-3+300", "const 300", "const -7.25", "zeros", "randn*1e-4",
              "randn*1e4", "randn, one 1e4", "one-hot 0", "one-hot D-1", "alternating 1e6 + randn")


def ln_v4(D):
    return 1 if D <= 256 else 2 if D <= 512 else 4 if D <= 1024 else 8


def ln_inputs(D, seed=0):
    """(x [15, D], gamma [D], beta [D], class name per row): the 13 row classes plus two randn rows of padding (15 rows:
    not a multiple of the 4 rows of a block)."""
    g = torch.Generator().manual_seed(1000 + D + seed)
    r = lambda: torch.randn(D, generator=g)
    alt = torch.where(torch.arange(D) % 2 == 0, 1e6, -1e6)
    hot0, hot1 = torch.zeros(D), torch.zeros(D)
    hot0[0], hot1[D - 1] = 1.0, 1.0
    outl = r()
    outl[D // 3] = 1e4
    rows = [r() * 3 + 1.5, r() + 1e3, r() + 1e4, r() * 1e-3 + 300, torch.full((D,), 300.0), torch.full((D,), -7.25),
            torch.zeros(D), r() * 1e-4, r() * 1e4, outl, hot0, hot1, alt + r(), r(), r() * 0.5 - 2]
    x = torch.stack(rows).float().contiguous()
    assert float(x.abs().max()) <= 1e15
    names = list(LN_CLASSES) + ["pad randn", "pad randn*0.5-2"]
    return x, r().float(), r().float(), names


def ln_ref64(x, gamma, beta, eps=LN_EPS):
    """float64 two-pass LayerNorm of fp32 tensors -> (y, mean, var, rstd), all float64 torch tensors"""
    x64 = x.double()
    mean = x64.mean(1, keepdim=True)
    var = ((x64 - mean) ** 2).mean(1, keepdim=True)
    rstd = (var + eps) ** -0.5
    return (x64 - mean) * rstd * gamma.double() + beta.double(), mean, var, rstd


def ln_bound(x, gamma, beta, eps=LN_EPS):
    """B_j = |gamma_j| rstd (c1 u max|x| + c2 u |x_j - mean| + c3 u |x_j - mean| var / (var + eps))
             + 2 u |y_j - beta_j| + 2 u |y_j|,    c1 = 2 (V4 + 9), c2 = 12, c3 = V4 + 12.

    mean: a lane adds V4 float4s, each as (x + y) + (z + w) (depth 2), into its sum (V4), six butterfly steps follow and
      the division by D: V4 + 9 roundings, each at most u times a partial sum of absolute values <= D max|x|; the error
      of the mean is <= (V4 + 9) u max|x| and shifts every x_j - mean by that much: c1.  (Honest about conditioning: a
      constant 300 row may move by c1 u 300 rstd |gamma| = c1 u 300 * 1000 |gamma|.)
    x_j - mean, times rstd, times gamma: 3 u; rstd = 1 / sqrt(var + eps) with correctly rounded division and square root:
      u each, and the addition's u halved by the root: 3 more: c2 = 6.
    var: every (x - mean) u, squared 2 u, the square's own rounding u, the sum of squares (all positive: relative)
      V4 + 8 deep like the mean's, the division u: V4 + 12 relative on var, that is (V4 + 12) / 2 on rstd through
      var / (var + eps): c3.  (The mean's error enters var only in second order: sum (x - m')^2 = sum (x - m)^2 + D dm^2.)
    The product by gamma leaves u |y_j - beta_j|, the addition of beta u |y_j|: the form's last two terms.  Every
    count is doubled (module docstring).  Returns (B, y, mean, var, rstd) in float64."""
    y, mean, var, rstd = ln_ref64(x, gamma, beta, eps)
    D = x.shape[1]
    v4 = ln_v4(D)
    c1, c2, c3 = 2 * (v4 + 9), 12, v4 + 12
    d = (x.double() - mean).abs()
    xmax = x.double().abs().amax(1, keepdim=True)
    B = gamma.double().abs() * rstd * (c1 * U * xmax + c2 * U * d + c3 * U * d * var / (var + eps)) \
        + 2 * U * (y - beta.double()).abs() + 2 * U * y.abs()
    return B, y, mean, var, rstd


def _wave_sum(v):
    """the xor butterfly of wave_sum(): v [..., 64] fp32 -> what lane 0 holds"""
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = (v + v[..., lanes ^ off]).astype(np.float32)
    return v[..., 0]


def ln_restated(x, gamma, beta, eps=LN_EPS, variant=None):
    """layernorm_kernel<V4> of csrc/elementwise.hip in its own order, fp32 (numpy; no contraction into fmas): row in
    registers as V4 float4 per lane, column (i * 64 + lane) * 4, zeros past D; two passes; xor butterfly."""
    assert variant is None or variant in LN_VARIANTS
    x = f32(x.numpy() if torch.is_tensor(x) else x)
    ga, be = f32(gamma.numpy() if torch.is_tensor(gamma) else gamma), f32(beta.numpy() if torch.is_tensor(beta) else beta)
    rows, D = x.shape
    v4 = ln_v4(D)
    W = v4 * 256
    xp = np.zeros((rows, W), np.float32)
    xp[:, :D] = x
    v = xp.reshape(rows, v4, 64, 4)
    live = (np.arange(W) < D).reshape(v4, 64, 4)[None, :, :, 0]          # c < D, per (i, lane)
    eps = F32(eps)
    with np.errstate(all="ignore"):
        s = np.zeros((rows, 64), np.float32)
        for i in range(v4):
            s = s + ((v[:, i, :, 0] + v[:, i, :, 1]) + (v[:, i, :, 2] + v[:, i, :, 3]))
        n_mean = F32(W if variant == "mean_over_padded_width" else D)
        mean = (_wave_sum(s) / n_mean).astype(np.float32)[:, None]
        q = np.zeros((rows, 64), np.float32)
        if variant == "one_pass_variance":
            for i in range(v4):
                q = q + ((v[:, i, :, 0] * v[:, i, :, 0] + v[:, i, :, 1] * v[:, i, :, 1])
                         + (v[:, i, :, 2] * v[:, i, :, 2] + v[:, i, :, 3] * v[:, i, :, 3]))
            var = (_wave_sum(q) / F32(D)).astype(np.float32)[:, None] - mean * mean
        else:
            for i in range(v4):
                a, b, c, d = (v[:, i, :, j] - mean for j in range(4))
                term = (a * a + b * b) + (c * c + d * d)
                if variant != "tail_in_variance":
                    term = np.where(live[:, i, :], term, F32(0.0))
                q = q + term
            var = (_wave_sum(q) / F32(D - 1 if variant == "divide_by_D_minus_1" else D)).astype(np.float32)[:, None]
        if variant == "eps_outside_sqrt":
            rstd = F32(1.0) / (np.sqrt(var) + eps)
        else:
            rstd = F32(1.0) / np.sqrt(var + eps)
        out = (x - mean) * rstd * ga[None, :] + be[None, :]
    return out.astype(np.float32)


# ------------------------------------------------------------------------------------------------ GaussianConditional

GC_VARIANTS = ("sqrt_half_0.70710", "one_minus_erf", "half_before_abs", "scale_bound_not_applied")
GC_SCALE_BOUND = 0.11
GC_LIK_BOUND = 1e-9
GC_C, GC_CP = 2 * 8, 2 * 4


def gc_inputs(scale_table, per_q=2000, seed=0):
    """(y, mu, scale, q) fp32 / int numpy arrays, flat: q in -40..40, per_q (mean, scale) pairs each.  Means uniform in
    [-3, 3]; y = fl(q + mu) moved a few ulps towards either side (never near the +-1/2 rounding edge).  Scales: the
    whole scale table, the values under the bound (0.01, 0.05, 0.11), the rest log-uniform in [0.11, 300]."""
    rng = np.random.default_rng(77 + seed)
    table = f32(scale_table)
    fixed = np.concatenate([table, f32([0.01, 0.05, 0.11])])
    assert per_q > fixed.size
    ys, mus, ss, qs = [], [], [], []
    for q in range(-40, 41):
        mu = f32(rng.uniform(-3, 3, per_q))
        s = f32(np.exp(rng.uniform(math.log(0.11), math.log(300.0), per_q)))
        s[: fixed.size] = fixed
        y = (F32(q) + mu).astype(np.float32)
        y = (y + y * f32(rng.integers(-3, 4, per_q)) * F32(2.0 ** -22)).astype(np.float32)   # |offset| <= 3 * 2^-22 |y|
        ys.append(y), mus.append(mu), ss.append(s), qs.append(np.full(per_q, q, np.int32))
    y, mu, s, q = (np.concatenate(t) for t in (ys, mus, ss, qs))
    assert np.array_equal(np.rint((y - mu).astype(np.float32)).astype(np.int32), q)      # rintf(y - mu) == q
    return y, mu, s, q


def gc_ref64(q, mu, scale, scale_bound=GC_SCALE_BOUND, lik_bound=GC_LIK_BOUND):
    """The two plain IEEE steps yh = fl(q + mu), v = |fl(yh - mu)| in fp32, then float64:
    lik64 = Phi((1/2 - v)/s) - Phi((-1/2 - v)/s), s = max(scale, fl32(scale_bound)).  Returns a dict of numpy arrays:
    yh (fp32), lik64 (unclamped), ref = max(lik64, fl32(lik_bound)) and the bound B.

    B = c u (Phi(a_up) + Phi(a_lo)) + c' u (phi(a_up) |a_up| + phi(a_lo) |a_lo|) + u ref,  c = 16, c' = 8
    (phi the normal density).  Each Phi is 0.5 erfcf(-fl(1/sqrt 2) a), a = fl(fl(+-1/2 - v) / s): erfcf to 4 ulp (the
    figure HIP documents for it) is 8 u relative: c; the argument carries the subtraction, the division, the constant
    and the product, 4 u relative, worth 4 u phi(a) |a| on Phi: c'; the halving is exact, the final subtraction leaves
    u lik, and max(., bound) is 1-Lipschitz.  c and c' doubled (module docstring)."""
    mu, scale = f32(mu), f32(scale)
    yh = (f32(q) + mu).astype(np.float32)
    v = np.abs((yh - mu).astype(np.float32)).astype(np.float64)
    s = np.maximum(scale, F32(scale_bound)).astype(np.float64)
    a_up, a_lo = (0.5 - v) / s, (-0.5 - v) / s
    P_up, P_lo = Phi64(a_up), Phi64(a_lo)
    lik64 = P_up - P_lo
    ref = np.maximum(lik64, float(F32(lik_bound)))
    dens = lambda a: np.exp(-0.5 * a * a) / math.sqrt(2 * math.pi)
    B = GC_C * U * (P_up + P_lo) + GC_CP * U * (dens(a_up) * np.abs(a_up) + dens(a_lo) * np.abs(a_lo)) + U * ref
    return dict(yh=yh, lik64=lik64, ref=ref, B=B)


def gc_restated(q, mu, scale, scale_bound=GC_SCALE_BOUND, lik_bound=GC_LIK_BOUND, variant=None):
    """gaussian_conditional_kernel's likelihood in fp32 on the host (torch's CPU erfc for erfcf)"""
    assert variant is None or variant in GC_VARIANTS
    mu, scale = f32(mu), f32(scale)
    c0 = F32(0.70710) if variant == "sqrt_half_0.70710" else F32(SQRT1_2)
    erf = lambda z, f: f(torch.from_numpy(np.ascontiguousarray(z, dtype=np.float32))).numpy()

    def phi(u):
        z = -c0 * u
        if variant == "one_minus_erf":
            return F32(0.5) * (F32(1.0) - erf(z, torch.erf))
        return F32(0.5) * erf(z, torch.erfc)

    with np.errstate(all="ignore"):
        s = scale if variant == "scale_bound_not_applied" else np.maximum(scale, F32(scale_bound))
        yh = (f32(q) + mu).astype(np.float32)
        d = (yh - mu).astype(np.float32)
        if variant == "half_before_abs":
            up, lo = phi(np.abs(F32(0.5) - d) / s), phi(-np.abs(F32(-0.5) - d) / s)
            # (|1/2 - d| and -|-1/2 - d|: the +-1/2 taken inside the absolute value)
        else:
            v = np.abs(d)
            up, lo = phi((F32(0.5) - v) / s), phi((F32(-0.5) - v) / s)
        return np.maximum((up - lo).astype(np.float32), F32(lik_bound))


# ------------------------------------------------------------------------------------------------ the probe

PROBE_SIZES = (1, 255, 256, 257, 65535, 65536, 65537, 3 * 65536 + 5)


def probe_positions(n, seed=0):
    """indices at which a non-finite value is planted: 0, 63, 64, 255, 256, n/2, n-2, n-1 where they exist, plus three
    seeded random ones"""
    rng = np.random.default_rng(n + seed)
    pos = [p for p in (0, 63, 64, 255, 256, n // 2, n - 2, n - 1) if 0 <= p < n]
    pos += [int(p) for p in rng.integers(0, n, 3)]
    return sorted(set(pos))


def probe_block_of(i):
    """the block (= partial) that reads sampled element i: 256 blocks of 256 threads, grid stride"""
    return (i // 256) % 256
