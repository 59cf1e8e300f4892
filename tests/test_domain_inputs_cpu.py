"""The bounds of tests/domain_helpers.py themselves, on the grids tests/test_domain_gpu.py runs: each is SOUND (the fp32
host restatement of the documented formula - and torch's fp32 CPU operator where it has the same operation - stays
within B / 2 on every element) and SENSITIVE (every listed wrong variant breaks B on at least one element).  A bound
that passes both is what the GPU tests assert, unchanged.  Also: the input builders deliver what they promise."""
import math

import numpy as np
import pytest
import torch

import domain_helpers as H
import exact_helpers as X
from oracle import torch_ref as R


def _err(got, ref):
    with np.errstate(all="ignore"):
        return np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64))


# ------------------------------------------------------------------------------------------------ GELU


@pytest.fixture(scope="module")
def gelu_grid():
    """every x of the GPU tests' two grids: the dense block (one period of rows and columns) and point list x rows"""
    a, b = H.gelu_dense_vectors(384, 256)
    dense = (a[:, None] + b[None, :]).astype(np.float32).reshape(-1)
    pts = (H.GELU_POINT_ROWS[:, None] + H.gelu_point_list()[None, :]).astype(np.float32).reshape(-1)
    x = np.concatenate([dense, pts])
    ref = H.gelu_ref64(x)
    return x, ref, H.gelu_bound(x, ref), np.isfinite(x)


def test_gelu_grids_are_what_they_claim():
    a, b = H.gelu_dense_vectors(192, 256)
    s64 = a.astype(np.float64)[:, None] + b.astype(np.float64)[None, :]
    s32 = (a[:, None] + b[None, :]).astype(np.float32)
    assert np.array_equal(s32.astype(np.float64), s64)                       # every sum exact
    flat = np.sort(s64.reshape(-1))
    assert flat[0] == -9.0 and flat[-1] == 9.0 - 3 * 2.0 ** -13 and np.all(np.diff(flat) == 3 * 2.0 ** -13)
    # a is exact in the split store: hi + lo reconstructs it, no f16 subnormal
    a_all, _ = H.gelu_dense_vectors(4224, 8)
    hi, lo = X.split_model(torch.from_numpy(a_all)[:, None])
    X.check_planes(torch.from_numpy(a_all)[:, None], hi, lo, 1.0, "dense a")
    rows = torch.from_numpy(H.GELU_POINT_ROWS)[:, None]
    X.check_planes(rows, *X.split_model(rows), 1.0, "point rows")
    pts = H.gelu_point_list()
    assert pts.size == 2 * 57 * 8 + 89 + 8 + 3 and np.isnan(pts[-3]) and pts[-2] == np.inf and pts[-1] == -np.inf
    assert np.nanmin(np.abs(pts[pts != 0])) == H.FLT_TRUE_MIN and np.signbit(pts[pts == 0]).sum() == 1
    tail = pts[(pts <= -9) & (pts >= -14.5) & (pts * 16 == np.round(pts * 16))]
    assert tail.min() == -14.5 and tail.size >= 89
    assert np.abs(H.gelu_point_list(f16_range=True, nonfinite=False)).max() == 65504.0


def test_gelu_fit_error_in_float64():
    """the documented fit: in float64 its |erfc error| is <= 8.3e-9 for t >= 0.88 and <= 7.3e-8 below (7.26e-8 at
    t = 0: the coefficients sum to 1 - 7.26e-8); at most 4.5e-4 relative between t = 3 / sqrt 2 and 6 / sqrt 2"""
    t = np.linspace(0, 10, 1000001)
    k = 1 / (1 + 0.4 * t)
    err = np.abs(np.exp(-t * t) * k * np.polyval(H.GELU_COEF, k) - H.erfc64(t))
    assert err[t >= 0.88].max() <= H.GELU_E_FIT
    assert 7.2e-8 < err.max() <= 7.3e-8 and err.argmax() == 0
    tail = (t >= 3 / math.sqrt(2)) & (t <= 6 / math.sqrt(2))
    assert (err[tail] / H.erfc64(t[tail])).max() < 4.6e-4


def test_gelu_bound_constants_are_the_derived_ones():
    """the two figures the derivation of c(t) quotes, evaluated: sensitivity x error of k <= 9, Horner condition <= 12"""
    t = np.linspace(0, 12, 120001)
    k = 1 / (1 + 0.4 * t)
    c = np.array(H.GELU_COEF)
    P, dP = np.polyval(c, k), np.polyval(np.polyder(c), k)
    S = np.abs(1 + k * dP / P)
    assert abs(S[0] - 2 / math.sqrt(math.pi) / 0.4) < 1e-3 and S.max() == S[0]
    assert (S * (3 * (1 - k) + 3)).max() <= 9
    p, partials = np.full_like(k, c[0]), np.zeros_like(k)
    for ci in c[1:]:
        p = p * k + ci
        partials += np.abs(p)
    assert ((partials + np.polyval(np.abs(c), k)) / P).max() <= 12
    assert (H.GELU_CA, H.GELU_CB) == (2 * (9 + 12 + 2 + 2), 36)


def test_gelu_bound_is_sound(gelu_grid):
    x, ref, B, fin = gelu_grid
    out = H.gelu_restated(x)
    r = H.ratio(_err(out, ref)[fin], B[fin])
    print(f"ERR gelu restatement: max |err| / B = {r.max():.3f} at x = {x[fin][r.argmax()]!r} ({int(fin.sum())} points)")
    assert r.max() <= 0.5
    H.gelu_exact_expectations(x, out, "restatement")


def test_gelu_bound_is_tight_where_it_matters(gelu_grid):
    """it holds [-4, -3] to a RELATIVE 1e-3 of |ref| and everything below to 4e-8 absolute (the E_fit term) - and
    torch's own fp32 GELU, the aggregate tests' yardstick, does not pass it on [-6, -3]"""
    x, ref, B, fin = gelu_grid
    near = fin & (x <= -3) & (x >= -4)
    assert (B[near] / np.abs(ref[near])).max() < 1e-3
    assert B[fin & (x < -4) & (x >= -9)].max() < 4e-8
    tail = fin & (x <= -3) & (x >= -6)
    tg = torch.nn.functional.gelu(torch.from_numpy(x)).numpy()
    assert H.ratio(_err(tg, ref)[tail], B[tail]).max() > 1


@pytest.mark.parametrize("variant", H.GELU_VARIANTS)
def test_gelu_bound_catches(gelu_grid, variant):
    x, ref, B, fin = gelu_grid
    r = H.ratio(_err(H.gelu_restated(x, variant), ref)[fin], B[fin])
    print(f"gelu {variant}: max |err| / B = {r.max():.3g}, {int((r > 1).sum())} elements outside B")
    assert r.max() > 1


def test_gelu_f32_engine_bound_is_sound(gelu_grid):
    x, ref, _, fin = gelu_grid
    B = H.gelu_f32_bound(x, ref)
    for name, out in (("restatement", H.gelu_f32_restated(x)),
                      ("torch fp32 gelu", torch.nn.functional.gelu(torch.from_numpy(x)).numpy())):
        r = H.ratio(_err(out, ref)[fin], B[fin])
        print(f"ERR gelu f32 engine, {name}: max |err| / B = {r.max():.3f} at x = {x[fin][r.argmax()]!r}")
        assert r.max() <= 0.5
        H.gelu_exact_expectations(x, out, name)
    # and it would notice the 0.5 dropped or the sign of erf flipped
    x32 = H.f32(x)
    with np.errstate(all="ignore"):
        erf = torch.erf(torch.from_numpy(x32 * np.float32(H.SQRT1_2))).numpy()
        for wrong in (x32 * (1 + erf), np.float32(0.5) * x32 * (1 - erf)):
            assert H.ratio(_err(wrong, ref)[fin], B[fin]).max() > 1


# ------------------------------------------------------------------------------------------------ LayerNorm


@pytest.fixture(scope="module")
def ln_cases():
    out = {}
    for D in H.LN_DIMS:
        x, ga, be, names = H.ln_inputs(D)
        B, y, mean, var, rstd = H.ln_bound(x, ga, be)
        out[D] = (x, ga, be, names, B.numpy(), y.numpy())
    return out


def test_ln_inputs_are_what_they_claim(ln_cases):
    for D, (x, ga, be, names, B, y) in ln_cases.items():
        assert x.shape == (15, D) and x.shape[0] % 4 != 0 and len(names) == 15 and names[:13] == list(H.LN_CLASSES)
        m, s = x.double().mean(1), x.double().std(1, unbiased=False)
        assert bool((x[4] == 300).all()) and bool((x[5] == -7.25).all()) and bool((x[6] == 0).all())
        assert float(x[10, 0]) == 1 and float(x[10].abs().sum()) == 1 and float(x[11, D - 1]) == 1
        assert float(x[9].max()) == 1e4 and float(x.abs().max()) <= 1e15
        assert float(x[12].abs().min()) > 9e5
        if D >= 144:
            assert 500 < float(m[1] / s[1]) < 2000 and 5000 < float(m[2] / s[2]) < 20000      # mean / std of 1e3, 1e4
            assert float(s[7]) ** 2 < 2e-2 * H.LN_EPS                                          # variance far below eps
        # a zero row's reference is beta, exactly
        assert np.array_equal(y[6], be.double().numpy())
    assert {H.ln_v4(D) for D in H.LN_DIMS} == {1, 2, 4, 8}
    assert [H.ln_v4(D) for D in (256, 260, 512, 516, 1024, 1028)] == [1, 2, 2, 4, 4, 8]


def test_ln_bound_is_sound(ln_cases):
    for D, (x, ga, be, names, B, y) in ln_cases.items():
        rest = H.ln_restated(x, ga, be)
        tor = torch.nn.functional.layer_norm(x, (D,), ga, be, H.LN_EPS).numpy()
        r1, r2 = H.ratio(_err(rest, y), B), H.ratio(_err(tor, y), B)
        print(f"ERR layernorm D={D}: restatement max |err| / B = {r1.max():.3f} ({names[int(r1.max(1).argmax())]}), "
              f"torch fp32 {r2.max():.3f} ({names[int(r2.max(1).argmax())]})")
        assert r1.max() <= 0.5 and r2.max() <= 0.5
        assert np.array_equal(rest[6], be.numpy())                       # zeros -> beta, bit for bit


def test_ln_bound_is_honest_about_conditioning(ln_cases):
    """the constant-300 row is allowed about c1 u 300 * 1000 |gamma|; a well-conditioned row about a hundred ulps of its output
    (c1 u max|x| rstd |gamma| = 26 u * 11 / 3)"""
    x, ga, be, names, B, y = ln_cases[1024]
    c1 = 2 * (4 + 9)
    want = c1 * H.U * 300 * H.LN_EPS ** -0.5 * ga.abs().double().numpy()
    assert np.all(B[4] >= want) and np.all(B[4] <= want + 4 * H.U * np.abs(y[4]) + 1e-12)
    assert np.median(B[0] / np.maximum(np.abs(y[0]), 1e-3)) < 256 * H.U


@pytest.mark.parametrize("variant", H.LN_VARIANTS)
def test_ln_bound_catches(ln_cases, variant):
    worst, caught = 0.0, []
    for D, (x, ga, be, names, B, y) in ln_cases.items():
        r = H.ratio(_err(H.ln_restated(x, ga, be, variant=variant), y), B)
        r = np.where(np.isnan(r), np.inf, r)                             # (a NaN output is outside every bound)
        if r.max() > 1:
            caught.append(D)
        worst = max(worst, float(r.max()))
    print(f"layernorm {variant}: max |err| / B = {worst:.3g}, caught at D in {caught}")
    assert caught
    if variant in ("one_pass_variance", "divide_by_D_minus_1", "eps_outside_sqrt"):
        assert caught == list(H.LN_DIMS)            # whatever the width
    else:                                           # the two that need pad lanes: every D below its template's width
        assert caught == [D for D in H.LN_DIMS if D != H.ln_v4(D) * 256]


def test_ln_one_pass_variance_fails_on_the_offset_rows(ln_cases):
    """the rows the issue is about: mean / std of 1e3 and 1e4 - and NOT the randn * 3 + 1.5 row the old test uses"""
    x, ga, be, names, B, y = ln_cases[1024]
    r = H.ratio(_err(H.ln_restated(x, ga, be, variant="one_pass_variance"), y), B)
    r = np.where(np.isnan(r), np.inf, r).max(1)
    assert r[1] > 1 and r[2] > 1 and r[0] <= 1


# ------------------------------------------------------------------------------------------------ GaussianConditional


@pytest.fixture(scope="module")
def gc_case():
    y, mu, s, q = H.gc_inputs(R.get_scale_table().numpy())
    return y, mu, s, q, H.gc_ref64(q, mu, s)


def test_gc_inputs_are_what_they_claim(gc_case):
    y, mu, s, q, ref = gc_case
    table = R.get_scale_table().numpy()
    assert y.size == 81 * 2000 and set(np.unique(q)) == set(range(-40, 41))
    assert np.array_equal(np.rint((y - mu).astype(np.float32)).astype(np.int32), q)
    assert np.abs(mu).max() <= 3 and s.max() <= 300 * (1 + 1e-6)
    per = s.reshape(81, -1)
    assert np.array_equal(per[:, : table.size], np.broadcast_to(table, (81, table.size)))
    assert np.array_equal(per[0, table.size: table.size + 3], H.f32([0.01, 0.05, 0.11]))
    clamped = ref["lik64"] < 1e-9
    assert 0.3 < clamped.mean() < 0.5 and (ref["lik64"] < 1e-6).mean() > 0.35
    # the bound is a RELATIVE one where the rate lives: a few 1e-5 of the likelihood down to the clamp
    small = (ref["lik64"] >= 1e-9) & (ref["lik64"] < 1e-6)
    assert (ref["B"][small] / ref["ref"][small]).max() < 2e-4


def test_gc_bound_is_sound(gc_case):
    y, mu, s, q, ref = gc_case
    out = H.gc_restated(q, mu, s)
    r = H.ratio(_err(out, ref["ref"]), ref["B"])
    print(f"ERR gaussian_conditional restatement (torch fp32 erfc): max |err| / B = {r.max():.3f}")
    assert r.max() <= 0.5
    deep = ref["lik64"] < 1e-9 * (1 - 1e-3)
    assert np.all(out[deep] == np.float32(1e-9))


@pytest.mark.parametrize("variant", H.GC_VARIANTS)
def test_gc_bound_catches(gc_case, variant):
    y, mu, s, q, ref = gc_case
    r = H.ratio(_err(H.gc_restated(q, mu, s, variant=variant), ref["ref"]), ref["B"])
    r = np.where(np.isnan(r), np.inf, r)
    print(f"gaussian_conditional {variant}: max |err| / B = {r.max():.3g}, {int((r > 1).sum())} elements outside B")
    assert r.max() > 1


def test_gc_old_absolute_tolerance_bounds_nothing_in_the_tail(gc_case):
    """why this bound exists: |d lik| < 2e-7 lets 1 - erf through on every element whose rate it decides"""
    y, mu, s, q, ref = gc_case
    wrong = H.gc_restated(q, mu, s, variant="one_minus_erf")
    small = ref["lik64"] < 1e-7
    assert _err(wrong, ref["ref"])[small].max() < 2e-7
    assert H.ratio(_err(wrong, ref["ref"])[small], ref["B"][small]).max() > 100


# ------------------------------------------------------------------------------------------------ the probe


def test_probe_positions_and_blocks():
    for n in H.PROBE_SIZES:
        pos = H.probe_positions(n)
        assert all(0 <= p < n for p in pos) and 0 in pos and n - 1 in pos
        if n > 256:
            assert {63, 64, 255, 256, n // 2, n - 2} <= set(pos)
    assert [H.probe_block_of(i) for i in (0, 255, 256, 65535, 65536, 65537)] == [0, 0, 1, 255, 0, 0]
