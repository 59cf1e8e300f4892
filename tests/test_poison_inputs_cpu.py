"""The helpers of tests/test_poison_gpu.py, on the CPU: the expected sets E (built from the geometry alone) equal the
non-finite set of a float64 torch evaluation of the same operation with a NaN in the poisoned operand; a bare +-inf in a
K element leaves both row classes populated; the site lists name every structural role; the checker catches a laundered
element, a leaked NaN and a changed low bit, and says where."""
import numpy as np
import pytest
import torch

import exact_helpers as X
import patch_geometry_helpers as G
import poison_helpers as P
import softmax_helpers as S

# (label, case key, heads, hd, waves per work-group of each engine that runs the case, roles the sites must cover)
WINDOW_CASES = [(f"{H}x{W} {ws}", ("win", H, W, ws), 2, 64, (4,),
                 P.PADDED_ROLES if (H % ws[0] or W % ws[1]) else P.WINDOW_ROLES | {P.Q_OTHER_WIN}) for H, W, ws in S.WINDOWED]
WINDOW_CASES.append(("global plain", ("global",), 2, 64, (12,), P.WINDOW_ROLES))
F32_WINDOW_CASES = [("f32 20x44 (24, 24) hd 64", ("win",) + S.F32_CASES[0], 2, 64, (6,), P.PADDED_ROLES),
                    ("f32 18x36 (18, 36) hd 72", ("win",) + S.F32_CASES[1], 2, 72, (4,), P.WINDOW_ROLES | {P.D_TAIL})]


def _small_balanced():
    """a balanced plan in small: 56 wave-tiles on 4 slots - 48 full ones, 8 key-split ones merged from 4 pieces"""
    return S.build(32, 56, 32, 56, 2, 64, seed=3, sites=S.balanced_sites(56, 4))


@pytest.mark.parametrize("label,key,heads,hd,nws,roles", WINDOW_CASES + F32_WINDOW_CASES, ids=lambda v: v if isinstance(v, str) else None)
def test_attention_expected_sets_equal_the_float64_nonfinite_set(label, key, heads, hd, nws, roles):
    qkv, pad, wins, _ = S.case(*key)
    for nw in nws:
        sites = P.attention_sites(wins, heads, hd, nw)
        assert P.roles_of(sites) == roles, (label, sorted(P.roles_of(sites) ^ roles))
        for site in sites:
            q2, p2 = P.poisoned(qkv, pad, site, P.NAN, heads, hd)
            assert int(torch.isnan(q2).sum()) + int(torch.isnan(p2).sum()) == 1
            got = torch.isnan(X.attention_float64(q2, p2, wins, heads))
            E = P.attention_expected(wins, heads, hd, site)
            assert torch.equal(got, E), (label, site.name, int(got.sum()), int(E.sum()))
            if site.operand == "q":
                A = P.wave_block(wins, heads, hd, site)
                assert bool((A & E).sum() == E.sum()) and int(A.sum()) <= 32 * hd
                assert len({int(wins.win_of[r]) for r in A.any(1).nonzero().reshape(-1).tolist()}) == 1


def test_balanced_expected_sets_equal_the_float64_nonfinite_set_of_the_piecewise_evaluation():
    qkv, pad, wins, _ = _small_balanced()
    heads, hd, groups = 2, 64, 4
    tile0, grps = S.bal_cuts(56, groups)
    assert tile0 == 48 and [len(p) for _, p in grps] == [4] and grps[0][0] == 8
    clean = P.balanced_float64(qkv, wins, heads, groups)
    ref = X.attention_float64(qkv, pad, wins, heads)
    assert float((clean - ref).abs().max()) < 1e-9                        # the piecewise evaluation IS the attention
    sites = P.attention_sites(wins, heads, hd, 12, groups=groups)
    assert P.roles_of(sites) == P.BALANCED_ROLES, sorted(P.roles_of(sites) ^ P.BALANCED_ROLES)
    for site in sites:
        q2, _ = P.poisoned(qkv, pad, site, P.NAN, heads, hd)
        got = torch.isnan(P.balanced_float64(q2, wins, heads, groups))
        assert torch.equal(got, P.attention_expected(wins, heads, hd, site)), site.name


@pytest.mark.parametrize("n,heads,hd", S.HYPER)
def test_hyper_expected_sets_equal_the_float64_nonfinite_set(n, heads, hd):
    qkv, pad, _, _ = S.case("hyper", n, heads, hd)
    wins, sites = P.hyper_sites(n, heads, hd)
    for site in sites:
        q2, p2 = P.poisoned(qkv, pad, site, P.NAN, heads, hd)
        got = torch.isnan(X.attention_float64(q2, p2, wins, heads))
        assert torch.equal(got, P.attention_expected(wins, heads, hd, site)), site.name


def test_hyper_sites_name_every_role():
    roles = set()
    for n, heads, hd in S.HYPER:
        roles |= P.roles_of(P.hyper_sites(n, heads, hd)[1])
    assert roles == P.HYPER_ROLES, sorted(roles ^ P.HYPER_ROLES)


def _class_conditions(label, qkv, pad, wins, heads, hd, sites, family, values):
    n = 0
    for site in sites:
        if site.operand not in ("k", "pad_k"):
            continue
        assert site.d in P.random_sign_features(hd, wins.L), (label, site.name)
        for value in values:
            q2, p2 = P.poisoned(qkv, pad, site, value, heads, hd)
            mand, either, drop = P.classify(q2, p2, wins, heads, hd, site, family)
            affected = np.zeros(qkv.shape[0], bool)
            affected[P._reader_rows(wins, site)] = True
            assert not (mand & either).any() and np.array_equal(mand | either, affected), (label, site.name, value)
            assert mand.sum() * 4 >= affected.sum(), (label, site.name, value, int(mand.sum()), int(affected.sum()))
            assert either.any() and drop.any(), (label, site.name, value)
            n += 1
    return n


@pytest.mark.parametrize("label,key,heads,hd,nws,roles", WINDOW_CASES, ids=lambda v: v if isinstance(v, str) else None)
def test_bare_inf_keys_leave_both_row_classes_populated_reduced_precision(label, key, heads, hd, nws, roles):
    """hi_only 1 / 3: 70 000 is stored as +inf, -70 000 as -inf, with no lo plane beside it"""
    qkv, pad, wins, _ = S.case(*key)
    assert _class_conditions(label, qkv, pad, wins, heads, hd, P.attention_sites(wins, heads, hd, nws[0]), "hi",
                             (70000.0, -70000.0, P.INF)) >= 9


@pytest.mark.parametrize("label,key,heads,hd,nws,roles", F32_WINDOW_CASES, ids=lambda v: v if isinstance(v, str) else None)
def test_bare_inf_keys_leave_both_row_classes_populated_f32(label, key, heads, hd, nws, roles):
    qkv, pad, wins, _ = S.case(*key)
    assert _class_conditions(label, qkv, pad, wins, heads, hd, P.attention_sites(wins, heads, hd, nws[0]), "f32",
                             (P.INF, -P.INF)) >= 6


@pytest.mark.parametrize("n,heads,hd", S.HYPER)
def test_bare_inf_keys_leave_both_row_classes_populated_hyper(n, heads, hd):
    qkv, pad, _, _ = S.case("hyper", n, heads, hd)
    wins, sites = P.hyper_sites(n, heads, hd)
    assert _class_conditions(f"hyper {n}", qkv, pad, wins, heads, hd, sites, "hyper", (P.INF, -P.INF)) >= 4


def test_bare_inf_keys_leave_both_row_classes_populated_balanced():
    b = S.BALANCED
    qkv, pad, wins, _ = S.case("balanced")
    sites = P.attention_sites(wins, b["heads"], 64, 12, groups=b["groups"])
    assert P.roles_of(sites) == P.BALANCED_ROLES, sorted(P.roles_of(sites) ^ P.BALANCED_ROLES)
    assert _class_conditions("balanced", qkv, pad, wins, b["heads"], 64, sites, "hi", (70000.0, -70000.0, P.INF)) >= 18


def test_a_poison_in_the_split_store_is_nan_in_every_product():
    """fp32-accurate engines: hi = +-inf, lo = -+inf (NaN for a non-finite input): hi + lo is NaN, and so is every product
    sum that reads the pair - no classification there; the control value stays finite"""
    for _, v in P.F16_POISONS:
        assert bool(torch.isnan(P.stored(torch.tensor([v]), "split")).all())
        hi, lo = X.split_model(torch.tensor([v]))
        for other in (0.0, 1.0, -3.0):
            assert bool(torch.isnan(hi * other + lo * other))
    assert float(P.stored(torch.tensor([P.F16_CONTROL]), "split")) == 65504.0 + 15.0
    assert float(P.stored(torch.tensor([P.F16_CONTROL]), "hi")) == 65504.0
    assert [float(P.stored(torch.tensor([v]), "hi")) for v in (70000.0, -70000.0)] == [P.INF, -P.INF]


# ------------------------------------------------------------------------------------------------ GEMM family


GEMM_SHAPES = [((256, 256, 96), (64, 64), P.GEMM_ROLES), ((2048, 2048, 360), (256, 256), P.GEMM_ROLES),
               ((4224, 1024, 96), (192, 256), P.GEMM_ROLES), ((648, 360, 360), (64, 64), P.GEMM_RAGGED_ROLES),
               ((100, 77, 144), (64, 64), P.GEMM_RAGGED_ROLES), ((1000, 1080, 360), (128, 128), P.GEMM_RAGGED_ROLES)]


@pytest.mark.parametrize("shape,tile,roles", GEMM_SHAPES)
def test_gemm_sites_name_every_role(shape, tile, roles):
    M, N, K = shape
    sites = P.gemm_sites(M, N, K, *tile)
    assert P.roles_of(sites) == roles, sorted(P.roles_of(sites) ^ roles)
    assert all(0 <= s.row < (M if s.operand == "a" else N) and 0 <= s.k < K for s in sites)


def test_gemm_expected_sets_equal_the_float64_nonfinite_set():
    M, N, K = 100, 77, 144
    g = torch.Generator().manual_seed(0)
    a, w = torch.randn(M, K, generator=g).double(), torch.randn(N, K, generator=g).double()
    for site in P.gemm_sites(M, N, K, 64, 64):
        a2, w2 = a.clone(), w.clone()
        (a2 if site.operand == "a" else w2)[site.row, site.k] = P.NAN
        assert torch.equal(torch.isnan(a2 @ w2.t()), P.gemm_expected(M, N, site)), site.name


def test_unembed_expected_set_equals_the_float64_nonfinite_set():
    """the fold indicator against the overlap-add of a float64 column matrix with one NaN token row: the token's 11 x 10
    patch in every channel, seam rows included"""
    C, Hp, Wp, K = 2, 20, 16, 16
    g = torch.Generator().manual_seed(1)
    a, w = torch.randn(Hp * Wp, K, generator=g).double(), torch.randn(C * 110, K, generator=g).double()
    sites = P.unembed_sites(Hp, Wp, K)
    assert P.roles_of(sites) == P.UNEMBED_ROLES and P.roles_of(P.unembed_sites(72, 144, 128)) == P.UNEMBED_ROLES
    for site in sites:
        a2 = a.clone()
        a2[site.row, site.k] = P.NAN
        got = torch.isnan(G.col2im_reference(a2 @ w.t(), C, Hp, Wp))
        E = P.unembed_expected(C, Hp, Wp, site)
        assert torch.equal(got, E), site.name
        i, j = site.row // Wp, site.row % Wp
        box = torch.zeros_like(E)
        box[:, 10 * i:10 * i + 11, 10 * j:10 * j + 10] = True
        assert torch.equal(E, box)


# ------------------------------------------------------------------------------------------------ the checker


def _simulated():
    qkv, pad, wins, _ = S.case("win", *S.WINDOWED[1])
    heads, hd = 2, 64
    sites = P.attention_sites(wins, heads, hd, 4)
    clean = X.attention_float64(qkv, pad, wins, heads).float()
    return wins, heads, hd, sites, clean


def test_the_checker_accepts_the_prescribed_output_and_catches_its_mutants():
    wins, heads, hd, sites, clean = _simulated()
    loc = X.attention_locator(wins, heads, hd)
    for site in sites:
        E = P.attention_expected(wins, heads, hd, site)
        good = torch.where(E, torch.full_like(clean, P.NAN), clean)
        n = P.check(clean, good, E, site, 70000.0, "simulated", locate=loc)
        assert n == int(E.sum())
        r, c = (int(v) for v in E.nonzero()[len(E.nonzero()) // 2])
        outside = (~E).nonzero()
        ro, co = (int(v) for v in outside[len(outside) // 3])
        # a laundered element: the clean value where a non-finite one is due
        bad = good.clone()
        bad[r, c] = clean[r, c]
        with pytest.raises(P.PoisonMismatch) as ei:
            P.check(clean, bad, E, site, 70000.0, "simulated", locate=loc)
        msg = str(ei.value)
        assert "LAUNDERED" in msg and site.name in msg and f"operand {site.operand}" in msg and f"element ({r}, {c})" in msg
        assert f"head {c // hd}" in msg
        # a NaN outside E
        bad = good.clone()
        bad[ro, co] = P.NAN
        with pytest.raises(P.PoisonMismatch) as ei:
            P.check(clean, bad, E, site, 70000.0, "simulated", locate=loc)
        msg = str(ei.value)
        assert "LEAKED" in msg and site.name in msg and f"operand {site.operand}" in msg and f"element ({ro}, {co})" in msg
        # one low bit outside E
        bad = good.clone()
        bad.view(torch.int32)[ro, co] ^= 1
        with pytest.raises(P.PoisonMismatch) as ei:
            P.check(clean, bad, E, site, 70000.0, "simulated", locate=loc)
        msg = str(ei.value)
        assert "CHANGED" in msg and site.name in msg and f"operand {site.operand}" in msg and f"element ({ro}, {co})" in msg


def test_the_checker_on_split_planes_the_relaxed_block_and_the_either_rows():
    wins, heads, hd, sites, clean = _simulated()
    site = next(s for s in sites if s.operand == "q")
    E, A = P.attention_expected(wins, heads, hd, site), P.wave_block(wins, heads, hd, site)
    hi, lo = X.split_model(clean)
    g_hi, g_lo = torch.where(E, torch.full_like(hi, P.INF), hi), torch.where(E, torch.full_like(lo, -P.INF), lo)
    P.check((hi, lo), (g_hi, g_lo), E, site, P.INF, "planes")
    bad_lo = g_lo.clone()
    ro, co = (int(v) for v in (~E).nonzero()[7])
    bad_lo[ro, co] += 2.0 ** -24                                          # the lo plane alone: hi + lo rounds it away or not
    with pytest.raises(P.PoisonMismatch, match="CHANGED"):
        P.check((hi, lo), (g_hi, bad_lo), E, site, P.INF, "planes")
    # the wave block: other bits are accepted inside it, a NaN is not, and nothing outside it
    soft = (A & ~E).nonzero()
    rs, cs = (int(v) for v in soft[3])
    moved = torch.where(E, torch.full_like(clean, P.NAN), clean)
    moved.view(torch.int32)[rs, cs] ^= 1
    with pytest.raises(P.PoisonMismatch, match="CHANGED"):
        P.check(clean, moved, E, site, P.NAN, "block")
    P.check(clean, moved, E, site, P.NAN, "block", allow=A)
    moved[rs, cs] = P.NAN
    with pytest.raises(P.PoisonMismatch, match="LEAKED"):
        P.check(clean, moved, E, site, P.NAN, "block", allow=A)
    # either rows: non-finite or within the bound; mandatory rows: non-finite
    ksite = next(s for s in sites if s.operand == "k")
    E = P.attention_expected(wins, heads, hd, ksite)
    rows = E.any(1).nonzero().reshape(-1)
    either = torch.zeros_like(E)
    either[rows[::2]] = E[rows[::2]]
    ref, B = clean.double() + 1.0, torch.full_like(clean, 0.5, dtype=torch.float64)
    out = torch.where(E & ~either, torch.full_like(clean, P.NAN), torch.where(either, (ref + 0.25).float(), clean))
    P.check(clean, out, E, ksite, P.INF, "either", either=either, bound=(ref, B))
    P.check(clean, torch.where(E, torch.full_like(clean, P.NAN), clean), E, ksite, P.INF, "either", either=either, bound=(ref, B))
    with pytest.raises(P.PoisonMismatch, match="outside the softmax bound"):
        P.check(clean, out, E, ksite, P.INF, "either", either=either, bound=(ref, B / 4))
    r, c = (int(v) for v in (E & ~either).nonzero()[5])
    out[r, c] = 1.0
    with pytest.raises(P.PoisonMismatch, match="LAUNDERED"):
        P.check(clean, out, E, ksite, P.INF, "either", either=either, bound=(ref, B))
    # at_least_one (the reduced-precision GELU rows) and the control
    gs = P.Site("A[3, 5]", "a", [], row=3, k=5)
    c2 = torch.zeros(8, 6)
    E2 = P.gemm_expected(8, 6, gs)
    row = c2.clone()
    row[3, 2] = P.INF
    P.check(c2, row, E2, gs, P.INF, "gelu", at_least_one=True)
    with pytest.raises(P.PoisonMismatch, match="LAUNDERED"):
        P.check(c2, row, E2, gs, P.INF, "gelu")
    with pytest.raises(P.PoisonMismatch, match="LAUNDERED"):
        P.check(c2, c2, E2, gs, P.INF, "gelu", at_least_one=True)
    P.check_control(c2, gs, P.F16_CONTROL, "control")
    with pytest.raises(P.PoisonMismatch, match="no poison"):
        P.check_control(row, gs, P.F16_CONTROL, "control")


def test_reference_and_bound_without_dropped_keys_is_the_softmax_of_the_rest():
    """softmax_helpers.reference_and_bound(drop=...): the reference is the float64 softmax over the remaining keys, the
    dropped keys' stored k rows are not read (they may be non-finite), and without drop nothing changes"""
    qkv, pad, wins, _ = S.case("win", *S.WINDOWED[1])
    heads, hd = 2, 64
    z = torch.zeros_like(qkv, dtype=torch.float64)
    planes, pad_planes = (qkv.double(), z), (pad.double(), z[0])
    rows = [0, 5, 700]
    ref0, B0 = S.reference_and_bound(planes, pad_planes, wins, heads, "f32", rows=rows)
    none = np.zeros((wins.tok_of.shape[0], wins.L), bool)
    ref1, B1 = S.reference_and_bound(planes, pad_planes, wins, heads, "f32", rows=rows, drop=none)
    assert torch.equal(ref0, ref1) and torch.equal(B0, B1)
    drop = none.copy()
    gone = [3, 40, 300]
    drop[0, gone] = True
    q2 = qkv.clone()
    toks = wins.tok_of[0, gone]
    q2[toks, heads * hd:2 * heads * hd] = P.INF                             # their k rows hold inf: never read
    ref2, B2 = S.reference_and_bound((q2.double(), z), pad_planes, wins, heads, "f32", rows=rows, drop=drop)
    x = qkv.double().view(-1, 3, heads, hd)
    idx = wins.tok_of[0]
    keep = torch.from_numpy(~drop[0])                                       # (pad positions are keys: the pad rule)
    ext = torch.cat([x, pad.double().view(1, 3, heads, hd)], 0)[np.where(idx >= 0, idx, qkv.shape[0])]
    for r in (0, 5):
        for h in range(heads):
            t = (x[r, 0, h] @ ext[keep, 1, h].t()) * hd ** -0.5
            want = torch.softmax(t, -1) @ ext[keep, 2, h]
            assert float((ref2[r, h * hd:(h + 1) * hd] - want).abs().max()) < 1e-12
    assert bool(torch.isfinite(B2[[0, 5]]).all()) and torch.equal(ref2[700], ref0[700])
