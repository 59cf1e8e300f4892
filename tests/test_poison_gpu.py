"""One out-of-range operand poisons every output that reads it, on the device.  The range rule of csrc/split.h rests on
every consumer kernel keeping a non-finite operand non-finite in every output that reads it: an activation beyond the
f16 range is stored as hi = +-inf, lo = -+inf, and the frame is re-run on the exact-f32 engines once the finiteness
probe sees the poison.  A kernel that turned a poisoned element back into a finite number (a row maximum that drops a
NaN, a clamp, a branch that skips it) would let a finite and wrong frame through.

Every test here runs a kernel twice on the same inputs: clean, and with ONE operand element replaced by a poison value
that arrives through the real producer (ops.split_f16; its hi plane for the plain rows of hi_only = 3).  The expected
set E of output elements that read the element comes from the geometry alone (tests/poison_helpers.py, checked against
float64 in tests/test_poison_inputs_cpu.py): every element of E must be non-finite, every other element must hold the
clean launch's bits, in the fp32 output and in the split output.  The negative control (65 519 for an f16-stored operand -
it rounds to 65 504 - and 70 000 for an fp32 operand) must leave everything finite.

Two documented exceptions, both inside cra5 window_attention_split_kernel (all its launches):
  * a poisoned Q element: the kernel decides its rescales per WAVE (`!__all(mloc - m_run <= 8)`, `!__all(psum <= P_SAFE)`),
    so the poisoned query makes its wave take the branch on every tile and its 31 wave neighbours are computed against
    another reference point: other bits, the same softmax.  There the non-finite set must still EQUAL E; the bits may
    differ inside head h of that one wave (poison_helpers.wave_block) and nowhere else.
  * a bare +-inf in a Q / K element (reduced precision and the fp32 engines: no lo plane turns it into NaN) gives scores
    of +-inf by sign: rows with a NaN or +inf score must be non-finite, rows whose affected scores are all -inf lose
    that key legitimately - non-finite, or within softmax_helpers' bound of the float64 softmax without it.

The last part holds the staged host copies (ops.copy_h2d_staged / copy_d2h_staged) to byte-exact round trips."""
import warnings

import numpy as np
import pytest
import torch

import exact_helpers as X
import patch_geometry_helpers as G
import poison_helpers as P
import softmax_helpers as S
from cra5_amd import ops, synth
from cra5_amd.vaeformer import VAEformer

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ part 1: attention


_REST = {}     # (case, family, site, stored value) -> (either rows, ref, B of the site's head): hi_only 1 and 3 store the same operand


def _rest_of_the_keys(case, qkv, pad, wins, heads, hd, site, value, family, dev, pieces_of_row):
    """A bare +-inf in a Q / K element: the row classes of poison_helpers.classify and, for the rows whose poisoned keys
    drop out, softmax_helpers' reference and bound of the softmax without those keys - evaluated on the site's head alone,
    from the operands as the family stores them (qkv, pad: the clean host tensors), once per stored value (70 000 and
    +inf are the same f16).  -> (check's keywords for the fp32 output, for the split output, rows that lost keys)"""
    N, C, h = qkv.shape[0], heads * hd, site.head
    key = (case, family, site.name, float(P.stored(torch.tensor([value]), family)))
    if key not in _REST:
        one = P.Site(site.name, site.operand, site.roles, token=site.token, head=0, d=site.d, window=site.window, loc=site.loc)
        qh, ph = P.poisoned(S.take_heads(qkv, heads, [h]), S.take_heads(pad, heads, [h]), one, value, 1, hd)
        mand, either, drop = P.classify(qh, ph, wins, 1, hd, one, family)
        assert mand.any() and not (site.operand == "q" and either.any())
        rows = np.nonzero(either)[0]
        ref = torch.zeros(N, hd, dtype=torch.float64, device=dev)
        B = torch.full((N, hd), float("inf"), dtype=torch.float64, device=dev)
        if len(rows):
            xh, pdh = qh.to(dev), ph.to(dev)
            z = torch.zeros_like(xh, dtype=torch.float64)
            planes, pad_planes = (P.stored(xh, family), z), (P.stored(pdh, family), z[0])
            groups = [(0, rows)] if pieces_of_row is None else [(n_, rows[pieces_of_row[rows] == n_]) for n_ in set(pieces_of_row[rows])]
            for pieces, rr in groups:
                r_, b_ = S.reference_and_bound(planes, pad_planes, wins, 1, family, pieces=int(pieces), rows=list(rr), drop=drop)
                idx = torch.as_tensor(rr, device=dev)
                ref[idx], B[idx] = r_[idx], b_[idx]
        _REST[key] = (rows, ref, B)
    rows, ref_h, B_h = _REST[key]
    if not len(rows):
        return {}, {}, 0
    cols = slice(h * hd, (h + 1) * hd)
    mask = torch.zeros(N, C, dtype=torch.bool, device=dev)
    mask[torch.as_tensor(rows, device=dev), cols] = True
    ref = torch.zeros(N, C, dtype=torch.float64, device=dev)
    B = torch.full((N, C), float("inf"), dtype=torch.float64, device=dev)
    ref[:, cols], B[:, cols] = ref_h, B_h
    return (dict(either=mask, bound=(ref, B)), dict(either=mask, bound=(ref, B + S.split_store_term(ref, family))), len(rows))


def _sweep(case, label, qkv, pad, wins, heads, hd, sites, launch, family, dev, wave_coupled, pieces_of_row=None, on_device=False):
    """clean launch, then one poisoned launch per (site, value) and one control per site; launch(qkv, pad) ->
    (out fp32 [N, C], (hi, lo) planes of the split output).  on_device: the launches run on device copies of the
    operands (the balanced case's 100 MB), the poisoned copy is made there."""
    f16 = family in ("split", "hi")
    poisons, control = (P.F16_POISONS, P.F16_CONTROL) if f16 else (P.F32_POISONS, P.F32_CONTROL)
    loc = X.attention_locator(wins, heads, hd)
    q_run, p_run = (qkv.to(dev), pad.to(dev)) if on_device else (qkv, pad)
    clean, clean_s = launch(q_run, p_run)
    assert bool(torch.isfinite(clean).all()) and bool(torch.isfinite(clean_s[0] + clean_s[1]).all())
    n_launch, n_bad, n_either = 1, 0, 0
    for site in sites:
        E = P.attention_expected(wins, heads, hd, site).to(dev)
        allow = P.wave_block(wins, heads, hd, site).to(dev) if wave_coupled and site.operand == "q" else None
        for name, value in poisons:
            got, got_s = launch(*P.poisoned(q_run, p_run, site, value, heads, hd))
            n_launch += 1
            kw, kw_s = {}, {}
            if family != "split" and site.operand in ("q", "k", "pad_k") and value == value:
                kw, kw_s, n = _rest_of_the_keys(case, qkv, pad, wins, heads, hd, site, value, family, dev, pieces_of_row)
                n_either += n
            n_bad += P.check(clean, got, E, site, value, f"{label}, fp32 out", allow=allow, locate=loc, **kw)
            P.check(clean_s, got_s, E, site, value, f"{label}, split out", allow=allow, locate=loc, **kw_s)
        got, got_s = launch(*P.poisoned(q_run, p_run, site, control, heads, hd))
        n_launch += 1
        P.check_control(got, site, control, f"{label}, fp32 out")
        if f16:
            P.check_control(got_s, site, control, f"{label}, split out")
        else:
            # (an fp32 V of 70 000 is an ordinary operand, and a query that puts nearly all its weight on that key gets an
            # fp32 output beyond the f16 range: the split STORE of that output poisons it, by csrc/split.h's rule - there
            # and nowhere else)
            over = got.abs() >= 65520.0
            assert torch.equal(~torch.isfinite(got_s[0] + got_s[1]), over), f"{label}: split out of the control at {site.name}"
            assert site.operand in ("v", "pad_v") or not bool(over.any())
    print(f"{label}: {len(sites)} sites x {len(poisons)} values + controls = {n_launch} launches; {n_bad} non-finite fp32 outputs, "
          f"all expected; {n_either} rows lost their poisoned keys legitimately")


def _split_launcher(heads, H, W, wh, ww, dev, hi, workspace=None):
    def launch(qkv, pad):
        qs, ps = ops.split_f16(qkv.to(dev)), ops.split_f16(pad.reshape(1, -1).to(dev))
        if hi == 3:      # plain rows: the hi plane the split store wrote, as the model's plain-output producers hold it
            qs, ps = X.plain_rows_of(qs), ps.plain_copy()
        N, C = H * W, qs.K // 3
        out = torch.full((N, C), float("nan"), device=dev)
        out_s = ops.SplitMat.empty(N, C, dev, zero=True)
        ops.window_attention_split(qs, ps, heads, H, W, wh, ww, out=out, out_split=out_s, hi_only=bool(hi), workspace=workspace)
        return out, out_s.planes()
    return launch


@pytest.mark.parametrize("hi", [0, 1, 3])
@pytest.mark.parametrize("H,W,ws", S.WINDOWED)
def test_window_attention_split_poison(dev, H, W, ws, hi):
    """cra5_window_attention_split, 4-wave work-groups, on the grids of test_softmax_gpu.py: Q / K / V elements in key tiles
    0, 1 and last, both lane halves, the first and last wave of a work-group, the half-empty last work-group, features
    0, 31, 32, 63, the pad row's K and V on the padded grids.  Set equality, but for the wave block of a poisoned Q
    (module docstring: the per-wave rescale decision is inherent to this kernel)."""
    heads, hd = 2, 64
    qkv, pad, wins, _ = S.case("win", H, W, ws)
    sites = P.attention_sites(wins, heads, hd, 4)
    _sweep(f"win {H}x{W} {ws}", f"window_attention_split hi_only {hi} {H}x{W} {ws}", qkv, pad, wins, heads, hd, sites,
           _split_launcher(heads, H, W, ws[0], ws[1], dev, hi), "hi" if hi else "split", dev, wave_coupled=True)


@pytest.mark.parametrize("hi", [0, 1, 3])
def test_global_attention_plain_launch_poison(dev, hi):
    """the whole-grid plain launch (12-wave work-groups, 1.5 of them: six idle waves in the second)"""
    heads, hd = 2, 64
    H, W = S.GLOBAL_PLAIN
    qkv, pad, wins, _ = S.case("global")
    sites = P.attention_sites(wins, heads, hd, 12)
    _sweep("global", f"global plain launch hi_only {hi}", qkv, pad, wins, heads, hd, sites, _split_launcher(heads, H, W, H, W, dev, hi),
           "hi" if hi else "split", dev, wave_coupled=True)


@pytest.mark.parametrize("hi", [0, 1, 3])
def test_global_attention_balanced_launch_poison(dev, hi):
    """the balanced launch with attention_merge_kernel (64 x 64 tokens, 32 heads, 256 CUs): queries in a full wave-tile
    and in key-split wave-tiles merged from 3 to 4 pieces (one of them in the group with idle waves), keys inside a
    piece, the last before and the first after a cut: the partial (m, l, O) of ONE piece is poisoned and the merge's
    fmaxf / exp2(m_p - M) weights have to carry it"""
    b = S.BALANCED
    H, W, heads, hd = b["H"], b["W"], b["heads"], 64
    N = H * W
    if torch.cuda.get_device_properties(dev).multi_processor_count != 256:
        pytest.skip("the plan (and the cuts the sites are built around) is written out for 256 CUs")
    ok, nb = ops.attention_balanced_plan(N, heads)
    tile0, grps = S.bal_cuts(N // 32, b["groups"])
    assert ok and nb == heads * len(grps) * max(len(p) for _, p in grps) * 12 * 32 * 68 * 4
    qkv, pad, wins, _ = S.case("balanced")
    sites = P.attention_sites(wins, heads, hd, 12, groups=b["groups"])
    ws = torch.empty(nb, dtype=torch.uint8, device=dev).fill_(0xFF)
    pieces_of_row = np.zeros(N, np.int64)
    pieces_of_row[tile0 * 32:] = max(len(p) for _, p in grps)
    _sweep("balanced", f"balanced launch hi_only {hi}", qkv, pad, wins, heads, hd, sites,
           _split_launcher(heads, H, W, H, W, dev, hi, workspace=ws), "hi" if hi else "split", dev, wave_coupled=True,
           pieces_of_row=pieces_of_row, on_device=True)


@pytest.mark.parametrize("H,W,ws,hd", S.F32_CASES)
def test_window_attention_f32_poison(dev, H, W, ws, hd):
    """cra5_window_attention_f32 (fp32 operands: +inf, -inf, NaN; control 70 000): the padded 20 x 44 grid at head dim 64
    (6-wave work-groups) and 18 x 36 as one window at head dim 72 - features 64 .. 71 and the masked ragged last key tile.
    No decision is shared between queries: set equality throughout."""
    heads = 2
    qkv, pad, wins, _ = S.case("win", H, W, ws, hd)
    sites = P.attention_sites(wins, heads, hd, 6 if (hd == 64 and wins.L % 192 == 0 and wins.L <= 1152) else 4)

    def launch(q, p):
        out = torch.full((H * W, heads * hd), float("nan"), device=dev)
        out_s = ops.SplitMat.empty(H * W, heads * hd, dev, zero=True)
        ops.window_attention(q.to(dev), p.to(dev), heads, H, W, ws[0], ws[1], out=out, out_split=out_s)
        return out, out_s.planes()
    _sweep(f"win {H}x{W} {ws} hd {hd}", f"window_attention_f32 {H}x{W} {ws} hd {hd}", qkv, pad, wins, heads, hd, sites, launch, "f32", dev, wave_coupled=False)


@pytest.mark.parametrize("n,heads,hd", S.HYPER)
def test_hyper_attention_poison(dev, n, heads, hd):
    """cra5_hyper_attention_f32: a key in each wave's share of the 16-key tiles, the ragged last tile, the first and the
    ragged last query tile; n = 17: a wave whose only key is the poisoned one.  Set equality throughout."""
    qkv, pad, _, _ = S.case("hyper", n, heads, hd)
    wins, sites = P.hyper_sites(n, heads, hd)

    def launch(q, p):
        out = torch.full((n, heads * hd), float("nan"), device=dev)
        out_s = ops.SplitMat.empty(n, heads * hd, dev, zero=True)
        ops.hyper_attention(q.to(dev), heads, out=out, out_split=out_s)
        return out, out_s.planes()
    _sweep(f"hyper {n}", f"hyper_attention n = {n}, {heads} x {hd}", qkv, pad, wins, heads, hd, sites, launch, "hyper", dev, wave_coupled=False)


# ------------------------------------------------------------------------------------------------ part 2: the GEMM family


def _gemm_inputs(M, N, K, dev, seed):
    g = torch.Generator().manual_seed(seed)
    # (|a| stays below 1 / 4 and |w| far below it: the control 65 519 times the largest partner - and with it every
    # finite output - stays inside the f16 range of the split output's own store)
    a = torch.randn(M, K, generator=g).clamp_(-4.5, 4.5) * 0.05
    w = torch.randn(N, K, generator=g).clamp_(-4.5, 4.5) * K ** -0.5
    bias, res = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    assert bool((a != 0).all()) and bool((w != 0).all())
    return a.to(dev), w.to(dev), bias.to(dev), res.to(dev)


def _gemm_sweep(label, M, N, K, tile, dev, run, poisons, control, seed=0, at_least_one=False):
    """run(a, w, bias, res) -> {name: tensor or (hi, lo) planes}.  A sites poison rows, W sites columns."""
    a, w, bias, res = _gemm_inputs(M, N, K, dev, seed)
    clean = run(a, w, bias, res)
    for name, t in clean.items():
        assert bool(torch.isfinite(t if torch.is_tensor(t) else t[0] + t[1]).all()), name
    sites = P.gemm_sites(M, N, K, *tile)
    n = 1
    for site in sites:
        E = P.gemm_expected(M, N, site)
        for vname, value in list(poisons) + [("control", control)]:
            a2, w2 = a, w
            if site.operand == "a":
                a2 = a.clone()
                a2[site.row, site.k] = value
            else:
                w2 = w.clone()
                w2[site.row, site.k] = value
            got = run(a2, w2, bias, res)
            n += 1
            for name, t in got.items():
                if vname == "control":
                    P.check_control(t, site, value, f"{label}, {name}")
                else:
                    P.check(clean[name], t, E, site, value, f"{label}, {name}", at_least_one=at_least_one and site.operand == "a")
    print(f"{label}: {len(sites)} sites ({', '.join(s.name for s in sites)}), {n} launches")


def _split_runs(dev, M, N, hi_only=False, plain=False, small=False):
    """the epilogues of one split engine: none (fp32 and split output together), bias + GELU + split output with and
    without the fp32 output, residual written in place.  The activations are split unscaled, like the model's; the
    weights too, so that a weight of 70 000 leaves the f16 range (the model's "auto" scale keeps a finite weight inside
    it by construction)."""
    def operands(a, w):
        sa, sw = ops.split_f16(a), ops.split_f16(w)
        if plain:
            sa, sw = X.plain_rows_of(sa), sw.plain_copy()
        return sa, sw
    kw = dict(hi_only=True, out_plain=plain) if hi_only else {}
    mm = ops.small_gemm_nt_split if small else ops.gemm_nt_split

    def none(a, w, bias, res):
        sa, sw = operands(a, w)
        out_s = ops.SplitMat.empty(M, N, dev, zero=True)
        out = mm(sa, sw, out_split=out_s, **kw)
        return {"fp32 out": out, "split out": out_s.planes()}

    def gelu(a, w, bias, res):
        sa, sw = operands(a, w)
        s1, s2 = ops.SplitMat.empty(M, N, dev, zero=True), ops.SplitMat.empty(M, N, dev, zero=True)
        out = mm(sa, sw, bias=bias, gelu=True, out_split=s1, **kw)
        mm(sa, sw, bias=bias, gelu=True, out_split=s2, want_f32=False, **kw)
        return {"bias + gelu, fp32 out": out, "bias + gelu, split out": s1.planes(), "bias + gelu, split out alone": s2.planes()}

    def res_in_place(a, w, bias, res):
        sa, sw = operands(a, w)
        out = res.clone()
        mm(sa, sw, bias=bias, res=out, out=out, **kw)
        return {"bias + res in place": out}
    return none, gelu, res_in_place


GEMM_TILES = [(256, 256, (64, 64)), (2048, 2048, (256, 256)), (4224, 1024, (192, 256))]     # test_domain_gpu.py's tile classes


@pytest.mark.parametrize("K", [96, 360])
@pytest.mark.parametrize("M,N,tile", GEMM_TILES)
def test_gemm_nt_split_poison(dev, M, N, tile, K):
    """cra5_gemm_nt_split, fp32-accurate, in its three tile classes: A[i, k] -> row i, W[n, k] -> column n, all else the
    clean launch's bits, under every epilogue (GELU keeps NaN as NaN)"""
    for run, name in zip(_split_runs(dev, M, N), ("no epilogue", "bias + gelu", "res in place")):
        _gemm_sweep(f"gemm_nt_split {M}x{N}x{K} {tile[0]}x{tile[1]} tiles, {name}", M, N, K, tile, dev, run, P.F16_POISONS, P.F16_CONTROL)


@pytest.mark.parametrize("M,N,tile,plain", [t + (False,) for t in GEMM_TILES] + [t + (True,) for t in GEMM_TILES[1:]])
def test_gemm_nt_split_hi_only_poison(dev, M, N, tile, plain):
    """the reduced-precision form, on split rows and (where the launch takes them) on plain rows, K = 360: the stored
    operand is a bare +-inf, a row holds +-inf by the sign of the weights.  Under GELU a row of +-inf need not stay
    non-finite element by element (gelu(-inf) is x * 0): there the expected set is "row i holds at least one
    non-finite value and no other row changed"; without GELU, and for a W element, set equality."""
    K = 360
    assert ops.plain_ok(M, N, 384) == ((M, N) != (256, 256))          # (the 64 x 64-tile launch takes no plain operands)
    for run, name in zip(_split_runs(dev, M, N, hi_only=True, plain=plain), ("no epilogue", "bias + gelu", "res in place")):
        _gemm_sweep(f"gemm_nt_split hi_only{' plain rows' if plain else ''} {M}x{N}x{K}, {name}", M, N, K, tile, dev, run,
                    P.F16_POISONS, P.F16_CONTROL, at_least_one=name == "bias + gelu")


@pytest.mark.parametrize("M,N,K", [(648, 360, 360), (100, 77, 144)])
def test_small_gemm_nt_split_poison(dev, M, N, K):
    """cra5_small_gemm_nt_split (csrc/hyper.hip): ragged last tiles in M and N"""
    for run, name in zip(_split_runs(dev, M, N, small=True), ("no epilogue", "bias + gelu", "res in place")):
        _gemm_sweep(f"small_gemm_nt_split {M}x{N}x{K}, {name}", M, N, K, (64, 64), dev, run, P.F16_POISONS, P.F16_CONTROL)


def test_gemm_nt_f32_poison(dev):
    """cra5_gemm_nt_f32 at 1000 x 1080 x 360 (ragged tiles): +inf, -inf, NaN; 70 000 is an ordinary fp32 operand"""
    M, N, K = 1000, 1080, 360

    def none(a, w, bias, res):
        return {"out": ops.gemm_nt(a, w)}

    def gelu(a, w, bias, res):
        return {"bias + gelu": ops.gemm_nt(a, w, bias=bias, gelu=True)}

    def res_in_place(a, w, bias, res):
        out = res.clone()
        ops.gemm_nt(a, w, bias=bias, res=out, out=out)
        return {"bias + res in place": out}
    for run, name in ((none, "no epilogue"), (gelu, "bias + gelu"), (res_in_place, "res in place")):
        _gemm_sweep(f"gemm_nt_f32 {M}x{N}x{K}, {name}", M, N, K, (128, 128), dev, run, P.F32_POISONS, P.F32_CONTROL)


@pytest.mark.parametrize("denorm", [False, True])
def test_fused_unembed_poison(dev, denorm):
    """cra5_gemm_nt_split_unembed at C = 8, K = 128 on the 72 x 144 token grid: a poisoned token row gives exactly the
    pixels whose fold indicator is non-zero (its 11 x 10 patch in every channel, seam rows included); every other pixel
    holds the clean launch's bits - through the side buffer and the seam fix-up, with and without de-normalisation"""
    C, Hp, Wp, K = 8, G.GRID_HP, G.GRID_WP, 128
    H, W = G.image_shape(Hp, Wp)
    g = torch.Generator().manual_seed(5)
    a = torch.randn(Hp * Wp, K, generator=g).to(dev)
    sw = ops.split_f16((torch.randn(C * G.KH * G.KW, K, generator=g) * K ** -0.5).to(dev), "auto")
    mean, std = (t.to(dev) for t in G.random_stats(C, 3)) if denorm else (None, None)
    nb = ops.unembed_side_bytes(C, H, W, G.KH, G.KW, G.SH, G.SW)
    locate = G.unembed_locator(H)

    def run(a_):
        side = torch.full((nb // 4,), float("nan"), device=dev)
        out = torch.full((C, H, W), float("nan"), device=dev)
        ops.gemm_unembed(ops.split_f16(a_), sw, C, H, W, G.KH, G.KW, G.SH, G.SW, side, mean=mean, std=std, out=out)
        return out
    clean = run(a)
    assert bool(torch.isfinite(clean).all())
    sites = P.unembed_sites(Hp, Wp, K)
    for site in sites:
        E = P.unembed_expected(C, Hp, Wp, site)
        assert int(E.sum()) == C * 110
        for vname, value in P.F16_POISONS + (("control", P.F16_CONTROL),):
            a2 = a.clone()
            a2[site.row, site.k] = value
            got = run(a2)
            if vname == "control":
                P.check_control(got, site, value, "fused un-embed")
            else:
                P.check(clean, got, E, site, value, f"fused un-embed, de-normalised {denorm}", locate=locate)
    print(f"fused un-embed, de-normalised {denorm}: sites {', '.join(s.name for s in sites)}")


# ------------------------------------------------------------------------------------------------ part 3: the thin model


def _thin(dev):
    net = VAEformer(0, **synth.thin_model_kwargs())
    synth.load_synthetic(net, seed=7)
    return net.to(dev)


@pytest.fixture(scope="module")
def thin(dev):
    return _thin(dev)


@pytest.fixture(scope="module")
def frame():
    return synth.synth_frame(8, seed=2).unsqueeze(0)


class _Modified:
    """the thin model with some weight rows scaled, restored on exit (the derived weight layouts are dropped both times)"""

    def __init__(self, net, edits):
        self.net, self.edits, self.saved = net, edits, []

    def __enter__(self):
        with torch.no_grad():
            for t, index, factor in self.edits:
                self.saved.append((t, t.detach().clone()))
                t[index] *= factor
        self.net._derived.clear()
        return self.net

    def __exit__(self, *exc):
        with torch.no_grad():
            for t, old in self.saved:
                t.copy_(old)
        self.net._derived.clear()


def _engines(net, precision=None, exact=False):
    net.precision = precision or "fp32"
    net.gemm_mode, net.attn_mode = ("f32", "f32") if exact else ("split", "split")
    net.range_fallbacks = [0, 0]


def _one_fallback(fn, net, side):
    """fn() under the split engines: exactly one range fallback on `side`, announced by exactly one warning"""
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        out = fn()
    told = [w for w in rec if issubclass(w.category, RuntimeWarning) and "exact-f32" in str(w.message)]
    want = [1, 0] if side == 0 else [0, 1]
    assert net.range_fallbacks == want and len(told) == 1, (net.range_fallbacks, [str(w.message) for w in rec])
    return out


def _attention_blocks(net):
    """(index of a windowed block, index of a global block) of g_a, each taking the split attention kernel"""
    D = net.cfg['embed_dim']
    win = next(i for i, b in enumerate(net.g_a.blocks) if b.window is not None)
    glo = next(i for i, b in enumerate(net.g_a.blocks) if b.window is None)
    for i in (win, glo):
        b = net.g_a.blocks[i]
        wh, ww = b.window if b.window is not None else (net.Hp, net.Wp)
        assert ops.split_attention_ok(D, b.heads, wh, ww, net.Hp, net.Wp), "the block would take another attention kernel"
    return win, glo


PIXELS = {"token (0, 0)": (2, 3, 4), "the last token": (5, 715, 1436), "the bottom seam row 720": (0, 720, 700),
          "the last column": (7, 301, 1439)}


@pytest.mark.parametrize("precision", ["fp32", "f16"])
def test_one_out_of_range_input_pixel_falls_back_to_the_exact_f32_engines(thin, frame, dev, precision):
    """one finite input pixel of 70 000 (normalised units: the patch gather's f16 store poisons it) at four positions:
    one fallback, one warning, and the streams of the exact-f32 engines"""
    win, glo = _attention_blocks(thin)
    try:
        for where, (c, r, col) in PIXELS.items():
            x = frame.clone()
            x[0, c, r, col] = 70000.0
            x = x.to(dev)
            _engines(thin, precision)
            out = _one_fallback(lambda: thin.compress(x), thin, 0)
            _engines(thin, exact=True)
            ref = thin.compress(x)
            assert thin.range_fallbacks == [0, 0]
            assert out["strings"] == ref["strings"], where
    finally:
        _engines(thin)


@pytest.mark.parametrize("precision", ["fp32", "f16"])
@pytest.mark.parametrize("operand", ["k", "v"])
def test_one_out_of_range_attention_feature_falls_back(thin, frame, dev, operand, precision):
    """one K (or V) feature of one block's qkv projection scaled by 3e5, once in a windowed and once in the global block
    of g_a: attention is the only reader of that column (for V the proj weight's column takes the factor back out, so the
    block's output stays O(1)).  A fallback, and the streams of the exact-f32 engines."""
    D = thin.cfg['embed_dim']
    x = frame.to(dev)
    try:
        for i in _attention_blocks(thin):
            blk = thin.g_a.blocks[i]
            col = 64 + 17                                               # head 1, feature 17
            row = (1 if operand == "k" else 2) * D + col
            edits = [(blk.attn.qkv.weight, row, 3e5), (blk.attn.qkv.bias, row, 3e5)]
            if operand == "v":
                edits.append((blk.attn.proj.weight, (slice(None), col), 1.0 / 3e5))
            with _Modified(thin, edits):
                _engines(thin, precision)
                out = _one_fallback(lambda: thin.compress(x), thin, 0)
                _engines(thin, exact=True)
                ref = thin.compress(x)
                assert thin.range_fallbacks == [0, 0]
                assert out["strings"] == ref["strings"], (operand, i)
    finally:
        _engines(thin)


@pytest.mark.parametrize("precision", ["fp32", "f16"])
def test_one_out_of_range_latent_element_falls_back_on_the_decode_side(thin, dev, precision):
    """y_hat[c, i, j] = 1e7: one fallback on the decode side, x_hat is the exact-f32 engines' bit for bit"""
    g = torch.Generator().manual_seed(11)
    y_hat = torch.round(2.0 * torch.randn(1, thin.cfg['latent_dim'], thin.Hp, thin.Wp, generator=g))
    y_hat[0, 5, 40, 100] = 1e7
    y_hat = y_hat.to(dev)
    try:
        _engines(thin, precision)
        got = _one_fallback(lambda: thin.decode_latent(y_hat), thin, 1)
        _engines(thin, exact=True)
        ref = thin.decode_latent(y_hat)
        assert thin.range_fallbacks == [0, 0] and bool(torch.isfinite(ref).all())
        assert torch.equal(got.view(torch.int32), ref.view(torch.int32))
    finally:
        _engines(thin)


# ------------------------------------------------------------------------------------------------ part 4: staged copies

MIB = 1 << 20
COPY_SIZES = (1, 63, 64, 65, 65535, 65536, 65537, MIB - 1, MIB, MIB + 1, 9 * MIB + 17)
COPY_THREADS = (1, 2, 3, 8, 64)


@pytest.mark.parametrize("chunk", [64 << 10, 4 * MIB], ids=["64 KiB chunks", "4 MiB chunks: the 1-2-4 MiB ramp"])
def test_staged_copies_round_trip_byte_exact(dev, monkeypatch, chunk):
    """ops.copy_h2d_staged / copy_d2h_staged (csrc/runtime.hip): random bytes host -> device -> host at sizes around the
    64-byte thread cut, the 64 KiB minimum chunk and the 1 MiB first chunk of the ramp, with 1 .. 64 host threads; the
    pinned buffer is larger than the payload and both destinations sit between guard bytes that must stay untouched"""
    monkeypatch.setattr(ops, "COPY_CHUNK", chunk)
    rng = np.random.default_rng(chunk)
    top = max(COPY_SIZES)
    pinned = torch.empty(top + 4096, dtype=torch.uint8).pin_memory()
    for n in COPY_SIZES:
        src = rng.integers(0, 256, n, dtype=np.uint8)
        for threads in COPY_THREADS:
            pinned.fill_(0xA5)
            dbuf = torch.full((n + 128,), 0x5A, dtype=torch.uint8, device=dev)
            dst = dbuf[64:64 + n]
            ops.copy_h2d_staged(dst, src, pinned, threads=threads)
            torch.cuda.synchronize()
            back = dbuf.cpu().numpy()
            assert np.array_equal(back[64:64 + n], src), (n, threads, "host -> device")
            assert (back[:64] == 0x5A).all() and (back[64 + n:] == 0x5A).all(), (n, threads, "device guard bytes")
            assert bool((pinned[n:] == 0xA5).all()), (n, threads, "pinned bytes past the payload")
            pinned.fill_(0xA5)
            hbuf = np.full(n + 128, 0xC3, dtype=np.uint8)
            ops.copy_d2h_staged(hbuf[64:64 + n], dst, pinned, threads=threads)
            assert np.array_equal(hbuf[64:64 + n], src), (n, threads, "device -> host")
            assert (hbuf[:64] == 0xC3).all() and (hbuf[64 + n:] == 0xC3).all(), (n, threads, "host guard bytes")
            assert bool((pinned[n:] == 0xA5).all()), (n, threads, "pinned bytes past the payload")


def test_staged_copies_refuse_what_they_cannot_copy(dev):
    n = 4096
    pinned = torch.empty(n, dtype=torch.uint8).pin_memory()
    d = torch.zeros(n, dtype=torch.uint8, device=dev)
    good = np.zeros(n, dtype=np.uint8)
    ops.copy_h2d_staged(d, good, pinned)
    ops.copy_d2h_staged(good, d, pinned)
    strided = np.zeros(2 * n, dtype=np.uint8)[::2]
    readonly = np.zeros(n, dtype=np.uint8)
    readonly.setflags(write=False)
    unpinned = torch.empty(n, dtype=torch.uint8)
    for what, fn in (("non-contiguous source", lambda: ops.copy_h2d_staged(d, strided, pinned)),
                     ("non-contiguous destination", lambda: ops.copy_d2h_staged(strided, d, pinned)),
                     ("short source", lambda: ops.copy_h2d_staged(d, good[:-1], pinned)),
                     ("long destination", lambda: ops.copy_d2h_staged(np.zeros(n + 1, dtype=np.uint8), d, pinned)),
                     ("read-only destination", lambda: ops.copy_d2h_staged(readonly, d, pinned)),
                     ("unpinned staging buffer, host -> device", lambda: ops.copy_h2d_staged(d, good, unpinned)),
                     ("unpinned staging buffer, device -> host", lambda: ops.copy_d2h_staged(good, d, unpinned)),
                     ("staging buffer too small", lambda: ops.copy_h2d_staged(d, good, pinned[: n // 2]))):
        with pytest.raises(ValueError):
            fn()
        assert not readonly.any(), what
