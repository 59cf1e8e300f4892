"""Per-element error bounds of the streaming softmax, on the device: every attention kernel against the float64
softmax of the operands it really read, |got - ref64| <= B on EVERY output element of every live query, with the bounds
of tests/softmax_helpers.py unchanged (tests/test_softmax_inputs_cpu.py shows them sound and sensitive).  The inputs
realise designed score profiles per query row - late spikes on either side of the deferral threshold (2^8) and of the
reduced-precision limit (2^13), staircases that rescale every (second) tile, a ramp into underflow, common offsets,
dominant pad keys, calm rows that share a wave with a spike row - so the running sum, the deferred reference point, the
alpha rescale of O and l, the hi / lo split of P, the per-lane-half l and the merge's exp2(m_p - M) weights are each
exercised on rows where they decide the result.  Both outputs (out, out_split) are checked; a failure names window, head,
wave tile, lane and class; each test prints its largest |err| / B and the maximum per class."""
import pytest
import torch

import exact_helpers as X
import softmax_helpers as S
from cra5_amd import ops

pytestmark = pytest.mark.gpu


def _split_inputs(qkv, pad, dev, hi):
    """(qkv SplitMat, pad SplitMat, stored planes of both as float64): the planes are READ BACK from the device store and
    must reconstruct the builder's values exactly; the reduced-precision modes read the hi plane alone"""
    qs, ps = ops.split_f16(qkv.to(dev)), ops.split_f16(pad.reshape(1, -1).to(dev))
    planes = []
    for sm, x in ((qs, qkv), (ps, pad.reshape(1, -1))):
        h, l = sm.planes()
        assert torch.equal(h + l, x.to(dev)), "the split store does not hold the builder's operands exactly"
        planes.append((h.double(), (torch.zeros_like(l) if hi else l).double()))
    if hi == 3:
        qs, ps = X.plain_rows_of(qs), ps.plain_copy()
    return qs, ps, planes[0], (planes[1][0].reshape(-1), planes[1][1].reshape(-1))


def _locator(wins, heads, hd, rows):
    base = X.attention_locator(wins, heads, hd)

    def locate(r, c, got_row=None):
        return base(r, c) + f", lane {int(wins.loc_of[r]) % 32}, class '{rows['cls'][r, c // hd]}'"
    return locate


def _check(out, out_s, ref, B, family, wins, heads, hd, rows, label, sel=None):
    """|out - ref| <= B and |out_split - ref| <= B + the store terms, on every element of the rows `sel` (default: all);
    prints the largest |err| / B, where it occurred, and the maximum per class"""
    loc = _locator(wins, heads, hd, rows)
    idx = torch.arange(out.shape[0], device=out.device) if sel is None else torch.as_tensor(sel, device=out.device)
    o, o_s, r, b = out[idx], out_s[idx], ref[idx], B[idx]
    assert bool(torch.isfinite(b).all())
    ratio = S.ratio((o.double() - r).abs(), b)
    ratio_s = S.ratio((o_s.double() - r).abs(), b + S.split_store_term(r, family))
    i = int(ratio.argmax())
    rr, cc = int(idx[i // o.shape[1]]), i % o.shape[1]
    print(f"{label}: max |err| / B {float(ratio.max()):.3f} (split output {float(ratio_s.max()):.3f}) at {loc(rr, cc)}")
    per = ratio.view(o.shape[0], heads, hd).amax(-1).cpu().numpy()
    cls = rows["cls"][idx.cpu().numpy()]
    print("    " + ", ".join(f"{n} {per[cls == n].max():.3f}" for n in sorted(set(cls.reshape(-1)))))
    full = lambda t: torch.zeros_like(ref).index_copy_(0, idx, t.double())
    tol = torch.full_like(B, float("inf")).index_copy_(0, idx, b)
    X.assert_exact(full(o), full(r), S.U, label + " fp32 out", tol=tol, locate=loc, gemm_tiles=False)
    tol_s = torch.full_like(B, float("inf")).index_copy_(0, idx, b + S.split_store_term(r, family))
    X.assert_exact(full(o_s), full(r), S.U, label + " split out", tol=tol_s, locate=loc, gemm_tiles=False)


def _run_split(qs, ps, heads, H, W, wh, ww, dev, hi, workspace=None, balanced=None):
    N, C = H * W, qs.K // 3
    out = torch.full((N, C), float("nan"), device=dev)
    out_s = ops.SplitMat.empty(N, C, dev, zero=True)
    ops.window_attention_split(qs, ps, heads, H, W, wh, ww, out=out, out_split=out_s, hi_only=bool(hi), workspace=workspace,
                               balanced=balanced)
    return out, out_s.to_float()


# ------------------------------------------------------------------------------------------------ the split kernels


@pytest.mark.parametrize("hi", [0, 1, 3])
@pytest.mark.parametrize("H,W,ws", S.WINDOWED)
def test_window_attention_split_softmax_bounds(dev, H, W, ws, hi):
    """cra5_window_attention_split, 4-wave work-groups: 24 x 48 (two 576-token windows, no padding, the half-empty fifth
    work-group), 20 x 44 (padding on both sides, pad keys taking part), 50 x 24 / 24 x 50 (the production windows' bottom /
    right padding)"""
    heads, hd = 2, 64
    qkv, pad, wins, rows = S.case("win", H, W, ws)
    fam = "hi" if hi else "split"
    qs, ps, planes, pad_planes = _split_inputs(qkv, pad, dev, hi)
    ref, B = S.reference_and_bound(planes, pad_planes, wins, heads, fam)
    out, out_s = _run_split(qs, ps, heads, H, W, ws[0], ws[1], dev, hi)
    _check(out, out_s, ref, B, fam, wins, heads, hd, rows, f"window_attention_split hi_only {hi} {H}x{W} {ws}")


@pytest.mark.parametrize("hi", [0, 1, 3])
def test_global_attention_plain_launch_softmax_bounds(dev, hi):
    """the whole-grid plain launch (12-wave work-groups): 8 x 72 = 576 tokens, 1.5 work-groups of 384 queries"""
    heads, hd = 2, 64
    H, W = S.GLOBAL_PLAIN
    qkv, pad, wins, rows = S.case("global")
    fam = "hi" if hi else "split"
    qs, ps, planes, pad_planes = _split_inputs(qkv, pad, dev, hi)
    ref, B = S.reference_and_bound(planes, pad_planes, wins, heads, fam)
    out, out_s = _run_split(qs, ps, heads, H, W, H, W, dev, hi)
    _check(out, out_s, ref, B, fam, wins, heads, hd, rows, f"global plain launch hi_only {hi} {H}x{W}")


@pytest.mark.parametrize("hi", [0, 1])
def test_global_attention_balanced_launch_softmax_bounds(dev, hi):
    """the balanced launch with attention_merge_kernel: 64 x 64 tokens, 32 heads - on 256 CUs 96 full wave-tiles + 32
    key-split ones in 3 groups over 8 slots, partials merged from 3-4 key ranges; a dominant key on either side of every
    cut, pieces with equal maxima, a piece more than 126 units below the group maximum (the ramp rows).  Workspace
    pre-filled with 0xFF.  Full-pass tokens equal the plain launch bit for bit; key-split tokens are held to the bound
    (float64 reference formed on the device)."""
    b = S.BALANCED
    H, W, heads, hd = b["H"], b["W"], b["heads"], 64
    N = H * W
    if torch.cuda.get_device_properties(dev).multi_processor_count != 256:
        pytest.skip("the plan (and the cuts the inputs are built around) is written out for 256 CUs")
    ok, nb = ops.attention_balanced_plan(N, heads)
    tile0, grps = S.bal_cuts(N // 32, b["groups"])
    assert ok and nb == heads * len(grps) * max(len(p) for _, p in grps) * 12 * 32 * 68 * 4
    qkv, pad, wins, rows = S.case("balanced")
    fam = "hi" if hi else "split"
    qs, ps, planes, pad_planes = _split_inputs(qkv, pad, dev, hi)
    plain, plain_s = _run_split(qs, ps, heads, H, W, H, W, dev, hi)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev).fill_(0xFF)
    out, out_s = _run_split(qs, ps, heads, H, W, H, W, dev, hi, workspace=ws)
    n_full = tile0 * 32
    # the key-split path really ran: exactly the partials of the plan were written over the 0xFF fill (68 floats per query
    # and key range: O[64], m, l, 2 pad; an unwritten l is a NaN pattern) - and the merge read them (the bound below)
    l_part = ws.view(torch.float32).view(-1, 68)[:, 65]
    written = torch.isfinite(l_part)
    assert int(written.sum()) == heads * sum(n_act * 32 * len(p) for n_act, p in grps) and bool((l_part[written] > 0).all())
    assert torch.equal(out[:n_full], plain[:n_full]) and torch.equal(out_s[:n_full], plain_s[:n_full])
    assert not torch.equal(out[n_full:], plain[n_full:])            # (merged from key ranges: another summation order)
    ks = list(range(n_full, N))
    ref, B = S.reference_and_bound(planes, pad_planes, wins, heads, fam, pieces=max(len(p) for _, p in grps), rows=ks)
    _check(out, out_s, ref, B, fam, wins, heads, hd, rows, f"balanced launch hi_only {hi} {H}x{W}, {heads} heads, key-split tokens",
           sel=ks)
    out2, _ = _run_split(qs, ps, heads, H, W, H, W, dev, hi, workspace=ws)
    assert torch.equal(out2, out)                                   # the merge adds the key ranges in a fixed order


# ------------------------------------------------------------------------------------------------ the exact-f32 kernels


@pytest.mark.parametrize("H,W,ws,hd", S.F32_CASES)
def test_window_attention_f32_softmax_bounds(dev, H, W, ws, hd):
    """cra5_window_attention_f32: the 20 x 44 padded grid at head dim 64; 18 x 36 as one window at head dim 72 (648 keys: the
    masked ragged last tile)"""
    heads = 2
    qkv, pad, wins, rows = S.case("win", H, W, ws, hd)
    z = torch.zeros_like(qkv, dtype=torch.float64, device=dev)
    planes, pad_planes = (qkv.double().to(dev), z), (pad.double().to(dev), z[0])
    ref, B = S.reference_and_bound(planes, pad_planes, wins, heads, "f32")
    out = torch.full((H * W, heads * hd), float("nan"), device=dev)
    out_s = ops.SplitMat.empty(H * W, heads * hd, dev, zero=True)
    ops.window_attention(qkv.to(dev), pad.to(dev), heads, H, W, ws[0], ws[1], out=out, out_split=out_s)
    _check(out, out_s.to_float(), ref, B, "f32", wins, heads, hd, rows, f"window_attention_f32 {H}x{W} {ws} hd {hd}")


@pytest.mark.parametrize("n,heads,hd", S.HYPER)
def test_hyper_attention_softmax_bounds(dev, n, heads, hd):
    """cra5_hyper_attention_f32: keys dealt to the 4 waves of a block in 16-key tiles and merged through LDS; a dominant key
    in each wave's share in turn; n = 17: two waves have no keys at all"""
    qkv, pad, wins, rows = S.case("hyper", n, heads, hd)
    z = torch.zeros_like(qkv, dtype=torch.float64, device=dev)
    planes, pad_planes = (qkv.double().to(dev), z), (pad.double().to(dev), z[0])
    ref, B = S.reference_and_bound(planes, pad_planes, wins, heads, "hyper")
    out = torch.full((n, heads * hd), float("nan"), device=dev)
    out_s = ops.SplitMat.empty(n, heads * hd, dev, zero=True)
    ops.hyper_attention(qkv.to(dev), heads, out=out, out_split=out_s)
    _check(out, out_s.to_float(), ref, B, "hyper", wins, heads, hd, rows, f"hyper_attention n = {n}, {heads} x {hd}")
