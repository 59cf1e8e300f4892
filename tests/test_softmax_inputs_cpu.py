"""The builder and the bounds of tests/softmax_helpers.py themselves, on the grids tests/test_softmax_gpu.py runs: the
inputs deliver what they promise (margins to the thresholds, class coverage per wave tile, operands exact in the split
model); each bound is SOUND (the fp32 host restatement - and torch's fp32 CPU attention for the fp32-accurate families -
stays within B / 2 on every element) and SENSITIVE (every listed wrong variant but the harmless one breaks B on a class
aimed at it); the restatement's branch record is the designed one.  A bound that passes is what the GPU tests assert,
unchanged.  The balanced grid (64 x 64 tokens, 32 heads) is checked on its key-split tokens for heads 0-2, which
between them put every theme into the key-split wave-tiles; the GPU test compares all 32."""
import numpy as np
import pytest
import torch

import softmax_helpers as S

WIN_IDS = [f"{H}x{W}-{ws[0]}x{ws[1]}" for H, W, ws in S.WINDOWED]
BAL_HEADS = [0, 1, 2]


def _planes(qkv, pad, family):
    fam = "f32" if family == "hyper" else family
    return S.stored_planes(qkv, fam), S.stored_planes(pad, fam)


def _class_max(r, rows, heads, sel=None):
    """largest |err| / B per class name: {name: ratio}"""
    hd = r.shape[1] // heads
    per = r.view(r.shape[0], heads, hd).amax(-1).numpy()
    cls = rows["cls"] if sel is None else rows["cls"][:, sel]
    return {name: float(per[cls == name].max()) for name in sorted(set(cls.reshape(-1)))}


def _all_cases():
    for H, W, ws in S.WINDOWED:
        for fam in ("split", "hi"):
            yield f"window {H}x{W} {ws} {fam}", S.case("win", H, W, ws), 2, fam
    for fam in ("split", "hi"):
        yield f"global 8x72 {fam}", S.case("global"), 2, fam
    for H, W, ws, hd in S.F32_CASES:
        yield f"f32 {H}x{W} {ws} hd {hd}", S.case("win", H, W, ws, hd), 2, "f32"
    for n, heads, hd in S.HYPER:
        yield f"hyper {n} x {heads} x {hd}", S.case("hyper", n, heads, hd), heads, "hyper"


# ------------------------------------------------------------------------------------------------ the builder


def test_operands_are_exact_in_the_split_model_and_carry_lo_planes():
    for label, (qkv, pad, wins, rows), heads, fam in _all_cases():
        for x in (qkv, pad):
            hi, lo = S.X.split_model(x)
            assert torch.equal(hi + lo, x), label
            assert float(x.abs().max()) < 60000.0 and bool(torch.isfinite(x).all())
        assert float(S.X.split_model(qkv)[1].abs().max()) > 0, label


@pytest.mark.parametrize("H,W,ws", S.WINDOWED + ((8, 72, None),), ids=WIN_IDS + ["global"])
def test_every_decision_keeps_its_margin(H, W, ws):
    """float64 scores, the documented rule: no wave's decision quantity comes within 2^-6 log2 units of its threshold (the
    fp32 error of a spike row's score, 28 roundings on 8 - 13 units, is 2e-5 units: three orders below; a staircase's 140
    units give 2.4e-4, and its steps stay 0.1 from the threshold)"""
    qkv, pad, wins, rows = S.case("global") if ws is None else S.case("win", H, W, ws)
    for fam in ("split", "hi"):
        m = S.decision_margins(*_planes(qkv, pad, fam), wins, 2, fam)
        print(f"{H}x{W} {ws} {fam}: smallest margin {m:.4f} log2 units")
        assert m >= S.MARGIN


def test_every_decision_of_the_balanced_streams_keeps_its_margin():
    """the same for the streams of the balanced launch (heads 0-2): the full-pass wave-tiles over the whole key loop and
    every key-split group over each of its key ranges, whose reference is set anew by the range's first tile"""
    qkv, pad, wins, rows = S.case("balanced")
    q3, p3 = S.take_heads(qkv, 32, BAL_HEADS), S.take_heads(pad, 32, BAL_HEADS)
    for fam in ("split", "hi"):
        m = S.decision_margins(*_planes(q3, p3, fam), wins, 3, fam, balanced_groups=S.BALANCED["groups"])
        print(f"balanced {fam}: smallest margin {m:.4f} log2 units")
        assert m >= S.MARGIN


def test_spike_heights_sit_on_the_designed_side():
    """realised spike height over the row's standing maximum (window-local key 0), float64 on the split operands, against
    the designed one: within 2^-10, and every designed height occurs (the reduced-precision mode's own rounding of q c is
    inside test_every_decision_keeps_its_margin)"""
    qkv, pad, wins, rows = S.case("win", 24, 48, (24, 24))
    hd = 64
    (hi, lo), _ = _planes(qkv, pad, "split")
    x = (hi + lo).view(-1, 3, 2, hd)
    seen = set()
    for i, h in zip(*np.nonzero(rows["site"] >= 0)):
        key = rows["sites"][rows["site"][i, h]][0]
        w = wins.win_of[i]
        tok, tok0 = wins.tok_of[w][key], wins.tok_of[w][0]
        d = float((x[i, 0, h] * (x[tok, 1, h] - x[tok0, 1, h])).sum()) * S.c_of(hd)
        assert abs(d - rows["delta"][i, h]) < 2.0 ** -10
        seen.add(rows["delta"][i, h])
    assert seen == set(S.SPIKE_FP32) | set(S.SPIKE_HI)


def test_class_coverage():
    """24 x 48 in (24, 24) windows: every wave tile holds >= 3 classes; every class occurs in a full work-group (waves
    0-15) and in the half-empty fifth (waves 16, 17) of some (window, head); the spike sets cover both lane halves and
    key tiles 0, 1, 2, last - 1, last.  Balanced grid: every class occurs among the key-split tokens of heads 0-2."""
    qkv, pad, wins, rows = S.case("win", 24, 48, (24, 24))
    wave = wins.loc_of // 32
    names = set(rows["cls"].reshape(-1))
    assert len(names) == 21, names
    for w in range(2):
        for h in range(2):
            for t in range(18):
                assert len(set(rows["cls"][(wins.win_of == w) & (wave == t), h])) >= 3
    assert set(rows["cls"][wave >= 16].reshape(-1)) == names == set(rows["cls"][wave < 16].reshape(-1))
    keys = [s[0] for s in rows["sites"]]
    assert [k // 32 for k in keys] == [0, 1, 2, 16, 17] and {(k % 32 >> 2) & 1 for k in keys} == {0, 1}
    qkv, pad, wins, rows = S.case("balanced")
    tile0, grps = S.bal_cuts(128, S.BALANCED["groups"])
    assert tile0 == 96 and [len(p) for _, p in grps] == [3, 4, 3]
    assert set(rows["cls"][tile0 * 32:, BAL_HEADS].reshape(-1)) == set(rows["cls"].reshape(-1))
    cuts = {16, 32, 48, 64, 80, 96, 112}
    assert {k // 32 + 1 for k in rows["sites"][0]} == cuts == {k // 32 for k in rows["sites"][1]}
    assert all(k % 32 == 31 for k in rows["sites"][0]) and all(k % 32 == 0 for k in rows["sites"][1])


def test_balanced_case_has_a_piece_far_below_and_pieces_with_equal_maxima():
    """float64 piece maxima of the key-split rows: a ramp row's last piece lies > 126 units under the group maximum; a row
    whose spike set is 'the last key before every cut' has two pieces with the same maximum"""
    qkv, pad, wins, rows = S.case("balanced")
    tile0, grps = S.bal_cuts(128, S.BALANCED["groups"])
    x = S.take_heads(qkv, 32, [0]).double().view(-1, 3, 64)
    t = (x[tile0 * 32:, 0] @ x[:, 1].t()) * S.c_of(64)
    far = equal = 0
    for g, (n_act, pieces) in enumerate(grps):
        tt = t[384 * g:384 * g + 32 * n_act]
        pm = torch.stack([tt[:, 32 * a:32 * b].amax(1) for a, b in pieces], 1)
        far += int(((pm.amax(1, keepdim=True) - pm) > 126).any(1).sum())
        srt = pm.sort(1, descending=True).values
        equal += int((srt[:, 0] == srt[:, 1]).sum())
    assert far >= 3 and equal >= 3, (far, equal)


# ------------------------------------------------------------------------------------------------ soundness


def test_bounds_are_sound_on_every_grid():
    worst = {}
    for label, (qkv, pad, wins, rows), heads, fam in _all_cases():
        pl, pp = _planes(qkv, pad, fam)
        ref, B = S.reference_and_bound(pl, pp, wins, heads, fam)
        assert bool(torch.isfinite(B).all()) and bool((B > 0).all())
        out, _ = S.restate(pl, pp, wins, heads, fam)
        r = S.ratio((out - ref).abs(), B)
        line = f"{label}: restated max |err| / B {float(r.max()):.3f}"
        assert float(r.max()) <= 0.5, line
        if fam != "hi":
            rt = S.ratio((S.torch_fp32_attention(pl, pp, wins, heads) - ref).abs(), B)
            line += f", torch fp32 {float(rt.max()):.3f}"
            assert float(rt.max()) <= 0.5, line
        print(line + "   " + ", ".join(f"{k} {v:.3f}" for k, v in _class_max(r, rows, heads).items()))
        worst[fam] = max(worst.get(fam, 0.0), float(r.max()))
    print("largest restated |err| / B per family:", worst)


@pytest.mark.parametrize("fam", ["split", "hi"])
def test_balanced_bound_is_sound(fam):
    qkv, pad, wins, rows = S.case("balanced")
    tile0, _ = S.bal_cuts(128, S.BALANCED["groups"])
    ks = list(range(tile0 * 32, 4096))
    q3, p3 = S.take_heads(qkv, 32, BAL_HEADS), S.take_heads(pad, 32, BAL_HEADS)
    pl, pp = _planes(q3, p3, fam)
    ref, B = S.reference_and_bound(pl, pp, wins, 3, fam, pieces=4, rows=ks)
    out, _ = S.restate(pl, pp, wins, 3, fam, balanced_groups=S.BALANCED["groups"], full_pass=False)
    r = S.ratio((out - ref).abs()[ks], B[ks])
    print(f"balanced {fam}: restated max |err| / B {float(r.max()):.3f}")
    assert float(r.max()) <= 0.5
    if fam == "split":
        rt = S.ratio((S.torch_fp32_attention(pl, pp, wins, 3) - ref).abs()[ks], B[ks])
        print(f"balanced {fam}: torch fp32 {float(rt.max()):.3f}")
        assert float(rt.max()) <= 0.5
        for var in ("merge_no_factor", "merge_norm_largest_l", "merge_drop_last"):
            out, _ = S.restate(pl, pp, wins, 3, fam, variant=var, balanced_groups=S.BALANCED["groups"], full_pass=False)
            rv = S.ratio((out - ref).abs()[ks], B[ks])
            print(f"balanced {fam}, {var}: max |err| / B {float(rv.max()):.3g}")
            assert float(rv.max()) > 1.0, var


# ------------------------------------------------------------------------------------------------ sensitivity

FIRING = {f"spike {d!r}" for d in S.SPIKE_FP32[2:] + S.SPIKE_HI}
AIMED = {
    "l_not_rescaled": FIRING, "O_not_rescaled": FIRING, "alpha_sign_flipped": FIRING,
    "p_against_new_max": {"spike 7.5", f"spike {S.SPIKE_FP32[1]!r}"},
    "reference_never_moved": {"spike 46.0", "spike 120.0"},
    "P_lo_dropped": {"spike 7.5", f"spike {S.SPIKE_FP32[1]!r}", "random", "calm"},
    "rowsum_unrounded": {"sharp spike 12.5"},
    "halves_not_added": {"flat"},
    "masked_key_counted": {"flat", "calm", "random"},
}


@pytest.mark.parametrize("fam,kind,key", [("split", "win", (24, 48, (24, 24))), ("hi", "win", (24, 48, (24, 24))),
                                          ("split", "global", ()), ("f32", "win", (18, 36, (18, 36), 72)),
                                          ("hyper", "hyper", (100, 3, 72))],
                         ids=["split", "hi", "split-global", "f32-ragged", "hyper"])
def test_wrong_variants_break_the_bound_on_the_class_aimed_at_them(fam, kind, key):
    qkv, pad, wins, rows = S.case(kind, *key)
    heads = key[1] if kind == "hyper" else 2
    pl, pp = _planes(qkv, pad, fam)
    ref, B = S.reference_and_bound(pl, pp, wins, heads, fam)
    variants = [v for v, fams in S.VARIANTS.items() if fam in fams] if fam != "hyper" else ["merge_no_factor", "halves_not_added"]
    assert variants
    for var in variants:
        out, _ = S.restate(pl, pp, wins, heads, fam, variant=var)
        cm = _class_max(S.ratio((out - ref).abs(), B), rows, heads)
        broken = {k for k, v in cm.items() if v > 1.0}
        print(f"{fam} {var}: max |err| / B {max(cm.values()):.3g}, classes broken: {sorted(broken)}")
        if var in S.HARMLESS:
            assert max(cm.values()) <= 0.5, (var, cm)       # the bound does not depend on who decides
        elif fam == "hyper":
            assert broken, var
        else:
            assert broken & AIMED[var], (var, cm)


# ------------------------------------------------------------------------------------------------ the branch record


@pytest.mark.parametrize("kind,key", [("win", (24, 48, (24, 24))), ("win", (20, 44, (24, 24))), ("global", ())],
                         ids=["24x48", "20x44-padded", "global"])
def test_branch_record_is_the_designed_one(kind, key):
    """per (window, head, wave, key tile): the fp32 restatement takes the rescale branch exactly where the float64 one
    does, and where the design of the wave's theme says (7.5 and 8 - 2^-6: never after the first tile; 8 + 2^-6 and
    above: at the spike's tile; staircases: every second / every tile)"""
    qkv, pad, wins, rows = S.case(kind, *key)
    padded = bool((wins.tok_of < 0).any())
    for fi, fam in enumerate(("split", "hi")):
        pl, pp = _planes(qkv, pad, fam)
        _, rec32 = S.restate(pl, pp, wins, 2, fam)
        _, rec64 = S.restate(pl, pp, wins, 2, fam, dtype=np.float64)
        checked = 0
        for (w, h), r32 in rec32.items():
            assert np.array_equal(r32, rec64[(w, h)]), (fam, w, h)
            nt = r32.shape[1]
            for wave in range(r32.shape[0]):
                toks = wins.tok_of[w][32 * wave:32 * wave + 32]
                toks = toks[toks >= 0]
                if not len(toks):
                    continue
                theme = int(rows["theme"][toks[0], h])
                assert (rows["theme"][toks, h] == theme).all()
                site_tile = rows["sites"][S.wave_site(rows, wave, w, h)][0] // 32
                want = S.designed_record(theme, site_tile, nt, padded)[fi]
                if want is not None:
                    assert tuple(np.nonzero(r32[wave])[0]) == want, (fam, w, h, wave, S.THEMES[theme])
                    checked += 1
        assert checked >= (5 if padded else 36)          # (unpadded: every wave of the launch)
