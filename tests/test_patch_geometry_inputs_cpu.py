"""The geometries, inputs and references of tests/test_patch_geometry_gpu.py, checked without a GPU: every superset
subset.token_plan can return falls in classes the case list covers, unembed_expectation is the float64 transposed
convolution away from 72 x 144 too, every exact input passes its exactness conditions (so a GPU run cannot fail with
InputNotExact), and the dispatch classifier restates the launchers' rule."""
import ast
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import exact_helpers as X
import patch_geometry_helpers as G
import split_helpers as S
from cra5_amd import subset

H, W = 721, 1440


def _planes(n_ti, n_tj, C, K):
    """the split planes of the exact un-embed operands as split_f16(a) / split_f16(w, 'auto') store them (the grid's
    max |w| is in [1, 2): 'auto' scales by 2^12), checked"""
    a, w = G.unembed_operands(n_ti, n_tj, C, K)
    assert 1.0 <= float(w.abs().max()) < 2.0
    pa, pw = X.split_model(a), X.split_model(w, 4096.0)
    X.check_planes(a, pa[0], pa[1], 1.0, "A")
    X.check_planes(w, pw[0], pw[1], 1.0 / 4096.0, "W")
    return pa, pw


# ------------------------------------------------------------------------------------------------ coverage


def test_case_list_is_well_formed():
    assert len(set(G.GEOMETRIES)) == len(G.GEOMETRIES)
    for n_ti, n_tj, stands_for in G.CASES:
        cls = G.geometry_classes(n_ti, n_tj)
        assert set(stands_for) <= cls, (n_ti, n_tj, set(stands_for) - cls)
        H_, W_ = G.image_shape(n_ti, n_tj)
        assert (H_, W_) == (10 * n_ti + 1, 10 * n_tj) and W_ % 4 == 0
        # the issue's size limit: no case above 1008 tokens x 880 columns x K = 128
        assert n_ti * n_tj <= 1008 and max(G.UNEMBED_CHANNELS) * 110 <= 880
    covered = frozenset().union(*(G.geometry_classes(a, b) for a, b in G.GEOMETRIES))
    assert covered == G.ALL_CLASSES, sorted(G.ALL_CLASSES - covered)
    # the classes the table of the case list names, by the geometry that stands for each
    table = {(1, 2): {G.M_SUB, G.ROWS_1}, (2, 2): {G.ROWS_2}, (2, 6): {G.ROWS_2}, (34, 2): {G.W_THIN, G.M_PART},
             (72, 2): {G.W_THIN, G.M_PART}, (16, 16): {G.M_ONE, G.TILED_W[1]}, (3, 86): {G.M_TAIL_SUB},
             (16, 30): {G.CUT_INSIDE}, (1, 16): {G.TILED_HP[1], G.TILED_W[1]}, (2, 16): {G.TILED_HP[2]},
             (3, 32): {G.TILED_HP[3], G.TILED_W[2]}, (1, 48): {G.TILED_W[3]}, (7, 144): {G.W_CIRCLE}}
    for (n_ti, n_tj), want in table.items():
        assert (n_ti, n_tj) in G.GEOMETRIES and want <= G.geometry_classes(n_ti, n_tj), (n_ti, n_tj)
    assert 3 * 86 == 258 and 16 * 30 == 480 and (256 // 30, 256 % 30) == (8, 16) and 7 * 144 == 1008


def _row_edges():
    r0s = sorted({v for t in range(73) for v in (10 * t, 10 * t + 1, 10 * t + 5, 10 * t + 9) if v < H})
    r1s = sorted({v for t in range(73) for v in (10 * t, 10 * t + 1, 10 * t + 2, 10 * t + 6) if 0 < v <= H} | {H})
    return r0s, r1s


def _col_edges():
    c0s = sorted({v for t in range(144) for v in (10 * t, 10 * t + 3, 10 * t + 9)})
    ncs = sorted({v for k in range(146) for v in (10 * k - 1, 10 * k, 10 * k + 1, 10 * k + 2) if 1 <= v <= W} | {1, W})
    return c0s, ncs


def test_every_reachable_superset_is_covered_by_a_case():
    """token_plan is separable (rows decide ti0 / n_ti, columns tj0 / n_tj): rows and columns are enumerated over aligned
    and unaligned edges each - the wrap at column 1440 and the cap to the whole circle included - and a seeded sample of
    whole boxes checks the two halves meet.  Every (ti0, n_ti) and every (tj0, n_tj) the plan can produce is reached."""
    r0s, r1s = _row_edges()
    c0s, ncs = _col_edges()
    rows, cols = set(), set()
    for r0 in r0s:
        for r1 in r1s:
            if r1 > r0:
                p = subset.token_plan((r0, r1, 0, 1), H, W)
                rows.add((p["ti0"], p["n_ti"]))
    wrapped = capped = 0
    for c0 in c0s:
        for nc in ncs:
            p = subset.token_plan((0, 1, c0, nc), H, W)
            cols.add((p["tj0"], p["n_tj"]))
            assert p["n_tj"] % 2 == 0 and p["Ws"] == 10 * p["n_tj"] and p["Hs"] == 10 * p["n_ti"] + 1
            wrapped += p["tj0"] + p["n_tj"] > G.GRID_WP
            capped += p["n_tj"] == G.GRID_WP and nc < W
    assert wrapped > 1000 and capped > 100
    assert rows == {(t0, n) for t0 in range(72) for n in range(1, 73 - t0)}
    assert cols == {(t0, n) for t0 in range(144) for n in range(2, 144, 2)} | {(0, 144)}
    rng = np.random.default_rng(0)
    for _ in range(20000):
        r0, c0 = int(rng.integers(0, H)), int(rng.integers(0, W))
        box = (r0, int(rng.integers(r0 + 1, H + 1)), c0, int(rng.integers(1, W + 1)))
        p = subset.token_plan(box, H, W)
        assert (p["ti0"], p["n_ti"]) in rows and (p["tj0"], p["n_tj"]) in cols
    covered = frozenset().union(*(G.geometry_classes(a, b) for a, b in G.GEOMETRIES))
    shapes = {(n_ti, n_tj) for _, n_ti in rows for _, n_tj in cols}
    assert len(shapes) == 72 * 72
    for n_ti, n_tj in shapes:
        cls = G.geometry_classes(n_ti, n_tj)
        assert cls <= covered, (n_ti, n_tj, sorted(cls - covered))
        assert len(cls) >= 3


def test_model_boxes_map_to_the_supersets_they_claim():
    want = {(16, "not circle"): 0, "M256": 0, "3x86": 0, "top": 0, "bottom": 0, "east": 0}
    for box, (ti0, n_ti, tj0, n_tj), why in G.MODEL_BOXES:
        p = subset.token_plan(box, H, W)
        assert (p["ti0"], p["n_ti"], p["tj0"], p["n_tj"]) == (ti0, n_ti, tj0, n_tj), (box, why, p)
        tiled = n_tj % 16 == 0 and n_tj != G.GRID_WP
        want[(16, "not circle")] += n_tj == 16 and tj0 + n_tj <= G.GRID_WP
        want["east"] += n_tj == 16 and tj0 + n_tj > G.GRID_WP
        want["M256"] += (n_ti, n_tj) == (16, 16)
        want["3x86"] += (n_ti, n_tj) == (3, 86)
        want["top"] += tiled and ti0 == 0
        want["bottom"] += tiled and ti0 + n_ti == G.GRID_HP
    assert all(v >= 1 for v in want.values()), want
    # ... and they are the boxes the model-level test really runs
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_subset_decode_gpu.py")).read()
    node = next(n for n in ast.parse(src).body if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", "") == "BOXES")
    boxes = ast.literal_eval(node.value)
    for box, _, why in G.MODEL_BOXES:
        assert box in boxes, (box, why)
    assert len(G.MODEL_BOXES) <= 10


# ------------------------------------------------------------------------------------------------ un-embed expectation


@pytest.mark.parametrize("n_ti,n_tj", G.GEOMETRIES)
def test_unembed_expectation_is_the_float64_transposed_convolution(n_ti, n_tj):
    """unembed_expectation off 72 x 144: equal, bit for bit in float64, to fold of the same column matrix and to
    conv_transpose2d of the operands themselves (on the grid every float64 partial sum is exact, so the order of the
    convolution's sums cannot show); the de-normalised form too."""
    Hs, Ws = G.image_shape(n_ti, n_tj)
    for C in G.UNEMBED_CHANNELS:
        pa, pw = _planes(n_ti, n_tj, C, 128)
        mean, std = G.exact_stats(C)
        for hi in (False, True):
            e, g, _ = X.three_product_expectation(pa, pw, 1.0 / 4096.0, hi_only=hi)
            for m_, s_ in ((None, None), (mean, std)):
                exp = X.unembed_expectation(e, C, n_ti, n_tj, G.KH, G.KW, mean=m_, std=s_)
                assert exp.dtype == torch.float64 and tuple(exp.shape) == (C, Hs, Ws)
                assert torch.equal(exp, G.col2im_reference(e, C, n_ti, n_tj, mean=m_, std=s_))
        # hi_only is one product: the transposed convolution of the hi planes
        tok = pa[0].double().t().reshape(1, 128, n_ti, n_tj)
        wt = pw[0].double().view(C, G.KH, G.KW, 128).permute(3, 0, 1, 2).contiguous()
        conv = F.conv_transpose2d(tok, wt, stride=(G.SH, G.SW))[0] / 4096.0
        assert torch.equal(conv, X.unembed_expectation(e, C, n_ti, n_tj, G.KH, G.KW))


@pytest.mark.parametrize("n_ti,n_tj", G.GEOMETRIES)
def test_exact_unembed_inputs_pass_every_exactness_condition(n_ti, n_tj):
    """every (geometry, C, K, form) the GPU test runs: check_planes and the three-product conditions hold, and the
    overlap-add and the de-normalisation are exact IN FP32 - evaluated here in fp32, seam partners in both orders"""
    for C in G.UNEMBED_CHANNELS:
        mean, std = G.exact_stats(C)
        assert bool((std == 2.0 ** torch.log2(std).round()).all()) and bool((mean == mean.round()).all())
        for _, K, hi, _ in G.UNEMBED_FORMS:
            pa, pw = _planes(n_ti, n_tj, C, K)
            e, g, worst = X.three_product_expectation(pa, pw, 1.0 / 4096.0, hi_only=hi)
            assert worst < X.LIMIT and g == (1.0 if hi else 2.0 ** -12)
            raw = X.unembed_expectation(e, C, n_ti, n_tj, G.KH, G.KW)
            den = X.unembed_expectation(e, C, n_ti, n_tj, G.KH, G.KW, mean=mean, std=std)
            assert torch.equal(raw.float().double(), raw) and torch.equal(den.float().double(), den)
            e32 = e.float()
            assert torch.equal(e32.double(), e)
            raw32 = G.col2im_reference(e32, C, n_ti, n_tj)                      # fp32 sums
            assert raw32.dtype == torch.float32 and torch.equal(raw32.double(), raw)
            prod = raw32 * std[:, None, None]                                    # fp32, rounded (un-contracted form)
            assert torch.equal(prod.double(), raw * std.double()[:, None, None])
            assert torch.equal((prod + mean[:, None, None]).double(), den)


@pytest.mark.parametrize("n_ti,n_tj", G.GEOMETRIES)
def test_col2im_inputs(n_ti, n_tj):
    for C in G.COL2IM_CHANNELS:
        mean, std = G.exact_stats(C)
        cols = G.exact_cols(n_ti, n_tj, C)
        s64 = G.col2im_reference(cols.double(), C, n_ti, n_tj)
        s32 = G.col2im_reference(cols, C, n_ti, n_tj)
        assert torch.equal(s32.double(), s64)
        den = G.col2im_reference(cols.double(), C, n_ti, n_tj, mean=mean, std=std)
        assert torch.equal(den.float().double(), den)
        assert torch.equal((s32 * std[:, None, None] + mean[:, None, None]).double(), den)
        q = G.quantised_cols(n_ti, n_tj, C)
        assert torch.equal(G.col2im_reference(q, C, n_ti, n_tj).double(), G.col2im_reference(q.double(), C, n_ti, n_tj))
        # the fp32 fold of random data is the correctly rounded two-term sum
        r = G.random_cols(n_ti, n_tj, C)
        assert torch.equal(G.col2im_reference(r, C, n_ti, n_tj), G.col2im_reference(r.double(), C, n_ti, n_tj).float())
        # the bound: both evaluation orders of s * std + mean lie inside it
        m, sd = G.random_stats(C, seed=C)
        sq = G.col2im_reference(q.double(), C, n_ti, n_tj)
        exact = sq * sd.double()[:, None, None] + m.double()[:, None, None]
        b = G.denorm_bound(sq, sd, m)
        two = sq.float() * sd[:, None, None] + m[:, None, None]
        one = exact.float()
        for got in (one, two):
            assert bool(((got.double() - exact).abs() <= b).all())


def test_col2im_reference_places_every_column():
    """a one-hot column matrix: element (token (ti, tj), column (c, ky, kx)) lands on x[c][10 ti + ky][10 tj + kx]"""
    C, Hp, Wp = 3, 3, 4
    for tok, c, ky, kx in [(0, 0, 0, 0), (5, 1, 10, 9), (11, 2, 10, 0), (6, 2, 0, 3), (9, 0, 4, 7)]:
        cols = torch.zeros(Hp * Wp, C * 110, dtype=torch.float64)
        cols[tok, (c * 11 + ky) * 10 + kx] = 1.0
        img = G.col2im_reference(cols, C, Hp, Wp)
        want = torch.zeros_like(img)
        want[c, 10 * (tok // Wp) + ky, 10 * (tok % Wp) + kx] = 1.0
        assert torch.equal(img, want)
        x = torch.arange(C * 36 * 44, dtype=torch.float64).view(C, 36, 44)      # larger than the patches cover
        assert float(G.im2col_reference(x, Hp, Wp)[tok, (c * 11 + ky) * 10 + kx]) == float(
            x[c, 10 * (tok // Wp) + ky, 10 * (tok % Wp) + kx])


def test_im2col_inputs():
    for Hp, Wp in G.IM2COL_GEOMETRIES:
        for C in G.IM2COL_CHANNELS:
            x, mean, std = G.im2col_image(Hp, Wp, C)
            assert x.shape[1] == 10 * Hp + 5 and x.shape[1] > G.image_shape(Hp, Wp)[0]
            assert x.shape[2] == (150 if Wp == 15 else 10 * Wp + 4)
            assert ((x.shape[1] - 11) // 10 + 1, (x.shape[2] - 10) // 10 + 1) == (Hp, Wp)     # what ops.im2col derives
            ref = G.im2col_reference(x, Hp, Wp, mean, std)
            assert ref.dtype == torch.float32 and tuple(ref.shape) == (Hp * Wp, C * 110)
            # the split model of that reference holds no value the store cannot carry
            assert not (S.classify(ref.numpy()) & ~np.uint8(S.FINITE_IN_RANGE)).any()


# ------------------------------------------------------------------------------------------------ dispatch


def test_dispatch_classification():
    for n_tj in range(2, 146, 2):
        for C in range(1, 9):
            K = C * 110
            for op in ("col2im", "im2col"):
                k = G.classify(3, n_tj, C, K, 0, op)["kernel"]
                # production: cols is (M, C * 110), freshly allocated (aligned)
                assert k == ("tiled" if n_tj % 16 == 0 and C % 2 == 0 else "generic"), (op, n_tj, C)
                assert G.classify(3, n_tj, C, K, 4, op)["kernel"] == "generic"                # unaligned pointers
                assert G.classify(3, n_tj, C, K, (0, 4), op)["kernel"] == "generic"         # unaligned image
                kp = G.classify(3, n_tj, C, G.padded_pitch(K), 0, op)["kernel"]
                assert kp == ("tiled" if n_tj % 16 == 0 else "generic")                      # odd C reaches the tiled kernel
                assert G.padded_pitch(K) % 4 == 0 and G.padded_pitch(K) >= K + 4
    assert G.classify(3, 16, 2, 220, (4, 0), "col2im")["kernel"] == "generic"                # unaligned column matrix
    assert G.classify(3, 16, 2, 220, (4, 0), "im2col")["kernel"] == "tiled"                  # (im2col only reads the image's)
    assert G.classify(3, 16, 2, 220, 0, "im2col", W=164)["kernel"] == "tiled"
    assert G.classify(3, 16, 2, 220, 0, "im2col", W=162)["kernel"] == "generic"              # W % 4 != 0
    assert G.kernel_choice("im2col", 15, 220, W=150) == "generic"
    for Hp, Wp in G.IM2COL_GEOMETRIES:                                                          # both kernels are in the list
        assert (G.kernel_choice("im2col", Wp, 224, W=150 if Wp == 15 else 10 * Wp + 4) == "tiled") == (Wp % 16 == 0)
    odd = G.classify(1, 16, 5, 550)["classes"]
    assert any("one channel" in c for c in odd) and any("3 tile column" in c for c in odd)
    assert any("2 block(s) per token tile, the last walks 1 chunk" in c for c in odd)
    assert any("inside a (c, ky) run" in c for c in G.channel_classes(3)) and (256 // 10) % 11 == 3 and 256 % 10 == 6
    assert not any("inside a (c, ky) run" in c for c in G.channel_classes(2))


def test_guarded_buffer_and_locator():
    buf = G.guarded(10, "cpu")
    assert buf.numel() == 10 + G.TAIL and bool(torch.isnan(buf[:10]).all()) and G.tail_intact(buf, 10)
    buf[10 + 5] = 0.0
    assert not G.tail_intact(buf, 10)
    loc = G.unembed_locator(31)
    assert loc(31 + 20, 47) == "channel 1, image row 20 (token row 2, seam of token rows 1 and 2), token column 4"
    assert loc(30, 0) == "channel 0, image row 30 (token row 2), token column 0"
