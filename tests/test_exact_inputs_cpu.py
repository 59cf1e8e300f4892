"""The exact-arithmetic inputs of tests/test_exact_gpu.py, checked without a GPU: on these inputs fp32 accumulation of
the three-product model gives the float64 expectation in ANY order, the in-test exactness conditions refuse inputs that
are not exact, the attention expectations equal a plain float64 softmax attention, and the mismatch report names the
right tile / key for deliberately broken outputs."""
import numpy as np
import pytest
import torch

import exact_helpers as X


def _planes(x, scale=1.0):
    hi, lo = X.split_model(x, scale)
    X.check_planes(x, hi, lo, 1.0 / scale, "operand")
    return hi, lo


@pytest.mark.parametrize("K,density", [(1024, 1.0), (4096, 0.75), (29480, 0.1), (32, 1.0)])
def test_three_product_model_is_order_independent_in_fp32(K, density):
    """All 3K terms of an output element accumulated in fp32 in shuffled orders (and as the MFMA would: 16-product
    blocks summed first) equal the float64 sum - so tile shape, k-step width, split-K and the MFMA's internal reduction
    order cannot show on these inputs.  The weight is stored scaled by 2^12, as split_f16(w, 'auto') stores it."""
    M, N = 6, 5
    a, w = X.grid_matrix(M, K, density, seed=K), X.grid_matrix(N, K, density, seed=K + 1)
    (ha, la), (hw, lw) = _planes(a), _planes(w, 4096.0)
    assert float(hw.abs().max()) == 4096.0 and float(lw.abs().max()) == 1.0 and float(la.abs().max()) == 2.0 ** -12
    e, g, worst = X.three_product_expectation((ha, la), (hw, lw), 1.0 / 4096.0)
    print(f"K = {K}, density {density}: max sum |term| = {worst:.3g} granules of {g!r}")
    assert g == 2.0 ** -12 and worst < X.LIMIT
    rng = np.random.default_rng(K)
    terms = np.concatenate([(ha[:, None] * hw[None]).numpy(), (ha[:, None] * lw[None]).numpy(),
                            (la[:, None] * hw[None]).numpy()], -1).astype(np.float32)          # [M, N, 3K]
    for _ in range(4):
        t = terms[:, :, rng.permutation(3 * K)]
        acc = np.zeros((M, N), dtype=np.float32)
        for k in range(3 * K):
            acc = (acc + t[:, :, k]).astype(np.float32)
        assert np.array_equal(acc.astype(np.float64) / 4096.0, e.numpy())
        blk = t[:, :, : 3 * K // 16 * 16].reshape(M, N, -1, 16).sum(-1, dtype=np.float32).sum(-1, dtype=np.float32)
        rest = t[:, :, 3 * K // 16 * 16:].sum(-1, dtype=np.float32)
        assert np.array_equal((blk + rest).astype(np.float64) / 4096.0, e.numpy())
    # the model tells "three products" from "four": the dropped lo.lo part is not a whole granule
    full = a.double() @ w.double().t()
    assert bool((full != e).any()) and float((full - e).abs().max()) < 2.0 ** -12
    # hi_only: the hi.hi sum alone
    e_hi, g_hi, _ = X.three_product_expectation((ha, la), (hw, lw), 1.0 / 4096.0, hi_only=True)
    assert g_hi == 1.0 and torch.equal(e_hi, ha.double() @ hw.double().t() / 4096.0)


def test_exactness_conditions_refuse_inexact_inputs():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(8, 64, generator=g)
    hi, lo = X.split_model(x)
    with pytest.raises(X.InputNotExact, match="hi \\+ lo differs"):          # 24-bit values do not fit 22 bits
        X.check_planes(x, hi, lo, 1.0, "random operand")
    tiny = X.grid_matrix(4, 32, 1.0, seed=2) * 2.0 ** -6                     # lo = 2^-18: an f16 subnormal
    hi, lo = X.split_model(tiny)
    with pytest.raises(X.InputNotExact, match="subnormal"):
        X.check_planes(tiny, hi, lo, 1.0, "tiny operand")
    a, w = X.grid_matrix(4, 29480, 1.0, seed=3), X.grid_matrix(4, 29480, 1.0, seed=4)   # density 1 at K = 29 480
    with pytest.raises(X.InputNotExact, match="2\\^24"):
        X.three_product_expectation(_planes(a), _planes(w, 4096.0), 1.0 / 4096.0)
    a, w = X.grid_matrix(4, 64, 1.0, seed=5), X.grid_matrix(4, 64, 1.0, seed=6)
    _, g, _ = X.three_product_expectation(_planes(a), _planes(w), 1.0, bias=torch.full((4,), 2.0 ** -13))
    assert g == 2.0 ** -13                                                   # a finer bias refines the granule of the sum
    with pytest.raises(X.InputNotExact, match="not an fp32 number|2\\^24"):
        X.three_product_expectation(_planes(a), _planes(w), 1.0, bias=torch.full((4,), 2.0 ** -30))
    e, g, _ = X.three_product_expectation(_planes(a), _planes(w), 1.0, bias=X.grid_vector(4, 7), res=X.grid_matrix(4, 4, 1.0, 8))
    assert g == 2.0 ** -12
    with pytest.raises(X.InputNotExact, match="gap"):
        X.permutation_case(4, 16, 4, 16, 1, 64, seed=1, s=1, max_draws=2)     # s = 1: the gap cannot reach 48


def _gemm_pair(M=600, N=520, K=64):
    a, w = X.grid_matrix(M, K, 1.0, seed=11), X.grid_matrix(N, K, 1.0, seed=12)
    e, g, _ = X.three_product_expectation(_planes(a), _planes(w), 1.0)
    return e, g


def test_report_names_one_element_and_its_granule():
    e, g = _gemm_pair()
    got = e.float().clone()
    assert X.assert_exact(got, e, g, "clean") == 0.0
    got[300, 515] += 2.0 ** -12
    with pytest.raises(X.ExactMismatch) as ei:
        X.assert_exact(got, e, g, "gemm 600x520x64")
    msg = str(ei.value)
    print(msg)
    assert "1 of 312000 elements differ" in msg and "rows 300..300, columns 515..515" in msg
    assert "256x256: tile row 1, tile column 2" in msg and "192x256: tile row 1, tile column 2" in msg
    assert "128x128: tile row 2, tile column 4" in msg and "64x64: tile row 4, tile column 8" in msg
    assert "whole number of granules" in msg and ": 1" in msg and "(300, 515," in msg and "+1)" in msg
    got[300, 515] = float("nan")                                             # a NaN is a difference, not a pass
    with pytest.raises(X.ExactMismatch):
        X.assert_exact(got, e, g, "nan")


def test_report_names_a_shifted_tile():
    """one 64 x 64 tile written one column to the right: every difference lies in that tile (+ the column it spilt into)"""
    e, g = _gemm_pair()
    got = e.float().clone()
    got[128:192, 257:321] = e.float()[128:192, 256:320]
    with pytest.raises(X.ExactMismatch) as ei:
        X.assert_exact(got, e, g, "shifted tile")
    msg = str(ei.value)
    print(msg)
    assert "64x64: tile row 2, tile column 4..5" in msg and "128x128: tile row 1, tile column 2" in msg
    box = [ln for ln in msg.splitlines() if ln.startswith("bounding box")][0]
    r = [int(v) for v in box.replace("..", " ").replace(",", " ").split() if v.isdigit()]
    assert 128 <= r[0] and r[1] <= 191 and 257 <= r[2] and r[3] <= 320


def test_report_names_a_missing_lo_product():
    """the lo_a.hi_w product dropped in the last tile row only: whole granules, confined to that tile row"""
    M, N, K = 300, 200, 64
    a, w = X.grid_matrix(M, K, 1.0, seed=21), X.grid_matrix(N, K, 1.0, seed=22)
    (ha, la), (hw, lw) = _planes(a), _planes(w)
    e, g, _ = X.three_product_expectation((ha, la), (hw, lw), 1.0)
    got = e.clone()
    got[256:] -= (la.double() @ hw.double().t())[256:]
    with pytest.raises(X.ExactMismatch) as ei:
        X.assert_exact(got.float(), e, g, "edge tiles without lo_a.hi_w")
    msg = str(ei.value)
    print(msg)
    assert "256x256: tile row 1, tile column 0" in msg and "rows 256..299" in msg and "whole number of granules" in msg


@pytest.mark.parametrize("H,W,ws,heads,hd", [(72, 144, (48, 12), 2, 64), (72, 100, (24, 24), 1, 64), (70, 140, (24, 24), 1, 64),
                                             (24, 48, (24, 48), 2, 64), (1, 41, (1, 41), 2, 64), (18, 36, (18, 36), 1, 72)])
def test_uniform_expectation_is_the_float64_attention(H, W, ws, heads, hd):
    """(48, 12): bottom padding; 72 x 100: right only; 70 x 140: both; whole grids: none"""
    qkv, pad, exp, wins = X.uniform_case(H, W, ws[0], ws[1], heads, hd, seed=H + W)
    ref = X.attention_float64(qkv, pad, wins, heads)
    assert float((ref - exp).abs().max()) < 1e-13
    n_pad = wins.n_pad()
    assert int(n_pad.sum()) == wins.Hp * wins.Wp - H * W
    if (H, W, ws) == (72, 100, (24, 24)):
        assert wins.Wp == 120 and wins.Hp == 72 and set(n_pad.tolist()) == {0, 20 * 24}
    if (H, W, ws) == (70, 140, (24, 24)):
        assert (wins.Hp, wins.Wp) == (72, 144) and int(n_pad.max()) == 576 - 22 * 20


@pytest.mark.parametrize("H,W,ws,heads,hd", [(72, 144, (24, 24), 1, 64), (70, 140, (24, 24), 2, 64), (72, 100, (24, 24), 1, 64),
                                             (18, 36, (18, 36), 2, 72), (1, 41, (1, 41), 2, 64)])
def test_permutation_expectation_is_the_float64_attention(H, W, ws, heads, hd):
    qkv, pad, exp, wins, info = X.permutation_case(H, W, ws[0], ws[1], heads, hd, seed=3 * H + W)
    print(f"permutation {H}x{W} {ws}: {info['draws']} draw(s), largest cross-correlation {info['max_cross']} of {hd}, "
          f"gap {info['gap_log2']:.1f} log2 units")
    assert info["gap_log2"] >= 48.0
    ref = X.attention_float64(qkv, pad, wins, heads)
    # the other keys hold < 2^-48 * (keys) of the probability mass
    assert float(((ref - exp).abs() / exp.abs()).max()) < 2.0 ** -30
    assert bool((exp != 0).all()) and len({tuple(r) for r in info["v"][:, :hd].tolist()}) == H * W


def test_permutation_gap_holds_on_the_whole_grid():
    """10 368 tokens as one window, one head: how many draws of u the 48-unit gap takes (the GPU test draws per head)"""
    qkv, pad, exp, wins, info = X.permutation_case(72, 144, 72, 144, 1, 64, seed=5)
    print(f"whole grid: {info['draws']} draw(s), largest cross-correlation {info['max_cross']} of 64, gap {info['gap_log2']:.1f}")
    assert info["gap_log2"] >= 48.0 and info["draws"] <= 20


def test_report_names_swapped_keys():
    """two keys of one 32-key tile swapped (what a wrong transposed V read does): the two queries that match them"""
    H, W, heads, hd = 24, 48, 2, 64
    qkv, pad, exp, wins, info = X.permutation_case(H, W, 24, 24, heads, hd, seed=9)
    got = exp.float().clone()
    j0, j1 = int(wins.tok_of[1][32 * 5 + 3]), int(wins.tok_of[1][32 * 5 + 4])      # window 1, key tile 5, keys 3 and 4
    q0, q1 = int(np.nonzero(info["src"] == j0)[0][0]), int(np.nonzero(info["src"] == j1)[0][0])
    got[q0, hd:], got[q1, hd:] = exp[q1, hd:].float(), exp[q0, hd:].float()         # head 1 only
    with pytest.raises(X.ExactMismatch) as ei:
        X.assert_exact(got, exp, 1.0, "swapped keys", tol=exp.abs() * 2.0 ** -21,
                       locate=X.attention_locator(wins, heads, hd, info), gemm_tiles=False)
    msg = str(ei.value)
    print(msg)
    assert f"key {j0} (window-local {32 * 5 + 3}) expected, got key {j1} (window-local {32 * 5 + 4}, key tile 5)" in msg
    assert f"key {j1} (window-local {32 * 5 + 4}) expected, got key {j0} (window-local {32 * 5 + 3}, key tile 5)" in msg
    assert "window 1, head 1" in msg and "window 0" not in msg and "head 0" not in msg


def test_report_names_a_masked_pad_token():
    """one pad token of one window masked out of the softmax: numerator and count change for that window only"""
    H, W, heads, hd = 72, 100, 1, 64
    qkv, pad, exp, wins = X.uniform_case(H, W, 24, 24, heads, hd, seed=4)
    b = pad[2 * hd:].double()
    w = 9                                                     # window row 1, column 4: the right-hand, padded one
    assert wins.n_pad()[w] == 480
    got = exp.clone()
    rows = torch.from_numpy(wins.tok_of[w][wins.tok_of[w] >= 0])
    got[rows] = (exp[rows] * 576 - b) / 575
    tol = torch.from_numpy(np.spacing(np.abs(exp.float().numpy()))).double() * 4
    with pytest.raises(X.ExactMismatch) as ei:
        X.assert_exact(got.float(), exp, 1.0 / 576, "masked pad token", tol=tol,
                       locate=X.attention_locator(wins, heads, hd), gemm_tiles=False)
    msg = str(ei.value)
    print(msg)
    assert "window 9, head 0" in msg and "window 8" not in msg and "rows 2496..4799, columns 0..63" in msg
    assert f"{96 * 64} of" in msg                            # every element of the window's 96 real tokens
