"""The hand-staged key-tile body of the fp32-accurate split attention kernels (cra5_amd/csrc/attention_split_f16.hip:
every MFMA of a tile followed by its own share of the softmax, the wait state in front of the v_fma_mix pair kept by the
layout instead of an s_nop) at the shapes where a mis-placed stage would show: 1, 2 and 3 key tiles (the odd and even
tails of the loop unrolled by two), a tall window whose grid needs pad rows, a window whose last 128-query work-group has
idle waves, and the balanced whole-grid launch with its short key-split segments.  Two input sets each: random normal, and
one whose per-query maximum rises by 16 log2 units (more than the deferral threshold 2^8) in the second and in the third
key tile, so that the rescale branch at the top of the tile is taken after the first tile.

Reference: oracle.torch_ref.attention_window in float64, on the operands as the split store holds them.  Bound: the
per-element B of tests/softmax_helpers.py as it stands, |got - ref| <= B on every element of every live query, for the fp32
output and (with the store's own term) the split output."""
import numpy as np
import pytest
import torch

import exact_helpers as X
import softmax_helpers as S
from cra5_amd import ops
from oracle import torch_ref as R

pytestmark = pytest.mark.gpu

HEADS, HD = 2, 64
RISE = 16.0          # log2 units per key tile, tiles 1 and 2: twice DEFER_LOG2, the random part of a score has sigma 1.44

# (label, H, W, (wh, ww)): 2 heads x 64
WINDOWED = (("1 key tile", 8, 16, (4, 8)), ("2 key tiles", 16, 16, (8, 8)), ("3 key tiles", 16, 24, (8, 12)),
            ("pad rows", 50, 24, (48, 12)), ("idle waves", 16, 20, (16, 10)))
_CASES = {}


def _inputs(H, W, wh, ww, heads, kind, seed):
    """(qkv fp32 [N, 3C], pad row fp32 [3C], windows): random normal, every value replaced by what the split store keeps
    of it (22 bits).  kind "rescale": feature 0 of every query holds RISE / c and feature 0 of a key its key tile, capped at
    2 (the pad row's: 0) - the scores of tile 1 stand RISE log2 units above tile 0's, those of tiles 2.. another RISE
    (tiles of pad positions do not rise: the 48 x 12 windows of the 50 x 24 grid's second window row see a fall instead)."""
    key = (H, W, wh, ww, heads, kind)
    if key not in _CASES:
        wins = X.Windows(H, W, wh, ww)
        N = H * W
        g = torch.Generator().manual_seed(seed)
        qkv = torch.randn(N, 3, heads, HD, generator=g)
        pad = torch.randn(3, heads, HD, generator=g)
        if kind == "rescale":
            qkv[:, 0, :, 0] = RISE / S.c_of(HD)
            qkv[:, 1, :, 0] = torch.from_numpy(np.minimum(wins.loc_of // 32, 2)).float()[:, None]
            pad[1, :, 0] = 0.0
        exact = lambda a: sum(X.split_model(a.float())).contiguous()
        _CASES[key] = (exact(qkv.reshape(N, -1)), exact(pad.reshape(-1)), wins)
    return _CASES[key]


def _split_inputs(qkv, pad, dev):
    """(qkv SplitMat, pad SplitMat, float64 (hi, lo) planes of both, read back from the device store)"""
    qs, ps = ops.split_f16(qkv.to(dev)), ops.split_f16(pad.reshape(1, -1).to(dev))
    planes = []
    for sm, x in ((qs, qkv), (ps, pad.reshape(1, -1))):
        h, l = sm.planes()
        assert torch.equal(h + l, x.to(dev)), "the split store does not hold the inputs exactly"
        planes.append((h.double(), l.double()))
    return qs, ps, planes[0], (planes[1][0].reshape(-1), planes[1][1].reshape(-1))


def _oracle(qkv, pad, heads, H, W, ws, device):
    """oracle.torch_ref.attention_window in float64 -> [N, C], the attention alone.  The oracle runs qkv = x Wq^T + b,
    windows, softmax, proj; one head at a time it gets x = [q_h | k_h | v_h] - b with b the head's pad-row slice (a zero-
    padded position then carries exactly the pad row), 0 / 1 weights that copy x's columns into the (q, k, v) of three
    identical heads, and the identity as proj: every product and sum of those two linear maps is exact in float64."""
    N = qkv.shape[0]
    q3, p3 = qkv.double().to(device).view(N, 3, heads, HD), pad.double().to(device).view(3, heads, HD)
    sel = torch.zeros(3, 3, HD, 3, HD, dtype=torch.float64, device=device)      # (part, head', d) <- (part, d)
    for s in range(3):
        for hh in range(3):
            sel[s, hh, :, s, :] = torch.eye(HD, dtype=torch.float64, device=device)
    sel = sel.view(9 * HD, 3 * HD)
    out = torch.zeros(N, heads * HD, dtype=torch.float64, device=device)
    for h in range(heads):
        b = p3[:, h].reshape(-1)
        full = q3[:, :, h].reshape(N, -1)
        x = full - b
        assert torch.equal(x + b, full), "x + pad row does not give the stored operands back exactly"
        sd = {"attn.qkv.weight": sel, "attn.qkv.bias": sel @ b, "attn.proj.weight": torch.eye(3 * HD, dtype=torch.float64, device=device),
              "attn.proj.bias": torch.zeros(3 * HD, dtype=torch.float64, device=device)}
        out[:, h * HD:(h + 1) * HD] = R.attention_window(x[None], sd, "attn", 3, H, W, ws)[0][:, :HD]
    return out


def _check(out, out_s, ref, B, label, rows=None):
    """|out - ref| <= B and |out_split - ref| <= B + the store's term on every element of `rows` (default: all)"""
    idx = torch.arange(out.shape[0], device=out.device) if rows is None else torch.as_tensor(rows, device=out.device)
    o, o_s, r, b = out[idx].double(), out_s[idx].double(), ref.to(out.device)[idx], B.to(out.device)[idx]
    assert bool(torch.isfinite(b).all()) and bool(torch.isfinite(r).all())
    ratio, ratio_s = S.ratio((o - r).abs(), b), S.ratio((o_s - r).abs(), b + S.split_store_term(r, "split"))
    i = int(ratio.argmax())
    print(f"{label}: max |err| / B {float(ratio.max()):.3f} (split output {float(ratio_s.max()):.3f}) at token "
          f"{int(idx[i // o.shape[1]])}, column {i % o.shape[1]}; max |err| {float((o - r).abs().max()):.3e}")
    assert float(ratio.max()) <= 1.0, f"{label}: fp32 output outside the bound, |err| / B = {float(ratio.max()):.3f}"
    assert float(ratio_s.max()) <= 1.0, f"{label}: split output outside the bound, |err| / B = {float(ratio_s.max()):.3f}"


def _run(qs, ps, heads, H, W, wh, ww, dev, workspace=None):
    N, C = H * W, qs.K // 3
    out = torch.full((N, C), float("nan"), device=dev)
    out_s = ops.SplitMat.empty(N, C, dev, zero=True)
    ops.window_attention_split(qs, ps, heads, H, W, wh, ww, out=out, out_split=out_s, workspace=workspace)
    return out, out_s.to_float()


@pytest.mark.parametrize("kind", ["normal", "rescale"])
@pytest.mark.parametrize("label,H,W,ws", WINDOWED, ids=[c[0].replace(" ", "_") for c in WINDOWED])
def test_staged_key_tile_windowed(dev, label, H, W, ws, kind):
    """4-wave work-groups: 32-, 64- and 96-token windows (1, 2, 3 key tiles), 48 x 12 windows on a 50 x 24 grid (the second
    window row holds 2 real and 46 pad rows; 18 key tiles), 16 x 10 windows (160 queries: the second work-group runs one live wave and three
    idle ones that only stage and synchronise)"""
    assert ops.split_attention_ok(HEADS * HD, HEADS, ws[0], ws[1], H, W)
    qkv, pad, wins = _inputs(H, W, ws[0], ws[1], HEADS, kind, seed=H * 100 + W)
    qs, ps, planes, pad_planes = _split_inputs(qkv, pad, dev)
    _, B = S.reference_and_bound(planes, pad_planes, wins, HEADS, "split")
    ref = _oracle(qkv, pad, HEADS, H, W, ws, "cpu")
    out, out_s = _run(qs, ps, HEADS, H, W, ws[0], ws[1], dev)
    _check(out, out_s, ref, B, f"staged key tile, {label}, {kind} inputs, {H}x{W} {ws}")


@pytest.mark.parametrize("kind", ["normal", "rescale"])
def test_staged_key_tile_balanced(dev, kind):
    """the balanced whole-grid launch of tests/test_softmax_gpu.py (64 x 64 tokens, 32 heads, 12-wave work-groups): on 256
    CUs 96 full wave-tiles and 32 key-split ones whose 128-tile key loops are cut into segments of 48 tiles, the last ones
    shorter.  Key-split tokens against the bound (float64 reference formed on the device); full-pass tokens equal the plain
    launch bit for bit, and the plain launch is held to the bound on a sample of them."""
    b = S.BALANCED
    H, W, heads = b["H"], b["W"], b["heads"]
    N = H * W
    if torch.cuda.get_device_properties(dev).multi_processor_count != 256:
        pytest.skip("the plan is written out for 256 CUs")
    ok, nb = ops.attention_balanced_plan(N, heads)
    tile0, grps = S.bal_cuts(N // 32, b["groups"])
    assert ok and nb > 0
    qkv, pad, wins = _inputs(H, W, H, W, heads, kind, seed=77)
    qs, ps, planes, pad_planes = _split_inputs(qkv, pad, dev)
    plain, plain_s = _run(qs, ps, heads, H, W, H, W, dev)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev).fill_(0xFF)
    out, out_s = _run(qs, ps, heads, H, W, H, W, dev, workspace=ws)
    n_full = tile0 * 32
    assert torch.equal(out[:n_full], plain[:n_full]) and torch.equal(out_s[:n_full], plain_s[:n_full])
    ref = _oracle(qkv, pad, heads, H, W, (H, W), dev)
    ks = list(range(n_full, N))
    _, B = S.reference_and_bound(planes, pad_planes, wins, heads, "split", pieces=max(len(p) for _, p in grps), rows=ks)
    _check(out, out_s, ref, B, f"staged key tile, balanced launch key-split tokens, {kind} inputs", rows=ks)
    fs = list(range(0, n_full, 37))
    _, Bf = S.reference_and_bound(planes, pad_planes, wins, heads, "split", rows=fs)
    _check(plain, plain_s, ref, Bf, f"staged key tile, plain 12-wave launch full-pass sample, {kind} inputs", rows=fs)
