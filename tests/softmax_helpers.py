"""Per-element forward-error bounds for the streaming softmax of the attention kernels: an input builder that realises
prescribed score profiles per query row, the float64 reference with the bounds B, and an fp32 host restatement of the
documented algorithm (with the wrong variants a bound has to catch) - shared by tests/test_softmax_gpu.py (the
kernels) and tests/test_softmax_inputs_cpu.py (the builder and the bounds themselves: sound and sensitive).

House rules (those of domain_helpers.py): every reference is float64, computed from the operands AS STORED (hi + lo of
the split store; the f16 hi plane alone in the reduced-precision modes); every assertion is |got - ref64| <= B per
element; every constant of B is an operation count derived in the docstring of its function (u = 2^-24), then doubled
- the restatement (exact dot products, exact exp2 and 1/x, one rounding per documented operation) has to stay within
B / 2, the device's MFMA summation order, v_exp_f32 and reciprocal differ from the host's by about as much again.  No
constant comes from a run of a kernel.

Scores live in the log2 domain: t_ij = (q_i . k_j) c with c = head_dim^-0.5 log2 e, p_ij = 2^(t_ij - m).  Nothing here
calls a product kernel; the reference and the bounds run on whatever device their tensors live on."""
import math

import numpy as np
import torch

import exact_helpers as X

U = 2.0 ** -24
FLT_MIN = 2.0 ** -126
LN2 = math.log(2.0)
LOG2E = 1.4426950408889634
DEFER_LOG2 = 8.0            # cra5_amd/csrc/attention_split_f16.hip: the deferral threshold of the fp32-accurate form
P_SAFE = 8192.0             # ... and the row-sum limit of the reduced-precision form (2^13)
MARGIN = 2.0 ** -6          # every designed decision keeps this distance (log2 units) from its threshold

FAMILIES = ("split", "hi", "f32", "hyper")     # fp32-accurate split, reduced precision, exact-f32, hyper
SPIKE_FP32 = (7.5, 8 - 2.0 ** -6, 8 + 2.0 ** -6, 8.5, 16.0, 46.0, 120.0)
# Reduced precision: the kernel rounds q c to f16 once more (2^-11 relative on a 13.5-unit score: up to 0.0066 units), so
# the designed distance to log2 P_SAFE = 13 is 2^-5: the REALISED distance (checked on the kernel's own rounded q) then
# stays >= 2^-6.
SPIKE_HI = (12.5, 13 - 2.0 ** -5, 13 + 2.0 ** -5, 13.5)
THEMES = ("below both thresholds", "above both thresholds", "staircase 7.9", "staircase 8.1", "ramp / offset / pad key",
          "between the thresholds")
N_THEMES = len(THEMES)


def c_of(hd):
    return hd ** -0.5 * LOG2E


def cexp32(hd):
    """what the kernels multiply by: float(hd^-0.5) * 1.442695...f, both fp32, the product rounded"""
    return np.float32(np.float32(hd ** -0.5) * np.float32(1.44269504088896340736))


def ratio(err, B):
    """|err| / B per element (torch), 0 / 0 = 0; a NaN error counts as infinite"""
    r = torch.where(err == 0, torch.zeros_like(err), err / B)
    return torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)


# ------------------------------------------------------------------------------------------------ the input builder


def default_sites(L):
    """spike key sets of a plain case: one key each in key tiles 0, 1, 2, last - 1, last (32 keys per tile), in-tile slots
    3, 6, 17, 28, 12 - lane halves 0, 1, 0, 1, 1 of the split kernels ((slot >> 2) & 1) - clipped to the keys that exist"""
    nt = -(-L // 32)
    sites = []
    for tau, slot in zip((0, 1, 2, nt - 2, nt - 1), (3, 6, 17, 28, 12)):
        key = max(tau, 0) * 32 + slot
        while key >= L:
            key -= 16
        if key >= 0 and [key] not in sites:
            sites.append([key])
    return sites


def hyper_sites(n):
    """one dominant key in each of the four waves' key shares of cra5_hyper_attention_f32 (16-key tiles, tile j on wave
    j % 4), where those keys exist"""
    return [[k] for k in (3, 16 + 6, 32 + 1, 48 + 12, 64 + 9) if k < n] if n > 17 else [[3], [16]]


def bal_cuts(T, groups, nw=12):
    """Host restatement of the balanced plan's geometry (cra5_amd/csrc/attention_split_f16.hip, as
    test_kernels_gpu._bal_plan): (first key-split wave-tile, [(wave-tiles of the group, [(j0, j1) key-tile range of each piece])])."""
    n_full = T // (groups * nw)
    tile0 = n_full * groups * nw
    rem = T - tile0
    n_grp = -(-rem // nw)
    S = n_grp * T
    cut = lambda c: S * c // groups
    out = []
    for g in range(n_grp):
        pieces = []
        for c in range(groups):
            a, b = max(cut(c), g * T), min(cut(c + 1), (g + 1) * T)
            if b > a:
                pieces.append((a - g * T, b - g * T))
        out.append((min(nw, rem - g * nw), pieces))
    return tile0, out


def balanced_sites(T, groups):
    """spike key sets of the balanced case: set 0 = the last key before every key-range cut of the plan, set 1 = the
    first key after every cut (a row that uses one of them sees one equally dominant key in several pieces: pieces with
    EQUAL maxima), sets 2.. = single keys in tiles 0, 2 and last"""
    _, grps = bal_cuts(T, groups)
    cuts = sorted({j0 for _, pcs in grps for j0, _ in pcs if j0 > 0})
    return [[c * 32 - 1 for c in cuts], [c * 32 for c in cuts], [3], [2 * 32 + 17], [(T - 1) * 32 + 12]]


N_SPIKE, N_NEG = 5, 4


def layout(hd, L):
    """head-dim layout: 0 the constant feature, 1 .. nf the one-hot key-tile features (a block of tiles each where there are
    more tiles than 24), then N_SPIKE spike features, the pad-key feature, N_NEG non-positive features, the rest random"""
    nt = -(-L // 32)
    nf = min(nt, 24)
    sp0 = 1 + nf
    pad = sp0 + N_SPIKE
    neg0 = pad + 1
    rnd0 = neg0 + N_NEG
    assert rnd0 + 8 <= hd
    return dict(nt=nt, nf=nf, sp0=sp0, pad=pad, neg0=neg0, rnd0=rnd0, block=lambda tile: tile * nf // nt)


def build(H, W, wh, ww, heads, hd, seed, sites=None):
    """(qkv fp32 [H*W, 3C], pad row fp32 [3C], windows, rows): per (query, head) a designed score profile over the key
    tiles.  Keys depend on their window-local position only (every window sees the same key features): the constant
    feature is 1; the tile feature of the key's tile is 1; spike feature s is 1 on the keys of sites[s]; the non-positive
    features hold -n / 8 (0 for slot 0 of every tile - that key carries a spike-free row's maximum, exactly, in whichever
    tile a key range of the balanced launch starts - and for spike keys); the random
    features hold a +-1 grid in steps of 1/8 plus a lo-plane part.  The pad row's key: constant and pad feature.  A
    query holds (profile value) / c in the feature it uses.  v: normal values times 2^(-3 .. 3), mixed signs, lo planes
    non-zero.  `rows` records, per (token, head): theme, class name, spike height and spike set.

    Classes go by (wave tile, lane): theme = (wave + 2 window + 4 head) % 6 decides what may share a wave (the rescale
    is decided per wave), the lane picks the class inside it - so a wave holds 4-5 classes, 576-token windows x 2
    heads x 2 windows put every theme into the half-empty fifth work-group (waves 16, 17), and the spike sets cover
    both lane halves."""
    wins = X.Windows(H, W, wh, ww)
    N, C, L = H * W, heads * hd, wh * ww
    lay = layout(hd, L)
    sites = default_sites(L) if sites is None else sites
    assert 1 <= len(sites) <= N_SPIKE
    c = c_of(hd)
    rng = np.random.default_rng(seed)
    nrnd = hd - lay["rnd0"]
    # ---- keys and values by window-local position
    kpos = np.zeros((heads, L, hd))
    t = np.arange(L)
    kpos[:, :, 0] = 1.0
    kpos[:, t, 1 + np.array([lay["block"](j) for j in t // 32])] = 1.0
    for s, keys in enumerate(sites):
        kpos[:, keys, lay["sp0"] + s] = 1.0
    for n in range(N_NEG):
        kpos[:, :, lay["neg0"] + n] = -((t * 7 + n * 3 + 1) % 9) / 8.0
    kpos[:, ::32, lay["neg0"]:lay["rnd0"]] = 0.0         # slot 0 of every tile, see the docstring
    for keys in sites:                                   # (a spike key stands exactly its height over those keys)
        kpos[:, keys, lay["neg0"]:lay["rnd0"]] = 0.0
    kpos[:, :, lay["rnd0"]:] = rng.integers(-8, 9, (heads, L, nrnd)) / 8.0 + rng.integers(-3, 4, (heads, L, nrnd)) * 2.0 ** -13
    qkv = np.zeros((N, 3, heads, hd))
    loc, win = wins.loc_of, wins.win_of
    qkv[:, 1] = kpos[:, loc].transpose(1, 0, 2)
    qkv[:, 2] = rng.standard_normal((N, heads, hd)) * 2.0 ** rng.integers(-3, 4, (N, heads, hd))
    pad = np.zeros((3, heads, hd))
    pad[1, :, 0] = 1.0
    pad[1, :, lay["pad"]] = 1.0
    pad[2] = rng.standard_normal((heads, hd)) * 2.0
    # ---- queries
    q = np.zeros((N, heads, hd))
    rows = dict(theme=np.zeros((N, heads), np.int64), cls=np.empty((N, heads), object), delta=np.zeros((N, heads)),
                site=np.full((N, heads), -1, np.int64))
    rdir = rng.integers(-8, 9, (N, heads, nrnd)) / 8.0 + rng.integers(-3, 4, (N, heads, nrnd)) * 2.0 ** -13
    nb = lay["nf"]

    s_tile0 = next(s for s, keys in enumerate(sites) if all(k < 32 for k in keys))

    def spike(i, h, delta, s):
        # (2^-20 relative away from the nearer threshold: the 22-bit store must not eat into a margin of exactly 2^-6)
        thr = DEFER_LOG2 if abs(delta - DEFER_LOG2) < abs(delta - 13.0) else 13.0
        q[i, h, lay["sp0"] + s] = delta / c * (1 + math.copysign(2.0 ** -20, delta - thr))
        q[i, h, lay["neg0"]:lay["rnd0"]] = 0.25 / c / N_NEG          # in-tile spread of up to 1/4 unit, all below key 0
        rows["delta"][i, h], rows["site"][i, h] = delta, s
        return f"spike {delta!r}"

    for i in range(N):
        wave, lane = int(loc[i]) // 32, int(loc[i]) % 32
        for h in range(heads):
            theme = (wave + 2 * int(win[i]) + 4 * h) % N_THEMES
            s_wave = (wave // N_THEMES + h + int(win[i])) % len(sites)   # one spike set per firing wave: a designed record
            name = "flat"
            if theme == 0:
                if lane % 4 < 2:
                    name = spike(i, h, SPIKE_FP32[lane % 4], (lane // 4) % len(sites))
                elif lane % 4 == 2:
                    q[i, h, lay["rnd0"]:] = 2.5 * rdir[i, h]
                    name = "random"
            elif theme in (1, 5):
                pool = (SPIKE_HI[2:] + SPIKE_FP32[4:]) if theme == 1 else (SPIKE_FP32[2:4] + SPIKE_HI[:2])
                if lane % 4 == 0:
                    name = spike(i, h, pool[(lane // 4) % len(pool)], s_wave)
                elif lane % 4 == 3:
                    name = spike(i, h, pool[-1 - (lane // 4) % 3], s_wave)
                elif lane % 4 == 1:
                    q[i, h, lay["rnd0"]:] = 0.5 * rdir[i, h]
                    name = "calm"
                elif theme == 5:
                    # a key of tile 0 at +40 sets the reference, the wave's spike key stands 12.5 above it: nearly all the
                    # weight on ONE key whose p = 2^12.5 is no f16 number and is not redone (below P_SAFE)
                    q[i, h, lay["sp0"] + s_tile0] = 40.0 / c
                    if s_wave != s_tile0:
                        q[i, h, lay["sp0"] + s_wave] = 52.5 / c
                    name = "sharp spike 12.5"
            elif theme in (2, 3):
                step = 7.9 if theme == 2 else 8.1
                if lane % 4 < 2:
                    for b in range(nb):
                        q[i, h, 1 + b] = step * b / c
                    # (spread 1/16: where slot 0 of a tile is a pad position the tile's maximum lies up to that much
                    # under its level, and 8.1 - 1/16, 7.9 + 1/16 keep their distance from the threshold)
                    q[i, h, lay["neg0"]:lay["rnd0"]] = 0.0625 / c / N_NEG
                    name = f"staircase {step}"
                elif lane % 4 == 2:
                    q[i, h, lay["rnd0"]:] = 0.5 * rdir[i, h]
                    name = "calm"
            else:
                k5 = lane % 5
                if k5 == 0:
                    for b in range(nb):
                        q[i, h, 1 + b] = -200.0 * b / max(nb - 1, 1) / c
                    q[i, h, lay["neg0"]:lay["rnd0"]] = 0.25 / c / N_NEG
                    name = "ramp -200"
                elif k5 in (1, 2):
                    q[i, h, 0] = (100.0 if k5 == 1 else -100.0) / c
                    q[i, h, lay["rnd0"]:] = 0.5 * rdir[i, h]
                    name = "offset +100" if k5 == 1 else "offset -100"
                elif k5 == 3:
                    q[i, h, lay["pad"]] = 12.0 / c
                    q[i, h, lay["rnd0"]:] = 0.5 * rdir[i, h]
                    name = "pad key"
                else:
                    q[i, h, lay["rnd0"]:] = 0.5 * rdir[i, h]
                    name = "calm"
            rows["theme"][i, h], rows["cls"][i, h] = theme, name
    qkv[:, 0] = q
    rows["sites"], rows["layout"] = sites, lay
    # every value is replaced by what the split store keeps of it (hi + lo, 22 bits): the operands are exact in the split
    # model, and the fp32 engines read the very same numbers
    exact = lambda a: sum(X.split_model(torch.from_numpy(a.astype(np.float32)))).contiguous()
    return exact(qkv.reshape(N, 3 * C)), exact(pad.reshape(3 * C)), wins, rows


# the grids of tests/test_softmax_gpu.py: (H, W, (wh, ww)) at 2 heads x 64 unless stated
WINDOWED = ((24, 48, (24, 24)), (20, 44, (24, 24)), (50, 24, (48, 12)), (24, 50, (12, 48)))
GLOBAL_PLAIN = (8, 72)                        # 576 tokens as one window: 12-wave work-groups, 1.5 of them
BALANCED = dict(H=64, W=64, heads=32, groups=8)   # on 256 CUs: 96 full wave-tiles + 32 key-split ones in 3 groups
F32_CASES = ((20, 44, (24, 24), 64), (18, 36, (18, 36), 72))
HYPER = ((648, 5, 72), (100, 3, 72), (41, 2, 64), (17, 1, 72))
_CASES = {}


def case(kind, *key):
    """the inputs of one grid, built once per process: kind "win" (H, W, (wh, ww)[, hd]), "global", "balanced", "hyper"
    (n, heads, hd)"""
    k = (kind,) + key
    if k not in _CASES:
        if kind == "win":
            H, W, (wh, ww) = key[:3]
            hd = key[3] if len(key) > 3 else 64
            _CASES[k] = build(H, W, wh, ww, 2, hd, seed=H * 100 + W + wh)
        elif kind == "global":
            H, W = GLOBAL_PLAIN
            _CASES[k] = build(H, W, H, W, 2, 64, seed=5)
        elif kind == "balanced":
            b = BALANCED
            _CASES[k] = build(b["H"], b["W"], b["H"], b["W"], b["heads"], 64, seed=9,
                              sites=balanced_sites(b["H"] * b["W"] // 32, b["groups"]))
        else:
            n, heads, hd = key
            _CASES[k] = build(1, n, 1, n, heads, hd, seed=n, sites=hyper_sites(n))
    return _CASES[k]


def take_heads(x, heads, sel):
    """the columns of heads `sel` of a [N, 3 * heads * hd] (or [3 * heads * hd]) tensor, as a tensor of len(sel) heads"""
    lead = x.shape[:-1]
    return x.reshape(*lead, 3, heads, -1)[..., sel, :].reshape(*lead, -1).contiguous()


def wave_site(rows, wave, win, head):
    """the spike set the firing themes use in this wave (build's rule)"""
    return (wave // N_THEMES + head + win) % len(rows["sites"])


def designed_record(theme, site_tile, nt, padded):
    """Key tiles (after the first) at which a wave of this theme takes the rescale branch - the same set for the deferred
    rule (threshold 8) and the reduced-precision rule (threshold 13) except between the thresholds - or None where the
    design fixes none.  Staircase 7.9: 7.9 stays below either threshold, 15.8 exceeds both: every second tile.  Staircase
    8.1: the deferred rule fires on every tile; the reduced-precision rule on every second (8.1 < 13 < 16.2)."""
    if padded and theme != 0:   # (a pad position holds the pad row's key: no tile feature, no spike, and a dominant key
        return None, None       # for the pad-key class - there only "fp32 record = float64 record" is asserted)
    if theme in (0, 4):
        return (), ()
    if theme == 1:
        r = (site_tile,) if site_tile > 0 else ()
        return r, r
    if theme == 5:
        return ((site_tile,) if site_tile > 0 else ()), ()
    even = tuple(range(2, nt, 2))
    return (even if theme == 2 else tuple(range(1, nt))), even


def torch_fp32_attention(planes, pad_planes, wins, heads):
    """torch's fp32 CPU softmax(q k^T scale) v per window, on the stored operands rounded to fp32 -> float64 [N, C]"""
    N, C = planes[0].shape[0], planes[0].shape[1] // 3
    hd = C // heads
    out = torch.zeros(N, C, dtype=torch.float64)
    for idx, real, ph, pl in X.window_operands(planes, pad_planes, wins, heads):
        x = (ph + pl).float()
        o = torch.softmax(x[0] @ x[1].transpose(-1, -2) * hd ** -0.5, -1) @ x[2]
        out[torch.from_numpy(idx[real])] = o.permute(1, 0, 2).reshape(-1, C)[torch.from_numpy(real)].double()
    return out


def stored_planes(x, family):
    """(hi, lo) float64 of an fp32 tensor as the engine family reads it: the split store (exact_helpers.split_model), its
    hi plane alone (reduced precision: the f16-rounded operand), or the fp32 value itself"""
    if family == "split":
        hi, lo = X.split_model(x)
        return hi.double(), lo.double()
    if family == "hi":
        return x.float().half().double(), torch.zeros_like(x, dtype=torch.float64)
    return x.double(), torch.zeros_like(x, dtype=torch.float64)


# ------------------------------------------------------------------------------------------------ reference and bounds


def eps_terms(family, hd, nt, pieces=0):
    """(a, x, e, (sub_scale, sub_num, sub_den)), all BEFORE the doubling.  a counts the roundings of an EXPONENT (log2
    units), each relative to A_i = max_j c sum_d |q_id k_jd| (the absolute-value score: every error of a score is relative
    to it); x the relative errors of a p itself that numerator and row sum both see; a p then carries
    (a A_i ln 2 + x) u.  e = n + d + f counts the relative roundings of the numerator alone (n), the denominator alone (d) and the final step (f).  The last three
    describe the ABSOLUTE error of a p in the kernel's own scale, min(sub_scale 2^(t - t_max), sub_num) as the numerator
    reads it and min(.., sub_den) as the row sum does: half an f16 subnormal, 2^-25, where that p went through f16, and
    2^-126 where it is the fp32 p (v_exp_f32 returns no subnormal); sub_scale says how far above 2^(t - t_max) the
    kernel's p may lie (the error is at most p itself).  nt: key tiles of 32; pieces: merged key ranges (balanced launch
    only).

    split (fp32-accurate, 3 x v_mfma_f32_32x32x16_f16 per product):
      a: the dropped lo_q lo_k product, 2^-11 * 2^-11 = 4 u; the score sum - 12 chained MFMAs, each a 16-term dot
         product: any order has depth <= 16 + 12 = 28; c = fl(fl(hd^-0.5) fl(log2 e)): 3; fma(s, c, -m), one rounding of
         |t| + |m|: 2.  a = 37.  + 2 per merge (the subtraction m_p - M, on a difference of at most 2 A_i).
      x: v_exp_f32, 1 ulp: 2.
      n: P = hi + lo keeps 22 bits: 4; the dropped lo_p lo_v product: 4; O accumulates 6 chained MFMAs per key tile, each
         a 16-term dot product: depth 16 + 6 nt; one rounding per rescale, at most one per tile: nt.
      d: 16 additions into the tile's row sum, one into l per tile, one to join the lane halves: 17 + nt; rescales: nt.
         (alpha itself multiplies O and l alike: its own error cancels.)
      f: the reciprocal (allowed 1 ulp: 2) and the product: 3.
      per merged piece: exp2 (2) and one fma (1), in n and in d.
      sub: 2^-25 (the lo plane's f16 subnormals) in the numerator, 2^-126 in the row sum (it adds the fp32 p); sub_scale 2^8: a deferred
         reference lies at most DEFER_LOG2 below the row maximum.
    hi (reduced precision, hi.hi only):
      a: q c rounded to f16 once more: 2^-11 = 2^13 u; 4 chained MFMAs (the first one adds -m): depth 16 + 4 = 20; c: 3;
         the reference is an f16 sum moved by MFMAs: 2.  a = 2^13 + 25 (+ 2 per merge).
      x: v_exp_f32 2, p rounded to f16 2^-11 = 2^13 u (numerator and row sum read the same rounded p).
      n: depth 16 + 2 nt, rescales nt.  d: 17 + nt, rescales nt.  f: 3.
      sub: 2^-25, numerator and row sum; sub_scale 2^14: p may reach P_SAFE = 2^13 before the reference moves, and
         it moves to an f16 neighbour of the maximum.
    f32 (exact-f32, v_mfma_f32_32x32x2_f32):
      a: q fl(scale log2 e) - the constant 3, the product 1; hd / 2 chained MFMAs of 2 terms: 2 + hd / 2; s - m: 2.
         a = 8 + hd / 2.
      x: 2.  n: 16 chained MFMAs of 2 terms per tile: 2 + 16 nt; O alpha per tile: nt.  d: 17 + nt; l alpha: nt.  f: 3.
      sub: 2^-126 (p is never an f16: only v_exp_f32's flush to zero), numerator and row sum; sub_scale 1: the exact rule
         keeps the reference at the maximum.
    hyper (v_mfma_f32_16x16x4_f32, 16-key tiles dealt to 4 waves, merged through LDS):
      a: 4 + (4 + hd / 4) + 2 = 10 + hd / 4, + 2 for the merge's m_w - m_all.
      x: 2.  n: 4 chained MFMAs of 4 terms per 16-key tile, nt / 2 + 1 tiles per wave: 4 + 2 nt + 4; rescales nt / 2 + 1;
         merge: exp2 2, product 1, 4 additions: 7.  d: 4 + nt / 2 + 1 additions, rescales nt / 2 + 1, merge 7, joining the
         four slot groups 2.  f: 3.  sub: as f32."""
    if family == "split":
        a, x = 37 + (2 if pieces else 0), 2
        n = 8 + 16 + 6 * nt + nt + 3 * pieces
        d = 17 + nt + nt + 3 * pieces
        return a, x, n + d + 3, (2.0 ** 8, 2.0 ** -25, FLT_MIN)
    if family == "hi":
        a, x = 2 ** 13 + 25 + (2 if pieces else 0), 2 + 2 ** 13
        n = 16 + 2 * nt + nt + 3 * pieces
        d = 17 + nt + nt + 3 * pieces
        return a, x, n + d + 3, (2.0 ** 14, 2.0 ** -25, 2.0 ** -25)
    if family == "f32":
        return 8 + hd // 2, 2, (2 + 16 * nt + nt) + (17 + nt + nt) + 3, (1.0, FLT_MIN, FLT_MIN)
    assert family == "hyper"
    per_wave = nt // 2 + 1
    return 12 + hd // 4, 2, (8 + 2 * nt + per_wave + 7) + (4 + 2 * per_wave + 7 + 2) + 3, (1.0, FLT_MIN, FLT_MIN)


def reference_and_bound(planes, pad_planes, wins, heads, family, pieces=0, rows=None, drop=None):
    """(ref float64 [N, C], B float64 [N, C]) of the windowed softmax(q k^T hd^-0.5) v with the pad rule (pad positions
    carry the pad row, unmasked), from the operands as stored.  rows: restrict to these token rows (others: 0 / inf).
    drop: bool [windows, L] - window-local keys that take no part (score -inf: weight 0, none of A_i either; their
    stored k rows are not read, so they may hold non-finite values) - the softmax without them, same bound.

    B[i, d] = 2 (a A_i ln 2 + x) u D_id + 2 e u sum_j w_ij |v_jd| + 2 sub_id + 2^-126      (a, x, e: eps_terms)
    D_id = sum_j w_ij |v_jd - ref_id|.  The first term: an error of the exponent (or of exp2, or the f16 rounding of p in
    the reduced-precision modes) gives ONE perturbed p_ij (1 + delta_ij) that numerator and row sum both read, and
    sum_j w_ij (1 + delta_ij) v_jd / sum_j w_ij (1 + delta_ij) differs from ref by sum_j w_ij delta_ij (v_jd - ref_id) to
    first order: it vanishes where one key holds all the weight - which is what makes a row sum taken over a DIFFERENT
    p visible.
    sub_id = sum_j (min(sub_scale rho_ij, sub_num) |v_jd| + min(sub_scale rho_ij, sub_den) |ref_id|) / sum_j rho_ij,
    rho_ij = 2^(t_ij - max_j t_ij), per family (eps_terms): the absolute error of a p as the numerator and as the row sum
    read it, in the kernel's own scale, in which l >= sum_j rho_ij (the reduced-precision reference is an f16 NEIGHBOUR of
    the first tile's maximum and may lie 2^-11 |m| above it: l >= 0.96 sum rho for |m| <= 120, inside the doubling).  w are
    the float64 softmax weights; the factors 2 are the doubling rule."""
    hi, lo = planes
    N, C = hi.shape[0], hi.shape[1] // 3
    hd = C // heads
    c = c_of(hd)
    ref = torch.zeros(N, C, dtype=torch.float64, device=hi.device)
    B = torch.full((N, C), float("inf"), dtype=torch.float64, device=hi.device)
    keep = None if rows is None else torch.zeros(N + 1, dtype=torch.bool).index_fill_(0, torch.as_tensor(rows), True).numpy()
    for w, (idx, real, ph, pl) in enumerate(X.window_operands(planes, pad_planes, wins, heads)):
        sel = real if keep is None else real & keep[idx]
        if not sel.any():
            continue
        ts = torch.from_numpy(sel).to(hi.device)
        x = ph + pl
        q, k, v = x[0][:, ts], x[1], x[2]
        L = k.shape[1]
        a, x_, e, (sub_scale, sub_num, sub_den) = eps_terms(family, hd, -(-L // 32), pieces)
        gone = None if drop is None or not drop[w].any() else torch.from_numpy(drop[w]).to(hi.device)
        if gone is not None:
            k = torch.where(gone[None, :, None], torch.zeros_like(k), k)
        t = (q @ k.transpose(-1, -2)) * c
        A = (q.abs() @ k.abs().transpose(-1, -2)) * c
        if gone is not None:
            t = torch.where(gone[None, None, :], torch.full_like(t, float("-inf")), t)
        A = A.amax(-1, keepdim=True)
        rho = torch.exp2(t - t.amax(-1, keepdim=True))
        lam = rho.sum(-1, keepdim=True)
        w = rho / lam
        r = w @ v
        dev = torch.empty_like(r)
        step = max(1, 2 ** 24 // (L * r.shape[-1]))
        for i0 in range(0, r.shape[1], step):           # (a [heads, step, L, hd] block at a time)
            sl = slice(i0, i0 + step)
            dev[:, sl] = (w[:, sl, :, None] * (v[:, None] - r[:, sl, None]).abs()).sum(2)
        small = lambda cap: torch.minimum(rho * sub_scale, torch.full_like(rho, cap))
        sub = (small(sub_num) @ v.abs() + small(sub_den).sum(-1, keepdim=True) * r.abs()) / lam
        b = 2 * (a * A * LN2 + x_) * U * dev + 2 * e * U * (w @ v.abs()) + 2 * sub + FLT_MIN
        dst = torch.from_numpy(idx[sel]).to(hi.device)
        ref[dst] = r.permute(1, 0, 2).reshape(-1, C)
        B[dst] = b.permute(1, 0, 2).reshape(-1, C)
    return ref, B


def split_store_term(ref, family):
    """what out_split adds when it is read back: 22 bits and half an f16 subnormal (test_exact_gpu._check_uniform's terms);
    the reduced-precision modes store the f16 hi plane alone (2^-11, doubled)"""
    return ref.abs() * (2.0 ** -10 if family == "hi" else 2.0 ** -21) + 2.0 ** -24


# ------------------------------------------------------------------------------------------------ the host restatement

VARIANTS = {
    "l_not_rescaled": ("split",), "O_not_rescaled": ("split", "f32"), "alpha_sign_flipped": ("split",),
    "p_against_new_max": ("split",), "reference_never_moved": ("split", "hi"), "P_lo_dropped": ("split",),
    "rowsum_unrounded": ("hi",), "halves_not_added": ("split", "hi", "f32"), "per_query_decision": ("split", "hi"),
    "merge_no_factor": ("merge",), "merge_norm_largest_l": ("merge",), "merge_drop_last": ("merge",),
    "masked_key_counted": ("f32",),
}
HARMLESS = ("per_query_decision",)


def _f16(x):
    with np.errstate(over="ignore"):
        return np.asarray(x).astype(np.float16).astype(np.float64)


def _exp2(x, dtype):
    """2^x rounded to dtype; v_exp_f32 returns no subnormal"""
    with np.errstate(all="ignore"):
        r = np.exp2(np.asarray(x, np.float64))
        if dtype == np.float32:
            r = np.where(r < FLT_MIN, 0.0, r)
        return r.astype(dtype).astype(np.float64)


def restate_stream(ops, family, hd, variant=None, dtype=np.float32, j0=0, j1=None, partial=False, n_keys=None):
    """The key loop of one (window, head) as the kernels document it, 32 keys per tile, vectorised over the queries.
    ops = (qh, ql, kh, kl, vh, vl) float64 numpy [L, hd].  Dot products are exact (float64) and rounded once; every
    other documented operation is rounded to `dtype` once (float64: the builder's own trace of the decisions).  The
    running reference m is per query (both lanes of a query hold the same value), the row sum l per (query, lane
    half): slot s of a tile belongs to half (s >> 2) & 1.  family "split": deferred reference, moved for a whole wave of
    32 queries when any of them sees a tile maximum more than DEFER_LOG2 above it; "hi": reference set by the first
    tile, moved by an f16-representable delta when a lane's row sum of the ROUNDED p exceeds P_SAFE, exponentials
    redone; "f32": exact rule, keys past n_keys masked.  Returns (out [Lq, hd] - or the partial (m, l, O) -, fired
    [waves, tiles]: the rescale branch taken after the first tile's)."""
    assert family in FAMILIES[:3] and (variant is None or variant in VARIANTS)
    qh, ql, kh, kl, vh, vl = ops
    R = lambda z: np.asarray(z, np.float64).astype(dtype).astype(np.float64)
    nq, L = qh.shape[0], kh.shape[0]
    n_keys = L if n_keys is None else n_keys
    nt = -(-n_keys // 32)
    j1 = nt if j1 is None else j1
    c = float(cexp32(hd)) if dtype == np.float32 else c_of(hd)
    with np.errstate(all="ignore"):
        if family == "split":
            S = R(qh @ (kh + kl).T + ql @ kh.T)
            V = (vh, vl)
        elif family == "hi":
            S = _f16(R(qh * c)) @ kh.T                     # products of f16 numbers: exact; rounded with the reference below
            V = (vh, np.zeros_like(vh))
        else:
            S = R(R(qh * c) @ kh.T)
            V = (vh, np.zeros_like(vh))
        Sp = np.full((nq, nt * 32), -np.inf)
        Sp[:, :n_keys] = S[:, :n_keys]
        Vp = [np.zeros((nt * 32, hd)) for _ in V]
        for dst, src in zip(Vp, V):
            dst[:n_keys] = src[:n_keys]
        half = (np.arange(32) >> 2) & 1
        wave = np.arange(nq) // 32
        nwv = int(wave.max()) + 1
        per_query = variant == "per_query_decision"

        def any_wave(need):
            if per_query:
                return need
            f = np.zeros(nwv, bool)
            np.logical_or.at(f, wave, need)
            return f[wave]

        def row_sums(p):
            ps = np.zeros((nq, 2))
            for hh in (0, 1):
                for s_ in np.nonzero(half == hh)[0]:
                    ps[:, hh] = R(ps[:, hh] + p[:, s_])
            return ps

        m = np.zeros(nq) if family == "hi" else np.full(nq, -np.inf)
        l, o = np.zeros((nq, 2)), np.zeros((nq, hd))
        fired = np.zeros((nwv, nt), bool)
        for j in range(j0, j1):
            s = Sp[:, 32 * j:32 * j + 32]
            vt = [vp[32 * j:32 * j + 32] for vp in Vp]
            first = j == j0
            if family == "split":
                mloc = R(s.max(1) * c)
                upd = any_wave(~(R(mloc - m) <= DEFER_LOG2))
                if variant == "reference_never_moved" and not first:
                    upd = np.zeros(nq, bool)
                fired[:, j] = np.bincount(wave, upd, nwv) > 0
                m_new = np.where(upd, np.maximum(m, mloc), m)
                alpha = _exp2(R(m_new - m) if variant == "alpha_sign_flipped" and not first else R(m - m_new), dtype)
                alpha = np.where(upd, alpha, 1.0)
                if variant != "l_not_rescaled" or first:
                    l = R(l * alpha[:, None])
                if variant != "O_not_rescaled" or first:
                    o = R(o * alpha[:, None])
                m = m_new
                mref = np.maximum(m, mloc) if variant == "p_against_new_max" else m
                p = _exp2(R(s * c - mref[:, None]), dtype)
                ph = _f16(p)
                pl = np.zeros_like(p) if variant == "P_lo_dropped" else _f16(R(p - ph))
                l = R(l + row_sums(p))
                o = R(o + (ph + pl) @ vt[0] + ph @ vt[1])
            elif family == "hi":
                def shift(delta, rescale):
                    nonlocal m, l, o
                    delta = _f16(np.clip(delta, -60000.0, 60000.0))
                    if rescale:
                        alpha = _exp2(-delta, dtype)
                        l, o = R(l * alpha[:, None]), R(o * alpha[:, None])
                    m = R(m + delta)

                def exps():
                    p_ = _exp2(R(s - m[:, None]), dtype)
                    pr = _f16(p_)
                    return pr, row_sums(p_ if variant == "rowsum_unrounded" else pr)

                if first:
                    shift(R(s - m[:, None]).max(1), False)
                p, ps = exps()
                upd = any_wave(~((ps <= P_SAFE).all(1)))
                fired[:, j] = np.bincount(wave, upd, nwv) > 0
                if variant == "reference_never_moved":
                    upd = np.zeros(nq, bool)
                if upd.any():
                    keep_m, keep_l, keep_o = m.copy(), l.copy(), o.copy()
                    shift(np.maximum(R(s - m[:, None]).max(1), 0.0), True)
                    m, l, o = (np.where(upd.reshape((-1,) + (1,) * (a_.ndim - 1)), a_, b_)
                               for a_, b_ in ((m, keep_m), (l, keep_l), (o, keep_o)))
                    p, ps = exps()
                l = R(l + ps)
                o = R(o + p @ vt[0])
            else:
                mloc = s.max(1)
                m_new = np.maximum(m, mloc)
                alpha = _exp2(R(m - m_new), dtype)
                fired[:, j] = np.bincount(wave, m_new > m, nwv) > 0
                p = _exp2(R(s - m_new[:, None]), dtype)
                if variant == "masked_key_counted":
                    p = np.where(np.isneginf(s), 1.0, p)
                l = R(R(l * alpha[:, None]) + row_sums(p))
                o = R((o if variant == "O_not_rescaled" else R(o * alpha[:, None])) + p @ vt[0])
                m = m_new
        l_tot = l[:, 0] if variant == "halves_not_added" else R(l[:, 0] + l[:, 1])
        fired[:, j0] = False
        if partial:
            return (m, l_tot, o), fired
        return R(o * R(1.0 / l_tot)[:, None]), fired


def merge_restated(parts, variant=None, dtype=np.float32):
    """attention_merge_kernel: M = max_p m_p; piece p contributes exp2(m_p - M) (O_p, l_p), one fma each, in piece order"""
    R = lambda z: np.asarray(z, np.float64).astype(dtype).astype(np.float64)
    if variant == "merge_drop_last":
        parts = parts[:-1]
    with np.errstate(all="ignore"):
        M = np.max(np.stack([p[0] for p in parts]), 0)
        acc, ls = np.zeros_like(parts[0][2]), np.zeros_like(parts[0][1])
        for m_p, l_p, o_p in parts:
            a = np.ones_like(M) if variant == "merge_no_factor" else _exp2(R(m_p - M), dtype)
            ls = R(l_p * a + ls)
            acc = R(o_p * a[:, None] + acc)
        if variant == "merge_norm_largest_l":
            ls = np.max(np.stack([p[1] for p in parts]), 0)
        return R(acc * R(1.0 / ls)[:, None])


def hyper_restated(ops, hd, n, variant=None, dtype=np.float32):
    """cra5_hyper_attention_f32: 16-key tiles, tile j on wave j % 4, exact rule per wave, l per (query, slot group of 4
    keys), the four waves merged in fixed order (a wave without keys: factor 0), then the slot groups joined."""
    qh, _, kh, _, vh, _ = ops
    R = lambda z: np.asarray(z, np.float64).astype(dtype).astype(np.float64)
    c = float(cexp32(hd)) if dtype == np.float32 else c_of(hd)
    nq = qh.shape[0]
    nt = -(-n // 16)
    with np.errstate(all="ignore"):
        S = np.full((nq, nt * 16), -np.inf)
        S[:, :n] = R(R(qh * c) @ kh[:n].T)
        Vp = np.zeros((nt * 16, hd))
        Vp[:n] = vh[:n]
        grp = np.arange(16) >> 2
        res = []
        for w in range(4):
            m, l, o = np.full(nq, -np.inf), np.zeros((nq, 4)), np.zeros((nq, hd))
            for j in range(w, nt, 4):
                s = S[:, 16 * j:16 * j + 16]
                m_new = np.maximum(m, s.max(1))
                alpha = _exp2(R(m - m_new), dtype)
                p = _exp2(R(s - m_new[:, None]), dtype)
                ps = np.zeros((nq, 4))
                for s_ in range(16):
                    ps[:, grp[s_]] = R(ps[:, grp[s_]] + p[:, s_])
                l = R(R(l * alpha[:, None]) + ps)
                o = R(R(o * alpha[:, None]) + p @ Vp[16 * j:16 * j + 16])
                m = m_new
            res.append((m, l, o))
        m_all = np.max(np.stack([r[0] for r in res]), 0)
        lt, ot = np.zeros((nq, 4)), np.zeros((nq, hd))
        for i, (m, l, o) in enumerate(res):
            f = np.where(np.isneginf(m), 0.0, _exp2(R(m - m_all), dtype))
            if variant == "merge_no_factor":
                f = np.where(np.isneginf(m), 0.0, 1.0)
            if i == 0:
                lt, ot = R(l * f[:, None]), R(o * f[:, None])
            else:
                lt, ot = R(lt + R(l * f[:, None])), R(ot + R(o * f[:, None]))
        l_tot = R(R(lt[:, 0] + lt[:, 1]) + R(lt[:, 2] + lt[:, 3]))
        if variant == "halves_not_added":
            l_tot = lt[:, 0]
        return R(ot * R(1.0 / l_tot)[:, None])


def _np_ops(ph, pl, h, q_sel=None):
    """(qh, ql, kh, kl, vh, vl) numpy float64 of head h from exact_helpers.window_operands' [3, heads, L, hd] planes"""
    out = []
    for i in range(3):
        for p in (ph, pl):
            a = p[i, h].cpu().numpy()
            out.append(a if (i or q_sel is None) else a[q_sel])
    return out


def restate(planes, pad_planes, wins, heads, family, variant=None, dtype=np.float32, balanced_groups=None, full_pass=True):
    """The whole launch on the host -> (out float64 [N, C] torch, records {(window, head): fired [waves, tiles]}).
    family "split" / "hi": every window position is a query (pad positions run on the pad row and take part in their
    wave's decisions); balanced_groups: slots per head of the balanced launch - the key-split wave-tiles run their
    key ranges as separate streams and are merged, the others run the whole loop (full_pass False: left at 0).  "f32": the same without decisions
    between queries.  "hyper": hyper_restated."""
    hi = planes[0]
    N, C = hi.shape[0], hi.shape[1] // 3
    hd = C // heads
    out = torch.zeros(N, C, dtype=torch.float64)
    records = {}
    mvar = variant if variant in VARIANTS and VARIANTS[variant] == ("merge",) else None
    svar = None if mvar else variant
    for w, (idx, real, ph, pl) in enumerate(X.window_operands(planes, pad_planes, wins, heads)):
        L = len(idx)
        dst = torch.from_numpy(idx[real])
        for h in range(heads):
            ops = _np_ops(ph, pl, h)
            if family == "hyper":
                o = hyper_restated(ops, hd, L, mvar or svar, dtype)
            elif balanced_groups:
                tile0, grps = bal_cuts(L // 32, balanced_groups)
                o = np.zeros((L, hd))
                if tile0 and full_pass:
                    sub = [a[: tile0 * 32] if i < 2 else a for i, a in enumerate(ops)]
                    o[: tile0 * 32], records[(w, h)] = restate_stream(sub, family, hd, svar, dtype)
                for g, (n_act, pieces) in enumerate(grps):
                    r0 = (tile0 + 12 * g) * 32
                    sub = [a[r0:r0 + n_act * 32] if i < 2 else a for i, a in enumerate(ops)]
                    parts = [restate_stream(sub, family, hd, svar, dtype, j0, j1, partial=True)[0] for j0, j1 in pieces]
                    o[r0:r0 + n_act * 32] = merge_restated(parts, mvar, dtype)
            else:
                o, records[(w, h)] = restate_stream(ops, family, hd, svar, dtype, n_keys=L)
            out[dst, h * hd:(h + 1) * hd] = torch.from_numpy(o[real])
    return out, records


def decision_margins(planes, pad_planes, wins, heads, family, balanced_groups=None):
    """The smallest distance (log2 units) of any wave's decision quantity from its threshold, on float64 arithmetic with the
    decisions of the documented rule: family "split": max over the wave of (tile maximum - reference) against
    DEFER_LOG2; "hi": log2 of the wave's largest lane row sum against log2 P_SAFE (on the kernel's own q, rounded to
    f16 after the multiplication by c).  The first tile of a stream (no standing reference yet) is not a decision.
    balanced_groups: the streams of the balanced launch - the full-pass wave-tiles over the whole key loop, every
    key-split group over each of its key ranges."""
    hd = planes[0].shape[1] // 3 // heads
    c = c_of(hd)
    worst = np.inf
    half = (np.arange(32) >> 2) & 1
    for idx, real, ph, pl in X.window_operands(planes, pad_planes, wins, heads):
        L = len(idx)
        streams = [(0, L, 0, L // 32)]
        if balanced_groups:
            tile0, grps = bal_cuts(L // 32, balanced_groups)
            streams = [(0, tile0 * 32, 0, L // 32)] if tile0 else []
            for g, (n_act, pieces) in enumerate(grps):
                r0 = (tile0 + 12 * g) * 32
                streams += [(r0, r0 + n_act * 32, j0, j1) for j0, j1 in pieces]
        for h in range(heads):
            qh, ql, kh, kl, vh, vl = _np_ops(ph, pl, h)
            with np.errstate(all="ignore"):
                if family == "split":
                    T_all = ((qh + ql) @ (kh + kl).T - ql @ kl.T) * c
                else:
                    T_all = _f16((qh * float(cexp32(hd))).astype(np.float32)) @ kh.T
                for r0, r1, j0, j1 in streams:
                    T = T_all[r0:r1]
                    nwv = (r1 - r0) // 32
                    tile = lambda j: T[:, 32 * j:32 * j + 32]
                    if family == "split":
                        m = tile(j0).max(1)
                        for j in range(j0 + 1, j1):
                            d = (tile(j).max(1) - m).reshape(nwv, 32).max(1)
                            worst = min(worst, float(np.abs(d - DEFER_LOG2).min()))
                            upd = np.repeat(d > DEFER_LOG2, 32)
                            m = np.where(upd, np.maximum(m, tile(j).max(1)), m)
                    else:
                        m = _f16(tile(j0).max(1))
                        for j in range(j0 + 1, j1):
                            p = _f16(np.exp2(tile(j) - m[:, None]))
                            ps = np.stack([p[:, half == 0].sum(1), p[:, half == 1].sum(1)], 1).max(1).reshape(nwv, 32).max(1)
                            worst = min(worst, float(np.abs(np.log2(ps) - math.log2(P_SAFE)).min()))
                            upd = np.repeat(ps > P_SAFE, 32)
                            mrel = np.maximum((tile(j) - m[:, None]).max(1), 0.0)
                            m = np.where(upd, m + _f16(mrel), m)
    return worst
