"""One out-of-range operand element must poison every output that reads it - and nothing else.  The sites (one element
per structural role of a kernel), the expected sets E (from the geometry alone), the IEEE classification of the rows a
bare +-inf operand reaches, and the checker - shared by tests/test_poison_gpu.py (the kernels) and
tests/test_poison_inputs_cpu.py (these helpers themselves: E against a float64 evaluation, the class conditions, the
role lists, the checker against its mutants).

The oracle is a CLEAN launch against a POISONED launch of the same kernel on the same inputs but for one operand
element: every element of E is non-finite, every element outside E holds the clean launch's bits (it reads nothing that
changed, and the kernels are deterministic).  No tolerance anywhere but for the rows of a bare +-inf operand whose
affected scores are all -inf (the key drops out legitimately): those are non-finite, or within the bound of
softmax_helpers.reference_and_bound against the float64 softmax without those keys.

Nothing here calls a product kernel."""
import numpy as np
import torch
import torch.nn.functional as F

import exact_helpers as X
import patch_geometry_helpers as G
import softmax_helpers as S

INF, NAN = float("inf"), float("nan")
# operands stored as f16 (split or plain): 70 000 is a finite fp32 number beyond f16's rounding boundary 65 520
F16_POISONS = (("+70000", 70000.0), ("-70000", -70000.0), ("+inf", INF), ("nan", NAN))
F32_POISONS = (("+inf", INF), ("-inf", -INF), ("nan", NAN))
F16_CONTROL = 65519.0          # rounds to 65 504: no poison
F32_CONTROL = 70000.0          # an fp32 operand has no such range


class PoisonMismatch(AssertionError):
    """A poisoned launch differs from what its site prescribes; the message names site, operand and element."""


class Site:
    """one poisoned operand element: `operand` q / k / v / pad_k / pad_v (attention: grid token or None for the pad row,
    head, feature d) or a / w (GEMM: row, k)"""

    def __init__(self, name, operand, roles, **where):
        self.name, self.operand, self.roles = name, operand, tuple(roles)
        self.__dict__.update(where)

    def __repr__(self):
        return self.name


# ------------------------------------------------------------------------------------------------ attention: roles

Q_FIRST = "query in the first wave of a work-group"
Q_LAST = "query in the last wave of a work-group"
Q_IDLE = "query in a work-group whose last waves idle"
Q_OTHER_WIN = "query in the last window"
K_TILE0, K_TILE1, K_LAST = "key tile 0", "key tile 1", "last key tile"
HALF0, HALF1 = "lane half 0", "lane half 1"
PAD_KEY = "pad key"
OP_Q, OP_K, OP_V = "Q fragment", "K fragment", "V fragment"
D_0, D_31, D_32, D_LAST, D_TAIL = "d = 0", "d = 31", "d = 32", "d = hd - 1", "d in 64..71 (hd = 72)"
B_FULL_Q = "balanced: query in a full wave-tile"
B_SPLIT_Q = "balanced: query merged from 3 to 4 key-range pieces"
B_KEY_FULL = "balanced: key walked by the full wave-tile passes"
B_KEY_INSIDE = "balanced: key inside a key-split piece"
B_BEFORE, B_AFTER = "balanced: last key before a cut", "balanced: first key after a cut"
H_WAVE = tuple(f"hyper: key in the share of wave {w}" for w in range(4))
H_RAGGED_K, H_Q_FIRST, H_Q_LAST = "hyper: ragged last key tile", "hyper: first query tile", "hyper: ragged last query tile"

WINDOW_ROLES = frozenset([Q_FIRST, Q_LAST, Q_IDLE, K_TILE0, K_TILE1, K_LAST, HALF0, HALF1, OP_Q, OP_K, OP_V, D_0, D_31, D_32,
                          D_LAST])
PADDED_ROLES = WINDOW_ROLES | {PAD_KEY, Q_OTHER_WIN}
BALANCED_ROLES = WINDOW_ROLES | {B_FULL_Q, B_SPLIT_Q, B_KEY_FULL, B_KEY_INSIDE, B_BEFORE, B_AFTER}
HYPER_ROLES = frozenset(H_WAVE) | {H_RAGGED_K, H_Q_FIRST, H_Q_LAST, OP_Q, OP_K, OP_V, D_0, D_31, D_32, D_LAST, D_TAIL}


def feature_roles(d, hd):
    out = [r for r, v in ((D_0, 0), (D_31, 31), (D_32, 32), (D_LAST, hd - 1)) if d == v]
    if hd == 72 and 64 <= d < 72:
        out.append(D_TAIL)
    return out


def _half(t):
    return HALF1 if ((t % 32) >> 2) & 1 else HALF0


def _real_in_tile(wins, w, tile, slot):
    """window-local position of a real token in key tile `tile` of window w: `slot`, else the next real one of the tile
    in the same lane half, else any; None where the tile holds pad positions only"""
    cand = [tile * 32 + (slot + s) % 32 for s in range(32)]
    cand.sort(key=lambda t: _half(t) != _half(tile * 32 + slot))
    for t in cand:
        if t < wins.L and wins.tok_of[w, t] >= 0:
            return t
    return None


def _waves(wins, w, nw):
    """(active [waves of whole work-groups] bool, n work-groups) of window w for nw-wave work-groups"""
    n_wv = -(-wins.L // 32)
    n_wg = -(-n_wv // nw)
    act = np.zeros(n_wg * nw, bool)
    for v in range(n_wv):
        act[v] = bool((wins.tok_of[w, 32 * v:32 * v + 32] >= 0).any())
    return act, n_wg


def _last_real(wins, w, wave):
    ts = [t for t in range(32 * wave, min(32 * wave + 32, wins.L)) if wins.tok_of[w, t] >= 0]
    return ts[-1] if ts else None


def random_sign_features(hd, L):
    """the features of softmax_helpers.layout whose q and k carry random signs"""
    return list(range(S.layout(hd, L)["rnd0"], hd))


def attention_sites(wins, heads, hd, nw, groups=None):
    """The sites of one windowed / whole-grid case: nw waves per work-group; groups: the balanced launch's slots per head.
    K sites (and the pad row's K) take random-sign features only: a bare +-inf there gives scores of either sign."""
    L, n_win = wins.L, wins.tok_of.shape[0]
    nt = -(-L // 32)
    rnd = random_sign_features(hd, L)
    kf = [d for d in (32, hd - 1, 40) if d in rnd] + ([64] if hd == 72 else [])
    assert len(kf) >= 2
    sites = []
    n = [0]

    def add(operand, w, t, d, roles):
        tok = None if t is None else int(wins.tok_of[w, t])
        assert tok is None or tok >= 0
        h = n[0] % heads if groups is None else (0, 7, 13, heads - 1)[n[0] % 4] % heads
        n[0] += 1
        where = "pad row" if t is None else f"window {w}, position {t} (token {tok})"
        op_role = {"q": OP_Q, "k": OP_K, "v": OP_V, "pad_k": OP_K, "pad_v": OP_V}[operand]
        sites.append(Site(f"{operand}[{where}, head {h}, d {d}]", operand, list(roles) + [op_role] + feature_roles(d, hd),
                          token=tok, head=h, d=d, window=w, loc=t))

    # ---- queries
    act, n_wg = _waves(wins, 0, nw)
    first = nw if n_wg > 1 and act[nw] else 0
    add("q", 0, _real_in_tile(wins, 0, first, 5), 0, [Q_FIRST] + ([B_FULL_Q] if groups else []))
    add("q", 0, _real_in_tile(wins, 0, nw - 1 if act[nw - 1] else int(np.nonzero(act[:nw])[0][-1]), 20), 31,
        [Q_LAST] + ([B_FULL_Q] if groups else []))
    if groups:
        tile0, grps = S.bal_cuts(nt, groups, nw)
        assert 3 <= len(grps[0][1]) <= 4
        add("q", 0, (tile0 + 3) * 32 + 7, hd - 1, [B_SPLIT_Q])
        n_act = grps[-1][0]
        assert n_act < nw                                            # the last group holds idle waves
        add("q", 0, (tile0 + (len(grps) - 1) * nw + n_act - 1) * 32 + 9, 32, [Q_IDLE, B_SPLIT_Q])
    else:
        for w in range(n_win):
            act, n_wg = _waves(wins, w, nw)
            mixed = [g for g in range(n_wg) if act[g * nw:(g + 1) * nw].any() and not act[g * nw:(g + 1) * nw].all()]
            if mixed:
                wave = mixed[-1] * nw + int(np.nonzero(act[mixed[-1] * nw:(mixed[-1] + 1) * nw])[0][-1])
                add("q", w, _last_real(wins, w, wave), hd - 1, [Q_IDLE])
                break
        if n_win > 1:
            add("q", n_win - 1, _real_in_tile(wins, n_win - 1, 0, 9), 32, [Q_OTHER_WIN])
    if hd == 72:
        add("q", 0, _real_in_tile(wins, 0, 1, 3), 71, [])
    # ---- keys: tiles 0, 1, last real one; both lane halves (the slots of softmax_helpers.default_sites)
    last_tile = {w: max(t for t in range(L) if wins.tok_of[w, t] >= 0) // 32 for w in range(n_win)}
    w1 = n_win - 1 if last_tile[n_win - 1] >= 1 else 0
    keys = [(0, 0, 3, [K_TILE0]), (w1, 1, 6, [K_TILE1]), (0, last_tile[0], 12, [K_LAST])]
    if groups:
        cuts = sorted({j0 for _, pcs in grps for j0, _ in pcs if j0 > 0})
        keys = [(0, 0, 3, [K_TILE0, B_KEY_FULL]), (0, 1, 6, [K_TILE1, B_KEY_FULL]), (0, nt - 1, 12, [K_LAST, B_KEY_FULL]),
                (0, cuts[0] - 1, 31, [B_BEFORE]), (0, cuts[0], 0, [B_AFTER]), (0, (cuts[0] + cuts[1]) // 2, 17, [B_KEY_INSIDE])]
    for i, (w, tile, slot, roles) in enumerate(keys):
        t = _real_in_tile(wins, w, tile, slot)
        add("k", w, t, kf[i % len(kf)], roles + [_half(t)])
    vfeat = [0, 31, 32, hd - 1] + ([64, 71] if hd == 72 else [])
    vkeys = keys + [(0, 0, 28, [K_TILE0])] + ([(0, 1, 17, [K_TILE1]), (0, last_tile[0], 3, [K_LAST])] if hd == 72 else [])
    for i, (w, tile, slot, roles) in enumerate(vkeys):
        t = _real_in_tile(wins, w, tile, slot)
        add("v", w, t, vfeat[i % len(vfeat)], roles + [_half(t)])
    if wins.n_pad().any():
        add("pad_k", None, None, kf[0], [PAD_KEY])
        add("pad_v", None, None, 31, [PAD_KEY])
    return sites


def hyper_sites(n, heads, hd):
    """cra5_hyper_attention_f32: 16-key tiles dealt to 4 waves, 16-query tiles"""
    wins = X.Windows(1, n, 1, n)
    rnd = random_sign_features(hd, n)
    kf = [d for d in (32, hd - 1, 40, 20) if d in rnd]
    keys = [(ks[0], [H_WAVE[(ks[0] // 16) % 4]]) for ks in S.hyper_sites(n) if ks[0] < n - 1]
    keys.append((n - 1, [H_RAGGED_K if n % 16 else H_WAVE[((n - 1) // 16) % 4]]))
    sites = []

    def add(operand, tok, d, roles, i):
        op_role = {"q": OP_Q, "k": OP_K, "v": OP_V}[operand]
        sites.append(Site(f"{operand}[token {tok}, head {i % heads}, d {d}]", operand, list(roles) + [op_role] + feature_roles(d, hd),
                          token=tok, head=i % heads, d=d, window=0, loc=tok))
    add("q", 5 if n > 5 else 0, 0, [H_Q_FIRST], 0)
    add("q", n - 1, 31, [H_Q_LAST], 1)
    vfeat = [0, 31, 32, hd - 1] + ([64, 71] if hd == 72 else [])
    for i, (k, roles) in enumerate(keys):
        add("k", k, kf[i % len(kf)], roles, i)
        add("v", k, vfeat[i % len(vfeat)], roles, i + 1)
    return wins, sites


def roles_of(sites):
    return frozenset(r for s in sites for r in s.roles)


# ------------------------------------------------------------------------------------------------ attention: sets


def column_of(site, heads, hd):
    """column of the poisoned element in the [N, 3C] qkv matrix (or the [3C] pad row)"""
    which = {"q": 0, "k": 1, "v": 2, "pad_k": 1, "pad_v": 2}[site.operand]
    return which * heads * hd + site.head * hd + site.d


def poisoned(qkv, pad, site, value, heads, hd):
    """(qkv, pad) with the site's element replaced by `value` (copies)"""
    qkv, pad = qkv.clone(), pad.clone()
    col = column_of(site, heads, hd)
    if site.token is None:
        pad[col] = value
    else:
        qkv[site.token, col] = value
    return qkv, pad


def _reader_rows(wins, site):
    """grid tokens whose output rows read the site's element"""
    if site.operand == "q":
        return np.array([site.token])
    if site.token is None:
        ws = np.nonzero(wins.n_pad() > 0)[0]
    else:
        ws = [int(wins.win_of[site.token])]
    return np.concatenate([wins.tok_of[w][wins.tok_of[w] >= 0] for w in ws])


def attention_expected(wins, heads, hd, site):
    """E bool [N, C], from the geometry alone: Q[i, h, d] -> out[i, head h]; K[j, h, d] -> head h of every query of the
    window that holds key j; V[j, h, d] -> column h hd + d of those queries; the pad row's K / V -> the same in every
    window that has pad positions"""
    E = torch.zeros(wins.H * wins.W, heads * hd, dtype=torch.bool)
    rows = torch.from_numpy(_reader_rows(wins, site))
    if site.operand in ("v", "pad_v"):
        E[rows, site.head * hd + site.d] = True
    else:
        E[rows, site.head * hd:(site.head + 1) * hd] = True
    return E


def wave_block(wins, heads, hd, site):
    """bool [N, C]: head h of the 32 queries that share a wave with the site's query.  cra5 window_attention_split_kernel
    decides its rescales per WAVE (`!__all(mloc - m_run <= 8)`, `!__all(psum <= P_SAFE)`): a poisoned query makes its wave
    take the branch on every tile, which moves its 31 neighbours' reference point - other bits, the same softmax."""
    assert site.operand == "q"
    w, wave = int(wins.win_of[site.token]), int(wins.loc_of[site.token]) // 32
    toks = wins.tok_of[w, 32 * wave:32 * wave + 32]
    A = torch.zeros(wins.H * wins.W, heads * hd, dtype=torch.bool)
    A[torch.from_numpy(toks[toks >= 0]), site.head * hd:(site.head + 1) * hd] = True
    return A


def stored(x, family):
    """float64 of an fp32 operand as the engine family reads it, non-finite values kept: "split" hi + lo of the split
    store (70 000 -> inf - inf = NaN), "hi" the f16 hi plane (70 000 -> inf), "f32" / "hyper" the value itself"""
    if family == "split":
        hi, lo = X.split_model(x)
        return hi.double() + lo.double()
    if family == "hi":
        return x.float().half().double()
    return x.double()


def classify(qkv, pad, wins, heads, hd, site, family):
    """Row classes of a poisoned Q / K element by a float64 IEEE evaluation of the scores, from the operands as stored
    (qkv, pad: fp32, the poison in place): (mandatory bool [N], either bool [N], drop bool [windows, L]).  Mandatory: a
    NaN or +inf score (or no finite score at all: 0 / 0); either: the affected scores are all -inf - the keys `drop`
    fall out of the softmax.  The finite part of a score is a float64 dot product without the poisoned feature; the
    poisoned term q_d k_d is added by itself (0 inf = NaN).  Reduced precision: the kernel's own q, f16(q_hi c)."""
    assert site.operand in ("q", "k", "pad_k") and family in ("hi", "f32", "hyper")
    N, C, L = wins.H * wins.W, heads * hd, wins.L
    h, d = site.head, site.d
    ext = torch.cat([stored(qkv, family), stored(pad.reshape(1, -1), family)], 0).view(N + 1, 3, heads, hd)[:, :, h]
    q_all, k_all = ext[:, 0], ext[:, 1]
    if family == "hi":
        q_all = torch.from_numpy(S._f16((q_all.numpy().astype(np.float32) * S.cexp32(hd)).astype(np.float32)))
    mand, either = np.zeros(N, bool), np.zeros(N, bool)
    drop = np.zeros((wins.tok_of.shape[0], L), bool)
    if site.token is None:
        ws = np.nonzero(wins.n_pad() > 0)[0]
    else:
        ws = [int(wins.win_of[site.token])]
    for w in ws:
        idx = np.where(wins.tok_of[w] >= 0, wins.tok_of[w], N)
        real = idx < N
        q, k = q_all[idx].clone(), k_all[idx].clone()
        if site.operand == "q":
            iq = int(wins.loc_of[site.token])
            qd = q[iq, d].clone()
            q[iq, d] = 0.0
            t = q @ k.t()
            t[iq] = t[iq] + qd * k[:, d]
            sel = np.zeros(L, bool)
            sel[iq] = True
        else:
            pos = torch.from_numpy(idx == (N if site.token is None else site.token))
            kd = k[pos, d].clone()
            k[pos, d] = 0.0
            t = q @ k.t()
            t[:, pos] = t[:, pos] + q[:, d:d + 1] * kd[None, :]
            sel = real
        assert bool(torch.isfinite(q).all()) and bool(torch.isfinite(k).all())
        bad = (torch.isnan(t) | (t == INF)).any(1) | ~torch.isfinite(t).any(1)
        gone = t == -INF
        m_w = bad.numpy() & sel
        e_w = ~bad.numpy() & gone.any(1).numpy() & sel
        mand[idx[m_w]] = True
        either[idx[e_w]] = True
        if e_w.any():
            rows = torch.from_numpy(e_w)
            assert bool((gone[rows] == gone[rows][0]).all()), "the rows of one window drop different keys"
            drop[w] = gone[rows][0].numpy()
    return mand, either, drop


# ------------------------------------------------------------------------------------------------ GEMM family

G_I_FIRST, G_I_FULL, G_I_RAGGED = "row in the first tile", "row in the last full tile", "row in the ragged last tile"
G_K_FIRST, G_K_MID, G_K_LAST = "k in the first k-step", "k in a middle k-step", "k = K - 1"
G_N_FIRST, G_N_FULL, G_N_RAGGED = "column in the first tile", "column in the last full tile", "column in the ragged last tile"
G_A, G_W = "A operand", "W operand"
GEMM_ROLES = frozenset([G_I_FIRST, G_I_FULL, G_K_FIRST, G_K_MID, G_K_LAST, G_N_FIRST, G_N_FULL, G_A, G_W])
GEMM_RAGGED_ROLES = GEMM_ROLES | {G_I_RAGGED, G_N_RAGGED}


def gemm_sites(M, N, K, tile_m, tile_n, k_step=32):
    """one A row and one W row per tile role (first tile, last full tile, ragged last tile where the shape has one),
    with k in the first k-step, a middle one and at K - 1 in turn"""
    ks = [(5 % K, G_K_FIRST), ((K // k_step // 2) * k_step + 9, G_K_MID), (K - 1, G_K_LAST)]
    assert k_step <= ks[1][0] < K - k_step or K <= 2 * k_step

    def axis(n, tile, first, full, ragged):
        nfull = n // tile
        out = [(min(3, n - 1), first)]
        if nfull >= 1:
            out.append((nfull * tile - 2, full))
        if n % tile:
            out.append((n - 1, ragged))
        return out
    sites = []
    for j, (i, role) in enumerate(axis(M, tile_m, G_I_FIRST, G_I_FULL, G_I_RAGGED)):
        k, krole = ks[j % 3]
        sites.append(Site(f"A[{i}, {k}]", "a", [G_A, role, krole], row=i, k=k))
    for j, (n, role) in enumerate(axis(N, tile_n, G_N_FIRST, G_N_FULL, G_N_RAGGED)):
        k, krole = ks[(j + 1) % 3]
        sites.append(Site(f"W[{n}, {k}]", "w", [G_W, role, krole], row=n, k=k))
    return sites


def gemm_expected(M, N, site):
    """A[i, k] -> row i of the output; W[n, k] -> column n of every row"""
    E = torch.zeros(M, N, dtype=torch.bool)
    if site.operand == "a":
        E[site.row] = True
    else:
        E[:, site.row] = True
    return E


U_FIRST, U_LAST, U_TILE_EDGE, U_INTERIOR = ("un-embed: token (0, 0)", "un-embed: the last token",
                                            "un-embed: last row of a 256-row GEMM tile", "un-embed: an interior token")
UNEMBED_ROLES = frozenset([U_FIRST, U_LAST, U_TILE_EDGE, U_INTERIOR])


def unembed_sites(Hp, Wp, K):
    M = Hp * Wp
    toks = [(0, U_FIRST, 5 % K), (M - 1, U_LAST, K - 1), (255, U_TILE_EDGE, K // 2), ((Hp // 2) * Wp + Wp // 3, U_INTERIOR, 40 % K)]
    return [Site(f"A[token ({m // Wp}, {m % Wp}), {k}]", "a", [role], row=m, k=k) for m, role, k in toks if m < M]


def unembed_expected(C, Hp, Wp, site):
    """bool [C, 10 Hp + 1, 10 Wp]: the pixels whose fold indicator is non-zero - F.fold of the 0 / 1 column matrix with
    the token's row set: its 11 x 10 patch in every channel, the seam rows it shares with its neighbours included"""
    cols = torch.zeros(Hp * Wp, C * G.KH * G.KW, dtype=torch.float64)
    cols[site.row] = 1.0
    return G.col2im_reference(cols, C, Hp, Wp) != 0


# ------------------------------------------------------------------------------------------------ the checker


def _bits(t):
    t = t.contiguous()
    return t.view({4: torch.int32, 2: torch.int16, 8: torch.int64}[t.element_size()])


def check(clean, got, E, site, value, label, allow=None, either=None, bound=None, at_least_one=False, locate=None):
    """clean, got: tuples of same-shaped planes of one output (an fp32 tensor alone, or the (hi, lo) planes of a split
    output: the value is their sum).  E bool: every element non-finite in `got`; outside E (and `allow`): every plane
    holds the clean launch's bits.  allow bool (a superset of E): elements outside E but inside it may hold other bits
    and must be finite.  either bool (inside E) with bound = (ref, B): non-finite, or |got - ref| <= B.
    at_least_one: instead of "every element of E", every ROW of E holds at least one non-finite element (the
    reduced-precision GELU epilogue).  Raises PoisonMismatch naming site, operand and element."""
    clean = clean if isinstance(clean, (tuple, list)) else (clean,)
    got = got if isinstance(got, (tuple, list)) else (got,)
    dev = got[0].device
    flat = lambda t: t.to(dev).reshape(-1, t.shape[-1])          # (an image [C, H, W] is checked as [C H, W])
    assert all(c_.shape == g_.shape for c_, g_ in zip(clean, got)) and tuple(E.shape) == tuple(got[0].shape)
    E = flat(E)
    val = flat(got[0] if len(got) == 1 else got[0] + got[1])
    nonfin = ~torch.isfinite(val)
    who = f"{label}: site {site.name} (operand {site.operand}) = {value!r}"

    def fail(kind, mask):
        idx = mask.nonzero()
        r, c = int(idx[0, 0]), int(idx[0, 1])
        where = f"element ({r}, {c})" + (": " + locate(r, c) if locate is not None else "")
        raise PoisonMismatch(f"{who}: {kind} at {where}; got {float(val[r, c])!r}, the clean launch "
                             f"{float(sum(flat(p)[r, c] for p in clean))!r} ({int(mask.sum())} such element(s), "
                             f"{int(E.sum())} expected non-finite)")
    must = E if either is None else E & ~flat(either)
    if at_least_one:
        rows = must.any(1)
        dry = rows & ~(nonfin & must).any(1)
        if bool(dry.any()):
            fail("LAUNDERED: an expected row holds no non-finite value", dry[:, None] & must)
    elif bool((must & ~nonfin).any()):
        fail("LAUNDERED: an expected element is finite", must & ~nonfin)
    if either is not None:
        ei = flat(either)
        ref, B = bound
        ok = nonfin | ((val.double() - flat(ref)).abs() <= flat(B))
        if bool((ei & ~ok).any()):
            fail("a row whose poisoned keys drop out is finite and outside the softmax bound", ei & ~ok)
    soft = torch.zeros_like(E) if allow is None else flat(allow) & ~E
    if bool((nonfin & ~E).any()):
        fail("LEAKED: a non-finite value outside the expected set", nonfin & ~E)
    same = torch.ones_like(E)
    for c_, g_ in zip(clean, got):
        same &= flat(_bits(c_) == _bits(g_))
    if bool((~same & ~E & ~soft).any()):
        fail("CHANGED: an element that reads nothing poisoned differs from the clean launch", ~same & ~E & ~soft)
    return int(nonfin.sum())


def check_control(got, site, value, label):
    """the negative control: finite everywhere"""
    got = got if isinstance(got, (tuple, list)) else (got,)
    val = got[0] if len(got) == 1 else got[0] + got[1]
    if not bool(torch.isfinite(val).all()):
        idx = (~torch.isfinite(val)).reshape(-1, val.shape[-1]).nonzero()[0]
        raise PoisonMismatch(f"{label}: site {site.name} (operand {site.operand}) = {value!r} is no poison, yet element "
                             f"({int(idx[0])}, {int(idx[1])}) is non-finite")


# ------------------------------------------------------------------------------------------------ float64 evaluations


def balanced_float64(qkv, wins, heads, groups, nw=12):
    """float64 whole-grid attention evaluated the balanced launch's way: full wave-tiles over the whole key loop, the
    key-split groups as per-piece partials (m, l, O) merged with exp2(m_p - M) - the same data flow, so a poisoned
    operand must come out non-finite in the same elements"""
    N, C = qkv.shape[0], qkv.shape[1] // 3
    hd = C // heads
    x = qkv.double().view(N, 3, heads, hd).permute(1, 2, 0, 3)
    c = S.c_of(hd)
    tile0, grps = S.bal_cuts(N // 32, groups, nw)
    out = torch.zeros(N, C, dtype=torch.float64)

    def part(q, k, v):
        t = (q @ k.transpose(-1, -2)) * c
        m = t.amax(-1, keepdim=True)
        p = torch.exp2(t - m)
        return m, p.sum(-1, keepdim=True), p @ v
    put = lambda r0, r1, o: out[r0:r1].copy_(o.permute(1, 0, 2).reshape(r1 - r0, C))
    if tile0:
        m, l, o = part(x[0][:, : tile0 * 32], x[1], x[2])
        put(0, tile0 * 32, o / l)
    for g, (n_act, pieces) in enumerate(grps):
        r0 = (tile0 + nw * g) * 32
        r1 = r0 + n_act * 32
        parts = [part(x[0][:, r0:r1], x[1][:, 32 * j0:32 * j1], x[2][:, 32 * j0:32 * j1]) for j0, j1 in pieces]
        M = torch.stack([p[0] for p in parts]).amax(0)
        l = sum(p[1] * torch.exp2(p[0] - M) for p in parts)
        o = sum(p[2] * torch.exp2(p[0] - M) for p in parts)
        put(r0, r1, o / l)
    return out
