"""Inputs on which fp32 arithmetic is exact in ANY order, their integer-exact expectations, and the mismatch report -
shared by tests/test_exact_gpu.py (the engines) and tests/test_exact_inputs_cpu.py (these builders themselves).

GEMM family.  Operands live on the grid x = p + q * 2^-12 (p = +-1, q in {-1, 0, 1}, plus a share of exact zeros): the
split-f16 store gives hi = p, lo = q * 2^-12 (a normal f16), every product hi.hi / hi.lo / lo.hi is a multiple of one
granule, and while sum_k |term| stays below 2^24 granules every partial sum of every summation order is an exact fp32
number.  The engines' documented result, wscale_inv * sum_k (hi_a hi_w + hi_a lo_w + lo_a hi_w), can then be compared
bit for bit with a float64 evaluation of the same three products.

Attention.  UNIFORM: k = 0 everywhere, so every score is 0, every p is 1 and the output is (sum of the window's v rows) /
(tokens of the window) - a count of keys.  PERMUTATION: q_i = s u_i, k_j = s u_pi(j) with u random +-1 vectors: the
matching key out-scores every other by >= 48 log2 units, so the output is that key's v row - a pairing of queries and
keys.

Everything here runs on whatever device its tensors live on; nothing calls a product kernel."""
import numpy as np
import torch

LIMIT = float(2 ** 24)
TILINGS = ((256, 256), (192, 256), (128, 128), (64, 64))     # (rows, columns) of the GEMM engines' output tiles


class InputNotExact(AssertionError):
    """The INPUT of an exact test breaks an exactness condition: the test is wrong, not the kernel."""


class ExactMismatch(AssertionError):
    """An engine's output differs from the integer-exact expectation; the message says where."""


# ------------------------------------------------------------------------------------------------ GEMM operands


def grid_matrix(rows, cols, density, seed, lo_shift=12):
    """fp32 [rows, cols] on the grid p + q * 2^-lo_shift; a (1 - density) share of exact zeros."""
    g = torch.Generator().manual_seed(seed)
    p = torch.randint(0, 2, (rows, cols), generator=g).float() * 2 - 1
    q = torch.randint(-1, 2, (rows, cols), generator=g).float()
    keep = torch.rand(rows, cols, generator=g) < density
    return ((p + q * 2.0 ** -lo_shift) * keep).contiguous()


def grid_vector(n, seed, span=3, granule=2.0 ** -12):
    """bias-like fp32 [n]: integers in [-span, span] plus a multiple of the granule"""
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-span, span + 1, (n,), generator=g).float()
            + torch.randint(-5, 6, (n,), generator=g).float() * granule)


def split_model(x, scale=1.0):
    """Host restatement of the split-f16 store (csrc/split.h): hi = f16(x * scale), lo = f16(x * scale - hi)."""
    xs = x.float() * scale
    hi = xs.half().float()
    lo = (xs - hi).half().float()
    return hi, lo


def _granule(p):
    """the largest power of two that divides every element of a plane; None for an all-zero plane"""
    u = torch.unique(p.abs().double())
    u = u[u != 0]
    if not u.numel():
        return None
    for e in range(-20, 60):
        r = u * 2.0 ** e
        if bool((r == r.round()).all()):
            return 2.0 ** -e
    raise InputNotExact("input not exact: plane values are not multiples of a power of two >= 2^-59")


def _term_granule(pairs):
    """granule of a sum of plane products: the smallest product of two plane granules, which must divide the others"""
    gs = [ga * gb for ga, gb in pairs if ga is not None and gb is not None]
    if not gs:
        raise InputNotExact("input not exact: an operand is all zeros")
    g = min(gs)
    if any((x / g) != round(x / g) for x in gs):
        raise InputNotExact(f"input not exact: the products' granules {gs!r} are not multiples of one another")
    return g


def check_planes(x, hi, lo, scale_inv, what):
    """The stored planes (read back from the SplitMat) reconstruct the input exactly and hold no f16 subnormal."""
    rec = (hi.double() + lo.double()) * scale_inv
    if not bool((rec == x.double().to(rec.device)).all()):
        n = int((rec != x.double().to(rec.device)).sum())
        raise InputNotExact(f"input not exact: {what}: hi + lo differs from the input on {n} element(s)")
    for name, p in (("hi", hi), ("lo", lo)):
        sub = (p != 0) & (p.abs() < 2.0 ** -14)
        if bool(sub.any()):
            raise InputNotExact(f"input not exact: {what}: {int(sub.sum())} subnormal f16 value(s) in the {name} plane")


def three_product_expectation(a_planes, w_planes, scale_inv, hi_only=False, bias=None, res=None):
    """float64 [M, N]: scale_inv * sum_k (hi_a hi_w [+ hi_a lo_w + lo_a hi_w]) [+ bias] [+ res], with the exactness
    conditions asserted: sum_k |term| (+ |bias| + |res|) below 2^24 granules, so that every fp32 partial sum of every
    order is exact, and the expectation itself an fp32 number.  Returns (expectation, granule of the result, the
    largest sum of |terms| in granules)."""
    ha, la = (t.double() for t in a_planes)
    hw, lw = (t.double() for t in w_planes)
    if hi_only:
        g = _term_granule([(_granule(ha), _granule(hw))])
        e = ha @ hw.t()
        mag = ha.abs() @ hw.abs().t()
    else:
        gha, gla, ghw, glw = _granule(ha), _granule(la), _granule(hw), _granule(lw)
        g = _term_granule([(gha, ghw), (gha, glw), (gla, ghw)])
        # (hw + lw is exact in float64: 11 + 11 bits at most 2^-12 apart; each float64 dot product is exact: < 2^53 granules)
        e = ha @ (hw + lw).t() + la @ hw.t()
        mag = ha.abs() @ (hw.abs() + lw.abs()).t() + la.abs() @ hw.abs().t()
    e, mag, g = e * scale_inv, mag * scale_inv, g * scale_inv
    for name, t in (("bias", bias), ("res", res)):
        if t is None:
            continue
        t = t.double().to(e.device)
        g = min(g, _granule(t) or g)          # (powers of two: the finer one divides the other)
        e = e + t
        mag = mag + t.abs()
    worst = float(mag.max()) / g
    if not worst < LIMIT:
        raise InputNotExact(f"input not exact: sum of |terms| reaches {worst:.3e} granules, the limit is 2^24 = {LIMIT:.3e}")
    if not bool((e.float().double() == e).all()):
        raise InputNotExact("input not exact: the expectation is not an fp32 number")
    return e, g, worst


def product_expectation(a, w, bias=None, res=None):
    """the exact-f32 engine: float64 a . w^T (+ bias, res) of fp32 operands whose products and partial sums are exact"""
    z = torch.zeros(1, 1, device=a.device)
    return three_product_expectation((a, z), (w, z), 1.0, hi_only=True, bias=bias, res=res)


def unembed_expectation(e_cols, C, Hp, Wp, kh, kw, mean=None, std=None):
    """float64 image [C, (Hp-1)*10 + kh, Wp*kw] of the overlap-add of e_cols [Hp*Wp, C*kh*kw] (column (c*kh + i)*kw + j;
    stride (kh - 1, kw): row 10 t takes kernel row 10 of token row t - 1 plus kernel row 0 of token row t), then
    x * std[c] + mean[c]."""
    assert kh == 11 and kw == 10
    body = e_cols.view(Hp, Wp, C, kh, kw).permute(2, 0, 3, 1, 4)            # [C, Hp, kh, Wp, kw]
    W = Wp * kw
    img = torch.zeros(C, Hp * 10 + 1, W, dtype=torch.float64, device=e_cols.device)
    img[:, : Hp * 10].view(C, Hp, 10, W).add_(body[:, :, :10].reshape(C, Hp, 10, W))
    img[:, 10::10].add_(body[:, :, 10].reshape(C, Hp, W))
    if std is not None:
        img = img * std.double().to(img.device)[:, None, None] + mean.double().to(img.device)[:, None, None]
    if not bool((img.float().double() == img).all()):
        raise InputNotExact("input not exact: the un-embedded expectation is not an fp32 number")
    return img


# ------------------------------------------------------------------------------------------------ attention inputs


class Windows:
    """Window geometry of the attention kernels: the H x W token grid padded bottom / right to multiples of (wh, ww)."""

    def __init__(self, H, W, wh, ww):
        self.H, self.W, self.wh, self.ww = H, W, wh, ww
        self.nwr, self.nwc = -(-H // wh), -(-W // ww)
        self.Hp, self.Wp, self.L = self.nwr * wh, self.nwc * ww, wh * ww
        pos = np.arange(self.Hp * self.Wp).reshape(self.Hp, self.Wp)
        gr, gc = pos // self.Wp, pos % self.Wp
        tok = np.where((gr < H) & (gc < W), gr * W + gc, -1)
        # tok_of[window, t]: grid token of window-local position t, -1 for a pad position
        self.tok_of = tok.reshape(self.nwr, wh, self.nwc, ww).transpose(0, 2, 1, 3).reshape(self.nwr * self.nwc, self.L)
        self.win_of = np.empty(H * W, dtype=np.int64)
        self.loc_of = np.empty(H * W, dtype=np.int64)
        w_idx, t_idx = np.nonzero(self.tok_of >= 0)
        self.win_of[self.tok_of[w_idx, t_idx]] = w_idx
        self.loc_of[self.tok_of[w_idx, t_idx]] = t_idx

    def n_pad(self):
        return (self.tok_of < 0).sum(1)


def uniform_case(H, W, wh, ww, heads, hd, seed):
    """(qkv fp32 [H*W, 3C], pad row fp32 [3C], expectation float64 [H*W, C]): all k = 0 (the pad row's too), q arbitrary,
    v integers in [-8, 8], the pad row's v = b, integers in [9, 16].  Every p is 1: out = (sum of the window's real v +
    n_pad * b) / (wh * ww), from int64."""
    C, N = heads * hd, H * W
    g = torch.Generator().manual_seed(seed)
    qkv = torch.zeros(N, 3 * C)
    qkv[:, :C] = torch.randn(N, C, generator=g) * 3.0
    v = torch.randint(-8, 9, (N, C), generator=g)
    qkv[:, 2 * C:] = v.float()
    pad = torch.zeros(3 * C)
    pad[:C] = torch.randn(C, generator=g)
    b = torch.randint(9, 17, (C,), generator=g)
    pad[2 * C:] = b.float()
    wins = Windows(H, W, wh, ww)
    vn, bn = v.numpy().astype(np.int64), b.numpy().astype(np.int64)
    v_ext = np.concatenate([vn, bn[None]], 0)                       # row N = the pad row
    sums = v_ext[np.where(wins.tok_of >= 0, wins.tok_of, N)].sum(1)  # [windows, C]
    exp = torch.from_numpy(sums[wins.win_of].astype(np.float64) / float(wins.L))
    return qkv, pad, exp, wins


def token_rows(n, hd):
    """int64 [n, hd]: rows that identify their token (base-16 digits of the index, + 1, sign alternating by column):
    distinct for n <= 65 536, never zero, |v| <= 16 - exact in f16."""
    t = np.arange(n, dtype=np.int64)[:, None]
    d = np.arange(hd, dtype=np.int64)[None, :]
    return (((t >> (4 * (d % 4))) & 15) + 1) * np.where(d % 2 == 0, 1, -1)


def permutation_case(H, W, wh, ww, heads, hd, seed, s=4, min_gap=48.0, max_draws=20, device="cpu"):
    """(qkv, pad row, expectation, windows, info): q_i = s u_i, k_j = s u_pi(j), u random +-1 vectors per (token, head), pi a
    fixed permutation of the REAL tokens of each window; pad rows: k = 0.  v[j] = token_rows (the same rows for every head,
    shifted by the head index so that heads differ).  Expectation: out_i = v[pi^-1(i)].  u is drawn again until the matching
    key's score exceeds every other key's (the pad row's included) by >= min_gap log2 units; info says how many draws and
    the gap."""
    C, N = heads * hd, H * W
    wins = Windows(H, W, wh, ww)
    rng = np.random.default_rng(seed)
    log2u = s * s * hd ** -0.5 * 1.4426950408889634                 # log2 units per unit of u_i . u_j
    for draw in range(1, max_draws + 1):
        u = (rng.integers(0, 2, (N, heads, hd)) * 2 - 1).astype(np.float32)
        worst = -hd
        for w in range(wins.tok_of.shape[0]):
            toks = wins.tok_of[w][wins.tok_of[w] >= 0]
            for h in range(heads):
                uw = torch.from_numpy(u[toks, h]).to(device).double()
                c = uw @ uw.t()                                       # exact: integers <= hd (torch, on `device`)
                c.fill_diagonal_(-hd)
                worst = max(worst, int(c.max()))
        has_pad = bool((wins.tok_of < 0).any())
        gap = log2u * min(hd - worst, hd if has_pad else 10 ** 9)
        if gap >= min_gap:
            break
    else:
        raise InputNotExact(f"input not exact: no draw of u in {max_draws} reached a score gap of {min_gap} log2 units")
    src = np.arange(N)                                                # src[i] = the key that query i matches
    for w in range(wins.tok_of.shape[0]):
        toks = wins.tok_of[w][wins.tok_of[w] >= 0]
        src[toks] = toks[rng.permutation(len(toks))]
    qkv = np.zeros((N, 3, heads, hd), dtype=np.float32)
    qkv[:, 0] = s * u
    qkv[src, 1] = s * u                                               # k[src[i]] = s u_i
    vrows = token_rows(N, hd)
    v = vrows[:, None, :] + np.sign(vrows[:, None, :]) * np.arange(heads, dtype=np.int64)[None, :, None]
    qkv[:, 2] = v
    pad = np.zeros((3, heads, hd), dtype=np.float32)
    pad[0] = rng.standard_normal((heads, hd))
    pad[2] = 40.0                                                      # a v row no real token has
    exp = v[src].astype(np.float64).reshape(N, C)
    info = dict(draws=draw, gap_log2=float(gap), max_cross=int(worst), src=src, v=v.reshape(N, C))
    return (torch.from_numpy(qkv.reshape(N, 3 * C)), torch.from_numpy(pad.reshape(3 * C)), torch.from_numpy(exp), wins, info)


def window_operands(planes, pad_planes, wins, heads):
    """The pad rule's gather, per window: (idx [L] rows of the extended matrix - N = the pad row -, real [L], the (q, k, v) of
    the hi plane and of the lo plane as [3, heads, L, hd]).  planes / pad_planes: (hi, lo) of the [N, 3C] matrix and of the
    pad row (lo zeros for an operand that is not split), on any device."""
    hi, lo = planes
    N = hi.shape[0]
    hd = hi.shape[1] // 3 // heads
    ext = [torch.cat([p, pp.reshape(1, -1).to(p.device)], 0) for p, pp in zip((hi, lo), pad_planes)]
    for w in range(wins.tok_of.shape[0]):
        idx = np.where(wins.tok_of[w] >= 0, wins.tok_of[w], N)
        ti = torch.from_numpy(idx).to(hi.device)
        parts = [e[ti].view(-1, 3, heads, hd).permute(1, 2, 0, 3) for e in ext]
        yield idx, idx < N, parts[0], parts[1]


def attention_float64(qkv, pad, wins, heads):
    """Plain float64 windowed attention with the pad rule (pad positions carry q = k = v = pad row, unmasked) -> [H*W, C];
    for the CPU tests of the builders above."""
    N, C = qkv.shape[0], qkv.shape[1] // 3
    hd = C // heads
    out = torch.zeros(N, C, dtype=torch.float64)
    z, zp = torch.zeros_like(qkv, dtype=torch.float64), torch.zeros_like(pad, dtype=torch.float64)
    for idx, real, x, _ in window_operands((qkv.double(), z), (pad.double(), zp), wins, heads):
        o = (torch.softmax(x[0] @ x[1].transpose(-1, -2) * hd ** -0.5, -1) @ x[2]).permute(1, 0, 2).reshape(-1, C)
        out[idx[real]] = o[torch.from_numpy(real)]
    return out


def plain_rows_of(s):
    """a plain f16 matrix living in the first half of every row of a split-layout buffer (what the model's workspaces hold in
    the reduced-precision mode): the hi plane of the SplitMat `s`, as a new SplitMat of the same class"""
    sm = type(s).empty(s.rows, s.K, s.data.device, zero=True)
    sm.data[:, : sm.Kp] = s.data.view(s.rows, s.Kp // 32, 2, 32)[:, :, 0].reshape(s.rows, s.Kp)
    sm.plain = True
    return sm


def ulps(got, exp64):
    """|got - exp| in units of the fp32 ulp of the expected value (float64 tensor)"""
    e32 = exp64.float()
    ulp = torch.from_numpy(np.spacing(np.abs(e32.cpu().numpy()))).double().to(exp64.device)
    return (got.double() - exp64).abs() / ulp


# ------------------------------------------------------------------------------------------------ the report


def _box_in_tiles(r0, r1, c0, c1):
    parts = []
    for tr, tc in TILINGS:
        rr = f"{r0 // tr}" if r0 // tr == r1 // tr else f"{r0 // tr}..{r1 // tr}"
        cc = f"{c0 // tc}" if c0 // tc == c1 // tc else f"{c0 // tc}..{c1 // tc}"
        parts.append(f"{tr}x{tc}: tile row {rr}, tile column {cc}")
    return "; ".join(parts)


def attention_locator(wins, heads, hd, info=None, q_tile=32):
    """(row, col, got) -> '(window, head, query tile, key)' of an attention output element; with the permutation case's
    info also the key whose v row the output landed on."""
    def locate(r, c, got_row=None):
        head = c // hd
        txt = f"window {int(wins.win_of[r])}, head {head}, query tile {int(wins.loc_of[r]) // q_tile} (window-local token {int(wins.loc_of[r])})"
        if info is not None:
            want = int(info["src"][r])
            txt += f", key {want} (window-local {int(wins.loc_of[want])}) expected"
            if got_row is not None:
                vv = torch.from_numpy(info["v"][:, head * hd:(head + 1) * hd].astype(np.float64))
                d = (vv - got_row[head * hd:(head + 1) * hd].double().cpu()[None]).abs().amax(1)
                j = int(d.argmin())
                if float(d[j]) < 0.25:
                    txt += f", got key {j} (window-local {int(wins.loc_of[j])}, key tile {int(wins.loc_of[j]) // 32})"
        return txt
    return locate


def mismatch_report(got, exp, bad, granule, label, locate=None, gemm_tiles=True):
    """The text of a failure: how many elements differ, the first ten, the bounding box of all of them, and that box in
    tile units (GEMM) / as (window, head, query tile, key) (attention, through `locate`)."""
    idx = bad.nonzero()
    n = idx.shape[0]
    rows, cols = idx[:, 0], idx[:, 1]
    r0, r1, c0, c1 = int(rows.min()), int(rows.max()), int(cols.min()), int(cols.max())
    lines = [f"{label}: {n} of {bad.numel()} elements differ from the exact expectation"]
    lines.append(f"bounding box: rows {r0}..{r1}, columns {c0}..{c1}")
    if gemm_tiles:
        lines.append("in tile units: " + _box_in_tiles(r0, r1, c0, c1))
    diffs = (got[rows, cols].double() - exp[rows, cols].double()) / granule
    fin = diffs[torch.isfinite(diffs)]
    if fin.numel() and bool((fin == fin.round()).all()):
        vals = sorted(set(int(v) for v in fin[:4096].tolist()))
        lines.append(f"every difference is a whole number of granules ({granule!r}): " + ", ".join(str(v) for v in vals[:8])
                     + (" ..." if len(vals) > 8 else ""))
    lines.append("first differences (row, col, got, expected, diff in granules):")
    for i in range(min(10, n)):
        r, c = int(rows[i]), int(cols[i])
        line = f"  ({r}, {c}, {float(got[r, c])!r}, {float(exp[r, c])!r}, {float(diffs[i]):+.6g})"
        if locate is not None:
            line += "  " + locate(r, c, got[r])
        lines.append(line)
    if locate is not None:
        urows = torch.unique(rows)
        lines.append(f"{urows.numel()} row(s) hold differences; the first ten:")
        for r in urows[:10].tolist():
            lines.append(f"  row {r}: " + locate(r, int(cols[rows == r].min()), got[r]))
        lines.append("box corners: " + locate(r0, c0) + "  ..  " + locate(r1, c1))
    return "\n".join(lines)


def assert_exact(got, exp, granule, label, tol=None, locate=None, gemm_tiles=True):
    """got, exp: 2-D tensors on one device.  tol None: bit for bit (a NaN differs); else a tensor / number of allowed
    |got - exp|.  Raises ExactMismatch with mismatch_report's text.  Returns the largest |got - exp|."""
    assert got.dim() == 2 and got.shape == exp.shape, (got.shape, exp.shape)
    d = (got.double() - exp.double()).abs()
    bad = ~(d <= (0.0 if tol is None else tol))                      # (NaN: not <=, so it is bad)
    if bool(bad.any()):
        raise ExactMismatch(mismatch_report(got, exp, bad, granule, label, locate, gemm_tiles))
    return float(d.max())
