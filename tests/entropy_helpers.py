"""The integer decisions of the entropy path restated in numpy, and fixed input domains that reach every edge of them -
shared by tests/test_entropy_ints_gpu.py (the device kernels), tests/test_entropy_inputs_cpu.py (these helpers
themselves), tests/test_rans.py and tests/test_reference_streams.py (the host coder on resolved records).

  gc_ref       gaussian_conditional_kernel / gaussian_conditional_compact_kernel: CDF row index, symbol, y_hat
  eb_ref       entropy_bottleneck_kernel: symbol, z_hat
  resolve_ref  resolve_symbols_kernel<WideRecords / CompactRecords> (csrc/rans_resolve.h): start | range << 16, escape
               payload, 1 + payload nibbles, the 16-bit record, the overflow word

Everything is compared for equality: integers as integers, y_hat / z_hat by their bit patterns.  Each reference takes
`mutant=`: one deliberately wrong variant per fault the domains are built to catch (MUTANTS); the CPU test shows that
every one of them differs from the true reference somewhere on the domain.  Nothing here touches a GPU."""
import numpy as np

F32 = np.float32
BOUND = 0.11          # the production lower bound of a scale (SCALES_MIN): the production table's first entry
INNER_BOUND = 0.5     # a bound with table entries under it, where dropping the bound changes rows
INT32_MAX = 2 ** 31 - 1
V_LIMIT = 2 ** 30 - 1     # |sym - offset| up to here cannot overflow rans_resolve.h's int32 arithmetic

MUTANTS = {
    "search_lt": "`<=` -> `<` in the table search",
    "round_half_away": "rint -> round half away from zero",
    "no_lower_bound": "the scale's lower bound dropped",
    "index_unclamped": "the index not clamped at n_table - 1",
    "compact_gt_4096": "`raw >= 4096` -> `raw > 4096` in the compact record",
    "nibbles_pow16": "a nibble count off by one at an exact power of 16",
    "escape_gt_max": "`value >= max_value` -> `value > max_value`",
    "range_unmasked": "the `& 0xFFFF` on the range dropped",
    "payload0_as_0": "the escape record of payload 0 stored as 0",
}


class IntMismatch(AssertionError):
    """A kernel's integers (or bit patterns) differ from the reference; the message names the first position, its class
    and its inputs."""


# ------------------------------------------------------------------------------------------------ references

def _rint(r, mutant):
    if mutant == "round_half_away":
        return (np.sign(r) * np.floor(np.abs(r) + F32(0.5))).astype(F32)
    return np.rint(r)


def scale_index_ref(scales, table, scale_bound=BOUND, mutant=None):
    """int64 CDF row of every scale: n_table - 1 - sum over t < n_table - 1 of (max(s, bound) <= table[t]).  float32
    values widened to float64 compare exactly."""
    s = np.asarray(scales, dtype=F32).reshape(-1)
    tb = np.asarray(table, dtype=F32).reshape(-1).astype(np.float64)
    if mutant != "no_lower_bound":
        s = np.maximum(s, F32(scale_bound))      # LowerBound: max(x, bound); -0.0, negatives and subnormals go to it
    s = s.astype(np.float64)
    idx = np.full(s.size, tb.size - 1, dtype=np.int64)
    if mutant == "index_unclamped":              # a plain count of the entries below the scale: n_table beyond the last
        return sum(((s > t) for t in tb), np.zeros(s.size, dtype=np.int64))
    for t in tb[:-1]:
        idx -= (s < t) if mutant == "search_lt" else (s <= t)
    return idx


def gc_ref(scales, means, table, scale_bound=BOUND, y=None, sym_in=None, mutant=None):
    """-> idx int64 (None without a table), sym int64, y_hat float32, all flat.  q = rint(y - mu) in float32 (half to
    even), or the given symbol as float32; y_hat = q + mu in float32."""
    mu = np.asarray(means, dtype=F32).reshape(-1)
    assert (y is None) != (sym_in is None)
    if y is not None:
        q = _rint(np.asarray(y, dtype=F32).reshape(-1) - mu, mutant)
    else:
        q = np.asarray(sym_in).reshape(-1).astype(F32)
    assert q.dtype == F32 and bool(np.isfinite(q).all()) and float(np.abs(q).max(initial=0)) < 2.0 ** 31
    idx = None if table is None else scale_index_ref(scales, table, scale_bound, mutant)
    return idx, q.astype(np.int64), (q + mu).astype(F32)


def eb_ref(medians, n_per_ch, z=None, sym_in=None, mutant=None):
    """-> sym int64, z_hat float32, flat [C * n_per_ch] (channel-major): the same arithmetic, median per channel"""
    med = np.repeat(np.asarray(medians, dtype=F32).reshape(-1), n_per_ch)
    _, sym, z_hat = gc_ref(None, med, None, y=z, sym_in=sym_in, mutant=mutant)
    return sym, z_hat


def row_valid(idx, cdf, lens):
    """rans_resolve.h row_ok(): in range, one bin and the escape bin at least, within the stride"""
    idx = np.asarray(idx).astype(np.int64)
    lens = np.asarray(lens).astype(np.int64)
    ok = (idx >= 0) & (idx < cdf.shape[0])
    ln = lens[np.where(ok, idx, 0)]
    return ok & (ln >= 2) & (ln <= cdf.shape[1])


def resolve_ref(sym, idx, cdf, lens, offs, mutant=None):
    """-> sr uint32, raw uint32, esc uint8, rec16 uint16, overflow (0 / 1).  All integer work in int64.
    value = sym - offset; value < 0 escapes with payload -2 value - 1, value >= max_value with 2 (value - max_value); an
    escape takes the row's last bin; esc = 1 + significant payload nibbles (0: regular symbol).  rec16 = esc << 12 | raw
    while raw < 4096, 0xFFFF beyond (overflow = 1).  An invalid row: sr = 0, raw = 0, esc = 255, rec16 = 0xFFFF
    (overflow = 1)."""
    sym = np.asarray(sym).reshape(-1).astype(np.int64)
    idx = np.asarray(idx).reshape(-1).astype(np.int64)
    cdf = np.asarray(cdf).astype(np.int64)
    lens, offs = np.asarray(lens).astype(np.int64), np.asarray(offs).astype(np.int64)
    ok = row_valid(idx, cdf, lens)
    ci = np.where(ok, idx, 0)
    max_v = np.where(ok, lens[ci] - 2, 0)
    v = np.where(ok, sym - offs[ci], 0)
    assert int(np.abs(v).max(initial=0)) <= V_LIMIT, "|sym - offset| beyond 2^30 - 1 is outside the resolve step's int32 range"
    neg = v < 0
    big = (v > max_v) if mutant == "escape_gt_max" else (v >= max_v)
    escape = neg | big
    raw = np.where(neg, -2 * v - 1, np.where(big, 2 * (v - max_v), 0))
    vc = np.where(escape, max_v, v)
    start = cdf[ci, vc] & 0xFFFF
    rng = cdf[ci, vc + 1] - cdf[ci, vc]
    if mutant != "range_unmasked":
        rng = rng & 0xFFFF
    sr = start | (rng << 16)
    nn = np.zeros(sym.size, dtype=np.int64)
    for k in range(8):      # significant nibbles: the smallest n <= 8 with raw >> 4 n == 0
        nn += (raw > 16 ** k) if mutant == "nibbles_pow16" else (raw >= 16 ** k)
    esc = np.where(escape, nn + 1, 0)
    wide = escape & ((raw > 4096) if mutant == "compact_gt_4096" else (raw >= 4096))
    stored = escape & (raw != 0) if mutant == "payload0_as_0" else escape
    rec = np.where(wide, 0xFFFF, np.where(stored, ((esc << 12) | raw) & 0xFFFF, 0))
    sr, raw, esc, rec = (np.where(ok, a, bad) for a, bad in ((sr, 0), (raw, 0), (esc, 255), (rec, 0xFFFF)))
    overflow = int(bool((wide | ~ok).any()))
    if mutant == "range_unmasked":      # (kept wide: packed into 32 bits the shift would drop the same bits again)
        return sr, raw.astype(np.uint32), esc.astype(np.uint8), rec.astype(np.uint16), overflow
    return sr.astype(np.uint32), raw.astype(np.uint32), esc.astype(np.uint8), rec.astype(np.uint16), overflow


# ------------------------------------------------------------------------------------------------ comparison

def class_names(mask, names):
    return [n for i, n in enumerate(names) if int(mask) & (1 << i)]


def compare_ints(got, want, cls, names, inputs, label):
    """array_equal on integers (or on the uint32 view of float32 arrays), no element left out.  Raises IntMismatch with
    the number of differences, the first position, its classes and its inputs.  Returns the number compared."""
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    if got.dtype == F32 or want.dtype == F32:
        assert got.dtype == want.dtype == F32, (label, got.dtype, want.dtype)
        g, w = got.view(np.uint32), want.view(np.uint32)
    else:
        assert got.dtype.kind in "iu" and want.dtype.kind in "iu", (label, got.dtype, want.dtype)
        g, w = got.astype(np.int64), want.astype(np.int64)
    assert g.size == w.size, (label, g.size, w.size)
    if np.array_equal(g, w):
        return g.size
    bad = np.nonzero(g != w)[0]
    i = int(bad[0])
    c = np.asarray(cls).reshape(-1)
    hist = {n: int(((c[bad] >> k) & 1).sum()) for k, n in enumerate(names)}
    ins = ", ".join(f"{k} = {_show(np.asarray(a).reshape(-1)[i])}" for k, a in inputs.items())
    err = IntMismatch(f"{label}: {bad.size} of {g.size} differ; first at {i}, class {class_names(c[i], names)}: "
                      f"got {_show(got[i])}, want {_show(want[i])}; inputs: {ins}; differences by class: "
                      + ", ".join(f"{n}: {k}" for n, k in hist.items() if k))
    err.n, err.first, err.first_classes, err.by_class = int(bad.size), i, class_names(c[i], names), hist
    raise err


def _show(v):
    if isinstance(v, np.floating):
        return f"{float(v)!r} ({np.asarray(v, dtype=F32).view(np.uint32):#010x})"
    return str(int(v))


def fill(n, *arrays, phase=0):
    """the arrays (one domain, equal lengths) repeated to n elements, starting `phase` elements in"""
    size = arrays[0].shape[0]
    at = (np.arange(n, dtype=np.int64) + phase) % size
    return tuple(a[at] for a in arrays)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------ residuals

RES_CLASSES = ("tie", "next-to-tie", "negative-zero", "integer", "large", "random")
R_TIE, R_NEAR, R_NEGZERO, R_INT, R_LARGE, R_RANDOM = (1 << i for i in range(6))
LARGE = (2.0 ** 23 - 0.5, 2.0 ** 23, 2.0 ** 24 + 2, 65504.0, 1e9)


def tie_means(seed=1):
    """means with few mantissa bits - multiples of 2^-10, |mu| < 64 - so that mu + k + 0.5 is a float32 for |k| <= 300"""
    rng = np.random.default_rng(seed)
    fixed = np.array([0.0, 2.0 ** -10, -2.0 ** -10, 0.5, -0.5, 0.25, 1.0, -1.0, 1.0 - 2.0 ** -10, 1.5, -2.5,
                      64 - 2.0 ** -10, -64 + 2.0 ** -10], dtype=np.float64)
    rnd = rng.integers(-65535, 65536, 11).astype(np.float64) / 1024.0
    return np.concatenate([fixed, rnd]).astype(F32)


def residual_domain():
    """(y, mu, class mask), fixed: for every mean of tie_means() the exact ties y = mu + k + 0.5 for every integer k in
    [-300, 300] and nextafter of each in both directions; residuals in (-0.5, 0) and the tie at -0.5 (q = -0.0); exact
    integers; |y - mu| at 2^23 - 0.5, 2^23, 2^24 + 2, 65504 and 1e9, both signs; 20 000 random pairs.  Every value is
    finite and |q| < 2^31.  The means are never -0.0: there, and only there, q = -0.0 makes the y path's y_hat (-0.0) and
    the sym_in path's (+0.0) differ by definition (signed_zero_cases())."""
    return _cached("res", _residual_domain)


def _residual_domain():
    mus = tie_means()
    k = np.arange(-300, 301, dtype=np.float64)
    ys, ms, cs = [], [], []

    def add(y, mu, c):
        y = np.asarray(y, dtype=F32).reshape(-1)
        ys.append(y)
        ms.append(np.broadcast_to(np.asarray(mu, dtype=F32), y.shape).copy())
        cs.append(np.full(y.size, c, dtype=np.uint8))

    for mu in mus:
        t64 = float(mu) + k + 0.5
        t = t64.astype(F32)
        assert np.array_equal(t.astype(np.float64), t64) and np.array_equal((t - mu).astype(np.float64), k + 0.5)
        add(t, mu, R_TIE)
        add(np.nextafter(t, F32(-np.inf)), mu, R_NEAR)
        add(np.nextafter(t, F32(np.inf)), mu, R_NEAR)
        r = -np.array([2.0 ** -10, 0.125, 0.25, 0.375, 0.5 - 2.0 ** -10, 0.5], dtype=np.float64)
        add((float(mu) + r), mu, R_NEGZERO)
        add(np.nextafter(mu, F32(-np.inf)), mu, R_NEGZERO)
        ki = np.array([0, 1, -1, 2, -2, 255, -256, 32767, -32768, 32768, -32769], dtype=np.float64)
        add(float(mu) + ki, mu, R_INT)
    for v in LARGE:
        for mu in (0.0, 0.5, -1.0, 63.5):
            for s in (1.0, -1.0):
                add([F32(mu) + F32(s * v)], mu, R_LARGE)
    rng = np.random.default_rng(20241018)
    mu_r = (rng.standard_normal(20000) * 8).astype(F32)
    add(mu_r + (rng.standard_normal(20000) * 40).astype(F32), 0.0, R_RANDOM)
    ms[-1] = mu_r
    y, mu, c = np.concatenate(ys), np.concatenate(ms), np.concatenate(cs)
    # what a class promises, by the reference itself
    q = np.rint(y - mu)
    assert bool(np.isfinite(y).all()) and float(np.abs(q).max()) < 2.0 ** 31
    assert not bool(np.signbit(mu[mu == 0]).any())
    tie = (c & R_TIE) != 0
    assert bool((np.abs((y - mu)[tie] % 1) == 0.5).all())
    nz = (c & R_NEGZERO) != 0
    assert bool(((q[nz] == 0) & np.signbit(q[nz])).all())
    big = (c & R_LARGE) != 0
    assert float(np.abs((y - mu)[big]).min()) >= 65503
    order = np.random.default_rng(7).permutation(y.size)      # classes spread over every part of a launch
    return _frozen(y[order], mu[order], c[order])


def signed_zero_cases():
    """(y, mu): q = -0.0 under a mean of -0.0 (and +0.0): the y path gives y_hat = -0.0 + -0.0 = -0.0, the sym_in path
    (float)0 + -0.0 = +0.0 - each its own reference's value, as in the reference model's forward() and decompress()"""
    y = np.array([-0.25, -0.5, -0.0, 0.0, -0.25, -0.5, -0.0, 0.0, 0.25], dtype=F32)
    mu = np.array([-0.0, -0.0, -0.0, -0.0, 0.0, 0.0, 0.0, 0.0, -0.0], dtype=F32)
    return y, mu


# ------------------------------------------------------------------------------------------------ scales

SCALE_CLASSES = ("entry", "below-entry", "above-entry", "bound", "next-to-bound", "under-bound", "FLT_MAX", "random")
S_ENTRY, S_BELOW, S_ABOVE, S_BOUND, S_NEARBOUND, S_UNDER, S_MAX, S_RANDOM = (1 << i for i in range(8))
FLT_MAX = np.finfo(F32).max


def production_table():
    from cra5_amd.entropy import get_scale_table
    t = get_scale_table().numpy().astype(F32)
    assert t.size == 64
    return t


def synthetic_table(n_table):
    """a strictly increasing float32 table of n_table entries from the bound to 256"""
    t = np.array([BOUND], dtype=F32) if n_table == 1 else np.geomspace(BOUND, 256.0, n_table).astype(F32)
    assert t.size == n_table and bool((np.diff(t.astype(np.float64)) > 0).all())
    return t


def scale_domain(table, scale_bound=BOUND, n_random=4096):
    """(scales, class mask) for one table: every entry and nextafter of it in both directions; the bound, nextafter of it
    in both directions; 0, -0.0, negative values and the smallest subnormal; FLT_MAX; random fill (log-uniform over and
    beyond the table, some below the bound)."""
    table = np.asarray(table, dtype=F32)
    return _cached(("scale", table.tobytes(), float(scale_bound), n_random), lambda: _scale_domain(table, scale_bound, n_random))


def _scale_domain(table, scale_bound, n_random):
    b = F32(scale_bound)
    under = np.array([0.0, -0.0, -1.0, -0.11, -FLT_MAX, np.finfo(F32).smallest_subnormal, 0.05,
                      np.nextafter(np.nextafter(b, F32(0)), F32(0))], dtype=F32)
    rng = np.random.default_rng(20241019)
    rnd = np.exp(rng.uniform(np.log(0.02), np.log(2000.0), n_random)).astype(F32)
    parts = [(table, S_ENTRY), (np.nextafter(table, F32(-np.inf)), S_BELOW), (np.nextafter(table, F32(np.inf)), S_ABOVE),
             (np.array([b]), S_BOUND), (np.array([np.nextafter(b, F32(0)), np.nextafter(b, F32(1))]), S_NEARBOUND),
             (under, S_UNDER), (np.array([FLT_MAX]), S_MAX), (rnd, S_RANDOM)]
    s = np.concatenate([p for p, _ in parts]).astype(F32)
    c = np.concatenate([np.full(p.size, bit, dtype=np.uint8) for p, bit in parts])
    c[s < b] |= S_UNDER
    assert bool(np.isfinite(s).all())
    order = np.random.default_rng(11).permutation(s.size)
    return _frozen(s[order], c[order])


# ------------------------------------------------------------------------------------------------ resolve inputs

RESOLVE_CLASSES = ("regular", "escape", "payload-0", "payload-edge", "wide-payload", "limit", "invalid", "full-range-row")
V_REGULAR, V_ESCAPE, V_PAYLOAD0, V_EDGE, V_WIDE, V_LIMIT_CLS, V_INVALID, V_FULLROW = (1 << i for i in range(8))
# payloads at each nibble edge and at the compact record's 4095 / 4096 edge: odd ones come from below the row
# (raw = -2 value - 1), even ones from above (raw = 2 (value - max_value)).  2^31 - 3 is the largest payload inside
# |sym - offset| <= 2^30 - 1 (2^31 - 1 needs value = -2^30, where -2 * value leaves int32).
PAYLOADS = (0, 1, 15, 16, 255, 256, 4094, 4095, 4096, 4097, 65535, 65536, 2 ** 20 - 1, 2 ** 20 + 1, 2 ** 24 - 1, 2 ** 24 + 1,
            2 ** 28 - 1, 2 ** 28 + 1, 2 ** 31 - 3, 2 ** 31 - 2)


def production_tables():
    """the production GaussianConditional tables (cdf [64, stride], lengths, offsets), int32 numpy"""
    def make():
        from cra5_amd.entropy import GaussianConditional, get_scale_table
        gc = GaussianConditional(None)
        assert gc.update_scale_table(get_scale_table(), force=True)
        return _frozen(*[a.copy() for a in gc.host_tables()])
    return _cached("gc_tables", make)


def ragged_tables():
    """Seeded ragged tables, stride 42: row 0 of length 3 (one bin and the escape bin), row 1 of length == stride, rows
    2-7 of random lengths; offsets positive, zero and negative; then three rows no stream can use: row 8 with length 1,
    row 9 with length stride + 1 (both invalid) and row 10 of length 2, whose only bin - the escape bin - spans the whole
    range (frequency 65536 = 0 in 16 bits: valid to resolve, refused by every encoder)."""
    return _cached("ragged", _ragged_tables)


def _ragged_tables():
    from oracle import cbind
    rng = np.random.default_rng(31)
    stride = 42
    n_bins = [2, stride - 1] + [int(v) for v in rng.integers(3, stride - 1, 6)]
    offsets = [5, 0, -3, 100000, -100000, 0, 17, -int(n_bins[7]) + 1]
    cdf = np.zeros((11, stride), dtype=np.int32)
    lens = np.zeros(11, dtype=np.int32)
    offs = np.zeros(11, dtype=np.int32)
    for r, n in enumerate(n_bins):
        p = rng.random(n).astype(F32) ** int(rng.integers(1, 6))
        q = np.asarray(cbind.pmf_to_cdf(p / p.sum()), dtype=np.int64)
        assert q.size == n + 1 and q[0] == 0 and q[-1] == 65536 and bool((np.diff(q) > 0).all())
        cdf[r, : n + 1], lens[r], offs[r] = q, n + 1, offsets[r]
    cdf[8, :2], lens[8], offs[8] = (0, 65536), 1, 0
    cdf[9], lens[9], offs[9] = np.linspace(0, 65536, stride).astype(np.int32), stride + 1, -4
    cdf[10, :2], lens[10], offs[10] = (0, 65536), 2, 3
    assert lens[0] == 3 and lens[1] == stride
    return _frozen(cdf, lens, offs)


def resolve_domain(which):
    """(sym, idx, class mask, (cdf, lens, offs)) for which = "production" | "ragged": on every valid row every symbol
    from offset - 40 to offset + length + 40, and both escape directions with every payload of PAYLOADS; the invalid
    indexes -1, n_cdfs and INT32_MAX (and, ragged, the rows of length 1 and stride + 1); the ragged full-range row."""
    return _cached(("resolve", which), lambda: _resolve_domain(which))


def _resolve_domain(which):
    cdf, lens, offs = production_tables() if which == "production" else ragged_tables()
    n_cdfs, stride = cdf.shape
    syms, idxs = [], []
    for r in range(n_cdfs):
        ln, off = int(lens[r]), int(offs[r])
        if ln < 2 or ln > stride:
            s = np.arange(off - 3, off + 4)
        else:
            mx = ln - 2
            v = [-(p + 1) // 2 if p % 2 else mx + p // 2 for p in PAYLOADS] + [-V_LIMIT, V_LIMIT]
            v = [x for x in v if abs(x) <= V_LIMIT]
            s = np.concatenate([np.arange(off - 40, off + ln + 41), off + np.array(v, dtype=np.int64)])
        syms.append(s.astype(np.int64))
        idxs.append(np.full(s.size, r, dtype=np.int64))
    for bad in (-1, n_cdfs, INT32_MAX):
        syms.append(np.array([0, 1, -7], dtype=np.int64))
        idxs.append(np.full(3, bad, dtype=np.int64))
    sym, idx = np.concatenate(syms), np.concatenate(idxs)
    assert int(np.abs(sym).max()) <= INT32_MAX
    ok = row_valid(idx, cdf, lens)
    ci = np.where(ok, idx, 0)
    mx = lens.astype(np.int64)[ci] - 2
    v = np.where(ok, sym - offs.astype(np.int64)[ci], 0)
    raw = np.where(v < 0, -2 * v - 1, np.where(v >= mx, 2 * (v - mx), 0))
    esc = ok & ((v < 0) | (v >= mx))
    c = np.zeros(sym.size, dtype=np.uint8)
    c[ok & ~esc] |= V_REGULAR
    c[esc] |= V_ESCAPE
    c[esc & (raw == 0)] |= V_PAYLOAD0
    c[esc & np.isin(raw, PAYLOADS)] |= V_EDGE
    c[esc & (raw >= 4096)] |= V_WIDE
    c[ok & (np.abs(v) == V_LIMIT)] |= V_LIMIT_CLS
    c[~ok] |= V_INVALID
    c[ok & (lens.astype(np.int64)[ci] == 2)] |= V_FULLROW
    order = np.random.default_rng(13).permutation(sym.size)
    sym, idx, c = sym[order].astype(np.int32), idx[order].astype(np.int32), c[order]
    return _frozen(sym, idx, c) + ((cdf, lens, offs),)


def codable(cls):
    """the part of a resolve domain the host coder can write: valid rows whose bins have a 16-bit frequency"""
    return (np.asarray(cls) & (V_INVALID | V_FULLROW)) == 0


# ------------------------------------------------------------------------------------------------ bottleneck inputs

EB_SHAPES = ((1, 1), (3, 257), (16, 648), (5, 1048576 // 4 + 3))


def eb_domain(C, n_per_ch):
    """(z [C, n_per_ch], medians [C], class mask [C, n_per_ch]; classes of RES_CLASSES).  A distinct median per channel:
    even channels multiples of 2^-10 (exact ties exist), odd channels full-mantissa values.  On the even channels ties
    for k cycling through [-300, 300], nextafter of them, residuals in (-0.5, 0) and integers; on the odd ones the
    float32 nearest to median + k + 0.5 and its neighbours (as near a tie as the median allows) and median + k; random
    fill on all."""
    return _cached(("eb", C, n_per_ch), lambda: _eb_domain(C, n_per_ch))


def _eb_domain(C, n_per_ch):
    rng = np.random.default_rng(1000 + C)
    med = np.empty(C, dtype=F32)
    med[0::2] = (rng.permutation(8192)[: (C + 1) // 2].astype(np.float64) - 4096) / 1024.0
    med[1::2] = (rng.standard_normal(C // 2) * 3).astype(F32) + F32(1.0 / 3.0)
    assert np.unique(med).size == C and not bool(np.signbit(med[med == 0]).any())
    z = np.empty((C, n_per_ch), dtype=F32)
    cls = np.empty((C, n_per_ch), dtype=np.uint8)
    j = np.arange(n_per_ch)
    for c in range(C):
        m = float(med[c])
        k = ((j // 8 * 37 + c * 11) % 601 - 300).astype(np.float64)
        t = (m + k + 0.5).astype(F32)
        kind = j % 8 if n_per_ch > 1 else np.zeros(1, dtype=np.int64)
        row = (rng.standard_normal(n_per_ch) * 30).astype(F32) + med[c]
        cl = np.full(n_per_ch, R_RANDOM, dtype=np.uint8)
        exact = c % 2 == 0
        for kk, vals, bit in ((0, t, R_TIE if exact else R_NEAR), (1, np.nextafter(t, F32(-np.inf)), R_NEAR),
                              (2, np.nextafter(t, F32(np.inf)), R_NEAR),
                              (3, (m - (0.03125 + (j % 13) / 32.0)).astype(F32), R_NEGZERO),
                              (4, (m + k).astype(F32), R_INT)):
            sel = kind == kk
            row[sel], cl[sel] = vals[sel], bit
        z[c], cls[c] = row, cl
    sym, _ = eb_ref(med, n_per_ch, z=z)
    q = np.rint(z - med[:, None])
    tie = (cls & R_TIE) != 0
    assert bool((np.abs((z - med[:, None])[tie] % 1) == 0.5).all())
    nz = (cls & R_NEGZERO) != 0
    assert bool(((q[nz] == 0) & np.signbit(q[nz])).all()) and int(np.abs(sym).max()) < 2 ** 31
    return _frozen(z, med, cls)
