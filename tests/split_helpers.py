"""The split-f16 store (csrc/split.h) restated in numpy, a fixed domain of fp32 values that reaches every rounding case
of it, and a bit-level comparison of a producer's RAW storage with that restatement - shared by
tests/test_split_store_gpu.py (every producer kernel) and tests/test_split_inputs_cpu.py (these helpers themselves).

The store: hi = f16(x), lo = f16(x - f32(hi)), both IEEE round-to-nearest-even with gradual underflow; a row is a
sequence of 128-byte chunks of 32 hi halves followed by 32 lo halves; a PLAIN row holds the hi halves alone, element n
at half n.  Nothing here touches a GPU."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

# Value classes.  A value may belong to several (a tie whose lo half is subnormal is both); `normal` is "none of the
# others".  Reports count every class a failing value belongs to.
CLASSES = ("normal", "tie", "hi-subnormal", "lo-subnormal", "zero", "65504..65520", "overflow", "non-finite")
NORMAL, TIE, HI_SUB, LO_SUB, ZERO, EDGE, OVERFLOW, NONFINITE = (1 << i for i in range(8))
FINITE_IN_RANGE = NORMAL | TIE | HI_SUB | LO_SUB | ZERO | EDGE        # what every producer can carry
ALL_CLASSES = FINITE_IN_RANGE | OVERFLOW | NONFINITE

F16_MIN_NORMAL = 2.0 ** -14


class SplitMismatch(AssertionError):
    """A producer's stored halves differ from split_ref; the message says how many, where and of which class."""


def split_ref(x):
    """(hi, lo) float16 arrays of the fp32 array x.  |x| >= 65520: hi = +-inf, lo = -+inf; NaN stays NaN.  The fp32
    subtraction is exact for every finite hi (tests/test_split_inputs_cpu.py checks it against float64 on the whole
    domain), so the two-conversion form and the fused multiply-add form of the kernels have this one expectation."""
    x = np.asarray(x, dtype=np.float32)
    if x.size >= 1 << 20:          # numpy's conversion runs on one core and releases the lock: eight slices at a time
        flat = np.ascontiguousarray(x).reshape(-1)
        with ThreadPoolExecutor(8) as pool:
            parts = list(pool.map(_split_ref_1, np.array_split(flat, 8)))
        return (np.concatenate([p[0] for p in parts]).reshape(x.shape), np.concatenate([p[1] for p in parts]).reshape(x.shape))
    return _split_ref_1(x)


def _split_ref_1(x):
    with np.errstate(over="ignore", invalid="ignore"):
        hi = x.astype(np.float16)
        lo = (x - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def classify(x):
    """uint8 class mask (bits in the order of CLASSES) of every element of the fp32 array x"""
    x = np.asarray(x, dtype=np.float32)
    hi, lo = split_ref(x)
    with np.errstate(over="ignore", invalid="ignore"):
        x64 = x.astype(np.float64)
        fin = np.isfinite(x)
        ax = np.abs(x64)
        inr = fin & (ax < 65520.0)
        d = np.where(inr, x64 - hi.astype(np.float64), 0.0)
        # the f16 neighbour of hi on x's side; x is a tie when it lies exactly half way
        other = np.nextafter(hi, np.where(d > 0, np.float16(np.inf), np.float16(-np.inf)).astype(np.float16))
        tie = inr & (d != 0) & (2.0 * x64 == hi.astype(np.float64) + other.astype(np.float64))
        m = np.zeros(x.shape, dtype=np.uint8)
        m[~fin] |= NONFINITE
        m[fin & (ax >= 65520.0)] |= OVERFLOW
        m[fin & (ax >= 65504.0) & (ax < 65520.0)] |= EDGE
        m[fin & (x == 0)] |= ZERO
        m[inr & (x != 0) & (np.abs(hi.astype(np.float64)) < F16_MIN_NORMAL)] |= HI_SUB
        m[inr & (d != 0) & (np.abs(lo.astype(np.float64)) < F16_MIN_NORMAL)] |= LO_SUB
        m[tie] |= TIE
        m[m == 0] = NORMAL
    return m


_DOMAIN = {}


def split_domain():
    """(values fp32 [n], class masks uint8 [n]), n ~ 4.5e5, fixed: every non-negative finite f16 as fp32; the fp32
    midpoint of each adjacent f16 pair (the exact ties) and its two fp32 neighbours; 65504, the largest fp32 below 65520,
    65520, 65536, 1e5; 2^-24, 2^-25, the next fp32 above 2^-25, 2^-26, an fp32 subnormal, 0; the negatives of all of
    these; +-inf and one NaN; 2e5 fp32 values of seeded random bit patterns.  Read-only arrays."""
    if "v" not in _DOMAIN:
        h = np.arange(0x7c00, dtype=np.uint16).view(np.float16).astype(np.float32)
        mid = ((h[:-1].astype(np.float64) + h[1:].astype(np.float64)) * 0.5).astype(np.float32)
        assert np.array_equal(mid.astype(np.float64) * 2, h[:-1].astype(np.float64) + h[1:].astype(np.float64))
        below, above = np.nextafter(mid, np.float32(-np.inf)), np.nextafter(mid, np.float32(np.inf))
        edge = np.array([65504.0, np.nextafter(np.float32(65520.0), np.float32(0)), 65520.0, 65536.0, 1e5], dtype=np.float32)
        tiny = np.array([2.0 ** -24, 2.0 ** -25, np.nextafter(np.float32(2.0 ** -25), np.float32(1)), 2.0 ** -26,
                         2.0 ** -140, 0.0], dtype=np.float32)
        pos = np.concatenate([h, mid, below, above, edge, tiny])
        special = np.array([np.inf, -np.inf, np.nan], dtype=np.float32)
        rnd = np.random.default_rng(20240607).integers(0, 2 ** 32, 200000, dtype=np.uint64).astype(np.uint32).view(np.float32)
        v = np.concatenate([pos, -pos, special, rnd]).astype(np.float32)
        c = classify(v)
        hi, lo = split_ref(v)
        fin = np.isfinite(v) & (np.abs(v) < 65520)
        n_hs = int((fin & (hi != 0) & (np.abs(hi.astype(np.float64)) < F16_MIN_NORMAL)).sum())
        n_ls = int((fin & (lo != 0) & (np.abs(lo.astype(np.float64)) < F16_MIN_NORMAL)).sum())
        assert n_hs > 0 and n_ls > 0, "the domain must hold subnormal hi and subnormal lo halves"
        for i, name in enumerate(CLASSES):
            assert bool((c & (1 << i)).any()), f"the domain holds no value of class {name}"
        v.setflags(write=False)
        c.setflags(write=False)
        _DOMAIN.update(v=v, c=c, subnormal_hi=n_hs, subnormal_lo=n_ls)
    return _DOMAIN["v"], _DOMAIN["c"]


def domain_counts():
    """(stored subnormal hi halves, stored subnormal lo halves) the reference gives on the finite part of the domain"""
    split_domain()
    return _DOMAIN["subnormal_hi"], _DOMAIN["subnormal_lo"]


def class_values(bit):
    """the domain's values of one class (a bit of the mask)"""
    v, c = split_domain()
    return v[(c & bit) != 0]


def class_names(mask):
    return [n for i, n in enumerate(CLASSES) if mask & (1 << i)]


def domain_matrix(rows, K, classes=ALL_CLASSES, seed=0):
    """fp32 [rows, K] filled from split_domain() restricted to `classes` (a seeded shuffle of it, repeated or cut to size),
    then arranged so that EVERY class of `classes` lands in every column residue mod 4 and in both the first and the last
    32-column chunk: class number c gets one representative at a column = r (mod 4) for each r, in the last chunk for
    r = c mod 4 (or any free column of it) and in the first chunk for the others.  The arrangement is asserted, not
    assumed; only a matrix whose last chunk has fewer places than there are classes goes without the last-chunk part."""
    v, c = split_domain()
    keep = (c & ~np.uint8(classes)) == 0
    pool, pool_c = v[keep], c[keep]
    rng = np.random.default_rng(seed)
    order = rng.permutation(pool.size)
    m = np.resize(pool[order], rows * K).reshape(rows, K).copy()
    last0 = (K - 1) // 32 * 32
    assert K >= 8, "a row needs two columns of every residue"
    used, placed = set(), []
    nrow, wlast = min(rows, 64), min(32, K - last0)
    ncls = sum(1 for ci in range(len(CLASSES)) if classes & (1 << ci))
    both_ends = last0 > 0 and nrow * wlast >= ncls           # (a one-row matrix with a 2-column last chunk cannot hold 8 classes)

    def take(ci, cols):
        spots = sorted(((row, col) for col in cols for row in range(nrow)), key=lambda s: ((s[0] - ci * 4) % nrow, s[1]))
        return next((s for s in spots if s not in used), None)

    for ci in range(len(CLASSES)):
        bit = 1 << ci
        if not classes & bit:
            continue
        reps = pool[(pool_c & bit) != 0]
        assert reps.size, f"no value of class {CLASSES[ci]} to place"
        todo = []
        if last0:
            spot = take(ci, range(last0 + ci % 4, K, 4)) or take(ci, range(last0, K))
            assert spot is not None or not both_ends
            if spot is not None:
                todo.append(spot)
        for r in range(4):
            if not any(sp[1] % 4 == r for sp in todo):
                spot = take(ci, range(r, min(32, K), 4))
                assert spot is not None, f"no free column for class {CLASSES[ci]}, residue {r} in a {rows} x {K} matrix"
                todo.append(spot)
            used.update(todo)
        for n, spot in enumerate(todo):
            m[spot] = reps[(n * 7919 + ci) % reps.size]
            placed.append((ci, spot))
    got = classify(np.array([m[s] for _, s in placed], dtype=np.float32))
    seen = {}
    for (ci, (row, col)), g in zip(placed, got):
        assert g & (1 << ci) and col < K
        seen.setdefault(ci, set()).update({("r", col % 4), ("c", col // 32)})
    for ci, sset in seen.items():
        assert all(("r", r) in sset for r in range(4)), f"class {CLASSES[ci]} misses a column residue"
        assert ("c", 0) in sset and (not both_ends or ("c", last0 // 32) in sset), f"class {CLASSES[ci]} misses the first or the last chunk"
    return m


def _as_bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


def expected_storage(x_expected, K, Kp, plain, lo_written=True, fill=0, width=None):
    """uint16 [rows, width] (width = 2 * Kp by default): what a producer must leave in a row buffer the caller filled
    with `fill`.  Split rows: columns K..Kp zero in both planes (with lo_written=False - the reduced-precision GEMM - the lo
    plane stays as filled).  Plain rows: hi halves at 0..K, zeros at K..Kp, `fill` beyond."""
    x = np.ascontiguousarray(x_expected, dtype=np.float32)
    rows = x.shape[0]
    assert x.shape == (rows, K) and Kp % 32 == 0 and Kp >= K
    width = 2 * Kp if width is None else width
    key = (hash(x.tobytes()), x.shape, Kp, bool(plain), bool(lo_written), int(fill), width)
    if _LAST.get("key") == key:    # (a producer's launches with and without an fp32 output share one expectation)
        return _LAST["want"]
    want = _expected_storage(x, rows, K, Kp, plain, lo_written, fill, width)
    want.setflags(write=False)
    _LAST.update(key=key, want=want)
    return want


_LAST = {}


def _expected_storage(x, rows, K, Kp, plain, lo_written, fill, width):
    hi, lo = split_ref(x)
    want = np.full((rows, width), fill, dtype=np.uint16)
    if plain:
        want[:, :K] = _as_bits(hi)
        want[:, K:Kp] = 0
        return want
    assert width == 2 * Kp
    w4 = want.reshape(rows, Kp // 32, 2, 32)
    hp = np.zeros((rows, Kp), dtype=np.uint16)
    hp[:, :K] = _as_bits(hi)
    w4[:, :, 0, :] = hp.reshape(rows, Kp // 32, 32)
    if lo_written:
        lp = np.zeros((rows, Kp), dtype=np.uint16)
        lp[:, :K] = _as_bits(lo)
        w4[:, :, 1, :] = lp.reshape(rows, Kp // 32, 32)
    return want


def _is_nan16(u):
    return (u & 0x7fff) > 0x7c00


def _f16(u):
    return float(np.array([u], dtype=np.uint16).view(np.float16)[0])


def compare_planes(data_u16, x_expected, K, Kp, plain=False, lo_written=True, fill=0, label="split store"):
    """data_u16: the producer's RAW storage, [rows, 2 * Kp] 16-bit words (any 16-bit dtype; a plain matrix of pitch Kp is
    taken too), not SplitMat.planes() - so that the padding is compared as well.  Equality is on bit patterns; every NaN
    equals every NaN.  Raises SplitMismatch: the number of differing halves, the first ten as (row, col, plane, x as hex,
    got, want), and histograms of the failures over value class and over position (col % 4, col % 32, last chunk or
    not).  Returns the number of halves compared."""
    got = np.ascontiguousarray(np.asarray(data_u16)).view(np.uint16)
    x = np.asarray(x_expected, dtype=np.float32)
    rows = x.shape[0]
    assert got.ndim == 2 and got.shape[0] == rows and got.shape[1] in ((Kp, 2 * Kp) if plain else (2 * Kp,)), \
        (got.shape, rows, Kp, plain)
    want = expected_storage(x, K, Kp, plain, lo_written, fill, width=got.shape[1])
    r, off = np.nonzero(got != want)
    if r.size:
        real = ~(_is_nan16(got[r, off]) & _is_nan16(want[r, off]))
        r, off = r[real], off[real]
    if not r.size:
        return got.size
    if plain:
        col = off.copy()
        plane = np.where(off < Kp, 0, 2)
    else:
        col = (off // 64) * 32 + off % 32
        plane = (off % 64) // 32
    pname = ("hi", "lo", "beyond the plain row")
    inside = (col < K) & (plane < 2)
    cls = np.zeros(r.size, dtype=np.uint8)
    cls[inside] = classify(x[r[inside], col[inside]])
    lines = [f"{label}: {r.size} of {got.size} stored halves differ from split_ref "
             f"({int((plane == 0).sum())} hi, {int((plane == 1).sum())} lo, {int((plane == 2).sum())} beyond a plain row; "
             f"rows x K = {rows} x {K}, Kp = {Kp}, {'plain' if plain else 'split'} rows)"]
    lines.append("first differences (row, col, plane, x as hex, got, want):")
    for i in range(min(10, r.size)):
        xv = x[r[i], col[i]] if inside[i] else None
        xs = f"{xv.view(np.uint32):#010x} = {float(xv)!r}" if xv is not None else "padding"
        g, w = int(got[r[i], off[i]]), int(want[r[i], off[i]])
        lines.append(f"  ({int(r[i])}, {int(col[i])}, {pname[plane[i]]}, {xs}, {g:#06x} = {_f16(g)!r}, {w:#06x} = {_f16(w)!r})")
    hist = {n: int(((cls & (1 << i)) != 0).sum()) for i, n in enumerate(CLASSES)}
    hist["padding"] = int((~inside).sum())
    lines.append("failures by value class (a value counts in every class it belongs to): "
                 + ", ".join(f"{n}: {k}" for n, k in hist.items() if k))
    last = (col // 32 == Kp // 32 - 1) & (plane < 2)
    lines.append("failures by position: col % 4: " + ", ".join(f"{q}: {int((col % 4 == q).sum())}" for q in range(4))
                 + f"; last chunk: {int(last.sum())}, other chunks: {int((~last).sum())}")
    c32 = np.bincount(col % 32, minlength=32)
    lines.append("col % 32: " + " ".join(str(int(k)) for k in c32))
    err = SplitMismatch("\n".join(lines))
    err.n, err.by_class, err.col4 = int(r.size), hist, [int((col % 4 == q).sum()) for q in range(4)]
    err.col32, err.last_chunk, err.planes = [int(k) for k in c32], int(last.sum()), [int((plane == q).sum()) for q in range(3)]
    raise err


def storage_from_ref(x, Kp=None, plain=False):
    """the raw uint16 [rows, 2 * Kp] storage of fp32 [rows, K] as split_ref defines it (tests of the reporter and of ops.py)"""
    x = np.asarray(x, dtype=np.float32)
    K = x.shape[1]
    Kp = (K + 31) // 32 * 32 if Kp is None else Kp
    return expected_storage(x, K, Kp, plain)
