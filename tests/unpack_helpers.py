"""The packed int16 INPUT definition ("Packed int16 input") in plain numpy, its wrong variants
("mutants") and the named inputs that tell them apart - shared by tests/test_unpack_cpu.py and tests/test_unpack_gpu.py.

    q == FILL[c] (FILL[c] not NaN)  ->  x = quiet NaN;  otherwise  d = fl64(fl64(double(q) * SCALE[c]) + OFFSET[c]),
    x = fl32(d) * fl32(MUL[c]).

A table is float64 [C, 4]: SCALE, OFFSET, FILL, MUL.  Codes are given by VALUE (native int16); the byte order the kernel
sees is the test's business."""
from fractions import Fraction

import numpy as np

FILL = -32768
QNAN = np.uint32(0x7fc00000)
MUTANTS = ("fma", "f32_arith", "no_swap", "fill_ignored", "unsigned", "mul_in_double")
SHAPES = [(3, 7, 13), (1, 1, 1), (5, 25, 40), (2, 35, 1440)]
FULL_SHAPE = (2, 64, 1024)        # plane = 65536: `random` holds every code value in every channel
TIE_CHANNELS = 16
INPUT_NAMES = ("random", "tp_like", "no_fill", "fma_ties")
# the mutants each input is there for
SEPARATES = dict(random=("f32_arith", "unsigned", "no_swap", "fill_ignored"), tp_like=("mul_in_double",), no_fill=(),
                 fma_ties=("fma",))


def _fma64(q, scale, offset):
    """fl64(q * scale + offset) with ONE rounding, exactly (Fraction -> float rounds to nearest even), per distinct code."""
    codes, inv = np.unique(q, return_inverse=True)
    lut = np.array([float(Fraction(int(v)) * Fraction(scale) + Fraction(offset)) for v in codes], dtype=np.float64)
    return lut[inv].reshape(q.shape)


def ref_unpack(q, table, mutant=None):
    """q int16 [C, H, W] (values), table float64 [C, 4] -> float32 [C, H, W]: the definition, or a mutant of it."""
    assert mutant is None or mutant in MUTANTS
    q = np.ascontiguousarray(q, dtype=np.int16)
    out = np.empty(q.shape, dtype=np.float32)
    for c in range(q.shape[0]):
        scale, offset, fill, mul = (np.float64(v) for v in table[c])
        qc = q[c]
        if mutant == "no_swap":
            qc = qc.byteswap()                                # the value a kernel sees that ignores the swap flag
        v = qc.astype(np.int64)
        if mutant == "unsigned":
            v = v & 0xffff
        with np.errstate(all="ignore"):
            if mutant == "fma":
                d = _fma64(v, scale, offset)
                x = d.astype(np.float32)
            elif mutant == "f32_arith":
                x = v.astype(np.float32) * np.float32(scale) + np.float32(offset)
            else:
                d = v.astype(np.float64) * scale
                d = d + offset
                x = d.astype(np.float32)
            if mutant == "mul_in_double":
                x = (d * mul).astype(np.float32)
            else:
                x = x * np.float32(mul)
        if mutant != "fill_ignored" and not np.isnan(fill):
            x = np.where(v == int(fill), QNAN.view(np.float32), x)
        out[c] = x
    return out


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _cds_table(C, rng, fill=FILL):
    """scale / offset as the CDS packs ERA5: a full-mantissa scale = range / 65534, the offset the range's middle."""
    lo = rng.uniform(-6e4, 200.0, size=C)
    span = 10.0 ** rng.uniform(-2, 5, size=C)
    t = np.empty((C, 4), dtype=np.float64)
    t[:, 0] = span / 65534.0
    t[:, 1] = lo + span * 0.5
    t[:, 2] = fill
    t[:, 3] = 1.0
    return t


def _codes(shape, rng, must=()):
    """Random codes; the values `must` lie at the head, the tail and the middle of every plane as far as it has room."""
    C, H, W = shape
    n = H * W
    if n >= 65536:
        q = np.stack([rng.permutation(np.arange(-32768, 32768).repeat(-(-n // 65536))[:n]) for _ in range(C)])
    else:
        q = rng.integers(-32768, 32768, size=(C, n))
    if n < 65536 and must:
        spots = [0, n - 1, n // 2, 1, n - 2, n // 2 + 1, 2, n - 3][:len(must)]
        k = len(spots) if n >= 16 else 1                 # (a plane too small for distinct spots: its first code)
        q[:, spots[:k]] = np.asarray(must[:k])
    return q.astype(np.int16).reshape(shape)


def tp_share(table_row):
    """Over all 65536 codes: the share where fl32(d) * 1000f and fl32(d * 1000.0) differ, and the codes where they do."""
    q = np.arange(-32767, 32768, dtype=np.int16).reshape(1, 1, -1)
    t = np.asarray(table_row, dtype=np.float64).reshape(1, 4)
    differ = bits(ref_unpack(q, t)) != bits(ref_unpack(q, t, "mul_in_double"))
    return float(differ.mean()), q.reshape(-1)[differ.reshape(-1)]


def tie_channel(rng):
    """One constructed channel -> (q*, SCALE, OFFSET, fl32 of the definition, fl32 of the fused mutant), or None when
    the two agree.  p = fl64(q* SCALE) ~ 1000 is inexact, m is an fp32 rounding midpoint in (1, 2), OFFSET = m - p
    exactly: the two-step rule lands ON the tie and rounds to even, a fused multiply-add lands beside it."""
    qs = int(rng.choice([3, 5, 7, 9, 11, 13, -3, -5, -7, 32767, 32765, -32767, -32765, 32763]))
    scale = float(rng.uniform(600.0, 1000.0) / qs)
    exact = Fraction(qs) * Fraction(scale)
    p = float(exact)                                                 # fl64(q* SCALE): Fraction -> float rounds to nearest even
    if Fraction(p) == exact or not 512.0 <= p < 1024.0:
        return None
    m = Fraction(1) + Fraction(2 * int(rng.integers(0, 1 << 23)) + 1, 1 << 24)      # between two neighbouring fp32
    offset = float(m - Fraction(p))
    assert Fraction(offset) == m - Fraction(p), "OFFSET = m - p must be exact in float64"
    two_step = float(Fraction(p) + Fraction(offset))
    assert Fraction(two_step) == m                                   # exactly the tie
    fused = float(exact + Fraction(offset))
    a, b = np.float32(two_step), np.float32(fused)
    if a == b:
        return None
    return qs, scale, offset, a, b


def unpack_inputs(shape, seed=0):
    """name -> (q int16 [C, H, W] by value, table float64 [C, 4]).  `fma_ties` has TIE_CHANNELS channels on the plane of
    `shape`; the others have shape's own channel count."""
    C, H, W = shape
    n = H * W
    rng = np.random.default_rng(seed + 1000 * C + n)
    inputs = {}
    # every code value where the plane holds them all (FULL_SHAPE), else a sample with the edge codes in place
    inputs["random"] = (_codes(shape, rng, must=(FILL, -1, 32767, 0x0102, -32767, 255, 256)), _cds_table(C, rng))
    # tp: metres in the file, the model works in mm - MUL = 1000 on the last channel
    t = _cds_table(C, rng)
    t[C - 1, :2] = (0.05 / 65534.0 * 1.0000001, 0.025)
    t[C - 1, 3] = 1000.0
    share, differing = tp_share(t[C - 1])
    assert share > 0.05, share
    inputs["tp_like"] = (_codes(shape, rng, must=tuple(int(v) for v in differing[[0, -1, len(differing) // 2]])), t)
    inputs["no_fill"] = (_codes(shape, rng, must=(FILL, FILL, FILL)), _cds_table(C, rng, fill=np.nan))
    # constructed ties: q* at the head, the tail and the middle of the plane, a few filler codes elsewhere
    tq = np.empty((TIE_CHANNELS, n), dtype=np.int16)
    tt = np.empty((TIE_CHANNELS, 4), dtype=np.float64)
    trng = np.random.default_rng(77)
    c = 0
    while c < TIE_CHANNELS:
        made = tie_channel(trng)
        if made is None:
            continue
        qs, scale, offset, _, _ = made
        tq[c] = trng.choice(np.array([-2, 0, 2, 4, 100, -100], dtype=np.int16), size=n)
        tq[c, [0, n - 1, n // 2]] = qs
        tt[c] = (scale, offset, FILL, 1.0)
        c += 1
    inputs["fma_ties"] = (tq.reshape(TIE_CHANNELS, H, W), tt)
    return inputs


def self_check(shape):
    """Every input separates the definition from the mutants it is there for (planes of one element excepted: they hold
    one code).  Returns {input: [mutants it separates]}."""
    inputs = unpack_inputs(shape)
    n = shape[1] * shape[2]
    seen = {}
    for name, (q, table) in inputs.items():
        ref = bits(ref_unpack(q, table))
        seen[name] = [m for m in MUTANTS if not np.array_equal(bits(ref_unpack(q, table, m)), ref)]
        if n > 1:
            for m in SEPARATES[name]:
                assert m in seen[name], (shape, name, m)
    q, table = inputs["no_fill"]
    x = ref_unpack(q, table)
    assert (q == FILL).any() and np.isfinite(x[q == FILL]).all(), "without a fill code -32768 is a number"
    filled = table.copy()
    filled[:, 2] = FILL
    assert np.isnan(ref_unpack(q, filled)[q == FILL]).all()
    q, table = inputs["fma_ties"]
    ref, fused = ref_unpack(q, table), ref_unpack(q, table, "fma")
    for c in range(TIE_CHANNELS):
        for j in {0, n - 1, n // 2}:
            a, b = ref[c].reshape(-1)[j], fused[c].reshape(-1)[j]
            assert a != b and (bits(a) & 1) == 0, (shape, c, j, a, b)       # the tie went to the even neighbour
    return seen
