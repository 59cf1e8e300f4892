"""The packed int16 definition ("Packed int16 output") in plain numpy float64, its wrong variants
("mutants") and the inputs that tell them apart - shared by tests/test_pack_cpu.py and tests/test_pack_gpu.py."""
import numpy as np

FILL = -32768
MUTANTS = ("f32_arith", "half_up", "trunc", "reciprocal", "fill_as_zero", "range_65535", "no_clamp")
TIE_RANGE = (-8191.75, 8191.75)      # scale = 0.25, offset = 0 exactly: k / 4 + 1 / 8 are exact ties
TIE2_RANGE = (-503792.625, 503792.625)   # scale = 15.375, offset = 0 exactly: 15.375 (k + 1 / 2) are exact ties in fp32, and
                                         # 1 / 15.375 is no double - x * (1 / scale) misses the tie for about half the k


def finite_mask(x):
    """The bit test of the definition: the exponent bits are not all ones."""
    return (np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) & np.uint32(0x7f800000)) != np.uint32(0x7f800000)


def ref_pack(x, fixed=None, mutant=None):
    """x float32 [C, H, W]; fixed None | [C, 2] float64 (NaN lo: that channel's own range)
    -> q int16 [C, H, W], scale float64 [C], offset float64 [C], vmin float32 [C], vmax float32 [C], nonfinite int64 [C],
    saturated bool [C]."""
    assert mutant is None or mutant in MUTANTS
    x = np.ascontiguousarray(x, dtype=np.float32)
    C = x.shape[0]
    q = np.empty(x.shape, dtype=np.int16)
    scale, offset = np.ones(C), np.zeros(C)
    vmin, vmax = np.full(C, np.nan, dtype=np.float32), np.full(C, np.nan, dtype=np.float32)
    nonfinite, saturated = np.zeros(C, dtype=np.int64), np.zeros(C, dtype=bool)
    fin = finite_mask(x)
    for c in range(C):
        ok = fin[c]
        nonfinite[c] = ok.size - ok.sum()
        if ok.any():
            vmin[c], vmax[c] = x[c][ok].min(), x[c][ok].max()
        given = fixed is not None and not np.isnan(fixed[c][0])
        lo, hi = (np.float64(fixed[c][0]), np.float64(fixed[c][1])) if given else (np.float64(vmin[c]), np.float64(vmax[c]))
        if given or ok.any():
            if lo == hi:
                offset[c] = lo
            else:
                scale[c] = (hi - lo) / (65535.0 if mutant == "range_65535" else 65534.0)
                offset[c] = (lo + hi) * 0.5
        saturated[c] = bool(given and (vmin[c] < lo or vmax[c] > hi))
        v = np.where(ok, x[c], np.float32(0))
        with np.errstate(all="ignore"):
            if mutant == "f32_arith":
                r = ((v - np.float32(offset[c])) / np.float32(scale[c])).astype(np.float64)
            elif mutant == "reciprocal":
                r = (v.astype(np.float64) - offset[c]) * (1.0 / scale[c])
            else:
                r = (v.astype(np.float64) - offset[c]) / scale[c]
            r = np.floor(r + 0.5) if mutant == "half_up" else np.trunc(r) if mutant == "trunc" else np.rint(r)
            if mutant == "no_clamp":
                code = np.clip(r, -2.0 ** 62, 2.0 ** 62).astype(np.int64).astype(np.int16)      # wraps like a bare conversion
            else:
                code = np.clip(r, -32767.0, 32767.0).astype(np.int16)
        q[c] = np.where(ok, code, np.int16(0 if mutant == "fill_as_zero" else FILL))
    return q, scale, offset, vmin, vmax, nonfinite, saturated


def unpack(q, scale, offset):
    out = q.astype(np.float64) * scale[:, None, None] + offset[:, None, None]
    out[q == FILL] = np.nan
    return out


def bound(scale, lo, hi):
    """|unpack(q) - x| <= scale (0.5 + 2^-30) + 2^-50 max(|lo|, |hi|) for a finite x inside (lo, hi)."""
    return scale * (0.5 + 2.0 ** -30) + 2.0 ** -50 * max(abs(lo), abs(hi))


def _all(C, rng):
    return np.tile(np.asarray(rng, dtype=np.float64), (C, 1))


def pack_inputs(shape=(3, 7, 13), seed=0):
    """name -> (x float32 [C, H, W], fixed float64 [C, 2] | None): the named inputs both test files use."""
    C, H, W = shape
    n = H * W
    rng = np.random.default_rng(seed + 1000 * C + n)
    normal = lambda: rng.standard_normal(shape)     # noqa: E731
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)      # noqa: E731
    inputs = {}
    inputs["physical"] = (f32(5e4 + 1e4 * normal()), None)
    inputs["zero_mean"] = (f32(normal()), None)
    k = rng.integers(-32767, 32767, size=shape)
    inputs["ties"] = (f32(k / 4.0 + 0.125), _all(C, TIE_RANGE))
    inputs["ties_recip"] = (f32(15.375 * (k + 0.5)), _all(C, TIE2_RANGE))
    x = f32(280.0 + 5.0 * normal())
    x[0] = np.float32(273.15)
    inputs["constant"] = (x, None)
    x = f32(normal())
    x[0] = np.nan
    inputs["all_nan"] = (x, None)
    # NaN / +inf / -inf at the start and the end of every plane and across float4 boundaries
    x = f32(1e3 * normal()).reshape(C, n)
    for j, bad in zip((0, 1, 3, 4, 5, 7, 8, n - 2, n - 1, n // 2), (np.nan, np.inf, -np.inf) * 4):
        x[:, j % n] = bad
    x[C - 1, (n // 3) % n] = -np.nan
    inputs["sprinkled"] = (x.reshape(shape), None)
    x = f32(normal())
    x[0] = 0.0
    x[rng.random(shape) < 0.4] = 0.0
    x = np.where(rng.random(shape) < 0.5, -x, x)       # +0 and -0 mixed (channel 0: nothing else)
    inputs["signed_zeros"] = (f32(x), None)
    bits = rng.integers(1, 0x800000, size=shape).astype(np.uint32) | (rng.integers(0, 2, size=shape).astype(np.uint32) << 31)
    inputs["denormals"] = (bits.view(np.float32).copy(), None)
    x = f32(1e37 * normal()).reshape(C, n)
    x[0, 0], x[0, n - 1] = np.float32(3.4e38), np.float32(-3.4e38)
    inputs["extremes"] = (x.reshape(shape), None)
    a = np.float32(5e4)
    inputs["adjacent"] = (np.where(rng.random(shape) < 0.5, a, np.nextafter(a, np.float32(np.inf))).astype(np.float32), None)
    fixed = _all(C, (-5.0, 5.0))
    if C > 1:
        fixed[1] = np.nan                              # a per-frame channel in a table of fixed ranges
    inputs["outside_fixed"] = (f32(10.0 * normal()), fixed)
    return inputs
