"""Shared by the quantile tests: the numpy reference of the definition ("Quantiles"), the bit-exact
comparison and the builders of the input families."""
import numpy as np

FIELDS = ("truth", "recon", "abs_error")
Q8 = (0.0, 1e-4, 0.01, 0.5, 0.5, 0.99, 0.9999, 1.0)
Q16 = (0.0, 1e-4, 1e-3, 0.01, 0.05, 0.1, 0.25, 0.5, 0.5, 0.75, 0.9, 0.95, 0.99, 0.999, 0.9999, 1.0)
INTERIOR_ZERO_ROWS = (1, 2, 5)    # rows that interior_zero_weights() switches off (where H reaches them)


def targets(q, row_w, W):
    """T(p) = min(Wtot, max(1, ceil(p * float(Wtot)))), Wtot = W * sum(row_w); float64, the product rounded once."""
    wtot = int(W) * int(np.asarray(row_w, dtype=np.int64).sum())
    t = np.ceil(np.asarray(q, dtype=np.float64) * float(wtot)).astype(np.int64)
    return np.minimum(wtot, np.maximum(1, t))


def ref_field_quantiles(f, row_w, T):
    """One channel of one field f [H, W] fp32, integer row weights [H], integer targets [Q] -> fp32 [Q]: the smallest
    element whose cumulative weight reaches the target (stable argsort, cumsum, searchsorted "left")."""
    f = np.asarray(f, dtype=np.float32) + np.float32(0.0)        # -0 -> +0
    w = np.asarray(row_w, dtype=np.int64)
    keep = w > 0
    v = f[keep].reshape(-1)
    ww = np.repeat(w[keep], f.shape[1])
    order = np.argsort(v, kind="stable")
    cum = np.cumsum(ww[order])
    return v[order][np.searchsorted(cum, np.asarray(T, dtype=np.int64), "left")]


def ref_quantiles(x_hat, x, q, row_w):
    """x_hat, x fp32 [C, H, W], q probabilities, row_w int [H] -> {field: fp32 [C, Q]}, nonfinite int64 [C]; a channel
    with a non-finite point in x or x_hat has NaN everywhere."""
    x_hat, x = np.asarray(x_hat, dtype=np.float32), np.asarray(x, dtype=np.float32)
    C, H, W = x.shape
    T = targets(q, row_w, W)
    nf = (~(np.isfinite(x) & np.isfinite(x_hat))).reshape(C, -1).sum(axis=1).astype(np.int64)
    out = {k: np.full((C, len(T)), np.nan, dtype=np.float32) for k in FIELDS}
    for c in range(C):
        if nf[c]:
            continue
        with np.errstate(over="ignore"):
            fields = dict(truth=x[c], recon=x_hat[c], abs_error=np.abs(x_hat[c] - x[c]))
        for k in FIELDS:
            out[k][c] = ref_field_quantiles(fields[k], row_w, T)
    return out, nf


def bits(a):
    """fp32 array -> its bytes with every zero made +0 (the sign of a returned zero is unspecified)."""
    a = np.array(a, dtype=np.float32)
    a[a == 0] = 0.0
    return a.tobytes()


def assert_same_bits(got, ref, what):
    """got: metrics.frame_quantiles' dict (float64, each value an fp32 widened exactly); ref: ref_quantiles' dict."""
    for k in FIELDS:
        g64 = np.asarray(got["quantile_" + k])
        g = g64.astype(np.float32)
        fin = ~np.isnan(g64)
        assert np.array_equal(g.astype(np.float64)[fin], g64[fin]), f"{what} {k}: not fp32 values"
        assert g.shape == ref[k].shape, (what, k, g.shape, ref[k].shape)
        assert np.array_equal(np.isnan(g), np.isnan(ref[k])), f"{what} {k}: NaN pattern"
        assert bits(np.nan_to_num(g, nan=0.0)) == bits(np.nan_to_num(ref[k], nan=0.0)), \
            f"{what} {k}:\n got {g}\n ref {ref[k]}"


def interior_zero_weights(H):
    """float64 [H] latitude-style weights with interior rows of weight 0 (and unequal weights elsewhere)."""
    L = 0.25 + np.arange(H, dtype=np.float64) % 3
    for r in INTERIOR_ZERO_ROWS:
        if r < H:
            L[r] = 0.0
    if not np.any(L > 0):
        L[0] = 1.0
    return L


# ---- input families: each (x_hat, x) fp32 [C, H, W] -----------------------------------------------------------------------

def smooth(shape, seed=0):
    """Mean 280, amplitude 30, smooth in both directions; x_hat = x + a small perturbation: a whole channel sits in one
    first-digit bin (sign, exponent) - the contention path, and every quantile shares its first prefix."""
    C, H, W = shape
    rng = np.random.default_rng(seed)
    lat = np.linspace(0.0, np.pi, H)[None, :, None]
    lon = np.linspace(0.0, 2 * np.pi, W, endpoint=False)[None, None, :]
    ph = rng.uniform(0, 2 * np.pi, size=(C, 1, 1))
    x = (280.0 + 20.0 * np.cos(lat + ph) + 10.0 * np.sin(2 * lon + ph) * np.sin(lat)).astype(np.float32)
    x_hat = (x + 0.3 * rng.standard_normal(shape)).astype(np.float32)
    return x_hat, x


def low_mantissa(shape, seed=1):
    """Values that differ only in the lowest 8 mantissa bits: only the last digit pass decides."""
    rng = np.random.default_rng(seed)
    base = np.float32(280.0).view(np.uint32) & np.uint32(0xffffff00)
    x = (base | rng.integers(0, 256, size=shape, dtype=np.uint32)).view(np.float32)
    x_hat = (base | rng.integers(0, 256, size=shape, dtype=np.uint32)).view(np.float32)
    return x_hat, x


def random_bits(shape, seed=2):
    """Uniformly random bit patterns over all finite fp32: every exponent, both signs, denormals."""
    rng = np.random.default_rng(seed)

    def draw():
        u = rng.integers(0, 1 << 32, size=shape, dtype=np.uint64).astype(np.uint32)
        bad = (u & np.uint32(0x7f800000)) == np.uint32(0x7f800000)
        u[bad] &= np.uint32(0xbfffffff)          # clear one exponent bit: finite
        return u.view(np.float32)
    return draw(), draw()


def constant(shape, seed=3):
    x = np.full(shape, 273.15, dtype=np.float32)
    return (x + np.float32(0.5)).astype(np.float32), x


def zeros_and_denormals(shape, seed=4):
    """+-0.0 mixed with tiny denormals of both signs."""
    rng = np.random.default_rng(seed)
    pool = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x00000002, 0x80000003, 0x00000100, 0x80000100],
                    dtype=np.uint32)
    x = pool[rng.integers(0, len(pool), size=shape)].view(np.float32)
    x_hat = pool[rng.integers(0, len(pool), size=shape)].view(np.float32)
    return x_hat, x


def half_equal(shape, seed=5):
    """Half of every channel's points share one value in the middle of the range: p = 0.5 falls inside the run of ties."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-5, 5, size=shape).astype(np.float32)
    x[rng.random(size=shape) < 0.5] = np.float32(0.125)
    x_hat = x.copy()
    x_hat[rng.random(size=shape) < 0.5] += np.float32(0.25)
    return x_hat, x


def identical(shape, seed=6):
    """x_hat = x exactly: abs_error is all zero."""
    _, x = smooth(shape, seed)
    return x.copy(), x


FAMILIES = dict(smooth=smooth, low_mantissa=low_mantissa, random_bits=random_bits, constant=constant,
                zeros_and_denormals=zeros_and_denormals, half_equal=half_equal, identical=identical)
