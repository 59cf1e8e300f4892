"""The numpy reference of the regridding kernel ("Regridding"), shared by the CPU and the GPU tests:
the definition as a sequential float64 loop over a plan's tables, in the stated order - vectorised over output points,
never over taps -, and small geometry helpers written from the definitions, not from cra5_amd/regrid.py."""
import numpy as np


def ref_regrid(full, plan, chans=None):
    """full: float32 [C, H, W], the GLOBAL field (columns wrap) -> (float32 [C', Ho, Wo], the float64 value before the
    cast), rows in the plan's (the caller's) order:
        inner(h, j) = 0;  for u west to east:   inner = inner + cw[j][u] * x[h][(col0[j] + u) mod W]
        acc = 0;          for t north to south: acc = acc + rw[i][t] * inner(row0[i] + t, j);   out = float32(acc)."""
    full = np.asarray(full)
    assert full.dtype == np.float32
    x = full if chans is None else full[list(chans)]
    C, H, W = x.shape
    assert (H, W) == tuple(plan["grid"])
    Ho, Wo = plan["Ho"], plan["Wo"]
    row0, ntap, rw = plan["row0"], plan["ntap"], plan["rw"]
    col0, ctap, cw = plan["col0"].astype(np.int64), plan["ctap"], plan["cw"]
    inners = {}

    def inner(h):
        if h not in inners:
            v = np.zeros((C, Wo))
            for u in range(int(ctap.max())):
                m = np.nonzero(ctap > u)[0]                   # a column past its window adds nothing, not even 0 * x
                v[:, m] = v[:, m] + cw[m, u] * x[:, h, (col0[m] + u) % W].astype(np.float64)
            inners[h] = v
        return inners[h]

    out64 = np.empty((C, Ho, Wo), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(Ho):
            acc = np.zeros((C, Wo))
            for t in range(int(ntap[i])):
                acc = acc + rw[i, t] * inner(int(row0[i]) + t)
            out64[:, i] = acc
        return out64.astype(np.float32), out64


def abs_regrid(full, plan):
    """sum |w| |x| of every output point, float64 [C, Ho, Wo]: the scale of the summation error bounds."""
    a = dict(plan, rw=np.abs(plan["rw"]), cw=np.abs(plan["cw"]))
    return ref_regrid(np.abs(np.asarray(full)), a)[1]


def source_lat(H):
    return 90.0 - np.arange(H) * (180.0 / (H - 1))


def source_lon(W):
    return np.arange(W) * (360.0 / W)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.int32), b.view(np.int32))


def field(C, Hg, Wg, seed, physical=True):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((C, Hg, Wg))
    if physical:
        x = 5e4 * (1 + 0.2 * rng.random((C, 1, 1))) + 1e4 * x
    return x.astype(np.float32)
