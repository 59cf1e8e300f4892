"""The numpy reference of the residual layer (cra5_amd/residual.py, csrc/residual.hip), shared by the CPU and GPU tests: the
five rules of DESIGN.md section 4 ("Residual layer") restated in numpy float32 / float64, and the apply with its subset
mapping through subset.kept_points."""
import numpy as np

from cra5_amd.subset import kept_points

ULP = 2.0 ** -8            # one fp32 ulp of a value in [2^15, 2^16): the fields of 5e4 +- 1e4


def ref_quantize(x, x_hat, tol):
    """x, x_hat float32 [C, H, W], tol float32 [C] (+inf: not corrected) -> (idx uint32 [n], q int16 [n], eidx uint32 [m],
    ebits uint32 [m], per_channel int64 [C, 2]), idx / eidx ascending."""
    x, x_hat, tol = np.asarray(x), np.asarray(x_hat), np.asarray(tol)
    assert x.dtype == x_hat.dtype == tol.dtype == np.float32 and x.shape == x_hat.shape and tol.shape == x.shape[:1]
    C = x.shape[0]
    on = np.isfinite(tol)[:, None, None]
    step32 = (np.float32(2) * tol)[:, None, None]
    with np.errstate(all="ignore"):
        d = x.astype(np.float64) - x_hat.astype(np.float64)                      # rule 1
        qd = np.rint(d / step32.astype(np.float64))
        esc = ~np.isfinite(d) | ~(np.abs(qd) <= 32767.0)                         # rule 2
        qi = np.where(esc, 0.0, qd).astype(np.int32)
        corr = qi.astype(np.float32) * step32                                    # rule 3: two fp32 roundings
        assert corr.dtype == np.float32
        xt = np.where(qi == 0, x_hat, x_hat + corr)
        assert xt.dtype == np.float32
        ok = np.abs(x.astype(np.float64) - xt.astype(np.float64)) <= tol.astype(np.float64)[:, None, None]   # rule 4
    rec = on & ~esc & ok & (qi != 0)
    out = on & (esc | ~ok)                                                       # rule 5
    idx = np.flatnonzero(rec.reshape(-1)).astype(np.uint32)
    eidx = np.flatnonzero(out.reshape(-1)).astype(np.uint32)
    per = np.stack([rec.reshape(C, -1).sum(axis=1), out.reshape(C, -1).sum(axis=1)], axis=1).astype(np.int64)
    return idx, qi.reshape(-1)[idx].astype(np.int16), eidx, x.reshape(-1).view(np.uint32)[eidx].copy(), per


def ref_apply(out, grid, tol, idx, q, eidx, ebits, channels=None, box=None, stride=None):
    """The corrected copy of `out` float32 [C', Ho, Wo]: the decode's output for `channels` (global channel indexes in
    output order; None: all), `box` (r0, r1, c0, nc) and `stride` (s_lat, s_lon) of the global grid = (C, H, W)."""
    C, H, W = grid
    out = np.array(out, dtype=np.float32, copy=True)
    rows, cols = kept_points(box if box is not None else (0, H, 0, W), stride if stride is not None else (1, 1), W)
    chans = list(range(C)) if channels is None else list(channels)
    assert out.shape == (len(chans), len(rows), len(cols))
    lut = np.full(C, -1, dtype=np.int64)
    lut[chans] = np.arange(len(chans))
    orow = np.full(H, -1, dtype=np.int64)
    orow[rows] = np.arange(len(rows))
    ocol = np.full(W, -1, dtype=np.int64)
    ocol[cols] = np.arange(len(cols))
    step32 = np.float32(2) * np.asarray(tol, dtype=np.float32)

    def where(i):
        i = np.asarray(i, dtype=np.int64)
        c, r, col = i // (H * W), i // W % H, i % W
        keep = (lut[c] >= 0) & (orow[r] >= 0) & (ocol[col] >= 0)
        return keep, c[keep], (lut[c[keep]], orow[r[keep]], ocol[col[keep]])

    keep, c, at = where(idx)
    with np.errstate(all="ignore"):
        corr = np.asarray(q, dtype=np.int16)[keep].astype(np.float32) * step32[c]
        assert corr.dtype == np.float32
        out[at] = out[at] + corr
    keep, _, at = where(eidx)
    out.view(np.uint32)[at] = np.asarray(ebits, dtype=np.uint32)[keep]
    return out


def guarantee_holds(x, xt, tol):
    """At every point of a corrected channel: xt is x bit for bit, or |x - xt| <= tol in float64."""
    x, xt = np.asarray(x, dtype=np.float32), np.asarray(xt, dtype=np.float32)
    tol = np.asarray(tol, dtype=np.float32)
    on = np.isfinite(tol)
    with np.errstate(all="ignore"):
        close = np.abs(x.astype(np.float64) - xt.astype(np.float64)) <= tol.astype(np.float64)[:, None, None]
    return bool(((x.view(np.uint32) == xt.view(np.uint32)) | close)[on].all())


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- inputs ------------------------------------------------------------------------------------------------------------

TOLS = {"0.7ulp": 0.7 * ULP, "1.3ulp": 1.3 * ULP, "8ulp": 8 * ULP, "1.0": 1.0, "100": 100.0}
SHAPES = [(3, 5, 37), (2, 9, 1440), (5, 33, 250)]


def field(shape, kind, tol, seed, inf_channel=True):
    """-> (x, x_hat, tol [C]): x = 5e4 +- 1e4 ("offset") or 0 +- 1e4 ("zero"), x_hat = x + 3 tol * noise in fp32; the last
    channel of a multi-channel frame is not corrected."""
    rng = np.random.default_rng(seed)
    C = shape[0]
    x = (rng.standard_normal(shape) * 1e4 + (5e4 if kind == "offset" else 0.0)).astype(np.float32)
    t = np.full(C, tol, dtype=np.float32)
    x_hat = (x + (np.float32(3) * t)[:, None, None] * rng.standard_normal(shape).astype(np.float32)).astype(np.float32)
    if inf_channel and C > 1:
        t[-1] = np.inf
    return x, x_hat, t


def inject(x, x_hat, tol):
    """Overwrite points of channel 0 (in place) with the edge cases: d exactly +-tol and +-3 tol (ties of rint), |q| > 32767,
    x_hat = NaN / +inf / -0.0, a NaN truth; when there are three or more channels, channel 1 gets x_hat = x (no records)."""
    t = np.float32(tol[0])
    a, h = x[0].reshape(-1), x_hat[0].reshape(-1)
    base = np.float32(1024.0) * t               # base and base +- k t are exact in fp32 for small k
    cases = [(base + t, base), (base - t, base), (base + 3 * t, base), (base - 3 * t, base), (base + 5 * t, base),
             (base + np.float32(70000.0) * t, base), (base - np.float32(70000.0) * t, base),
             (np.float32(1.0), np.float32(np.nan)), (np.float32(1.0), np.float32(np.inf)),
             (np.float32(0.0), np.float32(-0.0)), (np.float32(7.0) * t, np.float32(-0.0)),
             (np.float32(np.nan), np.float32(1.0))]
    pos = np.linspace(0, a.size - 1, len(cases)).astype(np.int64)
    assert len(set(pos.tolist())) == len(cases)
    for p, (xv, hv) in zip(pos, cases):
        a[p], h[p] = xv, hv
    if x.shape[0] >= 3:
        x_hat[1] = x[1]
    return x, x_hat, tol
