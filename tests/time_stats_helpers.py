"""The numpy reference of the per-grid-point time statistics (cra5_amd.timestats), shared by the CPU and the GPU tests:
float64 s and q updated frame by frame in order, the statistics from them, min / max through np.minimum / np.maximum."""
import numpy as np


class RefTimeStats:
    """Sequential reference: add(x) per frame in order; .s / .q / .mn / .mx are the raw accumulators after each add."""

    def __init__(self):
        self.n = 0
        self.s = self.q = self.mn = self.mx = None

    def add(self, x):
        x = np.asarray(x)
        assert x.dtype == np.float32
        v = x.astype(np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            if self.n == 0:
                self.s, self.q, self.mn, self.mx = v.copy(), v ** 2, x.copy(), x.copy()
            else:
                self.s += v
                self.q += v ** 2
                self.mn = np.minimum(self.mn, x)
                self.mx = np.maximum(self.mx, x)
        self.n += 1
        return self

    def mean(self):
        with np.errstate(invalid="ignore"):
            return (self.s / self.n).astype(np.float32)

    def std(self, ddof=0):
        with np.errstate(invalid="ignore", over="ignore"):
            var = (self.q - self.s * self.s / self.n) / (self.n - ddof)
            return np.sqrt(np.maximum(0.0, var)).astype(np.float32)

    def stats(self, ddof=0):
        return dict(n=self.n, mean=self.mean(), std=self.std(ddof), min=self.mn, max=self.mx)


def ref_time_stats(frames, ddof=0):
    r = RefTimeStats()
    for x in frames:
        r.add(x)
    return r.stats(ddof)


def within_one_ulp(got, ref):
    """got within one fp32 ulp (np.spacing of the reference) of ref, NaN where ref is NaN."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.dtype == np.float32 and ref.dtype == np.float32 and got.shape == ref.shape
    nan = np.isnan(ref)
    if not np.array_equal(np.isnan(got), nan):
        return False
    ok = ~nan
    with np.errstate(invalid="ignore"):
        d = np.abs(got[ok].astype(np.float64) - ref[ok].astype(np.float64))
        return bool(np.all((d <= np.spacing(np.abs(ref[ok])).astype(np.float64)) | (got[ok] == ref[ok])))
