"""Shared by the zonal-spectrum tests: the float64 reference of the definition, the test fields and
the comparison with its tolerance."""
import numpy as np

SPECTRA = ("power_truth", "power_recon", "power_error")

# |got(k) - ref(k)| <= TOL * sqrt(ref(k) * sum_k ref) per channel and bin.  A float64 FFT is bounded a priori by
# eps * log2(W) = 1.2e-15 in these units (numpy's rfft and the two-rows-in-one-transform packing measure <= 1.5e-16
# against an 80-bit direct DFT); an error spectrum from X_hat(k) - X(k) sits at 1e-13, fp32 coefficients at 5e-9 and above.
TOL = 2e-14


def weights32(lat, H):
    """The weights as the device holds them: rounded to fp32 (the C ABI takes `const float *lat_w`), then float64."""
    if lat is None:
        return np.ones(H, dtype=np.float64)
    w = np.asarray(lat, dtype=np.float64)
    assert w.shape == (H,)
    return w.astype(np.float32).astype(np.float64)


def zonal_power(f, L):
    """P_f [C, K] of a float64 field [C, H, W] with float64 weights L [H]: the definition, with numpy's rfft."""
    C, H, W = f.shape
    K = W // 2 + 1
    F = np.fft.rfft(f, axis=-1)
    m = np.full(K, 2.0)
    m[0] = 1.0
    if W % 2 == 0:
        m[-1] = 1.0
    p = (F.real * F.real + F.imag * F.imag) * L[None, :, None]
    return p.sum(axis=1) * m[None, :] / (float(H) * float(W) * float(W))


def resolved(pt, pe, nonfinite):
    C, K = pt.shape
    out = np.full(C, K, dtype=np.int64)
    for c in range(C):
        if nonfinite[c] > 0:
            out[c] = -1
            continue
        for k in range(1, K):
            if pe[c, k] >= pt[c, k]:
                out[c] = k
                break
    return out


def ref_spectrum(x_hat, x, lat):
    """The reference: x_hat, x fp32 numpy [C, H, W]; lat None or an [H] array (rounded to fp32 as on the device).  d is
    formed in fp32, everything after in float64; a channel with a non-finite value in either frame is NaN in every bin."""
    assert x_hat.dtype == np.float32 and x.dtype == np.float32 and x_hat.shape == x.shape and x.ndim == 3
    C, H, W = x.shape
    K = W // 2 + 1
    L = weights32(lat, H)
    nf = (~(np.isfinite(x_hat) & np.isfinite(x))).reshape(C, -1).sum(axis=1).astype(np.int64)
    ok = nf == 0
    r = {k: np.full((C, K), np.nan) for k in SPECTRA}
    if ok.any():
        d = x_hat[ok] - x[ok]                       # fp32
        assert d.dtype == np.float32
        r["power_truth"][ok] = zonal_power(x[ok].astype(np.float64), L)
        r["power_recon"][ok] = zonal_power(x_hat[ok].astype(np.float64), L)
        r["power_error"][ok] = zonal_power(d.astype(np.float64), L)
    r["wavenumber"] = np.arange(K, dtype=np.int64)
    r["nonfinite"] = nf
    r["resolved_wavenumber"] = resolved(r["power_truth"], r["power_error"], nf)
    return r


def smooth_pair(C, H, W, seed):
    """x = 5e4 + a field whose harmonics k >= 1 have amplitude 1e4 (1 + k)^-3 and random phases per row, rounded to fp32;
    x_hat = x + 10 N(0, 1).  fp32 numpy [C, H, W] each.  The spectrum of x spans more than 10 decades."""
    rng = np.random.default_rng(seed)
    K = W // 2 + 1
    k = np.arange(K, dtype=np.float64)
    amp = 1e4 * (1.0 + k) ** -3
    amp[0] = 0.0
    phase = rng.uniform(0.0, 2.0 * np.pi, size=(C, H, K))
    coef = amp * np.exp(1j * phase) * (W / 2.0)        # irfft divides by W: a cosine of amplitude a has coefficient a W / 2
    if W % 2 == 0:
        coef[..., -1] = amp[-1] * np.cos(phase[..., -1]) * W
    x = (5e4 + np.fft.irfft(coef, n=W, axis=-1)).astype(np.float32)
    x_hat = (x.astype(np.float64) + 10.0 * rng.standard_normal((C, H, W))).astype(np.float32)
    return np.ascontiguousarray(x_hat), np.ascontiguousarray(x)


def worst_ratio(got, ref):
    """max over the three spectra, the finite channels and the bins of |got - ref| / sqrt(ref(k) * sum_k ref)."""
    worst = 0.0
    for name in SPECTRA:
        g, r = got[name], ref[name]
        ok = ~np.isnan(r).any(axis=1)
        if not ok.any():
            continue
        scale = np.sqrt(r[ok] * r[ok].sum(axis=1, keepdims=True))
        err = np.abs(g[ok] - r[ok])
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(err == 0.0, 0.0, err / scale)
        worst = max(worst, float(q.max()))
    return worst


def assert_spectra_match(got, ref, what=""):
    for name in SPECTRA:
        assert got[name].dtype == np.float64 and got[name].shape == ref[name].shape, (what, name)
        assert np.array_equal(np.isnan(got[name]), np.isnan(ref[name])), (what, name)
    assert got["wavenumber"].dtype == np.int64 and np.array_equal(got["wavenumber"], ref["wavenumber"]), what
    if "nonfinite" in got:
        assert got["nonfinite"].dtype == np.int64 and np.array_equal(got["nonfinite"], ref["nonfinite"]), what
    q = worst_ratio(got, ref)
    print(f"spectrum {what}: worst |got - ref| / sqrt(ref(k) sum ref) = {q:.3g} (bound {TOL:g})")
    assert q <= TOL, (what, q)
    # the crossing is decided by got's own bins (two spectra that agree to 1e-14 may still cross one bin apart)
    assert got["resolved_wavenumber"].dtype == np.int64
    assert np.array_equal(got["resolved_wavenumber"], resolved(got["power_truth"], got["power_error"], ref["nonfinite"])), what
