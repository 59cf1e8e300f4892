"""Rate estimate from the entropy models' likelihoods, and the per-variable reconstruction error of a frame.

`estimated_bits(out)` / `estimated_bpp(out, num_pixels)` follow the rate term of the reference's
RateDistortionLoss (losses/rate_distortion.py:71-74): sum over the likelihood tensors of
log(likelihood) / (-ln 2 * num_pixels), without the training-time `bpp_weight` factor.  Applied to
`VAEformer.forward(x)["likelihoods"]` it predicts the size of the rANS streams `compress(x)` writes
(with trained weights the coder's overhead over the model entropy is ~1 %; residuals outside the
CDF tables are charged the likelihood floor of 1e-9 = 30 bits by the estimate but cost less as escapes).
"""
import math

import numpy as np
import torch


def estimated_bits(out):
    """Total model entropy in bits of a forward() output dict (or of its "likelihoods" dict)."""
    lik = out["likelihoods"] if "likelihoods" in out else out
    return float(sum(torch.log(v.double()).sum() for v in lik.values()) / -math.log(2.0))


def estimated_bpp(out, num_pixels):
    """Bits per pixel, num_pixels = N * H * W of the input frames (rate_distortion.py:66, 71-74)."""
    return estimated_bits(out) / float(num_pixels)


# ---- reconstruction error (csrc/metrics.hip) ----------------------------------------------------------------------------
# For frames x (truth) and x_hat (reconstruction), fp32 [C, H, W] in the same units, d = x_hat - x in fp32; per channel c:
#   mse = mean_(h,w) d^2          rmse = sqrt(mse)          wrmse = sqrt(mean_(h,w) L(h) d^2)
#   bias = mean d                 mae = mean |d|            max_abs = max |d| (the fp32 value, exact)
#   nonfinite = count of (h, w) where x or x_hat is NaN / +-inf; a channel with nonfinite > 0 reports NaN in every other
#   statistic (channels without non-finite values are unaffected).
# L(h) is the WeatherBench latitude weight: cos(phi_h) / mean_h' cos(phi_h'), phi_h = 90 - 180 h / (H - 1) degrees.

_LAT_CACHE = {}


def latitude_weights(H):
    """WeatherBench latitude weights L(h) of an H-row equiangular grid from 90 N (row 0) to 90 S (row H - 1), float64
    [H]: mean 1, symmetric, ~0 at the poles.  H >= 2 (the row spacing is 180 / (H - 1) degrees)."""
    H = int(H)
    if H < 2:
        raise ValueError(f"latitude weights need H >= 2 rows from pole to pole (got H = {H})")
    phi = np.deg2rad(90.0 - 180.0 * np.arange(H, dtype=np.float64) / (H - 1))
    c = np.cos(phi)
    return c / c.mean()


def _device_weights(lat_weights, H, device):
    if lat_weights is None:
        return None
    if isinstance(lat_weights, str):
        if lat_weights != "era5":
            raise ValueError(f"lat_weights must be 'era5', None or an [H] array (got {lat_weights!r})")
        key = (H, str(device))
        w = _LAT_CACHE.get(key)
        if w is None:
            w = _LAT_CACHE[key] = torch.from_numpy(latitude_weights(H).astype(np.float32)).to(device)
        return w
    w = lat_weights.detach().cpu().numpy() if isinstance(lat_weights, torch.Tensor) else np.asarray(lat_weights)
    if w.shape != (H,):
        raise ValueError(f"lat_weights must have shape [{H}] (got {tuple(w.shape)})")
    return torch.from_numpy(np.ascontiguousarray(w, dtype=np.float32)).to(device)


def _frame_pair(what, x_hat, x):
    """The tensor checks of reconstruction_error / zonal_spectrum -> the pair as [C, H, W]."""
    if not (isinstance(x_hat, torch.Tensor) and isinstance(x, torch.Tensor)):
        raise TypeError(f"{what}: x_hat and x must be torch tensors on the GPU")
    if tuple(x_hat.shape) != tuple(x.shape):
        raise ValueError(f"{what}: x_hat {tuple(x_hat.shape)} and x {tuple(x.shape)} differ in shape")
    for name, t in (("x_hat", x_hat), ("x", x)):
        if not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
            raise TypeError(f"{what}: {name} must be a contiguous fp32 GPU tensor")
    if x.dim() == 4 and x.shape[0] == 1:
        x_hat, x = x_hat[0], x[0]
    if x.dim() != 3:
        raise ValueError(f"{what} takes [C, H, W] or [1, C, H, W] frames (got {tuple(x.shape)})")
    return x_hat, x


def reconstruction_error(x_hat, x, lat_weights="era5"):
    """Per-channel error of the reconstruction `x_hat` against the truth `x`: device fp32 tensors [C, H, W] or
    [1, C, H, W] of the same shape.  lat_weights: "era5" (latitude_weights(H)), None (L = 1: wrmse = rmse) or an [H]
    array.  One streaming pass on the GPU (ops.recon_error, the current stream); only C x 6 numbers come back.
    Returns {"mse", "rmse", "wrmse", "bias", "mae", "max_abs"}: float64 numpy [C], and "nonfinite": int64 numpy [C]."""
    x_hat, x = _frame_pair("reconstruction_error", x_hat, x)
    from . import ops
    C, H, W = x.shape
    r = ops.recon_error(x_hat, x, _device_weights(lat_weights, H, x.device)).cpu().numpy()
    f = {k: r[:, i] for i, k in enumerate(ops.RECON_FIELDS)}
    return dict(mse=f["mse"].copy(), rmse=np.sqrt(f["mse"]), wrmse=np.sqrt(f["wmse"]), bias=f["bias"].copy(),
                mae=f["mae"].copy(), max_abs=f["max_abs"].copy(), nonfinite=f["nonfinite"].astype(np.int64))


# ---- zonal power spectra (csrc/spectrum.hip) ----------------------------------------------------------------------------
# For a row f(c, h, .) of W points:  F(c, h, k) = sum_w f(c, h, w) e^(-2 pi i k w / W),  k = 0 .. K - 1,  K = W // 2 + 1.
#   P_f(c, k) = (1 / H) sum_h L(h) m_k |F(c, h, k)|^2 / W^2,   m_k = 1 for k = 0 and for k = W / 2 of an even W, else 2
# with the weights L(h) of the error metric (fp32 on the device, as there); d = x_hat - x is formed in fp32, every later
# operation is float64.  Parseval: sum_k P_f(c, k) = mean_(h,w) L(h) f^2, so sum_k P_d(c, k) is the metric's wmse.


def resolved_wavenumber(power_truth, power_error, nonfinite=None):
    """The smallest k >= 1 with power_error[c, k] >= power_truth[c, k] - the scale below which the error exceeds the
    signal - per channel, int64 [C]: K if there is no such k, -1 for a channel with non-finite values."""
    pt, pe = np.asarray(power_truth), np.asarray(power_error)
    C, K = pt.shape
    over = pe[:, 1:] >= pt[:, 1:]
    k = np.where(over.any(axis=1), over.argmax(axis=1) + 1, K).astype(np.int64)
    bad = np.isnan(pt).any(axis=1) | np.isnan(pe).any(axis=1)
    if nonfinite is not None:
        bad |= np.asarray(nonfinite) > 0
    k[bad] = -1
    return k


def zonal_spectrum(x_hat, x, lat_weights="era5"):
    """Zonal (east-west) power spectra of the truth `x`, the reconstruction `x_hat` and the codec error d = x_hat - x:
    device fp32 tensors [C, H, W] or [1, C, H, W] of the same shape, lat_weights as reconstruction_error.  W must have no
    prime factor above 5 and be at most ops.SPECTRUM_MAX_W (ValueError otherwise).  One streaming pass on the GPU
    (ops.zonal_spectrum, the current stream) with the row transforms in LDS; only 3 x C x K numbers come back.
    Returns {"wavenumber": int64 [K] (cycles around the latitude circle), "power_truth", "power_recon", "power_error":
    float64 [C, K] in squared units of the frames (each row sums to the latitude-weighted mean square of its field),
    "resolved_wavenumber": int64 [C] (resolved_wavenumber()), "nonfinite": int64 [C]}; a channel with nonfinite > 0 has
    NaN in every bin and resolved_wavenumber -1."""
    x_hat, x = _frame_pair("zonal_spectrum", x_hat, x)
    from . import ops
    C, H, W = x.shape
    K = W // 2 + 1
    out = torch.empty((3 * C * K + C,), device=x.device, dtype=torch.float64)
    ops.zonal_spectrum(x_hat, x, _device_weights(lat_weights, H, x.device), out=out)
    r = out.cpu().numpy()      # the spectra and the counts: one copy
    p, nf = r[:3 * C * K].reshape(3, C, K), r[3 * C * K:].astype(np.int64)
    return dict(wavenumber=np.arange(K, dtype=np.int64), power_truth=p[0].copy(), power_recon=p[1].copy(),
                power_error=p[2].copy(), resolved_wavenumber=resolved_wavenumber(p[0], p[2], nf), nonfinite=nf)
