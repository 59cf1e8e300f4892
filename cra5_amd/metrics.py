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


# ---- exact quantiles (csrc/quantile.hip) ----------------------------------------------------------------------------------
# Per channel three fields - truth x, recon x_hat, abs_error |x_hat - x| (the metric's fp32 difference) - and integer row
# weights w_h = rint(float64 L(h) * 2^16) (None: 1; a row of weight 0 does not count).  Wtot = W * sum_h w_h, and for a
# probability p the target T(p) = min(Wtot, max(1, ceil(p * float(Wtot)))), in float64, the product rounded once.
# Q_f(c, p) = the smallest value v of field f in channel c whose points with value <= v weigh >= T(p): an element of the
# field with its own fp32 bits, nothing interpolated; numpy's "inverted_cdf" when all weights are 1.

QUANTILE_WEIGHT_ONE = 1 << 16     # the integer weight of L(h) = 1
QUANTILE_WEIGHT_MAX = 1 << 20     # cra5_frame_quantiles_f32's limit per row
_QUANTILE_CACHE = {}              # (weights identity, H, W, q, device) -> (keep-alive, row_w dev, targets dev, q array)
_QUANTILE_CACHE_MAX = 64


def quantile_weights(lat_weights, H):
    """The integer row weights of the quantiles, int64 [H]: ones for None, else rint(float64 L(h) * 2^16) of "era5"
    (latitude_weights(H)) or of an [H] array.  ValueError for a negative or non-finite weight, a weight above 2^20
    (L(h) > 16) and for weights that are all 0."""
    H = int(H)
    if lat_weights is None:
        return np.ones(H, dtype=np.int64)
    if isinstance(lat_weights, str):
        if lat_weights != "era5":
            raise ValueError(f"lat_weights must be 'era5', None or an [H] array (got {lat_weights!r})")
        L = latitude_weights(H)
    else:
        L = lat_weights.detach().cpu().numpy() if isinstance(lat_weights, torch.Tensor) else np.asarray(lat_weights)
        if L.shape != (H,):
            raise ValueError(f"lat_weights must have shape [{H}] (got {tuple(L.shape)})")
        L = L.astype(np.float64)
    if not np.all(np.isfinite(L)) or np.any(L < 0):
        raise ValueError("quantile weights must be finite and >= 0")
    w = np.rint(L * float(QUANTILE_WEIGHT_ONE))
    if np.any(w > QUANTILE_WEIGHT_MAX):
        raise ValueError(f"quantile weights: rint(L(h) * 2^16) must not exceed 2^20 = {QUANTILE_WEIGHT_MAX} "
                         f"(L(h) <= 16; got max L = {float(L.max()):g})")
    w = w.astype(np.int64)
    if not np.any(w > 0):
        raise ValueError("quantile weights: every row has integer weight 0 - nothing to count")
    return w


def quantile_targets(q, row_w, W):
    """The integer targets T(p) of the probabilities `q` under the integer row weights `row_w` [H] and the width W, int64
    [Q] in the order given (duplicates allowed).  ValueError unless q is a non-empty sequence of at most 16 finite floats
    in [0, 1]."""
    from .ops import QUANTILE_MAX_Q
    if isinstance(q, (str, bytes)) or not hasattr(q, "__len__") or np.ndim(q) != 1:
        raise ValueError(f"quantiles must be a sequence of 1 to {QUANTILE_MAX_Q} probabilities in [0, 1] (got {q!r})")
    n = len(q)
    if not 1 <= n <= QUANTILE_MAX_Q:
        raise ValueError(f"quantiles must be a sequence of 1 to {QUANTILE_MAX_Q} probabilities in [0, 1] (got {n})")
    try:
        p = np.array([float(v) for v in q], dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"quantiles must be a sequence of 1 to {QUANTILE_MAX_Q} probabilities in [0, 1] (got {q!r})")
    if not np.all(np.isfinite(p)) or np.any(p < 0.0) or np.any(p > 1.0):
        raise ValueError(f"quantiles must be finite probabilities in [0, 1], at most {QUANTILE_MAX_Q} of them "
                         f"(got {p.tolist()})")
    wtot = int(W) * int(np.asarray(row_w, dtype=np.int64).sum())
    if not 1 <= wtot < 1 << 53:
        raise ValueError(f"quantiles: the total weight W * sum(row_w) = {wtot} must be in 1 .. 2^53 - 1")
    t = np.ceil(p * float(wtot))                 # float64: the product rounds once
    return np.minimum(wtot, np.maximum(1, t.astype(np.int64))).astype(np.int64)


def quantile_plan(q, lat_weights, H, W, device):
    """(row_w device int32 [H] or None, targets device int64 [Q], q float64 [Q]) - validated, and cached per (weights
    identity, H, W, q, device), so that a batch uploads them once."""
    try:
        qkey = tuple(float(v) for v in q)
    except (TypeError, ValueError):
        qkey = None
    wkey = lat_weights if lat_weights is None or isinstance(lat_weights, str) else id(lat_weights)
    key = (wkey, int(H), int(W), qkey, str(device))
    hit = _QUANTILE_CACHE.get(key) if qkey is not None else None
    if hit is not None:
        return hit[1:]
    w = quantile_weights(lat_weights, H)
    t = quantile_targets(q, w, W)
    row_w = None if lat_weights is None else torch.from_numpy(w.astype(np.int32)).to(device)
    plan = (lat_weights, row_w, torch.from_numpy(t).to(device), np.array(qkey, dtype=np.float64))
    if len(_QUANTILE_CACHE) >= _QUANTILE_CACHE_MAX:
        _QUANTILE_CACHE.clear()
    _QUANTILE_CACHE[key] = plan        # (holds lat_weights: its id cannot be reused while the entry lives)
    return plan[1:]


def frame_quantiles(x_hat, x, q, lat_weights="era5"):
    """Exact quantiles of the truth `x`, the reconstruction `x_hat` and the error magnitude |x_hat - x|, per channel:
    device fp32 tensors [C, H, W] or [1, C, H, W] of the same shape; q: 1 to 16 probabilities in [0, 1], any order;
    lat_weights as reconstruction_error ("era5", None or an [H] array), turned into integer row weights by
    quantile_weights - with weights the quantiles are area-true, a row of weight 0 (the poles) does not count.  Four
    streaming digit passes on the GPU (ops.frame_quantiles, the current stream); only 3 x C x Q numbers come back, each an
    element of its field with its own fp32 bits (with lat_weights=None: np.quantile(..., method="inverted_cdf")).
    Returns {"quantile": float64 [Q] (q as given), "quantile_truth", "quantile_recon", "quantile_abs_error": float64
    [C, Q], "quantile_shift" = quantile_recon - quantile_truth (negative at p = 0.9999: the upper tail was damped),
    "nonfinite": int64 [C]}; a channel with nonfinite > 0 has NaN in every quantile."""
    x_hat, x = _frame_pair("frame_quantiles", x_hat, x)
    from . import ops
    C, H, W = x.shape
    row_w, targets, qa = quantile_plan(q, lat_weights, H, W, x.device)
    Q = len(qa)
    out = torch.empty((3 * C * Q + C,), device=x.device, dtype=torch.float64)
    ops.frame_quantiles(x_hat, x, row_w, targets, out=out)
    r = out.cpu().numpy()      # the quantiles and the counts: one copy
    v, nf = r[:3 * C * Q].reshape(3, C, Q), r[3 * C * Q:].astype(np.int64)
    return dict(quantile=qa.copy(), quantile_truth=v[0].copy(), quantile_recon=v[1].copy(),
                quantile_abs_error=v[2].copy(), quantile_shift=v[1] - v[0], nonfinite=nf)
