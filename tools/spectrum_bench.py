"""Zonal power spectra (csrc/spectrum.hip, cra5_api.evaluate_batch(spectrum=True)): kernel time and effective HBM rate at
the ERA5 frame size, its accuracy against numpy's float64 rfft, two yardsticks that are NOT in the product, then
evaluate_batch frames/s with and without spectrum=True on the same synthetic 268-channel frames, alternating.
  python tools/spectrum_bench.py [--kernel-only] [--frames 12] [--workers 12] [--reps 2]
--kernel-only: just the kernel loop (the run to put under `rocprofv3 --kernel-trace --stats --`).
Yardsticks, on the same frames: (1) torch.fft.rfft of the float64-cast frames on the device, reduced to the same three
spectra; (2) the host route - decode_batch to host arrays, then numpy.fft.rfft of truth, reconstruction and difference;
numpy is timed on --host-channels channels of one frame and extrapolated to 268 (the output says so)."""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from cra5_amd import metrics, ops, synth  # noqa: E402

C, H, W = 268, 721, 1440
K = W // 2 + 1


def _pair(dev, channels=C):
    g = torch.Generator(device=dev).manual_seed(0)
    x = 5e4 + 1e4 * torch.randn((channels, H, W), generator=g, device=dev)
    xh = x + 100 * torch.randn((channels, H, W), generator=g, device=dev)
    return xh, x


def _events(fn, iters, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def kernel_rate(dev, xh, x, iters=20):
    lat = torch.from_numpy(metrics.latitude_weights(H).astype(np.float32)).to(dev)
    out = torch.empty((3 * C * K + C,), device=dev, dtype=torch.float64)
    ms = _events(lambda: ops.zonal_spectrum(xh, x, lat, out=out), iters, 3)
    nbytes = 2 * C * H * W * 4
    # 1.5 complex transforms of W points per row (two real rows per transform, three spectra): 5 W log2 W flops each
    flop = 1.5 * C * H * 5.0 * W * np.log2(W)
    return dict(shape=[C, H, W], iters=iters, ms_per_call=ms, bytes=nbytes, tb_per_s=nbytes / (ms * 1e-3) / 1e12,
                fp64_gflop_nominal=flop / 1e9, fp64_tflop_per_s_nominal=flop / (ms * 1e-3) / 1e12,
                floor_ms_at_6_3_tb_per_s=nbytes / 6.3e12 * 1e3)


def accuracy(dev, xh, x, channels=4):
    """Worst |got - ref| / sqrt(ref(k) sum_k ref) over `channels` channels of the timed pair, against numpy's rfft."""
    got = metrics.zonal_spectrum(xh[:channels].contiguous(), x[:channels].contiguous())
    L = metrics.latitude_weights(H).astype(np.float32).astype(np.float64)
    a, b = xh[:channels].cpu().numpy(), x[:channels].cpu().numpy()
    m = np.full(K, 2.0)
    m[0] = m[-1] = 1.0
    worst = {}
    for name, f in (("power_truth", b), ("power_recon", a), ("power_error", a - b)):
        F = np.fft.rfft(f.astype(np.float64), axis=-1)
        ref = ((F.real ** 2 + F.imag ** 2) * L[None, :, None]).sum(axis=1) * m / (float(H) * W * W)
        worst[name] = float((np.abs(got[name] - ref) / np.sqrt(ref * ref.sum(axis=1, keepdims=True))).max())
    return dict(channels=channels, worst_ratio=worst, bound=2e-14)


def torch_fft_yardstick(dev, xh, x, iters=3):
    """torch.fft.rfft of the float64-cast frames, reduced to the same three spectra on the device (not in the product)."""
    lat = torch.from_numpy(metrics.latitude_weights(H).astype(np.float32)).to(dev).double()
    m = torch.full((K,), 2.0, device=dev, dtype=torch.float64)
    m[0] = m[-1] = 1.0

    def power(f):
        F = torch.fft.rfft(f.double(), dim=-1)
        return ((F.real ** 2 + F.imag ** 2) * lat[None, :, None]).sum(dim=1) * m / (float(H) * W * W)

    def run():
        return power(x), power(xh), power(xh - x)

    ms = _events(run, iters, 1)
    return dict(iters=iters, ms_per_call=ms, peak_alloc_gb=torch.cuda.max_memory_allocated() / 1e9)


def numpy_yardstick(frame_hat, frame, channels):
    a, b = frame_hat[:channels], frame[:channels]
    t0 = time.perf_counter()
    for f in (b, a, a - b):
        F = np.fft.rfft(f.astype(np.float64), axis=-1)
        (F.real ** 2 + F.imag ** 2).sum(axis=1)
    dt = time.perf_counter() - t0
    return dict(channels_timed=channels, seconds_timed=dt, seconds_per_frame_extrapolated=dt * C / channels,
                note=f"numpy.fft.rfft timed on {channels} of {C} channels of one frame, one thread, scaled by {C}/{channels}")


def sweep(dev, n, workers, reps, host_channels):
    from cra5_amd.api import cra5_api
    from cra5_amd.zoo import vaeformer_pretrained
    net = vaeformer_pretrained(quality=268, pretrained=False)
    synth.load_synthetic(net, seed=7)
    tmp = tempfile.mkdtemp()
    api = cra5_api(local_root=tmp, device="cuda", weights=net.to(dev))
    mean, std = api.get_mean_std()
    base = [(synth.synth_frame(C, seed=5 + i).numpy() * std[:, None, None] + mean[:, None, None]).astype(np.float32)
            for i in range(4)]
    data = [base[i % 4] for i in range(n)]
    stamps = [f"2024-06-{1 + i // 24:02d}T{i % 24:02d}:00:00" for i in range(n)]
    # warm-up of both paths (pipeline threads, per-thread workspaces, the twiddle table); it also writes the .bin files
    api.evaluate_batch(stamps, data=data, workers=workers, save_root=tmp + "/E")
    api.evaluate_batch(stamps[:workers], data=data[:workers], workers=workers, spectrum=True)
    rows = []
    for r in range(reps):
        for spectrum in (False, True):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rep = api.evaluate_batch(stamps, data=data, workers=workers, spectrum=spectrum)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            rows.append(dict(method="evaluate_batch", spectrum=spectrum, rep=r, frames=n, seconds=dt, frames_per_s=n / dt))
            print(json.dumps(rows[-1]), flush=True)
    # the host route: every reconstruction crosses the link, then numpy (sized down, extrapolated)
    paths = [f"{tmp}/E/{ts[:4]}/{ts}.bin" for ts in stamps]
    t0 = time.perf_counter()
    kept = api.decode_batch(paths=paths, workers=workers,
                            sink=lambda i, a: a[:host_channels].copy() if i == 0 else None)
    dt = time.perf_counter() - t0
    host = dict(decode_batch_to_host=dict(frames=n, seconds=dt, frames_per_s=n / dt),
                numpy_rfft=numpy_yardstick(kept[0], data[0], host_channels))
    print(json.dumps(host), flush=True)
    k = rep[0]["resolved_wavenumber"]
    return dict(rows=rows, host_route=host,
                example={"variables": rep[0]["variables"][:3], "resolved_wavenumber": k[:3].tolist(),
                         "power_error_k1": rep[0]["power_error"][:3, 1].tolist(),
                         "power_truth_k1": rep[0]["power_truth"][:3, 1].tolist()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--workers", type=int, default=12)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--host-channels", type=int, default=8)
    ap.add_argument("--out", default=None, help="write the JSON result here too")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    xh, x = _pair(dev)
    res = dict(kernel=kernel_rate(dev, xh, x))
    print(json.dumps(res["kernel"]), flush=True)
    if not a.kernel_only:
        res["accuracy"] = accuracy(dev, xh, x)
        print(json.dumps(res["accuracy"]), flush=True)
        res["torch_fft_yardstick"] = torch_fft_yardstick(dev, xh, x)
        print(json.dumps(res["torch_fft_yardstick"]), flush=True)
        del xh, x
        torch.cuda.empty_cache()
        res["sweep"] = sweep(dev, a.frames, a.workers, a.reps, a.host_channels)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
