"""Reconstruction-error metric (csrc/metrics.hip, cra5_api.evaluate_batch): kernel time and HBM rate at the ERA5 frame
size, then evaluate_batch vs roundtrip_batch frames/s on the same synthetic 268-channel frames, alternating.
  python tools/recon_error_bench.py [--kernel-only] [--frames 24] [--workers 12] [--reps 2]
--kernel-only: just the kernel loop (the run to put under `rocprofv3 --kernel-trace --stats --`).
The evaluation sweep holds `--frames` host frames built from 8 distinct synthetic ones (1.11 GB each)."""
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


def kernel_rate(dev, iters=50):
    g = torch.Generator(device=dev).manual_seed(0)
    x = 5e4 + 1e4 * torch.randn((C, H, W), generator=g, device=dev)
    xh = x + 100 * torch.randn((C, H, W), generator=g, device=dev)
    lat = torch.from_numpy(metrics.latitude_weights(H).astype(np.float32)).to(dev)
    out = torch.empty((C, len(ops.RECON_FIELDS)), device=dev, dtype=torch.float64)
    for _ in range(5):
        ops.recon_error(xh, x, lat, out=out)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        ops.recon_error(xh, x, lat, out=out)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / iters
    nbytes = 2 * C * H * W * 4
    return dict(shape=[C, H, W], iters=iters, ms_per_call=ms, bytes=nbytes, tb_per_s=nbytes / (ms * 1e-3) / 1e12)


def sweep(dev, n, workers, reps):
    from cra5_amd.api import cra5_api
    from cra5_amd.zoo import vaeformer_pretrained
    net = vaeformer_pretrained(quality=268, pretrained=False)
    synth.load_synthetic(net, seed=7)
    tmp = tempfile.mkdtemp()
    api = cra5_api(local_root=tmp, device="cuda", weights=net.to(dev))
    mean, std = api.get_mean_std()
    base = [(synth.synth_frame(C, seed=5 + i).numpy() * std[:, None, None] + mean[:, None, None]).astype(np.float32)
            for i in range(8)]
    data = [base[i % 8] for i in range(n)]
    stamps = [f"2024-06-{1 + i // 24:02d}T{i % 24:02d}:00:00" for i in range(n)]
    # warm-up of both paths (pipeline threads, per-thread workspaces, pinned buffers)
    api.evaluate_batch(stamps[:workers], data=data[:workers], workers=workers)
    api.roundtrip_batch(stamps[:workers], data=data[:workers], save_root=tmp + "/R", workers=workers, sink=lambda i, a: 0)
    rows = []
    for r in range(reps):
        for name in ("evaluate_batch", "roundtrip_batch"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if name == "evaluate_batch":
                rep = api.evaluate_batch(stamps, data=data, workers=workers)
            else:
                api.roundtrip_batch(stamps, data=data, save_root=tmp + "/R", workers=workers, sink=lambda i, a: 0)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            rows.append(dict(method=name, rep=r, frames=n, seconds=dt, frames_per_s=n / dt))
            print(json.dumps(rows[-1]), flush=True)
    wr = rep[0]["wrmse"]
    return dict(rows=rows, example={"variables": rep[0]["variables"][:3], "wrmse": wr[:3].tolist(),
                                    "compression_ratio": rep[0]["compression_ratio"]})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--workers", type=int, default=12)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=None, help="write the JSON result here too")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = dict(kernel=kernel_rate(dev))
    print(json.dumps(res["kernel"]), flush=True)
    if not a.kernel_only:
        res["sweep"] = sweep(dev, a.frames, a.workers, a.reps)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
