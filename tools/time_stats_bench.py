"""Per-grid-point time statistics (csrc/timestats.hip, cra5_api.aggregate_batch): kernel time and HBM rate of the
accumulate kernel at the ERA5 frame size - all four statistics, then `mean` alone -, then frames/s of the ways to reduce
the same synthetic full-size .bin files over time, alternating:
  aggregate_batch                       the reduction on the GPU, only the statistics cross the host link (the timed call
                                        includes that final copy: four 1.11 GB arrays; aggregate_batch_device is the same
                                        call with to_host=False, the statistics left on the GPU)
  decode_batch(sink=discard)            the decode with its D2H and nothing else: the baseline
  decode_batch(sink=numpy accumulate)   float64 numpy accumulators of the same four statistics, updated in the sink
    python tools/time_stats_bench.py [--kernel-only] [--frames 24] [--workers 12] [--reps 2]
--kernel-only: just the kernel loops (the run to put under `rocprofv3 --kernel-trace --stats --`).
The sweep encodes 8 distinct synthetic frames and decodes `--frames` files built from them."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import threading
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from cra5_amd import ops, synth  # noqa: E402
from cra5_amd.timestats import TimeStats  # noqa: E402

C, H, W = 268, 721, 1440
BYTES = {"sum": 16, "sumsq": 16, "min": 8, "max": 8}      # read + write per point and frame


def kernel_rate(dev, stats, iters=20):
    g = torch.Generator(device=dev).manual_seed(0)
    x = 5e4 + 1e4 * torch.randn((C, H, W), generator=g, device=dev)
    ts = TimeStats((C, H, W), stats=stats, device=dev)
    ts.add(x)                                  # the first frame only stores
    for _ in range(3):
        ops.time_accumulate(x, ts.acc, first=False)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        ops.time_accumulate(x, ts.acc, first=False)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / iters
    per_point = 4 + sum(BYTES[k] for k in ts.acc)
    nbytes = C * H * W * per_point
    return dict(stats=list(ts.stats), shape=[C, H, W], iters=iters, ms_per_call=ms, bytes_per_point=per_point, bytes=nbytes,
                tb_per_s=nbytes / (ms * 1e-3) / 1e12)


class NumpySink:
    """The host-side reduction a user writes today: float64 sums, float32 extremes, one lock (the update is not atomic)."""

    def __init__(self):
        self.lock = threading.Lock()
        self.n = 0
        self.s = self.q = self.mn = self.mx = None

    def __call__(self, i, a):
        with self.lock:
            v = a.astype(np.float64)
            if self.n == 0:
                self.s, self.q, self.mn, self.mx = v, v * v, a.copy(), a.copy()
            else:
                self.s += v
                np.multiply(v, v, out=v)
                self.q += v
                np.minimum(self.mn, a, out=self.mn)
                np.maximum(self.mx, a, out=self.mx)
            self.n += 1
        return 0


def sweep(dev, n, workers, reps):
    from cra5_amd.api import cra5_api
    from cra5_amd.zoo import vaeformer_pretrained
    net = vaeformer_pretrained(quality=268, pretrained=False)
    synth.load_synthetic(net, seed=7)
    tmp = tempfile.mkdtemp()
    try:
        api = cra5_api(local_root=tmp, device="cuda", weights=net.to(dev))
        mean, std = api.get_mean_std()
        stamps8 = [f"2024-05-01T{i:02d}:00:00" for i in range(8)]
        base = [(synth.synth_frame(C, seed=5 + i).numpy() * std[:, None, None] + mean[:, None, None]).astype(np.float32)
                for i in range(8)]
        enc = api.encode_era5_batch(stamps8, data=base, save_root=tmp + "/CRA5", workers=min(workers, 8))
        del base
        paths = [enc[i % 8]["save_path"] for i in range(n)]
        # warm-up of both paths (pipeline threads, per-thread workspaces, pinned buffers)
        api.aggregate_batch(paths=paths[:workers], workers=workers)
        api.decode_batch(paths=paths[:workers], workers=workers, sink=lambda i, a: 0)
        rows, res = [], None
        for r in range(reps):
            for name in ("aggregate_batch", "aggregate_batch_device", "decode_batch_discard", "decode_batch_numpy"):
                if name == "aggregate_batch":
                    res = None          # (the previous result's 4.4 GB of host memory go back before the clock starts)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if name == "aggregate_batch":
                    res = api.aggregate_batch(paths=paths, workers=workers)
                elif name == "aggregate_batch_device":
                    on_dev = api.aggregate_batch(paths=paths, workers=workers, to_host=False)
                elif name == "decode_batch_discard":
                    api.decode_batch(paths=paths, workers=workers, sink=lambda i, a: 0)
                else:
                    api.decode_batch(paths=paths, workers=workers, sink=NumpySink())
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                on_dev = None
                rows.append(dict(method=name, rep=r, frames=n, workers=workers, seconds=dt, frames_per_s=n / dt))
                print(json.dumps(rows[-1]), flush=True)
        return dict(rows=rows, example={"variables": res["variables"][:2], "n": res["n"],
                                        "mean": res["mean"][:2, 360, 720].tolist(), "std": res["std"][:2, 360, 720].tolist()})
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--workers", type=int, default=12)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=None, help="write the JSON result here too")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = dict(kernel=[kernel_rate(dev, ("mean", "std", "min", "max")), kernel_rate(dev, ("mean",))])
    for k in res["kernel"]:
        print(json.dumps(k), flush=True)
    torch.cuda.empty_cache()
    if not a.kernel_only:
        res["sweep"] = sweep(dev, a.frames, a.workers, a.reps)
        print(json.dumps(res["sweep"]["example"]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
