"""Area-weighted coarsening (csrc/window_reduce.hip, coarsen= of cra5_api): kernel time and HBM rate of cra5_coarsen_f32 on a
268 x 721 x 1440 frame at k = 2, 6 and 24 - beside this project's own streaming yardsticks on the same box in the same
run, the overlap-add (csrc/elementwise.hip), the reconstruction-error kernel (csrc/metrics.hip) and the time-statistics
accumulate (csrc/timestats.hip); below half of the overlap-add's rate the report says which limit was hit -, then
frames/s of decode_batch on synthetic full-size .bin files for the full frame, stride=6 and coarsen=6, and of
aggregate_batch(stats=("mean",)) with and without coarsen=6, alternating.
    python tools/coarsen_bench.py [--kernel-only] [--frames 24] [--workers 12] [--reps 3] [--out FILE.json] [--txt FILE.txt]
Every kernel figure is the median of `--runs` timed loops after a warm-up, with the spread (min .. max) beside it."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from cra5_amd import metrics, ops, subset, synth  # noqa: E402
from cra5_amd.timestats import TimeStats  # noqa: E402

C, H, W = 268, 721, 1440


def _timed(fn, iters, runs):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / iters)
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def kernel_rates(dev, iters=20, runs=5):
    g = torch.Generator(device=dev).manual_seed(0)
    x = 5e4 + 1e4 * torch.randn((C, H, W), generator=g, device=dev)
    rows = []
    for k in (2, 6, 24):
        plan = subset.coarsen_plan(None, (k, k), H, W)
        t = ops.coarsen_tables(plan, dev)
        out = torch.empty((C, plan["Ho"], plan["Wo"]), device=dev)
        med, lo, hi = _timed(lambda: ops.coarsen(x, t, out=out), iters, runs)
        nbytes = 4 * (x.numel() + out.numel())
        rows.append(dict(kernel=f"coarsen k={k}", out=[C, plan["Ho"], plan["Wo"]], ms=med, ms_min=lo, ms_max=hi, bytes=nbytes,
                         tb_per_s=nbytes / (med * 1e-3) / 1e12))
    # yardsticks: the project's own streaming kernels, same frame, same run
    y = x + 1.0
    med, lo, hi = _timed(lambda: metrics.reconstruction_error(y, x), 5, runs)    # (includes its small D2H of the results)
    rows.append(dict(kernel="recon_error (2 frames read)", ms=med, ms_min=lo, ms_max=hi, bytes=8 * x.numel(),
                     tb_per_s=8 * x.numel() / (med * 1e-3) / 1e12))
    # the overlap-add (csrc/elementwise.hip, cra5_col2im_f32) at the un-embed's shape: 72 x 144 tokens of 268 x 11 x 10
    # patches, stride 10 -> the same 268 x 721 x 1440 frame, de-normalised in the store as the decode runs it
    cols = torch.randn((72 * 144, C * 11 * 10), generator=g, device=dev)
    mean, std = torch.randn(C, generator=g, device=dev), 1.0 + torch.rand(C, generator=g, device=dev)
    med, lo, hi = _timed(lambda: ops.col2im(cols, C, 11, 10, 10, 10, 72, 144, mean=mean, std=std, out=y), iters, runs)
    nbytes = 4 * (cols.numel() + y.numel())
    rows.append(dict(kernel="overlap-add (column matrix read, frame written)", ms=med, ms_min=lo, ms_max=hi, bytes=nbytes,
                     tb_per_s=nbytes / (med * 1e-3) / 1e12))
    del cols
    ts = TimeStats((C, H, W), stats=("mean",), device=dev)
    ts.add(x)
    med, lo, hi = _timed(lambda: ops.time_accumulate(x, ts.acc, first=False), iters, runs)
    rows.append(dict(kernel="time_accumulate mean (4 B read, 16 B read + written per point)", ms=med, ms_min=lo, ms_max=hi,
                     bytes=20 * x.numel(), tb_per_s=20 * x.numel() / (med * 1e-3) / 1e12))
    return rows


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
        discard = lambda i, a: 0   # noqa: E731
        methods = {
            "decode_batch_full": lambda: api.decode_batch(paths=paths, workers=workers, sink=discard),
            "decode_batch_stride6": lambda: api.decode_batch(paths=paths, workers=workers, sink=discard, stride=6),
            "decode_batch_coarsen6": lambda: api.decode_batch(paths=paths, workers=workers, sink=discard, coarsen=6),
            "aggregate_mean_full": lambda: api.aggregate_batch(paths=paths, workers=workers, stats=("mean",)),
            "aggregate_mean_coarsen6": lambda: api.aggregate_batch(paths=paths, workers=workers, stats=("mean",), coarsen=6),
        }
        for name, fn in methods.items():      # warm-up: pipeline threads, per-thread workspaces, pinned buffers
            fn()
        rows = []
        for r in range(reps):
            for name, fn in methods.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                rows.append(dict(method=name, rep=r, frames=n, workers=workers, seconds=dt, frames_per_s=n / dt))
                print(json.dumps(rows[-1]), flush=True)
        return rows
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def _row_steps(Ho, Wo, k):
    """(block, source row) steps of one launch on the whole frame and the floats one step stages - the launcher's tiling
    (csrc/window_reduce.hip): tiles of <= 256 output columns, >= 4096 blocks, a shared edge row read again per run of rows."""
    span_max = 256 * 8 * 4 - 16
    tc = min((span_max - 2 * (k // 2) - 1) // k + 1, 256, Wo)
    n_tiles = -(-Wo // tc)
    chunks = max(1, min(Ho, -(-4096 // (C * n_tiles))))
    n_chunks = -(-Ho // -(-Ho // chunks))
    shared = n_chunks - 1 if k % 2 == 0 else 0
    return C * n_tiles * (H + shared), (tc - 1) * k + 2 * (k // 2) + 1


def report(res):
    lines = ["coarsen_bench: cra5_coarsen_f32 on a 268 x 721 x 1440 frame (median of the timed loops, min .. max)"]
    for k in res["kernel"]:
        lines.append(f"  {k['kernel']:<66s} {k['ms']:8.3f} ms  ({k['ms_min']:.3f} .. {k['ms_max']:.3f})  {k['tb_per_s']:6.2f} TB/s")
    # the yardstick the kernel is held against: half of the overlap-add's rate in this run; below it, which limit
    oa = next(k for k in res["kernel"] if k["kernel"].startswith("overlap-add"))["tb_per_s"]
    slow = [k for k in res["kernel"] if k["kernel"].startswith("coarsen") and k["tb_per_s"] < 0.5 * oa]
    if not slow:
        lines.append(f"  every coarsen launch runs above half of the overlap-add's rate ({0.5 * oa:.2f} TB/s)")
    else:
        lines.append(f"  BELOW half of the overlap-add's rate ({0.5 * oa:.2f} TB/s): " + ", ".join(k["kernel"] for k in slow))
        lines.append("  a block stages ONE source row per step (loads -> barrier -> LDS -> barrier); steps and bytes per launch:")
        for k in (k for k in res["kernel"] if k["kernel"].startswith("coarsen")):
            steps, span = _row_steps(k["out"][1], k["out"][2], int(k["kernel"].split("=")[1]))
            lines.append(f"    {k['kernel']:<14s} {steps:8d} (block, row) steps of {4 * span:5d} B  ->  {k['ms'] * 1e6 / steps:5.2f} ns per step "
                         f"chip-wide, {k['ms'] * 1e6 / steps * 2048 / 1e3:4.1f} us per step and block at (at most) 2048 resident blocks")
        lines.append("  if the ns per step agree while the bytes per step differ, the limit is the latency of a row step - the chain table")
        lines.append("  loads -> row loads -> two barriers, with one row in flight per block - not HBM, LDS or fp64 throughput")
    if "sweep" in res:
        lines.append("frames/s (median over the repetitions, min .. max)")
        for name in dict.fromkeys(r["method"] for r in res["sweep"]):
            v = [r["frames_per_s"] for r in res["sweep"] if r["method"] == name]
            lines.append(f"  {name:<28s} {np.median(v):7.2f}  ({min(v):.2f} .. {max(v):.2f})   "
                         f"{res['sweep'][0]['frames']} frames, {res['sweep'][0]['workers']} workers")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--workers", type=int, default=12)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None, help="write the JSON result here")
    ap.add_argument("--txt", default=None, help="write the text report here (profiles/coarsen_bench.txt)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = dict(kernel=kernel_rates(dev, runs=a.runs))
    for k in res["kernel"]:
        print(json.dumps(k), flush=True)
    torch.cuda.empty_cache()
    if not a.kernel_only:
        res["sweep"] = sweep(dev, a.frames, a.workers, a.reps)
    txt = report(res)
    print(txt, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    if a.txt:
        with open(a.txt, "w") as f:
            f.write(txt)


if __name__ == "__main__":
    main()
