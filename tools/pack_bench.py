"""Packed int16 output (csrc/pack.hip, pack= of cra5_api, decode_to_nc): kernel time and HBM rate of the range pass
(cra5_pack_range_f32) and the pack pass (cra5_pack_i16_f32) on a 268 x 721 x 1440 frame, beside the yardstick in the same
run - the reconstruction-error pass of csrc/metrics.hip over a frame pair (2.2 GB read; the range pass moves half of that,
the pack pass three quarters) -, then frames/s of decode_batch(pack="int16") against the plain decode_batch, alternating,
and of decode_to_nc, on synthetic full-size .bin files.
    python tools/pack_bench.py [--kernel-only] [--frames 24] [--nc-frames 4] [--workers 12] [--reps 3] [--out FILE.json]
                               [--txt FILE.txt]
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

from cra5_amd import ops, synth  # noqa: E402

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
    y = x + 1.0
    n = x.numel()
    table = torch.empty((C, len(ops.PACK_FIELDS)), device=dev, dtype=torch.float64)
    q = torch.empty((C, H, W), device=dev, dtype=torch.int16)
    err = torch.empty((C, len(ops.RECON_FIELDS)), device=dev, dtype=torch.float64)
    fixed = torch.tensor([[0.0, 1e5]] * C, device=dev, dtype=torch.float64)
    rows = []

    def row(name, fn, nbytes):
        med, lo, hi = _timed(fn, iters, runs)
        rows.append(dict(kernel=name, ms=med, ms_min=lo, ms_max=hi, bytes=nbytes, tb_per_s=nbytes / (med * 1e-3) / 1e12))
    row("recon_error (yardstick: 2 frames read)", lambda: ops.recon_error(y, x, out=err), 8 * n)
    row("pack_range (1 frame read)", lambda: ops.pack_range(x, out=table), 4 * n)
    row("pack_range, fixed ranges (1 frame read)", lambda: ops.pack_range(x, fixed, out=table), 4 * n)
    ops.pack_range(x, out=table)
    row("pack_i16 (1 frame read, int16 written)", lambda: ops.pack_i16(x, table, out=q), 6 * n)
    row("recon_error again (drift of the run)", lambda: ops.recon_error(y, x, out=err), 8 * n)
    return rows


def sweep(dev, n, n_nc, workers, reps):
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
        nc_stamps = stamps8[:n_nc]
        discard = lambda i, a: 0   # noqa: E731
        nc_bytes = []

        def to_nc():
            res = api.decode_to_nc(nc_stamps, paths=paths[:n_nc], save_root=tmp + "/nc", workers=workers)
            nc_bytes.append(sum(r["bytes"] for r in res) / len(res))
            shutil.rmtree(tmp + "/nc", ignore_errors=True)
        methods = {
            "decode_batch_fp32": (n, lambda: api.decode_batch(paths=paths, workers=workers, sink=discard)),
            "decode_batch_pack_int16": (n, lambda: api.decode_batch(paths=paths, workers=workers, sink=discard, pack="int16")),
            "decode_to_nc": (n_nc, to_nc),
        }
        for name, (_, fn) in methods.items():      # warm-up: pipeline threads, per-thread workspaces, pinned buffers
            fn()
        rows = []
        for r in range(reps):
            for name, (m, fn) in methods.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                rows.append(dict(method=name, rep=r, frames=m, workers=workers, seconds=dt, frames_per_s=m / dt))
                if name == "decode_to_nc":
                    rows[-1]["nc_bytes_per_frame"] = nc_bytes[-1]
                print(json.dumps(rows[-1]), flush=True)
        return rows
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def report(res):
    lines = ["pack_bench: cra5_pack_range_f32 / cra5_pack_i16_f32 on a 268 x 721 x 1440 frame (median of the timed loops, min .. max)"]
    for k in res["kernel"]:
        lines.append(f"  {k['kernel']:<44s} {k['ms']:8.3f} ms  ({k['ms_min']:.3f} .. {k['ms_max']:.3f})  {k['tb_per_s']:6.2f} TB/s")
    yard = min(k["ms"] for k in res["kernel"] if k["kernel"].startswith("recon_error"))
    for k in (k for k in res["kernel"] if k["kernel"].startswith("pack_")):
        verdict = "not slower than" if k["ms"] <= yard else "SLOWER than"
        lines.append(f"  {k['kernel'].split(' (')[0]:<28s} {verdict} the recon_error pass of this run ({k['ms'] / yard:.2f} x its time)")
    for k in (k for k in res["kernel"] if k["kernel"].startswith("pack_") and k["ms"] > yard):
        # the bytes of the pass at the yardstick's rate: what HBM alone would take; the rest is issue time
        hbm = k["bytes"] / (8 * C * H * W) * yard
        lines.append(f"    {k['kernel'].split(' (')[0]}: its bytes at the yardstick's rate take {hbm:.3f} ms; the other "
                     f"{k['ms'] - hbm:.3f} ms are instruction issue" + (" - per element one float64 division (scale, reciprocal, "
                     "fused multiply-adds, fix-up), a subtraction, rint, two clamps and the conversion"
                                                                         if k["kernel"].startswith("pack_i16") else ""))
    if "sweep" in res:
        lines.append("frames/s (median over the repetitions, min .. max)")
        for name in dict.fromkeys(r["method"] for r in res["sweep"]):
            rs = [r for r in res["sweep"] if r["method"] == name]
            v = [r["frames_per_s"] for r in rs]
            lines.append(f"  {name:<28s} {np.median(v):7.2f}  ({min(v):.2f} .. {max(v):.2f})   {rs[0]['frames']} frames, "
                         f"{rs[0]['workers']} workers" + (f", {rs[0]['nc_bytes_per_frame'] / 1e6:.0f} MB of NetCDF per frame"
                                                          if "nc_bytes_per_frame" in rs[0] else ""))
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--nc-frames", type=int, default=4)
    ap.add_argument("--workers", type=int, default=12)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None, help="write the JSON result here")
    ap.add_argument("--txt", default=None, help="write the text report here (profiles/pack_bench.txt)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = dict(kernel=kernel_rates(dev, runs=a.runs))
    for k in res["kernel"]:
        print(json.dumps(k), flush=True)
    torch.cuda.empty_cache()
    if not a.kernel_only:
        res["sweep"] = sweep(dev, a.frames, min(a.nc_frames, 8), a.workers, a.reps)
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
