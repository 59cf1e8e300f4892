"""Packed int16 input (csrc/pack.hip unpack_i16_kernel, PackedFrame / ingest= of cra5_api): kernel time and HBM rate of the
unpack pass (cra5_unpack_i16_f32; native and byte-swapped codes) on a 268 x 721 x 1440 frame beside cra5_pack_i16_f32 and the
yardstick of the same run - the reconstruction-error pass of csrc/metrics.hip over a frame pair -, then frames/s of
encode_era5_batch(data=PackedFrame list) against encode_era5_batch(data=float32 arrays) of the same frames, and of
encode_era5_batch(ingest="packed") against ingest="host" from NetCDF files written by decode_to_nc, alternating.
    python tools/ingest_bench.py [--kernel-only] [--frames 24] [--nc-frames 8] [--workers 12] [--reps 3] [--out FILE.json]
                                 [--txt FILE.txt]
Every kernel figure is the median of `--runs` timed loops after a warm-up, with the spread (min .. max) beside it.  The
NetCDF files were written just before they are read: they come out of the page cache, not off a disk."""
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

from cra5_amd import ops, pack, synth  # noqa: E402
from pack_bench import _timed  # noqa: E402

C, H, W = 268, 721, 1440


def kernel_rates(dev, iters=20, runs=5):
    g = torch.Generator(device=dev).manual_seed(0)
    x = 5e4 + 1e4 * torch.randn((C, H, W), generator=g, device=dev)
    y = x + 1.0
    n = x.numel()
    t5 = ops.pack_range(x)
    q = ops.pack_i16(x, t5)
    t4 = torch.stack([t5[:, 3], t5[:, 4], torch.full_like(t5[:, 0], -32768.0), torch.ones_like(t5[:, 0])], 1).contiguous()
    t4_tp = t4.clone()
    t4_tp[:, 3] = 1000.0
    out = torch.empty((C, H, W), device=dev)
    err = torch.empty((C, len(ops.RECON_FIELDS)), device=dev, dtype=torch.float64)
    rows = []

    def row(name, fn, nbytes):
        med, lo, hi = _timed(fn, iters, runs)
        rows.append(dict(kernel=name, ms=med, ms_min=lo, ms_max=hi, bytes=nbytes, tb_per_s=nbytes / (med * 1e-3) / 1e12))
    row("recon_error (yardstick: 2 frames read)", lambda: ops.recon_error(y, x, out=err), 8 * n)
    row("pack_i16 (1 frame read, int16 written)", lambda: ops.pack_i16(x, t5, out=q), 6 * n)
    row("unpack_i16 (int16 read, 1 frame written)", lambda: ops.unpack_i16(q, t4, out=out), 6 * n)
    row("unpack_i16, swapped codes", lambda: ops.unpack_i16(q, t4, swapped=True, out=out), 6 * n)
    row("unpack_i16, multiplier 1000", lambda: ops.unpack_i16(q, t4_tp, out=out), 6 * n)
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
        stamps = [f"2024-05-01T{i:02d}:00:00" for i in range(8)]
        base = [(synth.synth_frame(C, seed=5 + i).numpy() * std[:, None, None] + mean[:, None, None]).astype(np.float32)
                for i in range(8)]
        enc = api.encode_era5_batch(stamps, data=base, save_root=tmp + "/CRA5", workers=min(workers, 8))
        del base
        paths = [e["save_path"] for e in enc]
        nc_stamps = stamps[:n_nc]
        written = api.decode_to_nc(nc_stamps, paths=paths[:n_nc], workers=workers)          # -> {tmp}/ERA5/2024/
        nc_bytes = sum(r["bytes"] for r in written) / len(written)
        # the same frames as PackedFrame and as float32 arrays: the packed decodes and their host unpacking
        packed = [pack.PackedFrame.from_decode(d) for d in api.decode_batch(paths=paths, workers=workers, pack="int16")]
        floats = [pack.unpack_f32(f) for f in packed]
        pf = [packed[i % 8] for i in range(n)]
        xf = [floats[i % 8] for i in range(n)]
        names = [stamps[i % 8] for i in range(n)]
        nc_names = [nc_stamps[i % n_nc] for i in range(n)]      # (every file several times: n frames per call here too)

        def batch(**kw):
            return api.encode_era5_batch(workers=workers, write=False, **kw)
        methods = {
            "encode_batch data=float32": (n, lambda: batch(time_stamps=names, data=xf)),
            "encode_batch data=PackedFrame": (n, lambda: batch(time_stamps=names, data=pf)),
            "encode_batch ingest=host": (n, lambda: batch(time_stamps=nc_names, ingest="host")),
            "encode_batch ingest=packed": (n, lambda: batch(time_stamps=nc_names, ingest="packed")),
        }
        same = [a["output"]["strings"] == b["output"]["strings"]
                for a, b in zip(methods["encode_batch ingest=host"][1](), methods["encode_batch ingest=packed"][1]())]
        same += [a["output"]["strings"] == b["output"]["strings"]
                 for a, b in zip(methods["encode_batch data=float32"][1](), methods["encode_batch data=PackedFrame"][1]())]
        rows = []
        for r in range(reps):
            for name, (m, fn) in methods.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                rows.append(dict(method=name, rep=r, frames=m, workers=workers, seconds=dt, frames_per_s=m / dt))
                print(json.dumps(rows[-1]), flush=True)
        # one more call each with the API's phase log on: mean host-side ms per frame and phase (cra5_api._log / _link)
        phases = {}
        for name, (m, fn) in methods.items():
            api.phase_log = []
            encs = fn()
            tot = dict(read_files=sum(e["reading_time"] for e in encs))
            for _, phase, a, b in api.phase_log:
                tot[phase] = tot.get(phase, 0.0) + (b - a)
            phases[name] = {k: 1e3 * v / m for k, v in sorted(tot.items())}
            api.phase_log = None
        return rows, dict(identical_streams=bool(all(same)), compared=len(same), nc_bytes_per_frame=nc_bytes, nc_files=n_nc,
                          phase_ms_per_frame=phases)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def report(res):
    lines = ["ingest_bench: cra5_unpack_i16_f32 on a 268 x 721 x 1440 frame (median of the timed loops, min .. max)"]
    for k in res["kernel"]:
        lines.append(f"  {k['kernel']:<44s} {k['ms']:8.3f} ms  ({k['ms_min']:.3f} .. {k['ms_max']:.3f})  "
                     f"{k['bytes'] / 1e9:5.2f} GB  {k['tb_per_s']:6.2f} TB/s")
    yard = min(k["ms"] for k in res["kernel"] if k["kernel"].startswith("recon_error"))
    for k in (k for k in res["kernel"] if "pack_i16" in k["kernel"]):
        # the bytes of the pass at the yardstick's rate: what HBM alone would take
        hbm = k["bytes"] / (8 * C * H * W) * yard
        lines.append(f"  {k['kernel'].split(' (')[0]:<30s} {k['ms'] / yard:.2f} x the recon_error pass of this run; its "
                     f"{k['bytes'] / 1e9:.2f} GB at the yardstick's rate take {hbm:.3f} ms ({k['ms'] / hbm:.2f} x)")
    if "sweep" in res:
        lines.append("frames/s (median over the repetitions, min .. max)")
        med = {}
        for name in dict.fromkeys(r["method"] for r in res["sweep"]):
            rs = [r for r in res["sweep"] if r["method"] == name]
            v = [r["frames_per_s"] for r in rs]
            med[name] = float(np.median(v))
            lines.append(f"  {name:<32s} {med[name]:7.2f}  ({min(v):.2f} .. {max(v):.2f})   {rs[0]['frames']} frames, "
                         f"{rs[0]['workers']} workers")
        lines.append(f"  data=PackedFrame / data=float32: {med['encode_batch data=PackedFrame'] / med['encode_batch data=float32']:.2f} x;  "
                     f"ingest=packed / ingest=host: {med['encode_batch ingest=packed'] / med['encode_batch ingest=host']:.2f} x")
        info = res["sweep_info"]
        lines.append(f"  the rANS strings of the two routes are identical: {info['identical_streams']} ({info['compared']} frames "
                     f"compared); {info['nc_files']} frames of NetCDF files, {info['nc_bytes_per_frame'] / 1e6:.0f} MB each, "
                     f"read from the page cache")
        lines.append("host-side ms per frame and phase, summed over the frame threads (one more call each, phase log on)")
        for name, ph in info["phase_ms_per_frame"].items():
            lines.append(f"  {name:<32s} " + "  ".join(f"{k} {v:.1f}" for k, v in ph.items()))
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--nc-frames", type=int, default=8)
    ap.add_argument("--workers", type=int, default=12)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None, help="write the JSON result here")
    ap.add_argument("--txt", default=None, help="write the text report here (profiles/ingest_bench.txt)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = dict(kernel=kernel_rates(dev, runs=a.runs))
    for k in res["kernel"]:
        print(json.dumps(k), flush=True)
    torch.cuda.empty_cache()
    if not a.kernel_only:
        res["sweep"], res["sweep_info"] = sweep(dev, a.frames, min(a.nc_frames, 8), a.workers, a.reps)
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
