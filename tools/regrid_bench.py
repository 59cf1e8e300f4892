"""Regridding (csrc/window_reduce.hip, regrid= of cra5_api): kernel time and HBM rate of cra5_regrid_f32 on a 268 x 721 x 1440
frame for three targets -
  (a) conservative onto coarsen=6's own 121 x 240 cells (bounds from grid_box(coarsen=6)), beside ops.coarsen on that grid;
  (b) conservative onto the 128 x 256 equiangular grid;
  (c) bilinear onto the cell-centred 720 x 1440 grid -
each beside the torch route that exists without the kernel, Rw @ (x.double() @ Cw.T) with dense fp64 weight matrices, in
the same run; then frames/s of decode_batch(regrid=(b)) against the plain decode_batch on synthetic full-size .bin files,
alternating.
    python tools/regrid_bench.py [--frames 24] [--workers 12] [--reps 3] [--runs 5] [--out FILE.json] [--txt FILE.txt]
GPU only.  The parent process never opens the GPU: every GPU step (`--step kernel`, `--step sweep`) is a child process
under its own `timeout`, and the first step that fails ends the run.  Every kernel figure is the median of `--runs` timed
loops after a warm-up, with the spread (min .. max) beside it."""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

C, H, W = 268, 721, 1440
STEP_TIMEOUT = {"kernel": 300, "sweep": 540}        # seconds, each with 10 s of grace before the kill


def _grids():
    from cra5_amd import subset
    from cra5_amd.regrid import Grid
    c6 = subset.grid_box((-90, 90, 0, 360), coarsen=6)
    return [("a", "conservative onto coarsen=6's 121 x 240 cells", Grid(c6["lat"], c6["lon"], "conservative", c6["lat_bnds"], c6["lon_bnds"])),
            ("b", "conservative onto 128 x 256 equiangular", Grid.equiangular(128, 256, method="conservative")),
            ("c", "bilinear onto cell-centred 720 x 1440", Grid.regular(0.25, 0.25))]


def _timed(torch, fn, iters, runs):
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


def _dense(plan):
    """The plan's tables as dense fp64 matrices Rw [Ho, H], Cw [Wo, W]."""
    Hg, Wg = plan["grid"]
    Rw, Cw = np.zeros((plan["Ho"], Hg)), np.zeros((plan["Wo"], Wg))
    for i in range(plan["Ho"]):
        for t in range(plan["ntap"][i]):
            Rw[i, plan["row0"][i] + t] += plan["rw"][i, t]
    for j in range(plan["Wo"]):
        for u in range(plan["ctap"][j]):
            Cw[j, (plan["col0"][j] + u) % Wg] += plan["cw"][j, u]
    return Rw, Cw


def _steps(plan, tiles):
    """(block, staged source row) steps of one launch on the whole frame - the launcher's chunks (csrc/window_reduce.hip): >= 4096
    blocks; a block stages every source row of its run of target rows once (the two kept inner), the rows two runs
    share again."""
    n_tiles = len(tiles)
    chunks = max(1, min(plan["Ho"], -(-4096 // (C * n_tiles))))
    rpb = -(-plan["Ho"] // chunks)
    order = plan["order"]
    rows = 0
    for k0 in range(0, plan["Ho"], rpb):
        kept, old = [None, None], 0
        for k in range(k0, min(plan["Ho"], k0 + rpb)):
            i = order[k]
            for t in range(plan["ntap"][i]):
                h = plan["row0"][i] + t
                if h not in kept:
                    kept[old] = h
                    old ^= 1
                    rows += 1
    return C * n_tiles * rows


def step_kernel(a):
    import torch
    from cra5_amd import ops, subset
    from cra5_amd.regrid import tile_table
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    x = 5e4 + 1e4 * torch.randn((C, H, W), generator=g, device=dev)
    rows = []
    for tag, what, grid in _grids():
        plan = grid.plan(H, W)
        assert plan["src_box"] == (0, H, 0, W)
        t = ops.regrid_tables(plan, dev)
        out = torch.empty((C, plan["Ho"], plan["Wo"]), device=dev)
        med, lo, hi = _timed(torch, lambda: ops.regrid(x, t, out=out), a.iters, a.runs)
        nbytes = 4 * (x.numel() + out.numel())
        tiles = tile_table(plan)[0]
        rows.append(dict(case=tag, kernel=f"regrid ({tag}) {what}", out=[C, plan["Ho"], plan["Wo"]], ms=med, ms_min=lo, ms_max=hi,
                         bytes=nbytes, tb_per_s=nbytes / (med * 1e-3) / 1e12, ntap=int(plan["ntap"].max()),
                         ctap=int(plan["ctap"].max()), tiles=len(tiles), steps=_steps(plan, tiles),
                         span_bytes=4 * int(tiles[:, 3].max())))
        if tag == "a":
            cp = subset.coarsen_plan(None, (6, 6), H, W)
            ct = ops.coarsen_tables(cp, dev)
            co = torch.empty_like(out)
            med, lo, hi = _timed(torch, lambda: ops.coarsen(x, ct, out=co), a.iters, a.runs)
            rows.append(dict(case=tag, kernel="coarsen k=6 (the same 121 x 240 cells)", ms=med, ms_min=lo, ms_max=hi, bytes=nbytes,
                             tb_per_s=nbytes / (med * 1e-3) / 1e12))
            d = (out.double() - co.double()).abs().max().item()
            rows[-1]["max_abs_diff_to_regrid"] = d
        Rw, Cw = (torch.from_numpy(m).to(dev) for m in _dense(plan))
        CwT = Cw.t().contiguous()
        route = lambda: torch.matmul(Rw, torch.matmul(x.double(), CwT))   # noqa: E731   (the cast is part of the route)
        med, lo, hi = _timed(torch, route, 2, a.runs)
        ref = route()
        rows.append(dict(case=tag, kernel=f"torch ({tag}) Rw @ (x.double() @ Cw.T), dense fp64", ms=med, ms_min=lo, ms_max=hi,
                         max_abs_diff_to_regrid=(ref - out.double()).abs().max().item()))
        del Rw, Cw, CwT, ref
        for r in rows[-3:]:
            if r["case"] == tag:
                print(json.dumps(r), flush=True)
    return rows


def step_sweep(a):
    import torch
    from cra5_amd import synth
    from cra5_amd.api import cra5_api
    from cra5_amd.zoo import vaeformer_pretrained
    dev = torch.device("cuda:0")
    n, workers = a.frames, a.workers
    grid = _grids()[1][2]
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
        discard = lambda i, fr: 0   # noqa: E731
        methods = {
            "decode_batch_full": lambda: api.decode_batch(paths=paths, workers=workers, sink=discard),
            "decode_batch_regrid_128x256": lambda: api.decode_batch(paths=paths, workers=workers, sink=discard, regrid=grid),
        }
        for fn in methods.values():      # warm-up: pipeline threads, per-thread workspaces, pinned buffers, the tables
            fn()
        rows = []
        for r in range(a.reps):
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


def report(res):
    lines = ["regrid_bench: cra5_regrid_f32 on a 268 x 721 x 1440 frame (median of the timed loops, min .. max)"]
    for k in res["kernel"]:
        rate = f"{k['tb_per_s']:6.2f} TB/s" if "tb_per_s" in k else " " * 11
        diff = f"   max |diff to regrid| {k['max_abs_diff_to_regrid']:.3g}" if "max_abs_diff_to_regrid" in k else ""
        lines.append(f"  {k['kernel']:<62s} {k['ms']:9.3f} ms  ({k['ms_min']:.3f} .. {k['ms_max']:.3f})  {rate}{diff}")
    lines.append("  a block stages ONE source row per step (loads -> barrier -> LDS -> barrier); steps and bytes per launch:")
    for k in (k for k in res["kernel"] if k["kernel"].startswith("regrid")):
        lines.append(f"    ({k['case']}) {k['tiles']:2d} column tiles, <= {k['ntap']:2d} x {k['ctap']:2d} taps: {k['steps']:8d} (block, row) steps of <= "
                     f"{k['span_bytes']:5d} B  ->  {k['ms'] * 1e6 / k['steps']:5.2f} ns per step chip-wide")
    by = {k["kernel"].split(" ")[0] + k["case"]: k for k in res["kernel"]}
    lines.append(f"  (a) against ops.coarsen on the same cells: {by['regrida']['ms'] / by['coarsena']['ms']:.2f} x its time")
    for tag in "abc":
        lines.append(f"  ({tag}) against the torch fp64 route: {by['torch' + tag]['ms'] / by['regrid' + tag]['ms']:.1f} x faster")
    if "sweep" in res:
        lines.append("frames/s (median over the repetitions, min .. max)")
        for name in dict.fromkeys(r["method"] for r in res["sweep"]):
            v = [r["frames_per_s"] for r in res["sweep"] if r["method"] == name]
            lines.append(f"  {name:<30s} {np.median(v):7.2f}  ({min(v):.2f} .. {max(v):.2f})   "
                         f"{res['sweep'][0]['frames']} frames, {res['sweep'][0]['workers']} workers")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEP_TIMEOUT), default=None, help="(internal) run one GPU step in this process")
    ap.add_argument("--json", default=None, help="(internal) where the step writes its rows")
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--workers", type=int, default=12)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None, help="write the JSON result here")
    ap.add_argument("--txt", default=None, help="write the text report here (profiles/regrid_bench.txt)")
    a = ap.parse_args()
    if a.step is not None:
        rows = step_kernel(a) if a.step == "kernel" else step_sweep(a)
        with open(a.json, "w") as f:
            json.dump(rows, f)
        return 0
    res = {}
    tmp = tempfile.mkdtemp()
    try:
        for step in ["kernel"] + ([] if a.kernel_only else ["sweep"]):
            path = os.path.join(tmp, step + ".json")
            cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT[step]), sys.executable, os.path.abspath(__file__), "--step", step,
                   "--json", path, "--frames", str(a.frames), "--workers", str(a.workers), "--reps", str(a.reps),
                   "--runs", str(a.runs), "--iters", str(a.iters)]
            rc = subprocess.call(cmd)
            if rc != 0:           # a fault, an abort or the time limit: nothing more is started on the GPU
                print(f"regrid_bench: step {step!r} ended with status {rc}; stopping", flush=True)
                return rc
            with open(path) as f:
                res[step] = json.load(f)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    txt = report(res)
    print(txt, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    if a.txt:
        with open(a.txt, "w") as f:
            f.write(txt)
    return 0


if __name__ == "__main__":
    sys.exit(main())
