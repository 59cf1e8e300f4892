"""Point decode (points= of cra5_api, csrc/points.hip): what a station list costs beside the full frame.
  sweep   frames/s of decode_batch of full frames, decode_batch(points=) and series_batch on synthetic full-size .bin files
          of the 268 model, for P = 100 and P = 10 000 random points, all variables and six, alternating over the
          repetitions after one warm-up pass;
  routes  GPU time of the un-embed step alone (VAEformer._unembed_points on one frame's final LayerNorm output, event
          bracket round the step's launches) on the sparse and on the dense route at several token counts M, to place
          VAEformer.POINT_DENSE_TOKENS.
    python tools/points_bench.py [--frames 24] [--workers 12] [--reps 3] [--runs 5] [--out FILE.json] [--txt FILE.txt]
GPU only.  The parent process never opens the GPU: every GPU step is a child process under its own `timeout`, and the first
step that fails ends the run.  Every figure is a median with its spread (min .. max) beside it."""
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
SIX = ["z_500", "q_500", "u_500", "v_500", "t_500", "w_500"]
STEP_TIMEOUT = {"sweep": 600, "routes": 420}        # seconds, each with 10 s of grace before the kill


def _model(dev):
    from cra5_amd import synth
    from cra5_amd.zoo import vaeformer_pretrained
    net = vaeformer_pretrained(quality=268, pretrained=False)
    synth.load_synthetic(net, seed=7)
    return net.to(dev)


def _random_points(P, seed):
    from cra5_amd.points import Points
    rng = np.random.default_rng(seed)
    # uniform on the sphere, as stations are not: the worst case for the token count
    return Points(np.rad2deg(np.arcsin(rng.uniform(-1, 1, P))), rng.uniform(0, 360, P))


def step_sweep(a):
    import torch
    from cra5_amd import synth
    from cra5_amd.api import cra5_api
    dev = torch.device("cuda:0")
    n, workers = a.frames, a.workers
    tmp = tempfile.mkdtemp()
    try:
        api = cra5_api(local_root=tmp, device="cuda", weights=_model(dev))
        mean, std = api.get_mean_std()
        stamps8 = [f"2024-05-01T{i:02d}:00:00" for i in range(8)]
        base = [(synth.synth_frame(C, seed=5 + i).numpy() * std[:, None, None] + mean[:, None, None]).astype(np.float32)
                for i in range(8)]
        enc = api.encode_era5_batch(stamps8, data=base, save_root=tmp + "/CRA5", workers=min(workers, 8))
        del base
        paths = [enc[i % 8]["save_path"] for i in range(n)]
        discard = lambda i, fr: 0   # noqa: E731
        methods = {"decode_batch full frames": lambda: api.decode_batch(paths=paths, workers=workers, sink=discard)}
        tokens = {}
        for P in (100, 10000):
            pts = _random_points(P, seed=P)
            tokens[P] = len(pts.plan(H, W)["tokens"])
            for tag, names in (("all 268 variables", None), ("six variables", SIX)):
                methods[f"decode_batch(points=) P={P}, {tag}"] = \
                    lambda pts=pts, names=names: api.decode_batch(paths=paths, workers=workers, sink=discard, points=pts, variables=names)
                methods[f"series_batch P={P}, {tag}"] = \
                    lambda pts=pts, names=names: api.series_batch(paths=paths, workers=workers, points=pts, variables=names)
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
                rows.append(dict(method=name, rep=r, frames=n, workers=workers, seconds=dt, frames_per_s=n / dt, tokens=tokens))
                print(json.dumps(rows[-1]), flush=True)
        return rows
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def step_routes(a):
    import torch
    from cra5_amd.api import variable_mapping
    from cra5_amd.points import Points
    from cra5_amd.subset import resolve_variables
    dev = torch.device("cuda:0")
    net = _model(dev)
    g = torch.Generator().manual_seed(5)
    y = (torch.round(2.0 * torch.randn(256, 72, 144, generator=g)) + torch.randn(256, 72, 144, generator=g)).to(dev)
    six = tuple(resolve_variables(SIX, variable_mapping()[1]))
    held = {}
    real = net._unembed

    def capture(h, *args, **kw):         # the final LayerNorm's output of one frame, on this thread's workspace
        held["h"] = h
        return real(h, *args, **kw)
    net._unembed = capture
    with torch.no_grad():
        net._decode_frame(y, channels=six)
    net._unembed = real
    h = held["h"]
    rng = np.random.default_rng(0)
    Hp, Wp = net.Hp, net.Wp
    rows = []
    for M in (100, 1000, 3000, 6000, 9438, Hp * Wp):
        tok = np.sort(rng.choice(Hp * Wp, M, replace=False))
        # the centre node of each chosen token: M points, M tokens
        pts = Points(90.0 - (10 * (tok // Wp) + 5) * 0.25, (10 * (tok % Wp) + 5) * 0.25, "nearest")
        plan = net._points_arg(pts)
        assert len(plan["tokens"]) == M
        for chans, tag in ((six, "six variables"), (None, "all 268 variables")):
            for route, bound in (("sparse", Hp * Wp), ("dense", 0)):
                net.POINT_DENSE_TOKENS = bound

                def fn():
                    with torch.no_grad():
                        return net._unembed_points(h, None, None, chans, plan)
                for _ in range(2):
                    fn()
                torch.cuda.synchronize()
                ms = []
                for _ in range(a.runs):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    torch.cuda.synchronize()
                    ms.append(e0.elapsed_time(e1))
                rows.append(dict(tokens=M, channels=tag, route=route, ms=float(np.median(ms)), ms_min=min(ms), ms_max=max(ms)))
                print(json.dumps(rows[-1]), flush=True)
    del net.POINT_DENSE_TOKENS
    return rows


def report(res):
    lines = []
    if "sweep" in res:
        s = res["sweep"]
        lines.append(f"points_bench: frames/s on {s[0]['frames']} full-size .bin files of the 268 model, {s[0]['workers']} workers "
                     "(median over the repetitions after one warm-up pass, min .. max)")
        lines.append("  random points, uniform on the sphere: " +
                     ", ".join(f"P = {P}: {m} of 10368 tokens" for P, m in s[0]["tokens"].items()))
        for name in dict.fromkeys(r["method"] for r in s):
            v = [r["frames_per_s"] for r in s if r["method"] == name]
            lines.append(f"  {name:<52s} {np.median(v):7.2f}  ({min(v):.2f} .. {max(v):.2f})")
    if "routes" in res:
        lines.append("un-embed step of one frame, GPU ms between events (median of the runs, min .. max): sparse = token gather + "
                     "two-call GEMM + points_from_cols, dense = whole-grid un-embed + points_from_image")
        for r in res["routes"]:
            lines.append(f"  M = {r['tokens']:5d} tokens, {r['channels']:<18s} {r['route']:<6s} {r['ms']:8.3f} ms  "
                         f"({r['ms_min']:.3f} .. {r['ms_max']:.3f})")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEP_TIMEOUT), default=None, help="(internal) run one GPU step in this process")
    ap.add_argument("--json", default=None, help="(internal) where the step writes its rows")
    ap.add_argument("--only", choices=sorted(STEP_TIMEOUT), default=None, help="run this step alone")
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--workers", type=int, default=12)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None, help="write the JSON result here")
    ap.add_argument("--txt", default=None, help="write the text report here (profiles/points_bench.txt)")
    a = ap.parse_args()
    if a.step is not None:
        rows = step_sweep(a) if a.step == "sweep" else step_routes(a)
        with open(a.json, "w") as f:
            json.dump(rows, f)
        return 0
    res = {}
    tmp = tempfile.mkdtemp()
    try:
        for step in ([a.only] if a.only else ["sweep", "routes"]):
            path = os.path.join(tmp, step + ".json")
            cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT[step]), sys.executable, os.path.abspath(__file__), "--step", step,
                   "--json", path, "--frames", str(a.frames), "--workers", str(a.workers), "--reps", str(a.reps),
                   "--runs", str(a.runs)]
            rc = subprocess.call(cmd)
            if rc != 0:           # a fault, an abort or the time limit: nothing more is started on the GPU
                print(f"points_bench: step {step!r} ended with status {rc}; stopping", flush=True)
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
