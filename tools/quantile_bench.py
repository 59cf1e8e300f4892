"""Exact quantiles (csrc/quantile.hip, cra5_api.evaluate_batch(quantiles=)): the nine-launch radix select for Q = 1, 6 and
16 at the ERA5 frame size on SMOOTH synthetic frames (uniform noise would hide the first-digit contention), against the
metric's streaming pass over the same pair (one read of the pair) and the torch routes on the device (torch.sort of the
three fields, torch.kthvalue per quantile), all in one run, alternating; then evaluate_batch frames/s with and without
quantiles= on the same synthetic 268-channel frames, alternating.
  python tools/quantile_bench.py [--kernel-only] [--frames 12] [--workers 12] [--reps 2] [--out profiles/quantile_bench.txt]
--kernel-only: just the kernel rounds (the run to put under `rocprofv3 --kernel-trace --stats --` for the time per pass:
quantile_count_kernel<1, true> is the first digit, quantile_count_kernel<NS, false> the three later ones)."""
import argparse
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from cra5_amd import metrics, ops, synth  # noqa: E402

C, H, W = 268, 721, 1440
QS = {1: (0.999,), 6: (0.0001, 0.01, 0.5, 0.99, 0.9999, 1.0),
      16: (0.0, 1e-4, 1e-3, 0.01, 0.05, 0.1, 0.25, 0.4, 0.5, 0.6, 0.75, 0.9, 0.99, 0.999, 0.9999, 1.0)}
PASSES = 4
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def smooth_pair(dev):
    """Truth: mean 280, amplitude 30, smooth in both directions, a different phase per channel; x_hat = x + 0.3 N(0, 1)."""
    g = torch.Generator(device=dev).manual_seed(0)
    lat = torch.linspace(0.0, np.pi, H, device=dev).view(1, H, 1)
    lon = (torch.arange(W, device=dev) * (2 * np.pi / W)).view(1, 1, W)
    ph = torch.rand((C, 1, 1), generator=g, device=dev) * (2 * np.pi)
    x = (280.0 + 20.0 * torch.cos(lat + ph) + 10.0 * torch.sin(2 * lon + ph) * torch.sin(lat)).float().contiguous()
    xh = (x + 0.3 * torch.randn((C, H, W), generator=g, device=dev)).contiguous()
    return xh, x


def timed(fn, iters, warm):
    """ms per call: device events around `iters` calls after `warm` warm-up calls."""
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


def spread(v):
    return f"median {np.median(v):7.3f} ms  (min {min(v):.3f}, max {max(v):.3f}, {len(v)} rounds)"


def kernel_rounds(dev, rounds, iters, torch_routes=True):
    xh, x = smooth_pair(dev)
    lat = torch.from_numpy(metrics.latitude_weights(H).astype(np.float32)).to(dev)
    err_out = torch.empty((C, len(ops.RECON_FIELDS)), device=dev, dtype=torch.float64)
    plans = {n: metrics.quantile_plan(q, "era5", H, W, dev) for n, q in QS.items()}
    outs = {n: torch.empty((3 * C * n + C,), device=dev, dtype=torch.float64) for n in QS}
    calls = {"recon_error (one read of the pair)": lambda: ops.recon_error(xh, x, lat, out=err_out)}
    for n in QS:
        calls[f"frame_quantiles Q = {n:2d}"] = (lambda n=n: ops.frame_quantiles(xh, x, plans[n][0], plans[n][1], out=outs[n]))
    times = {k: [] for k in calls}
    for r in range(rounds):                       # alternating: every round times every call
        for k, fn in calls.items():
            times[k].append(timed(fn, iters, 3 if r == 0 else 1))
    nbytes = 2 * C * H * W * 4
    say(f"1. kernels, {C} x {H} x {W} smooth frames, \"era5\" weights; device events around {iters} calls, {rounds} "
        f"alternating rounds")
    base = float(np.median(times["recon_error (one read of the pair)"]))
    for k, v in times.items():
        m = float(np.median(v))
        extra = f"  {nbytes / (m * 1e-3) / 1e12:5.2f} TB/s of the pair" if k.startswith("recon") else \
            f"  = {m / (PASSES * base):4.2f} x ({PASSES} digit passes x the streaming pass)"
        say(f"   {k:36s} {spread(v)}{extra}")
    if not torch_routes:
        return
    # the torch routes on the device, Q = 6, unit weights (they have no weighted form); checked against the kernel
    q = QS[6]
    n = H * W
    ks = [min(n, max(1, int(np.ceil(p * float(n))))) for p in q]

    def fields():
        return (x.view(C, n), xh.view(C, n), (xh - x).abs_().view(C, n))

    def by_sort():
        return torch.stack([f.sort(dim=1).values[:, [k - 1 for k in ks]] for f in fields()])

    def by_kth():
        return torch.stack([torch.stack([f.kthvalue(k, dim=1).values for k in ks], dim=1) for f in fields()])
    want = metrics.frame_quantiles(xh, x, q, lat_weights=None)
    want = np.stack([want["quantile_" + k] for k in ops.QUANTILE_FIELDS])
    say()
    say(f"2. the torch routes on the device, Q = 6, unit weights, same run ({rounds} rounds of 2 calls, alternating with "
        f"the kernel)")
    plan_u = metrics.quantile_plan(q, None, H, W, dev)
    routes = {"frame_quantiles Q =  6, unit weights": lambda: ops.frame_quantiles(xh, x, None, plan_u[1], out=outs[6]),
              "torch.sort of the three fields": by_sort, "torch.kthvalue per field and quantile": by_kth}
    rt = {k: [] for k in routes}
    peak = {}
    for r in range(rounds):
        for k, fn in routes.items():
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            rt[k].append(timed(fn, 2, 1 if r == 0 else 0))
            peak[k] = max(peak.get(k, 0), torch.cuda.max_memory_allocated() - before)
    for k, fn in routes.items():
        if not k.startswith("frame"):
            got = fn().double().cpu().numpy() + 0.0
            assert np.array_equal(got, want + 0.0), k               # the same elements, bit for bit
        say(f"   {k:36s} {spread(rt[k])}  peak extra memory {peak[k] / 2 ** 30:6.2f} GiB")
    say("   (both torch routes return the kernel's values bit for bit)")


def sweep(dev, n, workers, reps):
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
    q = QS[6]
    api.evaluate_batch(stamps[:workers], data=data[:workers], workers=workers)              # warm-up of both forms
    api.evaluate_batch(stamps[:workers], data=data[:workers], workers=workers, quantiles=q)
    say()
    say(f"3. evaluate_batch, synthetic weights, {n} frames of {C} x {H} x {W}, workers={workers}, quantiles=None and "
        f"quantiles={q} alternating")
    for r in range(reps):
        for qq in (None, q):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rep = api.evaluate_batch(stamps, data=data, workers=workers, quantiles=qq)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            say(f"   quantiles={'None' if qq is None else 'Q = 6'}  rep {r}  {dt:6.3f} s  {n / dt:6.2f} frames/s")
    i = rep[0]["variables"].index("t2m") if "t2m" in rep[0]["variables"] else 0
    say(f"   example, {rep[0]['variables'][i]} at p = 0.9999: truth {rep[0]['quantile_truth'][i, 4]:.4f}, recon "
        f"{rep[0]['quantile_recon'][i, 4]:.4f}, shift {rep[0]['quantile_shift'][i, 4]:+.4f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--workers", type=int, default=12)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None, help="write the report here too")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    say("exact quantiles (csrc/quantile.hip), 1 x MI355X, synthetic data")
    say("python tools/quantile_bench.py" + (" --kernel-only" if a.kernel_only else ""))
    say()
    kernel_rounds(dev, a.rounds, a.iters, torch_routes=not a.kernel_only)
    torch.cuda.empty_cache()
    if not a.kernel_only:
        sweep(dev, a.frames, a.workers, a.reps)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
