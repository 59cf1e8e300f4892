"""Residual layer (csrc/residual.hip, cra5_api max_error= / residual=): kernel times at the ERA5 frame size for record
densities of about 0.1 %, 1 % and 10 %, the sidecar size per density, and the pipeline rates with and without the layer.
  python tools/residual_bench.py [--kernel-only] [--frames 12] [--workers 12] [--reps 2] [--out FILE]
Yardstick of the streaming passes: metrics.hip's single pass over the same pair of frames, timed in the same run.
The pipeline sweep alternates encode_era5_batch(max_error=) with roundtrip_batch (the new encode does a round trip's GPU work
plus the residual) and decode_batch(residual=True) with decode_batch, on the same synthetic 268-channel frames."""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from cra5_amd import _lib, metrics, ops, residual, synth  # noqa: E402

C, H, W = 268, 721, 1440
SIGMA = 100.0
DENSITIES = {"0.1%": 3.2905, "1%": 2.5758, "10%": 1.6449}      # tol = z * sigma: P(|d| > tol) for Gaussian d


def _timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def kernels(dev, iters=20):
    g = torch.Generator(device=dev).manual_seed(0)
    x = 5e4 + 1e4 * torch.randn((C, H, W), generator=g, device=dev)
    xh = x + SIGMA * torch.randn((C, H, W), generator=g, device=dev)
    frame_bytes = 2 * C * H * W * 4
    lat = torch.from_numpy(metrics.latitude_weights(H).astype(np.float32)).to(dev)
    out = torch.empty((C, len(ops.RECON_FIELDS)), device=dev, dtype=torch.float64)
    ms = _timed(lambda: ops.recon_error(xh, x, lat, out=out), iters)
    rows = [dict(kernel="recon_error (yardstick)", ms=ms, tb_per_s=frame_bytes / (ms * 1e-3) / 1e12)]
    print(json.dumps(rows[-1]), flush=True)
    L, st = _lib.lib(), ops._stream()
    S = L.cra5_residual_spans(C, H, W)
    counts = torch.empty((S, 2), device=dev, dtype=torch.int32)
    offs = torch.empty((S + 1, 2), device=dev, dtype=torch.int32)
    chan = torch.empty((C, 2), device=dev, dtype=torch.int64)
    for name, z in DENSITIES.items():
        tol = np.full(C, z * SIGMA, dtype=np.float32)
        tol_d = torch.from_numpy(tol).to(dev)
        idx, q, eidx, ebits, per = ops.residual_quantize(x, xh, tol)
        n, m = len(idx), len(eidx)
        t_count = _timed(lambda: L.cra5_residual_count_f32(x.data_ptr(), xh.data_ptr(), tol_d.data_ptr(), C, H, W,
                                                           counts.data_ptr(), st), iters)
        t_scan = _timed(lambda: L.cra5_residual_scan(counts.data_ptr(), C, H, W, offs.data_ptr(), chan.data_ptr(), st), iters)
        t_emit = _timed(lambda: L.cra5_residual_emit_f32(x.data_ptr(), xh.data_ptr(), tol_d.data_ptr(), C, H, W,
                                                         offs.data_ptr(), idx.data_ptr(), q.data_ptr(), n,
                                                         eidx.data_ptr() if m else None, ebits.data_ptr() if m else None, m,
                                                         st), iters)
        work = xh.clone()
        step = torch.from_numpy(np.float32(2) * tol).to(dev)
        t_apply = _timed(lambda: ops.residual_apply(work, (idx, q, eidx, ebits), step, (C, H, W)), iters)
        del work
        t0 = time.perf_counter()
        widx = residual.witness_indices(C, H, W)
        blob = residual.pack(C, H, W, tol, widx, np.zeros(len(widx), np.uint32), idx.cpu().numpy().view(np.uint32),
                             q.cpu().numpy(), eidx.cpu().numpy().view(np.uint32), ebits.cpu().numpy().view(np.uint32))
        t_pack = time.perf_counter() - t0
        t0 = time.perf_counter()
        residual.unpack(blob)
        t_unpack = time.perf_counter() - t0
        rows.append(dict(density=name, records=n, escapes=m, share=(n + m) / (C * H * W),
                         count_ms=t_count, count_tb_per_s=frame_bytes / (t_count * 1e-3) / 1e12,
                         scan_ms=t_scan, emit_ms=t_emit, emit_tb_per_s=frame_bytes / (t_emit * 1e-3) / 1e12,
                         apply_ms=t_apply, apply_records_per_us=(n + m) / (t_apply * 1e3),
                         sidecar_bytes=len(blob), bytes_per_record=len(blob) / max(1, n + m),
                         host_pack_s=t_pack, host_unpack_s=t_unpack))
        print(json.dumps(rows[-1]), flush=True)
    return rows


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
    plain = api.evaluate_batch(stamps[:1], data=data[:1], workers=1)[0]
    # every variable at 2.58 x its own rmse: about 1 % of the points if the codec error were Gaussian
    max_error = {v: 2.5758 * float(r) for v, r in zip(plain["variables"], plain["rmse"])}
    root = tmp + "/CRA5"
    enc = api.encode_era5_batch(stamps[:workers], data=data[:workers], save_root=root, workers=workers, max_error=max_error)
    api.roundtrip_batch(stamps[:workers], data=data[:workers], save_root=tmp + "/R", workers=workers, sink=lambda i, a: 0)
    r0 = enc[0]["residual"]
    info = dict(records=r0["records"], escapes=r0["escapes"], share=(r0["records"] + r0["escapes"]) / (C * H * W),
                res_bytes=r0["bytes"], bin_bytes=os.path.getsize(enc[0]["save_path"]))
    print(json.dumps(info), flush=True)
    rows = []

    def run(name, fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        rows.append(dict(method=name, frames=n, seconds=dt, frames_per_s=n / dt))
        print(json.dumps(rows[-1]), flush=True)

    for _ in range(reps):
        run("encode_era5_batch(max_error)", lambda: api.encode_era5_batch(stamps, data=data, save_root=root, workers=workers,
                                                                          max_error=max_error))
        run("roundtrip_batch", lambda: api.roundtrip_batch(stamps, data=data, save_root=tmp + "/R", workers=workers,
                                                           sink=lambda i, a: 0))
    paths = [e["save_path"] for e in enc]
    paths = [paths[i % len(paths)] for i in range(n)]
    api.decode_batch(paths=paths[:workers], workers=workers, sink=lambda i, a: 0, residual=True)
    for _ in range(reps):
        run("decode_batch(residual=True)", lambda: api.decode_batch(paths=paths, workers=workers, sink=lambda i, a: 0,
                                                                    residual=True))
        run("decode_batch", lambda: api.decode_batch(paths=paths, workers=workers, sink=lambda i, a: 0))
    return dict(sidecar=info, rows=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--workers", type=int, default=12)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=None, help="write the JSON result here too")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = dict(kernels=kernels(dev))
    if not a.kernel_only:
        torch.cuda.empty_cache()
        res["sweep"] = sweep(dev, a.frames, a.workers, a.reps)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
