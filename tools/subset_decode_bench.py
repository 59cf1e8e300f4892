"""Subset decode throughput and kernel split (268 model, synthetic weights).

  python tools/subset_decode_bench.py [--frames 24] [--workers 12] [--repeats 1] [--out FILE]
      decode_batch frames/s on the same .bin files (written once by encode_era5_batch from host frames) in five cases:
      full frames; six 500 hPa variables over the globe; the same six over Europe (35-72 N, -25-45 E); all 268 variables
      thinned by stride 4 (the 1 deg grid, 181 x 360) and by stride 6 (1.5 deg, 121 x 240) over the globe.  Every frame
      goes .bin -> rANS -> g_s -> D2H -> a host consumer that copies it into its own pageable array (bench.py
      api_pipelined).  One warm-up pass per case, then the timed pass; --repeats N times the pass N times and reports
      every rate (`repeats`: the run-to-run spread; `frames_per_s` stays the first timed pass).  Prints / writes one JSON
      object.
  python tools/subset_decode_bench.py --profile
      two full decodes, two Europe six-variable decodes, then two stride-6 decodes (all variables, globe) of one latent
      (de-normalised): the workload of a `rocprofv3 --kernel-trace --stats` run that splits one subset decode into gather /
      un-embed GEMM / fix-up / crop and one thinned decode into lattice gathers / class GEMMs / scatter.
"""
import argparse
import contextlib
import json
import os
import shutil
import sys
import tempfile
import threading
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cra5_amd import synth  # noqa: E402
from cra5_amd.api import cra5_api  # noqa: E402
from cra5_amd.vaeformer import VAEformer  # noqa: E402

SIX = ["z_500", "q_500", "u_500", "v_500", "t_500", "w_500"]
EUROPE = (35, 72, -25, 45)


def _api(tmp):
    net = VAEformer(268)
    synth.load_synthetic(net, seed=0)
    with contextlib.redirect_stdout(sys.stderr):        # (the API prints its device)
        return cra5_api(local_root=tmp, device="cuda", weights=net.to("cuda"))


def bench(n, workers, repeats=1):
    tmp = tempfile.mkdtemp(prefix="cra5_subset_bench_")
    try:
        api = _api(tmp)
        std, mean = api.std.cpu(), api.mean.cpu()
        host = [(synth.synth_frame(268, seed=s) * std + mean).numpy() for s in range(8)]
        stamps = [f"2024-06-01T{i:02d}:00:00" for i in range(n)]
        enc = api.encode_era5_batch(stamps, data=[host[i % 8] for i in range(n)], save_root=tmp + "/CRA5", workers=workers)
        paths = [e["save_path"] for e in enc]
        tls = threading.local()

        def consumer(i, arr):                            # the frame leaves the pinned buffer into a pageable array
            dst = getattr(tls, "dst", None)
            if dst is None or dst.shape != arr.shape:
                dst = tls.dst = np.empty(arr.shape, np.float32)
            np.copyto(dst, arr)
            return float(dst.reshape(-1)[0])
        res = {}
        for name, kw in (("full", {}), ("six_500hPa_global", dict(variables=SIX)),
                         ("six_500hPa_europe", dict(variables=SIX, region=EUROPE)),
                         ("all_stride4_global", dict(stride=4)), ("all_stride6_global", dict(stride=6))):
            dts = []
            for rep in range(1 + repeats):                # rep 0 warms the pinned / device buffers of the case
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                api.decode_batch(paths=paths, workers=workers, sink=consumer, **kw)
                torch.cuda.synchronize()
                dts.append(time.perf_counter() - t0)
            g = cra5_api.grid_box(kw.get("region", (-90, 90, 0, 360)), stride=kw.get("stride"))
            shape = (len(kw.get("variables", range(268))), len(g["lat"]), len(g["lon"]))
            res[name] = dict(frames_per_s=n / dts[1], seconds=dts[1], frame_shape=shape,
                             d2h_bytes_per_frame=4 * int(np.prod(shape)), repeats=[n / dt for dt in dts[1:]])
        return dict(frames=n, workers=workers, cases=res,
                    what="cra5_api.decode_batch(paths, sink=host consumer) of the same .bin files, 268 model, synthetic "
                         "weights; the timed pass follows one warm-up pass of the same case")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def profile():
    tmp = tempfile.mkdtemp(prefix="cra5_subset_prof_")
    try:
        api = _api(tmp)
        net = api.net
        g = torch.Generator().manual_seed(5)
        y = torch.round(2.0 * torch.randn(256, 72, 144, generator=g)).to("cuda")
        chans = cra5_api.resolve_variables(SIX, api.vname_to_channels)
        ch, box = net._subset_args(chans, cra5_api.grid_box(EUROPE)["box"])
        with torch.no_grad():
            for _ in range(2):
                net._decode_guarded(y, mean=api._mean_flat, std=api._std_flat)
            torch.cuda.synchronize()
            for _ in range(2):
                net._decode_guarded(y, mean=api._mean_flat, std=api._std_flat, channels=ch, box=box)
            torch.cuda.synchronize()
            for _ in range(2):
                net._decode_guarded(y, mean=api._mean_flat, std=api._std_flat, step=(6, 6))
            torch.cuda.synchronize()
        print("profile workload done: 2 full + 2 subset + 2 stride-6 decodes")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--workers", type=int, default=12)
    ap.add_argument("--repeats", type=int, default=1)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    if a.profile:
        profile()
        return
    s = json.dumps(bench(a.frames, a.workers, max(1, a.repeats)))
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
