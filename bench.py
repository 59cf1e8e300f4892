#!/usr/bin/env python
"""bench.py - ERA5 frames/s (721x1440x268) encode+decode on N MI355X.

    python bench.py --gpus N --steps K --warmup W
N > 1: either launch it under `python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py ...`
(RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* from the env), or just run the line above - without WORLD_SIZE in
the env bench.py re-launches ITSELF under torch.distributed.run with N ranks (one per GPU, RCCL), rank 0 prints
the one JSON line, the exit code is the job's.

A "step" is one pass of the hot path over one synthetic frame on each rank:
    x (268x721x1440 fp32, resident in HBM) -> g_a -> y -> h_a/EB/h_s/GC -> rANS .bin
    -> rANS decode -> h_s -> y_hat -> g_s -> x_hat          (BASELINE.json configs[2])
with deterministic synthetic weights of the real 404.7 M-parameter architecture (there
is no network for the checkpoint / ERA5 samples).  Frames shard over ranks with no
data-path collective (weak scaling: one frame per rank per step); the only exchange is
the RCCL all-gather of per-frame bitstream stats after the timed region.

A plain run sets up, warms up, times the K steps, writes --dump-outputs and prints ONE JSON line (rank 0) with the
driver contract fields and what the timed region itself recorded (stream stats, shader clock, sampled kernel timer).
--full adds everything that needs work of its own after the timed region (rank 0, N = 1 unless noted):
  "roofline":     achieved fp32-equivalent TFLOP/s of the big-tile GEMM, HIP events around every launch of an
                  un-overlapped pass (every N), and the kernel on its best-case shape;
  "precision_f16", "api_single_frame", "entropy_matched", "api_pipelined": the same frames through the
                  reduced-precision mode, the reference-named API and the entropy-matched weights;
  "reference_pinned_frames": frames 0 / 1 against the streams the reference's Python wrote (every N);
  "cpu_baseline": the CPU oracle (oracle/torch_ref.py = restatement of the reference's
                  math path + oracle C rANS) on this box's host cores.

--dump-outputs DIR writes what the last timed step returned (rank 0) as float32 DIR/<name>.npy, at most 64 MB: the y / z
streams and z_shape in full and a fixed seeded sample of x_hat.  The same arguments give the same inputs (seeded frames
and weights), so two builds can be compared array for array.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
# (no HIP runtime knobs: GPU_MAX_HW_QUEUES=16 - one hardware queue per frame stream - measured 18.9 instead
# of 26.2 frames/s with 12 frames in flight, tools/region_repeat.py; the runtime's default 4 queues are kept)

import torch  # noqa: E402

PEAK_FP32_MFMA_TFLOPS = 157.3  # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 dense peak
PEAK_HBM_GBPS = 8000.0          # MI355X_MICROARCH.md: HBM3E peak
PEAK_F16_MFMA_TFLOPS = 2500.0  # MI355X_MICROARCH.md: dense bf16/f16 MFMA peak (no sparsity)
FLOP_PER_FRAME = 11.57e12      # encode 6.132 + decode 5.415 + hyper-prior
_T, _D = 10368, 1024            # tokens, width of the 268 model
# algorithmic flops per frame served by the two big-tile GEMM instantiations: 25 blocks x (qkv + proj + fc1 + fc2)
# + patch-embed + un-embed (K = N = 268*11*10) + post_quant_conv + quant_conv = 7.80 TFLOP
GEMM_BIGTILE_FLOP_PER_FRAME = 2.0 * _T * (25 * (_D * 3 * _D + _D * _D + 2 * _D * 4 * _D) + 2 * _D * 29480
                                          + 256 * _D + 2 * _D * 512)


def host_cpu_info():
    """(model string, physical cores, hardware threads) of the box."""
    model, phys = "unknown", set()
    try:
        pid = cid = None
        for line in open("/proc/cpuinfo"):
            k, _, v = line.partition(":")
            k, v = k.strip(), v.strip()
            if k == "model name":
                model = v
            elif k == "physical id":
                pid = v
            elif k == "core id":
                cid = v
            elif not k and pid is not None:
                phys.add((pid, cid))
                pid = cid = None
    except OSError:
        pass
    threads = os.cpu_count() or 1
    return model, (len(phys) or threads), threads


def cpu_baseline_full(quality, n_threads):
    """BASELINE.json configs[0] for real: ONE full compress -> decompress of the oracle
    (oracle/torch_ref.py: the reference's math path, materialised attention scores; oracle C rANS on one
    thread) on x = torch.rand(1, C, 721, 1440) seed 0 (Readme.md:139), same synthetic weights as the GPU
    run.  Minutes of CPU and ~20 GB of RAM: not part of the default run (`--cpu-baseline full`)."""
    from cra5_amd import synth
    from cra5_amd.zoo import vaeformer_pretrained
    from oracle import cbind
    from oracle import torch_ref as R
    torch.set_num_threads(n_threads)
    net = vaeformer_pretrained(quality=quality, pretrained=False)   # parameter container only (CPU tensors)
    synth.load_synthetic(net, seed=7)
    sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    del net
    cfg = R.cfg_268(quality)
    tb = R.tables(sd, cbind.pmf_to_cdf)
    x = synth.synth_frame(quality, seed=0, kind="uniform").unsqueeze(0)
    spans = {}
    with torch.no_grad():
        t0 = time.perf_counter()
        out, _ = R.compress(x, sd, cfg, tb, cbind.rans_encode)
        t1 = time.perf_counter()
        rec = R.decompress(out["strings"], out["z_shape"], sd, cfg, tb, cbind.rans_decode)["x_hat"]
        t2 = time.perf_counter()
    assert rec.shape == x.shape and bool(torch.isfinite(rec).all())
    spans = {"compress_s": t1 - t0, "decompress_s": t2 - t1,
             "y_bytes": len(out["strings"][0][0]), "z_bytes": len(out["strings"][1][0])}
    model, phys, threads = host_cpu_info()
    return {"value": 1.0 / (t2 - t0), "unit": "frames/s", "cores": n_threads, "physical_cores": phys,
            "hardware_threads": threads, "cpu": model, "kind": "port",
            "sample": (f"ONE full frame, BASELINE configs[0]: oracle/torch_ref.py compress {t1 - t0:.1f}s + decompress "
                       f"{t2 - t1:.1f}s on {n_threads} torch threads (rANS on 1), x = rand seed 0, quality={quality}"),
            "spans": spans}


def cpu_baseline(quality, n_threads):
    """Bounded CPU sample of the same workload with the oracle (kind = "port")."""
    from cra5_amd import synth
    from oracle import cbind
    from oracle import torch_ref as R
    import numpy as np
    torch.set_num_threads(n_threads)
    cfg = R.cfg_268(quality)
    D, heads = cfg["embed_dim"], cfg["num_heads"]
    names = {}
    for k, shp in (("g_a.patch_embed.proj.weight", (D, quality, 11, 10)), ("g_a.patch_embed.proj.bias", (D,)),
                   ("g_a.pos_embed", (1, 10368, D))):
        names[k] = shp
    for b in (0, 3):
        p = f"g_a.blocks.{b}"
        names.update({f"{p}.norm1.weight": (D,), f"{p}.norm1.bias": (D,), f"{p}.attn.qkv.weight": (3 * D, D),
                      f"{p}.attn.qkv.bias": (3 * D,), f"{p}.attn.proj.weight": (D, D), f"{p}.attn.proj.bias": (D,),
                      f"{p}.norm2.weight": (D,), f"{p}.norm2.bias": (D,), f"{p}.mlp.fc1.weight": (4 * D, D),
                      f"{p}.mlp.fc1.bias": (4 * D,), f"{p}.mlp.fc2.weight": (D, 4 * D), f"{p}.mlp.fc2.bias": (D,)})
    sd = synth.fill_state_dict(names, seed=7)
    x = synth.synth_frame(quality, seed=2).unsqueeze(0)
    with torch.no_grad():
        t0 = time.perf_counter()
        t = torch.nn.functional.conv2d(x, sd["g_a.patch_embed.proj.weight"], sd["g_a.patch_embed.proj.bias"],
                                       stride=(10, 10)).flatten(2).transpose(1, 2) + sd["g_a.pos_embed"]
        t1 = time.perf_counter()
        t = R.block(t, sd, "g_a.blocks.0", heads, 72, 144, (24, 24))
        t2 = time.perf_counter()
        t = R.block(t, sd, "g_a.blocks.3", heads, 72, 144, None)
        t3 = time.perf_counter()
    # entropy coder on a full frame's worth of symbols (default GC tables, unit-scale data)
    tb = R.gc_tables(R.get_scale_table(), cbind.pmf_to_cdf)
    rng = np.random.default_rng(0)
    n = 256 * 72 * 144
    idx = rng.integers(0, 40, size=n).astype(np.int32)
    sym = np.rint(rng.standard_normal(n) * 2).astype(np.int32)
    t4 = time.perf_counter()
    s = cbind.rans_encode(sym, idx, tb[0], tb[1], tb[2])
    t5 = time.perf_counter()
    d = cbind.rans_decode(s, idx, tb[0], tb[1], tb[2])
    t6 = time.perf_counter()
    assert np.array_equal(d.numpy(), sym)
    t_pe, t_win, t_glob = t1 - t0, t2 - t1, t3 - t2
    # 13 encoder + 12 decoder blocks = 18 windowed + 7 global; un-embed costs about one patch-embed
    est = 2 * t_pe + 18 * t_win + 7 * t_glob + (t5 - t4) + (t6 - t5)
    model, phys, threads = host_cpu_info()
    return {"value": 1.0 / est, "unit": "frames/s", "cores": n_threads, "physical_cores": phys,
            "hardware_threads": threads, "cpu": model, "kind": "port", "extrapolated": True,
            "sample": (f"oracle/torch_ref.py on {n_threads} host threads, quality={quality}, full 721x1440 frame: "
                       f"patch-embed {t_pe:.2f}s + 1 windowed block {t_win:.2f}s + 1 global block (materialised "
                       f"scores) {t_glob:.2f}s, + oracle C rANS encode {t5 - t4:.2f}s / decode {t6 - t5:.2f}s of "
                       f"2.65M symbols; frame time extrapolated as 2*pe + 18*win + 7*glob + rANS = {est:.1f}s; the "
                       f"un-extrapolated figure (`--cpu-baseline full`, one whole frame) is committed under profiles/")}


class HwmonSampler:
    """Board power / sclk from the amdgpu hwmon files, sampled every 20 ms by a host thread (tools/power_probe.py).  On
    some boxes the files are static (the same values idle or busy): `static` says so and the in-kernel shader clock
    (ops.ClockSampler) is the attributable figure."""

    def __init__(self):
        import glob
        self.dir = None
        for d in sorted(glob.glob("/sys/class/drm/card*/device/hwmon/hwmon*")):
            if any(n.startswith("power1") for n in os.listdir(d)):
                self.dir = d
                break
        self.rows, self.on, self.th = [], False, None

    @staticmethod
    def _read(path):
        try:
            with open(path) as f:
                return int(f.read().strip())
        except Exception:  # noqa: BLE001
            return None

    def start(self):
        if not self.dir:
            return
        import threading
        pf = next((os.path.join(self.dir, n) for n in ("power1_average", "power1_input")
                   if os.path.exists(os.path.join(self.dir, n))), None)
        ff = os.path.join(self.dir, "freq1_input")
        self.on = True

        def run():
            while self.on:
                self.rows.append((self._read(pf) if pf else None, self._read(ff)))
                time.sleep(0.02)
        self.th = threading.Thread(target=run, daemon=True)
        self.th.start()

    def stop(self):
        self.on = False
        if self.th:
            self.th.join()
        if not self.dir:
            return None
        pw = [r[0] / 1e6 for r in self.rows if r[0]]
        fq = [r[1] / 1e6 for r in self.rows if r[1]]
        cap = self._read(os.path.join(self.dir, "power1_cap"))
        return {"power_cap_w": cap / 1e6 if cap else None,
                "power_avg_w": sum(pw) / len(pw) if pw else None, "power_max_w": max(pw) if pw else None,
                "sclk_hwmon_mhz_mean": sum(fq) / len(fq) if fq else None, "samples": len(self.rows),
                "static": bool(len(set(pw)) <= 1 and len(set(fq)) <= 1)}


def finite_probe(x_hat):
    """Bench-side evidence that a round trip produced a finite x_hat: ONE product kernel (256 partial sums of every
    9973rd element, cra5_probe_sums_f32) whose result is read after the region - no torch kernel on the frame path."""
    from cra5_amd import ops
    p = torch.empty(ops.PROBE_PARTIALS, device=x_hat.device, dtype=torch.float32)
    return ops.probe_sums(x_hat.view(-1), p, 9973)


def probe_ok(p):
    return bool(torch.isfinite(p).all())


def reference_pinned(seed, strings, suffix=""):
    """bench frames 0 / 1 (synth_frame(268, 1000 + f)) were also run through the REFERENCE's Python in the build container
    (tests/golden/make_golden.py --stage ints): does the product's end-to-end stream of this frame equal the
    reference-python-written one?  Informational - a single rounding flip among the frame's 2.8 M integers changes the
    stream (tests/test_model_gpu.py::test_full268_round5_reference_integers accounts for every flip); None = no fixture."""
    import hashlib
    import numpy as np
    path = os.path.join(ROOT, "tests", "golden", f"bench{seed}{suffix}_ints.npz")
    if not os.path.exists(path):
        return None
    g = np.load(path)
    y, z = strings[0][0], strings[1][0]
    return {"y_stream_equals_reference_written": bool(hashlib.sha256(y).digest() == g["y_string_sha256"].tobytes()),
            "z_stream_equals_reference_written": bool(z == g["z_string"].tobytes()),
            "y_bytes": len(y), "y_bytes_reference": int(g["y_string_len"][0]), "z_bytes": len(z),
            "z_bytes_reference": int(g["z_string"].size)}


DUMP_XHAT_SAMPLES = 1 << 22      # 16 MB of x_hat; the streams of one frame add ~20 MB as float32


def dump_outputs(out_dir, out, x_hat, limit_bytes=64 << 20):
    """--dump-outputs: what a caller of compress() -> decompress() received in the last timed step, as float32 .npy files
    that two builds can compare array for array - y_stream / z_stream (the .bin strings, one byte per element), z_shape,
    and x_hat_sample: x_hat at DUMP_XHAT_SAMPLES fixed positions (numpy PCG64 seed 0, sorted; x_hat itself is 1.11 GB)."""
    import numpy as np
    arrays = {"y_stream": np.frombuffer(out["strings"][0][0], np.uint8).astype(np.float32),
              "z_stream": np.frombuffer(out["strings"][1][0], np.uint8).astype(np.float32),
              "z_shape": np.asarray(out["z_shape"], np.float32)}
    flat = x_hat.reshape(-1)
    pos = np.sort(np.random.default_rng(0).integers(0, flat.numel(), DUMP_XHAT_SAMPLES))
    arrays["x_hat_sample"] = flat[torch.from_numpy(pos).to(flat.device)].float().cpu().numpy()
    total = sum(a.nbytes for a in arrays.values())
    if total > limit_bytes:
        raise RuntimeError(f"--dump-outputs: {total} bytes > {limit_bytes}")
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)


def host_phase_summary(log):
    """mean ms per frame of the host (rANS) phases from VAEformer.host_log: encode y + z | decode z | decode y."""
    out = {}
    for kind in ("enc", "dec_z", "dec_y"):
        v = [dt for k, dt in log if k == kind]
        out[kind] = 1e3 * sum(v) / len(v) if v else None
    out["note"] = ("wall time of the calling frame thread inside the host coder (one core per frame; 12 frames in flight "
                   "share the box's cores with the launch threads)")
    return out


def matched_sample(net, pipe, frames, n, default_line):
    """The same round trip under the entropy-matched synthetic weight variant (cra5_amd/synth.py: h_s emits sigma ~
    rms(y), mu ~ 0, so the y stream sits in a trained model's regime - ~1 MB per frame, escapes a rarity - instead of
    the default set's 4.5 MB with 37 % escape-coded symbols).  Identical transformer work per frame; only the entropy
    side (records over PCIe, host rANS phases) changes.  Outside the timed region."""
    from cra5_amd import dist as D
    from cra5_amd import synth

    def round_trip(x):
        out = net.compress(x)
        ne = net.last_n_escape()
        x_hat = net.decompress(out["strings"], out["z_shape"])["x_hat"]
        return out, ne, finite_probe(x_hat)
    synth.apply_variant(net, seed=7, variant="matched")
    try:
        net.gpu_exclusive = False
        pipe.map(round_trip, [frames[i % len(frames)] for i in range(pipe.workers)])
        torch.cuda.synchronize()
        net.host_log = log = []
        t0 = time.perf_counter()
        res = pipe.map(round_trip, [frames[i % len(frames)] for i in range(n)])
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        net.host_log = None
        assert all(probe_ok(ok) for _, _, ok in res)
        nbytes = [len(o["strings"][0][0]) + len(o["strings"][1][0]) for o, _, _ in res]
        nesc = [ne[0] for _, ne, _ in res]
        crc0 = D.frame_stats(0, res[0][0]["strings"], nesc[0])
        pinned = {str(1000 + f): reference_pinned(1000 + f, res[f][0]["strings"], "_m") for f in range(min(2, n, len(frames)))}
        return {"value": n / dt, "unit": "frames/s", "frames": n, "bytes_per_frame": sum(nbytes) / n,
                "escape_symbols_per_frame": sum(nesc) / n, "host_phase_ms": host_phase_summary(log),
                "frame0_stats": {"y_bytes": crc0[1], "z_bytes": crc0[2], "crc32": crc0[3], "n_escape": crc0[4]},
                "reference_pinned_frames": pinned,
                "default_set": default_line,
                "weights": "cra5_amd/synth.py seed 7, variant 'matched' (MATCHED_SIGMA = %.2f)" % synth.MATCHED_SIGMA,
                "what": "same pipeline, frames and transformer weights as the timed region; only h_s.norm / h_s.final differ"}
    finally:
        net.host_log = None
        synth.apply_variant(net, seed=7, variant="default")


def api_pipelined_sample(net, pipe, frames, inflight, n):
    """PCIe-inclusive throughput of the reference-named API, pipelined (cra5_api.py:81-125,153-192,
    test.py:14-59): HOST fp32 frames (pageable numpy arrays, physical units) -> `encode_era5_batch` (pinned staging,
    H2D of one frame under the GPU / rANS phases of the others, .bin files written) -> `decode_batch` (.bin files read,
    x_hat D2H through pinned buffers, handed to a host consumer that copies it into its own pageable array).  Beside
    each side, the same side with device-resident frames (no H2D / D2H, no files).  Outside the timed region."""
    import shutil
    import tempfile
    import threading
    import numpy as np
    from cra5_amd.api import cra5_api
    net.gpu_exclusive = False
    tmp = tempfile.mkdtemp(prefix="cra5_bench_pipe_")
    try:
        import contextlib
        with contextlib.redirect_stdout(sys.stderr):        # (the reference API prints its device: stdout is the JSON line's)
            api = cra5_api(local_root=tmp, device="cuda", weights=net)
        api._pipe = pipe                                     # the bench's frame threads (their workspaces exist already)
        n_host = min(8, len(frames))
        host = [(frames[i][0] * api.std + api.mean).cpu().numpy() for i in range(n_host)]
        stamps = [f"2024-06-{1 + i // 24:02d}T{i % 24:02d}:00:00" for i in range(n)]
        data = [host[i % n_host] for i in range(n)]
        tls = threading.local()

        def consumer(i, arr):                                # a host consumer: the frame leaves the pinned buffer
            dst = getattr(tls, "dst", None)
            if dst is None:
                dst = tls.dst = np.empty(arr.shape, np.float32)
            np.copyto(dst, arr)
            return float(dst[0, 0, 0])
        res = {}
        for rep in range(2):                                 # rep 0 warms the pinned buffers / page tables
            nn = n if rep else inflight
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            enc = api.encode_era5_batch(stamps[:nn], data=data[:nn], save_root=tmp + "/CRA5", workers=inflight)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            api.decode_batch(paths=[e["save_path"] for e in enc], workers=inflight, sink=consumer)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            res = {"encode_fps": nn / (t1 - t0), "decode_fps": nn / (t2 - t1), "round_trip_fps": nn / (t2 - t0)}
        # the reference's test.py loop as a stream: each frame host -> .bin -> host, H2D and D2H of different frames overlap
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        api.roundtrip_batch(stamps, data=data, save_root=tmp + "/RT", workers=inflight, sink=consumer)
        torch.cuda.synchronize()
        res["round_trip_streamed_fps"] = n / (time.perf_counter() - t0)
        # the same two sides on device-resident frames (what `value` measures, split by side)
        dev_frames = [frames[i % len(frames)] for i in range(n)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        outs = pipe.map(net.compress, dev_frames)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        pipe.map(lambda o: torch.isfinite(net.decompress(o["strings"], o["z_shape"])["x_hat"][0, 0, ::97, ::97]).all(), outs)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        # the batch path writes the file the serial reference-named call writes for the same host array
        ser = api.encode_era5_as_bin(stamps[0], save_root=tmp + "/SERIAL", data=data[0])
        same = open(ser["save_path"], "rb").read() == open(enc[0]["save_path"], "rb").read()
        res.update({
            "value": res["round_trip_streamed_fps"], "unit": "frames/s", "frames": n, "frames_in_flight": inflight,
            "encode_fps_device_resident": n / (t1 - t0), "decode_fps_device_resident": n / (t2 - t1),
            "encode_ratio": res["encode_fps"] / (n / (t1 - t0)), "decode_ratio": res["decode_fps"] / (n / (t2 - t1)),
            "bin_equals_serial_api_call": bool(same),
            "pcie_bytes_per_frame": {"h2d": int(frames[0].numel() * 4), "d2h": int(frames[0].numel() * 4)},
            "what": "cra5_api.encode_era5_batch(host fp32 arrays) -> .bin files -> decode_batch(sink=host consumer): pinned "
                    "double staging per in-flight frame, H2D / D2H of one frame under the other frames' GPU and rANS phases; "
                    "encode_fps / decode_fps: the two batch calls one after the other (round_trip_fps = n / (t_encode + "
                    "t_decode)); `value` = round_trip_streamed_fps: roundtrip_batch, every frame host array -> .bin -> host "
                    "consumer in one pipeline (the PCIe-inclusive counterpart of the line's device-resident `value`).  "
                    "Round 6: ONE frame per direction on the link at a time (api.link_serial) - the link itself runs 57 GB/s "
                    "= 51 frames/s either way and 97 GB/s both ways at once (profiles/r06_link_probe.txt), so encode / decode "
                    "are link-bound near 51 and the streamed round trip is bound by the GPU (`value`) with H2D transfers "
                    "stretched to ~31 ms under concurrent D2H + kernels (profiles/r06_api_phase_probe.txt)",
            "link_serial": bool(api.link_serial)})
        return res
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def _job_dir():
    """A directory every rank of THIS job agrees on (the error line's lock lives there): handed down by self_launch, or
    derived from what an external launcher gives all its ranks alike (run id / port / the launcher's pid)."""
    d = os.environ.get("CRA5_JOB_DIR")
    if not d:
        import tempfile
        # under torch.distributed.run every rank shares the launcher's pid (one launch = one directory); a process
        # nobody launched is its own job
        launched = "TORCHELASTIC_RUN_ID" in os.environ
        tag = "%s_%s_%d" % (os.environ.get("TORCHELASTIC_RUN_ID", "norun"), os.environ.get("MASTER_PORT", "noport"),
                            os.getppid() if launched else os.getpid())
        d = os.path.join(tempfile.gettempdir(), "cra5_bench_" + "".join(c if c.isalnum() or c in "_-" else "_" for c in tag))
    if not os.path.isdir(d):
        os.makedirs(d, exist_ok=True)
        if not os.environ.get("CRA5_JOB_DIR") and "TORCHELASTIC_RUN_ID" not in os.environ:
            import atexit
            import shutil
            atexit.register(shutil.rmtree, d, True)          # a one-process job cleans up after itself
    return d


def error_line(exc, stage):
    """A rank died before it could take part in the JSON line: print ONE parsable line - the first
    failing rank's, whichever rank that is - with the contract's keys, `value` null, "error" and the traceback; the
    launcher then ends the other ranks.  Returns True if this rank printed."""
    import traceback
    try:
        fd = os.open(os.path.join(_job_dir(), "error_line.lock"), os.O_CREAT | os.O_EXCL | os.O_WRONLY)
        os.close(fd)
    except FileExistsError:
        return False
    except OSError:
        pass                                      # no lock possible: better two lines than none
    tb = "".join(traceback.format_exception(type(exc), exc, exc.__traceback__))
    line = {"metric": "ERA5 frames/s (721x1440x268) encode+decode", "value": None, "unit": "frames/s",
            "n_gpus": int(os.environ.get("WORLD_SIZE", "1")), "higher_is_better": True,
            "error": f"{type(exc).__name__}: {exc}", "failed_rank": int(os.environ.get("RANK", "0")),
            "failed_local_rank": int(os.environ.get("LOCAL_RANK", "0")), "stage": stage,
            "hostname": os.uname().nodename, "traceback": tb[-6000:]}
    print(json.dumps(line), flush=True)
    return True


STAGE = ["startup"]     # where main() is (the error line names it)
# the measured terms of single_frame_budget(); `encode_other` / `decode_other` are what they leave of the totals
ENCODE_TERMS = ("h2d", "g1_g_a_and_latent_side", "g1b_other_gpu_phases", "h1_rans_encode", "bin_write")
DECODE_TERMS = ("h2z_rans_decode_z", "g2_h_s_indexes", "h2y_rans_decode_y", "g3_g_s")


def single_frame_budget(api, host_frame, reps=4):
    """Where the time of ONE serial call pair of the reference-named API goes (test.py:14-45 in the
    reference): encode_era5_as_bin(host array) = H2D | G1 (finite probe, g_a, h_a, h_s, GaussianConditional, records to the
    host) | H1 (rANS z beside y) | .bin write; decode_from_bin = .bin read | H2z (rANS z) | G2 (h_s, CDF indexes to the
    host) | H2y (rANS y) | G3 (de-quantise, g_s, probe).  Phases from VAEformer.phase_log / host_log + wall-clock stamps
    of the API calls; `other` = what the stamps do not cover (Python between the phases, stream syncs).  Median of the
    reps after the first."""
    import tempfile
    import shutil
    net = api.net
    tmp = tempfile.mkdtemp(prefix="cra5_budget_")
    ts = "2024-06-01T00:00:00"
    rows = []
    try:
        for _ in range(reps):
            net.phase_log, net.host_log = [], []
            orig_frame = api._frame
            stamp = {}

            def timed_frame(time_stamp, data, _o=orig_frame):
                t = time.perf_counter()
                r = _o(time_stamp, data)
                torch.cuda.current_stream().synchronize()
                stamp["h2d"] = time.perf_counter() - t
                return r
            api._frame = timed_frame
            try:
                t0 = time.perf_counter()
                enc = api.encode_era5_as_bin(ts, save_root=tmp + "/CRA5", data=host_frame)
                t1 = time.perf_counter()
            finally:
                api._frame = orig_frame
            g_enc = [e[3] - e[2] for e in net.phase_log]            # GPU phases (start -> end incl. the closing sync)
            h_enc = dict(net.host_log)
            net.phase_log, net.host_log = [], []
            t2 = time.perf_counter()
            api.decode_from_bin(ts, custom_path=enc["save_path"], return_format="de_normalized")
            t3 = time.perf_counter()
            g_dec = [e[3] - e[2] for e in net.phase_log]
            h_dec = dict(net.host_log)
            row = {"encode_total": t1 - t0, "h2d": stamp.get("h2d", 0.0),
                   "g1_g_a_and_latent_side": g_enc[0] if g_enc else 0.0, "g1b_other_gpu_phases": sum(g_enc[1:]),
                   "h1_rans_encode": h_enc.get("enc", 0.0), "bin_write": enc["saving_time"],
                   "decode_total": t3 - t2, "h2z_rans_decode_z": h_dec.get("dec_z", 0.0),
                   "g2_h_s_indexes": g_dec[0] if g_dec else 0.0, "h2y_rans_decode_y": h_dec.get("dec_y", 0.0),
                   "g3_g_s": sum(g_dec[1:])}
            rows.append(row)
    finally:
        net.phase_log = net.host_log = None
        shutil.rmtree(tmp, ignore_errors=True)
    use = rows[1:] or rows
    med = {k: 1e3 * sorted(r[k] for r in use)[len(use) // 2] for k in rows[0]}
    # `other` from the medians (each key's median may come from a different rep): the budget adds up to its totals
    med["encode_other"] = med["encode_total"] - sum(med[k] for k in ENCODE_TERMS)
    med["decode_other"] = med["decode_total"] - sum(med[k] for k in DECODE_TERMS)
    med["frames_per_s"] = 1e3 / (med["encode_total"] + med["decode_total"])
    return med


def self_launch(n):
    """`python bench.py --gpus N` without a launcher: re-run this command line as N ranks under
    torch.distributed.run (one process per GPU; standalone rendezvous on 127.0.0.1, port chosen by the launcher).  stdout / stderr are
    inherited, so rank 0's JSON line is this process's output; returns the job's exit code."""
    import subprocess
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC only on this host driver (RCCL needs it)
    env["CRA5_SELF_LAUNCHED"] = "1"
    # torch.distributed.run forces OMP_NUM_THREADS=1 when it is unset; every rank sizes its own pools from its
    # NUMA share of the cores instead (main())
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 8) // (2 * n))))
    # --standalone: the launcher's own c10d rendezvous on a port IT picks and keeps (picking a free port here and
    # closing it again was a bind / close race between concurrent jobs); 127.0.0.1: the container hostname may not resolve
    cmd = [sys.executable, "-m", "torch.distributed.run", "--standalone", "--local-addr", "127.0.0.1", "--nnodes=1",
           f"--nproc-per-node={n}", os.path.abspath(__file__)] + sys.argv[1:]
    import shutil
    import tempfile
    env["CRA5_JOB_DIR"] = jd = tempfile.mkdtemp(prefix="cra5_bench_job_")
    try:
        rc = subprocess.call(cmd, env=env, stdin=subprocess.DEVNULL)
        if rc != 0 and not (os.path.exists(os.path.join(jd, "error_line.lock")) or os.path.exists(os.path.join(jd, "line_printed"))):
            # a rank died without reaching Python's exception machinery (signal, out-of-memory kill, launcher failure)
            print(json.dumps({"metric": "ERA5 frames/s (721x1440x268) encode+decode", "value": None, "unit": "frames/s",
                              "n_gpus": n, "higher_is_better": True, "failed_rank": None, "stage": "unknown",
                              "error": f"the {n}-rank job exited with code {rc} and no rank reported a Python exception "
                                       "(killed by a signal / the out-of-memory killer, or the launcher itself failed): "
                                       "see stderr"}), flush=True)
        return rc
    finally:
        shutil.rmtree(jd, ignore_errors=True)


def dry_dist(args):
    """`--dry-dist`: everything of the N-rank job EXCEPT the GPU work, on gloo / CPU - launch, rendezvous,
    frame sharding, barrier, max-over-ranks, the all-gather of per-frame stats, one JSON line from rank 0.
    Stand-in streams (the stats only look at bytes).  Used by tests/test_dist_cpu.py."""
    from cra5_amd import dist as D
    rank, world, local = D.init_from_env("cpu", numa_bind=not args.no_numa_bind)
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    cpu = torch.device("cpu")
    STAGE[0] = "preflight"
    pre = D.preflight(cpu, args.inflight, min(args.frame_pool, args.steps))
    STAGE[0] = "warm-up"
    _test_failure_hook(rank)
    my = D.shard_frames(world * args.steps, rank, world)
    D.barrier()
    STAGE[0] = "timed region"
    t0 = time.perf_counter()
    rows = [D.frame_stats(f, [[bytes([f % 251]) * (100 + f)], [bytes([(7 * f) % 251]) * (10 + f)]]) for f in my]
    D.barrier()
    mine = time.perf_counter() - t0 + 1e-3 * (rank + 1)
    elapsed = D.max_over_ranks(mine, cpu)
    stats = D.gather_stats(rows, cpu)
    assert stats[:, 0].tolist() == list(range(world * args.steps)), "gathered stats do not cover the frame set"
    hosts = D.gather_objects(dict(D.host_report(), numa_bind=D.LAST_BIND))
    per_rank = D.gather_objects(per_rank_line(rank, args.steps, mine, None, []))
    if rank == 0:
        print(json.dumps({"metric": "dry-dist (no GPU work)", "dry": True, "n_gpus": world, "steps": args.steps,
                          "preflight": pre, "per_rank": per_rank,
                          "host_per_rank": [dict(h, cpus=[h["cpus"][0], h["cpus"][-1]] if h["cpus"] else []) for h in hosts],
                          "host_cpu_sets_disjoint": _disjoint([h["cpus"] for h in hosts]),
                          "stats_fields": list(D.STATS_FIELDS),
                          "warmup": args.warmup, "value": world * args.steps / elapsed, "unit": "frames/s",
                          "frames_of_rank0": [my[0], my[-1] + 1] if len(my) else [],
                          "stats_rows": int(stats.shape[0]), "stats_bytes": int(stats[:, 1:3].sum()),
                          "self_launched": os.environ.get("CRA5_SELF_LAUNCHED") == "1",
                          "backend": torch.distributed.get_backend() if torch.distributed.is_initialized() else None}),
              flush=True)
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()


def _test_failure_hook(rank):
    """tests/test_dist_cpu.py: CRA5_TEST_FAIL_RANK=r makes rank r die before the timed region (the error line's path)."""
    r = os.environ.get("CRA5_TEST_FAIL_RANK")
    if r is not None and int(r) == rank:
        raise RuntimeError(f"injected failure on rank {rank} (CRA5_TEST_FAIL_RANK)")


def per_rank_line(rank, steps, elapsed_own, clock, host_log):
    """What one rank contributes to `per_rank`: its OWN frames/s over the timed region (the job's
    `value` uses the slowest rank's time), the shader clock its GPU held, its host rANS phase times - so that a < N x
    result can be attributed to a slow GPU, host contention or power."""
    return {"rank": rank, "value": steps / elapsed_own if elapsed_own else None, "elapsed_s": elapsed_own,
            "shader_clock": clock, "host_phase_ms": {k: v for k, v in host_phase_summary(host_log).items() if k != "note"},
            "hostname": os.uname().nodename, "pid": os.getpid()}


def _disjoint(sets):
    seen = set()
    for c in sets:
        if seen & set(c):
            return False
        seen |= set(c)
    return True


def rocprof_gemm_frac(f16=False):
    """roofline fraction of the two big-tile GEMM instantiations from the newest committed rocprofv3 kernel
    summary (profiles/rNN_bench_exclusive_kernel_stats.csv; rNN_f16_bench_... for the reduced-precision mode):
    algorithmic flops per frame of the launches each instantiation serves / (calls x average
    duration).  None if the file is absent."""
    import csv
    import glob
    import re
    try:
        pat = re.compile(r"r\d+_f16_bench_exclusive_kernel_stats\.csv$" if f16 else r"r\d+_bench_exclusive_kernel_stats\.csv$")
        path = sorted(p for p in glob.glob(os.path.join(ROOT, "profiles", "r*_bench_exclusive_kernel_stats.csv"))
                      if pat.search(os.path.basename(p)))[-1]
        calls = dur = 0.0
        frames = None
        for row in csv.DictReader(open(path)):
            name = row.get("Name") or row.get("KernelName") or ""
            n, tot = float(row.get("Calls", 0) or 0), float(row.get("TotalDurationNs", 0) or 0)
            if "gemm_nt_split_kernel<2, 4," in name:     # the 256x256 and 192x256 tile instantiations
                calls += n
                dur += tot
            if "im2col_tiled_kernel" in name:
                frames = n       # one patch gather per frame
        if not calls or not frames:
            return None
        flops = GEMM_BIGTILE_FLOP_PER_FRAME * frames
        ach = flops / (dur * 1e-9) / 1e12
        return {"file": os.path.basename(path), "achieved": ach, "frac": ach / (PEAK_F16_MFMA_TFLOPS / (1.0 if f16 else 3.0)),
                "launches": int(calls), "frames": frames, "avg_launch_ms": dur / calls * 1e-6}
    except Exception:  # noqa: BLE001
        return None


def main():
    from cra5_amd.config import RuntimeConfig
    rc0 = RuntimeConfig.from_env()               # the ONE place CRA5_* settings are read; flags below override its fields
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=96)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--quality", type=int, default=268)
    ap.add_argument("--precision", choices=("fp32", "f16"), default=rc0.precision,
                    help="fp32 (default, the headline: fp32-accurate split MFMA) | f16: BASELINE.json configs[4], "
                         "reduced-precision g_a/g_s (plain f16 operands), RMSE-gated - NOT the headline metric")
    ap.add_argument("--settle-batches", type=int, default=40,
                    help="extra untimed warm-up batches (2 x inflight frames each) until the batch time settles")
    ap.add_argument("--settle-min-batches", type=int, default=3)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-baseline", choices=("sample", "full", "only-full"), default="full",
                    help="full (default, round 6): ONE whole frame through the oracle on this box's host cores, after the GPU "
                         "legs (BASELINE configs[0], ~1 min on 128 cores, ~20 GB of RAM); sample: bounded ~20 s sample, "
                         "extrapolated; only-full: just the whole frame, no GPU run (prints its JSON)")
    ap.add_argument("--cpu-threads", type=int, default=0, help="torch threads of the CPU baseline (0 = physical cores)")
    ap.add_argument("--no-kernel-timer", action="store_true")
    ap.add_argument("--timer-sample", type=int, default=29,
                    help="inside the timed region bracket every n-th GEMM / attention launch with HIP events "
                         "(event records are queue packets: bracketing all ~400 launches per frame costs ~5 %% "
                         "frames/s, every 7th still 5 %%: measured 26.3 vs 24.9-25.2); 29 is coprime with the 5 timed launches of a transformer block")
    ap.add_argument("--exclusive", action="store_true",
                    help="timed region with exclusive GPU phases (one frame's kernels at a time) instead of "
                         "overlapping HIP streams")
    ap.add_argument("--gpu-slots", type=int, default=rc0.gpu_slots,
                    help="at most this many frames inside a GPU phase at a time (0 = unlimited)")
    ap.add_argument("--roofline-steps", type=int, default=2,
                    help="frames of the un-overlapped kernel-timing pass run after the timed region")
    ap.add_argument("--frame-pool", type=int, default=24,
                    help="distinct synthetic frames kept resident per rank, 1.11 GB each (the rank's i-th frame uses "
                         "slot i %% pool; with --steps <= pool every frame of the job is distinct)")
    ap.add_argument("--dry-dist", action="store_true",
                    help="no GPU work: launch / rendezvous (gloo) / shard / barrier / all-gather / one JSON line only")
    ap.add_argument("--no-best-case", action="store_true",
                    help="skip the live best-case-shape launches of the GEMM kernel (`roofline.best_case_shape`): profiled runs")
    ap.add_argument("--no-f16-sample", action="store_true",
                    help="skip the short reduced-precision sample (`precision_f16`: BASELINE configs[4] on this GPU, rank 0, N = 1)")
    ap.add_argument("--no-api-sample", action="store_true",
                    help="skip the reference-named single-frame API sample (`api_single_frame`, rank 0, N = 1)")
    ap.add_argument("--api-frames", type=int, default=72,
                    help="frames of the pipelined PCIe-inclusive API sample (`api_pipelined`, rank 0, N = 1)")
    ap.add_argument("--no-matched-sample", action="store_true",
                    help="skip the entropy-matched weight-variant sample (`entropy_matched`, rank 0, N = 1)")
    ap.add_argument("--no-clock-sampler", action="store_true", help="no shader-clock sampler wave beside the timed region")
    ap.add_argument("--no-numa-bind", action="store_true",
                    help="do not pin a rank's threads to its GPU's NUMA node share of the host cores")
    ap.add_argument("--numa-bind-single", choices=("on", "off"), default="on" if rc0.numa_bind_single else "off",
                    help="N = 1: bind the process to the GPU's NUMA node as the N > 1 ranks are (frame threads, rANS work and "
                         "the pageable -> pinned copies of the API samples then run beside the GPU's root complex); the CPU "
                         "baseline leg lifts the bind again")
    ap.add_argument("--inflight", type=int, default=rc0.inflight,
                    help="frames in flight per GPU (host rANS of one frame overlaps GPU work of the others)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed region, write what the last timed step returned (rank 0) as DIR/<name>.npy: "
                         "the y / z streams and z_shape in full, a fixed seeded sample of x_hat (dump_outputs())")
    ap.add_argument("--full", action="store_true",
                    help="after the timed region, also run the legs that need work of their own: the un-overlapped roofline "
                         "pass (--roofline-steps, --no-best-case), the reduced-precision, API and entropy-matched samples "
                         "(--no-f16-sample, --no-api-sample, --api-frames, --no-matched-sample), the reference-pinned "
                         "frames and the CPU baseline (--cpu-baseline, --no-cpu-baseline); off: the line carries only what "
                         "the timed region measured")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    force_launch = os.environ.get("CRA5_FORCE_SELF_LAUNCH") == "1"    # tests: the launcher path on a 1-GPU box
    if (args.gpus > 1 or force_launch) and "WORLD_SIZE" not in os.environ and "RANK" not in os.environ:
        # `python bench.py --gpus N` as the driver calls it for N = 1: become the launcher of N ranks
        raise SystemExit(self_launch(args.gpus))
    if args.dry_dist:
        return dry_dist(args)

    from cra5_amd import dist as D
    from cra5_amd import ops, synth
    from cra5_amd._lib import LIB_PATH
    from cra5_amd.zoo import vaeformer_pretrained

    cpu_threads = args.cpu_threads or host_cpu_info()[1]
    if args.cpu_baseline == "only-full":
        print(json.dumps({"cpu_baseline": cpu_baseline_full(args.quality, cpu_threads)}), flush=True)
        return
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the HIP path is the only product path")
    lws = int(os.environ.get("LOCAL_WORLD_SIZE", os.environ.get("WORLD_SIZE", "1")))
    if lws > torch.cuda.device_count() and os.environ.get("CRA5_SHARE_GPU") != "1":
        raise SystemExit(f"bench.py: {lws} ranks on this node but {torch.cuda.device_count()} visible GPU(s) - one rank per GPU "
                         "(CRA5_SHARE_GPU=1 lets ranks share a GPU: tests only, gloo gather)")
    # (N > 1: the rank is pinned to its GPU's NUMA share of the host cores inside init_from_env, BEFORE the process group
    # and the HIP runtime start their helper threads - ADVICE r3)
    all_cpus = sorted(os.sched_getaffinity(0))       # (the CPU baseline leg lifts the bind again)
    rank, world, local = D.init_from_env("cuda", numa_bind=not args.no_numa_bind,
                                         bind_single=args.numa_bind_single == "on")
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    if os.environ.get("CRA5_SHARE_GPU") == "1":
        # tests on a 1-GPU box: N ranks (gloo collectives) share the visible GPUs - every piece of the N > 1 job but
        # the multi-GPU RCCL communicator runs for real (self-launch, sharding, per-rank pipelines, the stats gather)
        local = local % torch.cuda.device_count()
    if local >= torch.cuda.device_count():
        raise SystemExit(f"--gpus {args.gpus}: rank {rank} wants GPU {local} but only {torch.cuda.device_count()} are visible")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    # N ranks share the node's host cores.  Pin this rank (its frame threads, its rANS work, its torch CPU pool)
    # to its GPU's NUMA node, an equal share of that node's cores per rank on the node: pinned staging buffers
    # are then allocated node-local and 8 x 12 frame threads do not migrate over both sockets.  (Round 6: at N = 1 too.)
    numa = D.LAST_BIND
    if world > 1:
        share = len(os.sched_getaffinity(0)) if (numa and numa.get("bound")) else (os.cpu_count() or 8) // world
        torch.set_num_threads(max(1, share // 2))
    # first-contact preflight: the job's first collective, every rank's free device memory / host
    # CPUs / GPU identity; ALL ranks derive the same frames-in-flight figure from the gathered reports
    STAGE[0] = "preflight"
    pre = D.preflight(dev, args.inflight, min(args.frame_pool, args.steps))
    if pre["inflight"] != args.inflight:
        print(f"[bench] frames in flight lowered {args.inflight} -> {pre['inflight']}: {pre['lowered_because']}",
              file=sys.stderr, flush=True)
        args.inflight = pre["inflight"]
    STAGE[0] = "model build"

    rc = rc0.replace(precision=args.precision, gpu_slots=args.gpu_slots, inflight=args.inflight,
                     gpu_exclusive=bool(args.exclusive), numa_bind_single=args.numa_bind_single == "on")
    net = vaeformer_pretrained(quality=args.quality, pretrained=False, runtime=rc)
    synth.load_synthetic(net, seed=7)
    net = net.to(dev)
    C = args.quality
    # BASELINE.json configs[3]: the job's frames f = 0 .. world*K-1 are x_f ~ N(0,1) with seed 1000 + f,
    # rank r owns the contiguous block dist.shard_frames gives it ([8r, 8r+8) of 64 at K = 8).  They are
    # generated on the device and resident in HBM before the timed region; at most --frame-pool distinct
    # frames are kept per rank (1.11 GB each): the rank's i-th frame is the tensor of seed
    # 1000 + first + (i % pool) - with K <= pool (the driver's K = 20) every frame is its own tensor; beyond that the
    # tensors repeat and the JSON line says so (`config.distinct_frames_per_rank`, `frame_seeds`).
    my_frames = D.shard_frames(world * args.steps, rank, world)
    pool = max(1, min(args.frame_pool, len(my_frames)))
    gdev = torch.Generator(device=dev)
    frames = []
    for i in range(pool):
        f = my_frames[0] + i
        if f < 2:
            # the job's first two frames come from the CPU generator (synth.synth_frame: reproducible anywhere): the
            # reference was run on exactly these tensors in the build container, tests/golden/bench100{0,1}*_ints.npz
            # hold its integers and stream hashes (tests/test_model_gpu.py::test_bench_frames_*)
            frames.append(synth.synth_frame(C, seed=1000 + f).unsqueeze(0).to(dev))
            continue
        gdev.manual_seed(1000 + f)
        frames.append(torch.randn((1, C, 721, 1440), generator=gdev, device=dev, dtype=torch.float32))
    seed_of_step = [1000 + my_frames[0] + (i % pool) for i in range(len(my_frames))]

    from cra5_amd.pipeline import FramePipeline
    pipe = FramePipeline(net, workers=args.inflight, device=dev)

    # One step = one full round trip.  Only the byte streams and a finiteness probe of every reconstruction are
    # kept: x_hat is 1.11 GB per frame (600 retained frames would not fit 288 GB); it is fully produced on the
    # device either way.  The SAME function runs in the warm-up: every kernel the timed region launches (the
    # probe's strided copy / isfinite / reduction included) has been loaded before the clock starts - on a fresh
    # box the first use of a torch kernel pages its code object in from a cold disk cache (measured: 23.0-24.3
    # frames/s in the first process on a box vs 26.3-27.0 in the following ones when the probe first ran inside
    # the timed region).
    def decoded(x):
        out = net.compress(x)
        out = dict(out, n_escape=net.last_n_escape())      # (bench-side copy: compress() returns the reference's two keys)
        return out, net.decompress(out["strings"], out["z_shape"])["x_hat"]

    def round_trip(x):
        out, x_hat = decoded(x)
        return out, finite_probe(x_hat)

    # the timed region's scheduling mode applies to the warm-up too (it used to run in the default exclusive mode:
    # settle batches at 23.5 frames/s that said nothing about the overlapped region that followed)
    net.gpu_exclusive = bool(args.exclusive)
    net.gpu_slots = args.gpu_slots
    net.precision = args.precision
    # warm-up: W untimed steps (also builds the per-thread workspaces / derived weights)
    STAGE[0] = "warm-up"
    _test_failure_hook(rank)
    net.compress(frames[0])
    warm = pipe.map(round_trip, [frames[i % pool] for i in range(max(args.warmup, args.inflight))])
    # streams of the warm-up frames: the timed region codes the same tensors again and must reproduce them (sizes + CRC)
    warm_rows = {i % pool: D.frame_stats(0, out["strings"], out.get("n_escape", [-1])[0])[1:] for i, (out, _) in enumerate(warm)}
    del warm
    # A fresh box runs slow for its first MINUTE, not seconds (power state / clocks of GPU and host, page cache):
    # four consecutive bench processes on a new box measured 22.7, 23.5, 25.1, 26.3 frames/s with the round-1
    # rule (stop when two batches agree within 3 %).  Keep running untimed batches until the best batch time has
    # not improved by more than 1.5 % for three consecutive batches (at most --settle-batches of them);
    # reported as `warmup_settle_frames`.
    settle_frames, best, stale = 0, None, 0
    for _ in range(max(0, args.settle_batches)):
        torch.cuda.synchronize()
        tb = time.perf_counter()
        pipe.map(round_trip, [frames[i % pool] for i in range(2 * args.inflight)])
        torch.cuda.synchronize()
        tb = time.perf_counter() - tb
        settle_frames += 2 * args.inflight
        if os.environ.get("CRA5_BENCH_VERBOSE"):
            print(f"[settle] batch of {2 * args.inflight} frames: {2 * args.inflight / tb:.2f} frames/s", file=sys.stderr, flush=True)
        if best is None or tb < 0.985 * best:
            best, stale = (tb if best is None else min(best, tb)), 0
        else:
            best, stale = min(best, tb), stale + 1
            if stale >= 3 and settle_frames >= 2 * args.inflight * args.settle_min_batches:
                break
    timer = None if args.no_kernel_timer else ops.KernelTimer(sample_every=args.timer_sample)
    # attributable lines: the shader clock the chip sustains over the timed region - short one-wave
    # probes launched every 5 ms by a host thread on their own stream - and the board power / sclk the driver exposes
    clk = None
    if not args.no_clock_sampler:            # (round 6: every rank samples its own GPU's clock -> `per_rank`)
        try:
            clk = ops.ClockSampler(dev)
            clk.probe()
            clk.stop()
            if clk.summary() is None:
                clk = None
        except Exception:  # noqa: BLE001
            clk = None
    hw = HwmonSampler() if rank == 0 else None
    # Timed region: frames in flight on separate HIP streams.  By default their GPU phases
    # OVERLAP on the chip (blocks of one frame's kernels fill the tail / epilogue gaps of
    # another's: +15-25 % frames/s), which makes a single launch's start->stop duration
    # depend on what else is running; --exclusive serialises the phases instead.
    torch.cuda.synchronize()
    STAGE[0] = "timed region"
    D.barrier()
    ops.TIMER = timer
    net.host_log = host_log = []
    if clk is not None:
        clk.start()
    if hw is not None:
        hw.start()
    # two marker launches (clock_stamp_kernel) bracket the timed region in a rocprofv3 kernel trace: tools/trace_concurrency.py
    # restricts its GPU-busy / concurrency figures to the kernels between them
    import ctypes
    from cra5_amd._lib import lib as _cra5_lib
    region_marks = torch.zeros(2, dtype=torch.int64, device=dev)
    _cra5_lib().cra5_clock_stamp(ctypes.c_void_p(region_marks.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.current_stream().synchronize()
    t0 = time.perf_counter()
    # EXACTLY K steps = K full round trips; up to `inflight` frames overlap, all K complete
    # (streams synchronised, x_hat materialised) before the clock stops.
    if args.dump_outputs is None:
        results = pipe.map(round_trip, [frames[i % pool] for i in range(args.steps)])
    else:
        # the same steps; the last one also keeps a reference to its x_hat (no extra work inside the region)
        last = {}

        def timed_step(item):
            i, x = item
            out, x_hat = decoded(x)
            if i == args.steps - 1:
                last["out"], last["x_hat"] = out, x_hat
            return out, finite_probe(x_hat)
        results = pipe.map(timed_step, [(i, frames[i % pool]) for i in range(args.steps)])
    if clk is not None:
        clk.stop()               # joins the probe thread; its last 50 us probe is covered by the sync below
    torch.cuda.synchronize()
    elapsed_own = time.perf_counter() - t0           # this rank's K round trips (the job's time: after the barrier, max over ranks)
    D.barrier()
    elapsed = time.perf_counter() - t0
    STAGE[0] = "after the timed region"
    _cra5_lib().cra5_clock_stamp(ctypes.c_void_p(region_marks.data_ptr() + 8), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    ops.TIMER = None
    net.host_log = None
    clocks = {"timed_region": clk.summary() if clk is not None else None,
              "hwmon": hw.stop() if hw is not None else None,
              "how": "timed_region: a one-wave probe every 5 ms beside the workload (cra5_clock_probe: shader cycles over a "
                     "50 us window of the 100 MHz wall clock, on whichever CU the wave lands).  hwmon: amdgpu sysfs files read "
                     "every 20 ms by a host thread (`static` = they did not move)"}
    if args.dump_outputs is not None:
        if rank == 0:
            dump_outputs(args.dump_outputs, last["out"], last["x_hat"])
        last.clear()
    rows = [D.frame_stats(my_frames[i], out["strings"], out.get("n_escape", [-1])[0]) for i, (out, _) in enumerate(results)]
    assert all(probe_ok(ok) for _, ok in results)
    # frames that re-use a pool tensor must reproduce its streams byte for byte (sizes + CRC): a race or a
    # non-deterministic reduction anywhere in the path would show up here (96-step default: every tensor coded 4 times)
    first_seen = {1000 + my_frames[0] + slot: r for slot, r in warm_rows.items()}
    n_warm_keys = len(first_seen)
    for i, row in enumerate(rows):
        key = seed_of_step[i]
        if key in first_seen:
            assert row[1:] == first_seen[key], f"frame of seed {key} coded differently on re-use: {row[1:]} vs {first_seen[key]}"
        else:
            first_seen[key] = row[1:]
    repeats_checked = len(rows) - (len(first_seen) - n_warm_keys)
    elapsed = D.max_over_ranks(elapsed, dev)
    stats = D.gather_stats(rows, dev)  # RCCL all-gather of per-frame bitstream stats
    # every frame of the job is accounted for exactly once, on every rank
    assert stats[:, 0].tolist() == list(range(world * args.steps)), "gathered stats do not cover the frame set"
    hosts = D.gather_objects(dict(D.host_report(), numa_bind=D.LAST_BIND)) if world > 1 else None
    per_rank = D.gather_objects(per_rank_line(rank, args.steps, elapsed_own, clocks["timed_region"], host_log))

    if rank == 0 and os.environ.get("CRA5_BENCH_STATS_OUT"):
        json.dump(stats.cpu().tolist(), open(os.environ["CRA5_BENCH_STATS_OUT"], "w"))
    total_frames = world * args.steps
    fps = total_frames / elapsed
    result = {
        "metric": "ERA5 frames/s (721x1440x268) encode+decode",
        "value": fps, "unit": "frames/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": 1e3 * elapsed / args.steps, "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "f32" if net.gemm_mode == "f32" else (
            "f32 (3xf16-split MFMA, fp32 accumulate)" if net.precision == "fp32" else
            "f16 operands / fp32 accumulate in g_a,g_s (reduced precision, configs[4]); hyper-prior fp32-accurate"),
        "data": "synthetic",
        "config": {"workload": f"quality={C} single-frame full encode->bin->decode round trip per step "
                               f"(BASELINE.json configs[2]); 1 frame/rank/step; job frames f = 0..{world * args.steps - 1} "
                               f"block-sharded over ranks; " + (
                                   "every frame its own tensor x_f ~ N(0,1), seed 1000+f (configs[3]'s set)"
                                   if pool >= len(my_frames) else
                                   f"{pool} distinct tensors per rank (x ~ N(0,1), seeds 1000+first+(i % {pool})) REUSED "
                                   f"round-robin by the rank's {len(my_frames)} frames"),
                   "frame": [C, 721, 1440], "weights": "deterministic synthetic (cra5_amd/synth.py seed 7)",
                   "parallelism": f"frame-sharded x{world}, weights replicated",
                   "distinct_frames_per_rank": pool, "frame_seeds_rank0": [seed_of_step[0], seed_of_step[-1]],
                   "frames_in_flight_per_gpu": args.inflight, "preflight": pre,
                   # the run's settings as ONE object (cra5_amd/config.py: defaults < CRA5_* environment < bench.py flags)
                   "runtime": dict(rc.replace(inflight=args.inflight).describe(), native_library=os.path.basename(LIB_PATH)),
                   "host": {"frame_threads_total": args.inflight * world, "host_threads": os.cpu_count(),
                            "numa_bind_rank0": numa, "self_launched": os.environ.get("CRA5_SELF_LAUNCHED") == "1",
                            # N > 1: every rank's CPU mask after the bind, and how many of its threads (frame threads,
                            # rANS pool, RCCL / HIP helpers) have a mask outside it - must be 0
                            "per_rank": None if hosts is None else [
                                {"rank": h["rank"], "n_cpus": h["n_cpus"], "cpu_span": [h["cpus"][0], h["cpus"][-1]] if h["cpus"] else [],
                                 "threads": h["threads"], "threads_outside_mask": h["threads_outside_mask"],
                                 "outside_names": h.get("outside_names"), "gpu_check": h.get("gpu_check"),
                                 "numa_node": (h.get("numa_bind") or {}).get("numa_node")} for h in hosts],
                            "cpu_sets_disjoint": None if hosts is None else _disjoint([h["cpus"] for h in hosts])}},
        "warmup_settle_frames": settle_frames,
        # every rank's OWN frames/s, shader clock and host rANS phase times: attribution of a < N x result (item 5c)
        "per_rank": per_rank,
        "clocks": clocks,
        "host_phase_ms": host_phase_summary(host_log),
        "collectives": {"initialized": bool(torch.distributed.is_available() and torch.distributed.is_initialized()),
                        "backend": (torch.distributed.get_backend() if torch.distributed.is_initialized() else None),
                        "data_path": "none (frames are independent)", "after_timed_region": "all_gather of int64[K,5] stats"},
        "bytes_per_frame": float(stats[:, 1:3].sum().item()) / max(total_frames, 1),
        "determinism_check": {"repeated_frames_with_identical_streams_rank0": repeats_checked,
                              "note": "frames of the timed region whose tensor was coded before (in the warm-up or earlier in "
                                      "the region) and reproduced its stream sizes, CRC and escape count"},
        "stats_fields": list(D.STATS_FIELDS),
        "escape_symbols_per_frame": float(stats[:, 4].clamp(min=0).sum().item()) / max(total_frames, 1),
        "model_tflops": FLOP_PER_FRAME * fps / 1e12,
        # whole-path algorithmic rate against the engine's MFMA ceiling (SURVEY 8d "report both")
        "mfma_fraction_end_to_end": FLOP_PER_FRAME * fps / world / (
            (PEAK_FP32_MFMA_TFLOPS if net.gemm_mode == "f32" else
             PEAK_F16_MFMA_TFLOPS / (3.0 if net.precision == "fp32" else 1.0)) * 1e12),
    }
    if args.full:
        # frames 0 / 1 of the job (rank 0 owns them): product stream vs the stream the reference's Python wrote for the same tensor
        result["reference_pinned_frames"] = {str(1000 + f): reference_pinned(1000 + f, results[i][0]["strings"])
                                             for i, f in enumerate(my_frames) if f < 2 and i < pool} or None

    def measured_traffic():
        """HBM-side bytes per gemm launch from the committed rocprofv3 PMC passes (FETCH_SIZE
        x2 + WRITE_SIZE, corrected as MI355X_MICROARCH.md prescribes); PMC collection needs its
        own profiler runs, so bench.py reports the committed measurement, not a live one."""
        try:
            import glob
            import re
            # rNN_traffic.json: the fp32-accurate mode; rNN_f16_traffic.json: the reduced-precision mode (plain rows)
            pat = re.compile(r"r\d+_f16_traffic\.json$" if net.precision == "f16" else r"r\d+_traffic\.json$")
            latest = sorted(p for p in glob.glob(os.path.join(ROOT, "profiles", "r*_traffic.json"))
                            if pat.search(os.path.basename(p)))[-1]
            t = json.load(open(latest))
            return t["gemm_nt_split"]["avg_bytes_per_launch"]
        except Exception:  # noqa: BLE001
            return None

    def sustained_peak():
        """The independent yardstick for the all-CU ceiling: the vendor library's plain-f16 GEMM on
        random operands on an MI355X of this pool, committed under profiles/ (tools/vendor_gemm_yardstick.py - a
        measurement tool, never linked into the product).  Its best ISSUED f16 MFMA rate is what a dense f16 kernel
        sustains on all 256 CUs under the chip's power management; / 3 MFMAs per product = the fp32-equivalent ceiling."""
        try:
            import glob
            path = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_vendor_gemm_yardstick.json")))[-1]
            y = json.load(open(path))
            best = max((v["vendor_f16"]["tflops_issued"], k) for k, v in y["shapes"].items())
            k1024 = {k: {"vendor_f16_issued": v["vendor_f16"]["tflops_issued"],
                         "product_issued": max(v["product_split_f32out"]["tflops_issued"], v["product_split_splitout"]["tflops_issued"])}
                     for k, v in y["shapes"].items()}
            return {"file": "profiles/" + os.path.basename(path), "vendor_f16_tflops_issued_best": best[0], "shape": best[1],
                    "vendor_f16_zero_filled": y.get("big_zero_filled_vendor", {}).get("tflops_issued"), "per_shape": k1024}
        except Exception:  # noqa: BLE001
            return None

    def roofline_from(summ, steps, sample=1):
        """sample = n: the timer bracketed every n-th launch; per-step totals are scaled back up."""
        out = {}
        g = summ.get("gemm_nt_split")
        if g and g["ms"] > 0:
            # algorithmic (fp32-equivalent) flops: 2*M*N*K per launch.  The kernel issues 3 f16
            # MFMAs per algorithmic product (hi.hi + hi.lo + lo.hi), so its ceiling is the dense
            # f16 MFMA peak / 3.
            ach = g["work"] / (g["ms"] * 1e-3) / 1e12
            nprod = 3.0 if net.precision == "fp32" else 1.0
            peak = PEAK_F16_MFMA_TFLOPS / nprod
            out["roofline"] = {"kernel": "gemm_nt_split_kernel<2,4,{3|4},2> (192x256 / 256x256 tiles)", "bound": "mfma", "achieved": ach, "peak": peak,
                               "unit": "TFLOP/s", "frac": ach / peak, "traffic": measured_traffic(),
                               "traffic_note": "bytes/launch at the L2<->fabric boundary (Infinity-Cache hits "
                                               "included), newest profiles/rNN_traffic.json (rNN_f16_traffic.json in the reduced-precision mode); algorithmic minimum "
                                               "A + W + C = 55-230 MB/launch",
                               "peak_note": "dense f16 MFMA peak 2500 TF at the nominal 2.4 GHz / %d MFMA(s) per product.  The chip "
                                            "does not hold 2.4 GHz under this kernel: one round of 256x256 tiles (K = 8192) runs "
                                            "at 2.30 GHz on 32 CUs (main loop 791 TF-equivalent per 256 CUs = 95 %% of `peak`) and "
                                            "at 1.49 GHz on all 256 (502: 60 %%) - profiles/r04_active_cu_sweep.txt; the "
                                            "sustained all-CU ceiling of this instruction mix is ~0.62 x `peak`" % nprod,
                               "peak_sustained": (lambda sp: None if sp is None else dict(
                                   sp, value=sp["vendor_f16_tflops_issued_best"] / nprod, unit="TFLOP/s",
                                   frac_of_sustained=ach / (sp["vendor_f16_tflops_issued_best"] / nprod),
                                   note="pre-recorded yardstick, not a measurement of this run: the vendor BLAS's plain-f16 GEMM "
                                        "on random normal operands sustains this ISSUED f16 rate on all 256 CUs (2048 TF on "
                                        "zero-filled operands: the gap is data-dependent power management); per shape the "
                                        "product's kernel issues f16 MFMAs at the vendor's rate or above, so `peak` (2500 / 3 "
                                        "nominal) is not reachable by any kernel of this mix - `frac_of_sustained` is the "
                                        "fraction of what the chip sustains"))(sustained_peak()),
                               "mfma_tflops_issued": nprod * ach, "launches": g["launches"],
                               "avg_launch_ms": g["ms"] / g["launches"], "gemm_ms_per_step": g["ms"] * sample / steps,
                               "launches_sampled_every": sample}
        gs = summ.get("gemm_nt_split_small")
        if gs and gs["ms"] > 0 and "roofline" in out:
            out["roofline"]["small_tile_launches"] = {
                "kernel": "gemm_nt_split_kernel<2,2,1,1> (64x64 tiles: hyper-prior / head GEMMs, launch-bound)",
                "launches": gs["launches"], "ms_per_step": gs["ms"] * sample / steps,
                "achieved": gs["work"] / (gs["ms"] * 1e-3) / 1e12}
        g = summ.get("gemm_nt_f32")
        if g and g["ms"] > 0 and "roofline" not in out:
            ach = g["work"] / (g["ms"] * 1e-3) / 1e12
            out["roofline"] = {"kernel": "gemm_nt_f32_kernel", "bound": "mfma", "achieved": ach,
                               "peak": PEAK_FP32_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": ach / PEAK_FP32_MFMA_TFLOPS,
                               "traffic": None, "launches": g["launches"], "avg_launch_ms": g["ms"] / g["launches"],
                               "gemm_ms_per_step": g["ms"] * sample / steps}
        mem = {}
        for kind in ("layernorm", "im2col", "col2im"):
            k = summ.get(kind)
            if k and k["ms"] > 0:
                gbs = k["work"] / (k["ms"] * 1e-3) / 1e9
                mem[kind] = {"achieved_GBps": gbs, "frac_of_hbm_peak": gbs / PEAK_HBM_GBPS, "launches": k["launches"],
                             "ms_per_step": k["ms"] * sample / steps}
        if mem:
            out["hbm_bound_kernels"] = dict(mem, peak_GBps=PEAK_HBM_GBPS,
                                            note="algorithmic bytes / HIP-event duration per launch; 8 TB/s HBM3E peak")
        a = summ.get("window_attention_split") or summ.get("window_attention_f32")
        if a and a["ms"] > 0:
            out["attention"] = {"kernel": "window_attention_split_kernel" if "window_attention_split" in summ
                                else "window_attention_f32_kernel",
                                "achieved_tflops": a["work"] / (a["ms"] * 1e-3) / 1e12,
                                "launches": a["launches"], "ms_per_step": a["ms"] * sample / steps}
        return out

    if timer is not None:
        timed = roofline_from(timer.summary(), args.steps, args.timer_sample)
        # In the timed region only every n-th launch is bracketed (and, in the default mode, launches of
        # concurrent frames overlap, so start->stop of one launch also contains other frames' kernels).
        # Keep those numbers, and (--full) time EVERY launch of the same kernels un-overlapped in a short extra
        # pass outside the timed region.
        result["roofline_timed_region"] = timed.get("roofline")
        result["attention_timed_region"] = timed.get("attention")
    if timer is not None and args.full:
        net.gpu_exclusive = True
        ops.TIMER = t2 = ops.KernelTimer()
        pipe.roundtrip([frames[i % pool] for i in range(max(1, args.roofline_steps))])
        torch.cuda.synchronize()
        ops.TIMER = None
        result.update(roofline_from(t2.summary(), max(1, args.roofline_steps)))
        if "roofline" in result:
            rp = rocprof_gemm_frac(f16=args.precision == "f16")
            if rp:   # NOT a measurement of this run: the committed rocprofv3 summary of an earlier build, for comparison
                result["roofline"]["committed_reference"] = dict(
                    rp, note="pre-recorded profiles/" + rp["file"] + " (rocprofv3 --kernel-trace --stats of the exclusive "
                             "bench command at the commit that added the file; `git log -1 -- profiles/" + rp["file"] +
                             "`); everything else in `roofline` was measured by this run")
            if net.gemm_mode != "f32" and args.precision == "fp32" and rank == 0 and world == 1 and not args.no_best_case:
                # The same kernel on its best-case shape, measured live: ONE exact round of 256 x 256 tiles (256 tiles on
                # 256 CUs), K = 8192 - prologue / epilogue amortised over 256 k-steps, no partial round.  What is left
                # between this figure and `peak` is the clock the chip sustains under the instruction mix (DESIGN.md
                # section 6.1); what is left between `achieved` and this figure is the model's short-K shapes.
                try:
                    g = torch.Generator(device=dev).manual_seed(5)
                    Mb, Nb, Kb = 256 * (torch.cuda.get_device_properties(dev).multi_processor_count // 8), 2048, 8192
                    ab = ops.split_f16(torch.randn((Mb, Kb), generator=g, device=dev))
                    wb = ops.split_f16(torch.randn((Nb, Kb), generator=g, device=dev) * 0.02, "auto")
                    ob = torch.empty((Mb, Nb), device=dev)
                    for _ in range(3):
                        ops.gemm_nt_split(ab, wb, out=ob)
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    if clk is not None:
                        clk.n = 0
                    e0.record()
                    for i in range(20):
                        ops.gemm_nt_split(ab, wb, out=ob)
                        if clk is not None and 2 <= i < 18:
                            clk.probe()          # (lands beside one of the queued launches)
                    e1.record()
                    torch.cuda.synchronize()
                    tb = e0.elapsed_time(e1) / 20 * 1e-3
                    ach_b = 2.0 * Mb * Nb * Kb / tb / 1e12
                    result["roofline"]["best_case_shape"] = {
                        "shape_mnk": [Mb, Nb, Kb], "achieved": ach_b, "frac": ach_b / result["roofline"]["peak"],
                        "launch_ms": tb * 1e3, "clock": clk.summary() if clk is not None else None,
                        "note": "same kernel, one exact round of tiles, K = 8192, 20 back-to-back launches on the current "
                                "stream (256 x 256 tiles, 8 tile columns x CUs / 8 tile rows); the all-CU sustained clock, not the kernel, sets this "
                                "figure (profiles/r04_active_cu_sweep.txt)"}
                    del ab, wb, ob
                except Exception as ex:  # noqa: BLE001
                    result["roofline"]["best_case_shape"] = {"achieved": None, "error": repr(ex)}
            result["roofline"]["measured_over"] = (
                f"a separate un-overlapped pass of {max(1, args.roofline_steps)} frames run right after the timed "
                "region (HIP events around every launch, on the launch stream, exclusive GPU phases); "
                "`roofline_timed_region` holds the sampled measurement taken inside the timed region, where "
                "launches of concurrent frames overlap and per-launch durations are inflated")
    # the legs below run on rank 0 of a 1-rank job, with --full only
    side_legs = rank == 0 and world == 1 and args.full
    if side_legs and args.precision == "fp32" and not args.no_f16_sample and args.quality == 268 \
            and net.gemm_mode != "f32":
        # BASELINE.json configs[4] (reduced precision: plain f16 operands in g_a / g_s, fp32 accumulate, hyper-prior and
        # GaussianConditional fp32-accurate) on THIS GPU: a short sample outside the timed region - frames/s of the same
        # pipeline, and the error it buys against the fp32-accurate run on the same frame.  Never part of `value`.
        try:
            net.gpu_exclusive = False
            rm = lambda a, b: float(torch.sqrt(torch.mean((a.double() - b.double()) ** 2)))  # noqa: E731
            x0 = frames[0]
            y32 = net.encode_latent(x0, type='float')[0]
            y_hat = torch.round(y32)
            xh32 = net.decode_latent(y_hat)
            net.precision = "f16"
            y16 = net.encode_latent(x0, type='float')[0]
            xh16 = net.decode_latent(y_hat)
            e_y, e_x, y_rms = rm(y16, y32), rm(xh16, xh32), float(torch.sqrt(torch.mean(y32.double() ** 2)))
            del y32, y16, xh32, xh16, y_hat
            n16 = 10 * args.inflight
            pipe.map(round_trip, [frames[i % pool] for i in range(2 * args.inflight)])   # first use of the f16 instantiations
            torch.cuda.synchronize()
            t16 = time.perf_counter()
            r16 = pipe.map(round_trip, [frames[i % pool] for i in range(n16)])
            torch.cuda.synchronize()
            t16 = time.perf_counter() - t16
            assert all(probe_ok(ok) for _, ok in r16)
            result["precision_f16"] = {
                "value": n16 / t16, "unit": "frames/s", "frames": n16, "ratio_to_fp32_value": n16 / t16 / fps,
                "y_rmse_vs_fp32_run": e_y, "y_rms": y_rms, "x_hat_rmse_vs_fp32_run_same_y_hat": e_x,
                "gate": "BASELINE configs[4]: RMSE within 1e-2..1e-3 of the fp32 path (tests/test_model_gpu.py::"
                        "test_full268_reduced_precision_mode asserts it against the reference golden)",
                "what": "same pipeline and frames as the timed region with CRA5_PRECISION=f16 (1 MFMA per product in g_a / "
                        "g_s GEMMs and attention; h_a / h_s / entropy side unchanged so both sides derive the same CDF "
                        f"indexes); g_a / g_s activations and weights as PLAIN f16 rows (VAEformer.f16_layout = {net.f16_layout!r}); "
                        f"{n16}-frame region after two warm batches, outside the timed region",
                "frac_of_f16_roofline": FLOP_PER_FRAME * n16 / t16 / (PEAK_F16_MFMA_TFLOPS * 1e12)}
        except Exception as ex:  # noqa: BLE001
            result["precision_f16"] = {"value": None, "error": repr(ex)}
        finally:
            net.precision = "fp32"
    if side_legs and not args.no_api_sample and args.quality == 268:
        # What a drop-in caller of the REFERENCE-NAMED single-frame methods sees (test.py:14-45 in the reference):
        # encode_era5_as_bin(host array -> .bin on disk) + decode_from_bin(.bin -> x_hat on the device), one frame at
        # a time on one thread, PCIe-inclusive.  Outside the timed region; never part of `value`.
        try:
            import tempfile
            from cra5_amd.api import cra5_api
            net.gpu_exclusive = False
            tmp = tempfile.mkdtemp(prefix="cra5_bench_")
            import contextlib
            with contextlib.redirect_stdout(sys.stderr):    # (the reference API prints its device: stdout is the JSON line's)
                api = cra5_api(local_root=tmp, device="cuda", weights=net)
            host = (frames[0][0] * api.std + api.mean).cpu().numpy()      # physical units, pageable host memory
            ts, te, td = "2024-06-01T00:00:00", [], []
            for _ in range(4):
                t0 = time.perf_counter()
                api.encode_era5_as_bin(ts, save_root=tmp + "/CRA5", data=host)
                t1 = time.perf_counter()
                api.decode_from_bin(ts, return_format="de_normalized")
                td.append(time.perf_counter() - t1)
                te.append(t1 - t0)
            e, d = sorted(te[1:])[1], sorted(td[1:])[1]
            try:
                budget = single_frame_budget(api, host)
            except Exception as ex:  # noqa: BLE001
                budget = {"error": repr(ex)}
            # the same call pair under the entropy-matched weight variant (a trained model's stream sizes: the serial rANS
            # phases are what differs - cra5_amd/synth.py)
            matched_budget = None
            try:
                synth.apply_variant(net, seed=7, variant="matched")
                matched_budget = single_frame_budget(api, host)
            except Exception as ex:  # noqa: BLE001
                matched_budget = {"error": repr(ex)}
            finally:
                synth.apply_variant(net, seed=7, variant="default")
            result["api_single_frame"] = {
                "value": 1.0 / (e + d), "unit": "frames/s", "encode_s": e, "decode_s": d, "threads": 1,
                "budget_ms": budget, "entropy_matched_weights": matched_budget,
                "what": "cra5_api.encode_era5_as_bin(data=host fp32 array) + decode_from_bin('de_normalized'), serial, "
                        "H2D of the 1.11 GB frame and .bin write / read included, x_hat left on the device as the "
                        "reference does (tools/api_testpy_loop.py times every call of the reference's test.py loop)"}
            import shutil
            shutil.rmtree(tmp, ignore_errors=True)
        except Exception as ex:  # noqa: BLE001
            result["api_single_frame"] = {"value": None, "error": repr(ex)}
    if side_legs and not args.no_matched_sample and args.quality == 268 and args.precision == "fp32":
        try:
            result["entropy_matched"] = matched_sample(
                net, pipe, frames, max(20, 2 * args.inflight),
                {"value": fps, "bytes_per_frame": result["bytes_per_frame"],
                 "escape_symbols_per_frame": result["escape_symbols_per_frame"], "host_phase_ms": result["host_phase_ms"]})
        except Exception as ex:  # noqa: BLE001
            result["entropy_matched"] = {"value": None, "error": repr(ex)}
    if side_legs and not args.no_api_sample and args.quality == 268:
        try:
            result["api_pipelined"] = api_pipelined_sample(net, pipe, frames, args.inflight, args.api_frames)
        except Exception as ex:  # noqa: BLE001
            result["api_pipelined"] = {"value": None, "error": repr(ex)}
    if side_legs and not args.no_cpu_baseline:
        # The reference's CPU path on THIS box's host cores, in THIS run, after every GPU leg so that a
        # host busy with the oracle cannot touch `value`.  The pipeline's frame threads are idle by now; the NUMA bind of
        # the GPU legs is lifted (the oracle gets every core of the box, as a CPU user of the reference would have).
        STAGE[0] = "cpu baseline"
        try:
            pipe.close()
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            try:
                D._pin_all_threads(all_cpus)
            except OSError:
                pass
            live = (cpu_baseline_full if args.cpu_baseline == "full" else cpu_baseline)(args.quality, cpu_threads)
            live["measured_in_this_run"] = True
            live["box"] = os.uname().nodename
            import glob
            full = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_cpu_baseline_full.json")))
            if full:
                # an earlier round's whole-frame run on another box of the pool, for comparison only (never `value`)
                cb = json.load(open(full[-1])).get("cpu_baseline", {})
                live["whole_frame_committed"] = {"value": cb.get("value"), "cores": cb.get("cores"), "cpu": cb.get("cpu"),
                                                 "file": "profiles/" + os.path.basename(full[-1]), "pre_recorded": True}
            result["cpu_baseline"] = live
        except Exception as e:  # noqa: BLE001
            result["cpu_baseline"] = {"value": None, "error": repr(e)}
    if rank == 0:
        print(json.dumps(result), flush=True)
        try:
            open(os.path.join(_job_dir(), "line_printed"), "w").close()
        except OSError:
            pass
    pipe.close()
    if torch.distributed.is_available() and torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    import faulthandler
    faulthandler.enable()            # a rank killed by SIGSEGV / SIGABRT at least leaves its Python stack on stderr
    try:
        main()
    except SystemExit as e:
        # a refusal with a message (WORLD_SIZE mismatch, no GPU, ...) is a death before the timed region too; an integer
        # code is the self-launcher handing the job's exit code through
        if isinstance(e.code, str):
            error_line(e, STAGE[0])
        raise
    except BaseException as e:  # noqa: BLE001
        error_line(e, STAGE[0])
        raise
