"""A/B of two builds of the library on the attention launches of the model, interleaved in ONE process (needs the GPU):

    tools/build_variant.sh parent build_variants/parent_attention_split_f16.hip "" attention_split_f16.hip
    python tools/attn_ab.py --other build_variants/libcra5_parent.so [--rounds 30]

Shapes: the balanced whole-grid launch (10 368 tokens x 16 heads) and the windows (24, 24) / (12, 48) / (48, 12) of the
72 x 144 grid, fp32-accurate mode, split output.  Per shape: are the two builds' outputs torch.equal, and per build the
median and min..p90 of the per-launch time (device events), the launches of the two builds alternating A B A B ...; a
difference counts where one build's median lies outside the other's whole min..max spread."""
import argparse
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from cra5_amd import _lib, ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--other", required=True, help="the second library (the first is the product, or CRA5_LIB)")
ap.add_argument("--rounds", type=int, default=30)
a = ap.parse_args()

product = _lib.lib()
other = ctypes.CDLL(os.path.abspath(a.other))
for name, (res, args) in _lib.SIGNATURES.items():
    fn = getattr(other, name)
    fn.restype, fn.argtypes = res, args
LIBS = (("product", product), ("other", other))

dev = torch.device("cuda:0")
H, W, C, heads = 72, 144, 1024, 16
N = H * W
g = torch.Generator().manual_seed(1)
qkv = torch.randn(N, 3 * C, generator=g).to(dev)
bias = torch.randn(3 * C, generator=g).to(dev)
qs, ps = ops.split_f16(qkv), ops.split_f16(bias.reshape(1, -1))
ok, nb = ops.attention_balanced_plan(N, heads)
ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=dev) if ok else None
print(f"product = {_lib.LIB_PATH}\nother   = {os.path.abspath(a.other)}")
for name, (wh, ww) in (("global", (H, W)), ("w24", (24, 24)), ("w12x48", (12, 48)), ("w48x12", (48, 12))):
    kw = dict(workspace=ws) if name == "global" else {}
    outs, times = {}, {k: [] for k, _ in LIBS}
    for k, L in LIBS:
        _lib._lib = L
        o = ops.SplitMat.empty(N, C, dev, zero=True)
        for _ in range(2):
            ops.window_attention_split(qs, ps, heads, H, W, wh, ww, out_split=o, **kw)
        torch.cuda.synchronize()
        outs[k] = o
    same = torch.equal(outs["product"].data, outs["other"].data)
    for _ in range(a.rounds):
        for k, L in LIBS:
            _lib._lib = L
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.window_attention_split(qs, ps, heads, H, W, wh, ww, out_split=outs[k], **kw)
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3)
    _lib._lib = product
    print(f"{name:7s} outputs torch.equal: {same}")
    for k, _ in LIBS:
        t = np.array(times[k])
        print(f"    {k:8s} median {np.median(t):8.1f} us   min {t.min():8.1f} .. p90 {np.percentile(t, 90):8.1f}   max {t.max():8.1f}   (n = {len(t)})")
    tp, to = np.array(times["product"]), np.array(times["other"])
    verdict = "product faster" if np.median(tp) < to.min() else "other faster" if np.median(to) < tp.min() else "inside the spread"
    print(f"    product / other median {np.median(tp) / np.median(to):.3f}: {verdict}", flush=True)
