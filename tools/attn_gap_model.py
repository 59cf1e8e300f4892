#!/usr/bin/env python
"""Static issue-slot model of the fp32-accurate attention key loop (no GPU needed).

    python tools/attn_gap_model.py [--source FILE.hip] [--keep-asm OUT.s]

Compiles cra5_amd/csrc/attention_split_f16.hip device-only to assembly with the release flags of cra5_amd/build.py,
finds in every fp32-accurate instantiation of window_attention_split_kernel the basic blocks that hold one key tile
(24 v_mfma) and prices what sits between consecutive MFMAs with the measured issue costs of one wave's stream:

    v_exp*            8 cycles
    any other v_*     4
    s_nop             4
    everything else   0   (LDS / global / scalar instructions go through other ports)

An MFMA holds the vector issue port for 8 of its 32 cycles, so a gap runs about max(32, 8 + fillers) and a tile about
the sum of that over its 24 gaps; 24 x 32 = 768 is the floor.  The gap that closes the block (after the last MFMA, up
to the block's end, plus the block's head in front of its first MFMA) is the loop-carried one and is listed first.
Opcodes are classified by these prefixes only: the model knows nothing about dependencies, LDS latency or the other
waves of the SIMD.  It says where a wave's own stream cannot keep the matrix pipe fed, not how long a tile takes.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cra5_amd import build as cbuild  # noqa: E402

SRC = "attention_split_f16.hip"
MFMA_CYCLES, MFMA_ISSUE, TILE_MFMAS = 32, 8, 24
KERNEL = re.compile(r"window_attention_split_kernelILi(\d+)ELb([01])ELb([01])ELb([01])ELb([01])EE")


def compile_asm(source, out):
    cmd = [cbuild.HIPCC, "--offload-arch=gfx950", "-std=c++17", "-fPIC"] + cbuild.FLAVOURS["release"]["dev"] + \
          cbuild.EXTRA.get(SRC, []) + ["-I", cbuild.CSRC, "--offload-device-only", "-S", source, "-o", out]
    subprocess.check_call(cmd, stderr=subprocess.DEVNULL)


def cost(op):
    if op.startswith("v_mfma"):
        return None
    if op.startswith("v_exp"):
        return 8
    if op.startswith("v_") or op.startswith("s_nop"):
        return 4
    return 0


def kernels(lines):
    """-> [(mangled name, body lines, {resource: value})] of every kernel in the assembly"""
    out, name, body = [], None, []
    for ln in lines:
        m = re.match(r"^(_Z\w+):", ln)
        if m:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        body.append(ln)
        if ln.startswith("; Occupancy:"):
            res = {}
            for b in body:
                r = re.match(r"^; (NumVgprs|ScratchSize|Occupancy): (\d+)", b)
                if r:
                    res[r.group(1)] = int(r.group(2))
            out.append((name, body, res))
            name = None
    return out


def blocks(body):
    """basic blocks: split at labels and behind branches; each a list of opcodes"""
    cur, out = [], []
    for ln in body:
        s = ln.split(";")[0].strip()
        if not s or s.startswith("."):
            if re.match(r"^\.LBB\w+:", s) and cur:
                out.append(cur)
                cur = []
            continue
        op = s.split()[0]
        cur.append(op)
        if op.startswith("s_cbranch") or op.startswith("s_branch") or op.startswith("s_endpgm"):
            out.append(cur)
            cur = []
    if cur:
        out.append(cur)
    return out


def gaps_of(block):
    """filler cycles by gap, the loop-carried gap (tail + head of the block) first; and the v_exp count by gap"""
    fill, exps = [0], [0]   # [0] collects the head, the tail is added to it
    seen = 0
    for op in block:
        c = cost(op)
        if c is None:
            seen += 1
            if seen < TILE_MFMAS:
                fill.append(0)
                exps.append(0)
            continue
        idx = 0 if seen in (0, TILE_MFMAS) else seen
        fill[idx] += c
        exps[idx] += 1 if op.startswith("v_exp") else 0
    return fill, exps


def report(asm_lines, out=sys.stdout):
    worst = 0
    for name, body, res in kernels(asm_lines):
        m = KERNEL.search(name)
        if not m or m.group(2) != "0":     # HI = false: the fp32-accurate form
            continue
        nw, _, glob, bal, _ = m.groups()
        tag = f"NW={nw} " + ("global balanced" if bal == "1" else "global plain" if glob == "1" else "windowed")
        print(f"== {tag}: VGPRs {res.get('NumVgprs')}  scratch {res.get('ScratchSize')}  occupancy {res.get('Occupancy')}", file=out)
        n = 0
        for blk in blocks(body):
            if sum(1 for op in blk if op.startswith("v_mfma")) != TILE_MFMAS:
                continue
            fill, exps = gaps_of(blk)
            model = sum(max(MFMA_CYCLES, MFMA_ISSUE + f) for f in fill)
            others = sum(1 for op in blk if op.startswith("v_") and not op.startswith("v_mfma"))
            nops = sum(1 for op in blk if op.startswith("s_nop"))
            worst = max(worst, model)
            print(f"  key-tile block {n}: {others} other vector instructions, {nops} s_nop", file=out)
            print(f"    fillers by gap (loop-carried first): {', '.join(str(f) for f in fill)}", file=out)
            print(f"    v_exp by gap:                        {', '.join(str(e) for e in exps)}", file=out)
            print(f"    filler cycles {sum(fill)}  empty gaps {sum(1 for f in fill if f == 0)} of {TILE_MFMAS}  "
                  f"largest gap {max(fill)}  model {model} cycles per tile  (floor {MFMA_CYCLES * TILE_MFMAS}, "
                  f"ratio {model / (MFMA_CYCLES * TILE_MFMAS):.3f})", file=out)
            n += 1
        if n == 0:
            print("  no basic block with 24 MFMAs found", file=out)
    return worst


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--source", default=os.path.join(cbuild.CSRC, SRC), help="the .hip file to model (default: the tree's)")
    ap.add_argument("--keep-asm", default=None, help="write the assembly here instead of a temporary file")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as td:
        asm = a.keep_asm or os.path.join(td, "attn.s")
        compile_asm(a.source, asm)
        with open(asm) as f:
            report(f.read().splitlines())


if __name__ == "__main__":
    main()
