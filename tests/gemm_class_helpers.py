"""Launch classes of cra5_gemm_nt_split, enumerated from the form rule (ops.gemm_form = cra5_gemm_split_form) over a fixed
grid of calls - shared by tests/test_gemm_classes_cpu.py (the enumeration, its representatives and their operands) and
tests/test_gemm_classes_gpu.py (one launch set per class).

The CLASS of a call is everything that selects code in the launcher and the kernel: the tile, the product count of the
instantiation (3, or in the reduced-precision mode 2 with 64-wide k-steps, else 1), one-launch long K, chaining, the
plain bits of the mode word, CRA5_GEMM_WIDE_K, the outputs and GELU.  Everything but the call's own flags is read off
the rule's answer; nothing here restates the rule.  A refused call's class is "refused" plus the inputs a refusal can
depend on.  The REPRESENTATIVE of a class is the grid member with the smallest M * N * Kp.

The operands of a representative live on the exact grid of tests/exact_helpers.py.  Nothing here initialises a GPU or
calls a product kernel (the form query is host arithmetic)."""
import functools
import itertools
from collections import namedtuple

import exact_helpers as X
from cra5_amd import ops

# M x N: 1 / 72 / 162 / 258 / 297 / 306 / 774 ... tiles of 128 x 128 - both sides of the 256-tile threshold with every
# combination of M >= 1024, N >= 512, N >= 2048; all ragged in M and N (no multiple of 64)
MS = (70, 1000, 1100, 2100, 4224 + 1, 11008 + 5)
NS = (77, 384 - 2, 1030, 2304 + 3)
# 1, 2 and 3 k-steps; the chaining boundary; long K with Kp % 64 = 32 and 0
KPS = (32, 64, 96, 8192, 8224, 8256)
OUTPUTS = ("f32", "split", "both")
MODE_BITS = (ops.GEMM_HI_ONLY, ops.GEMM_A_PLAIN, ops.GEMM_W_PLAIN, ops.GEMM_OUT_PLAIN, ops.GEMM_WIDE_K)
MODES = tuple(sum(b for b, on in zip(MODE_BITS, bits) if on) for bits in itertools.product((0, 1), repeat=len(MODE_BITS)))
PLAIN_ANY = ops.GEMM_A_PLAIN | ops.GEMM_W_PLAIN | ops.GEMM_OUT_PLAIN
PATTERN = 0x7e00                 # an f16 NaN: what an untouched half of a prefilled / poisoned buffer holds

Call = namedtuple("Call", "M N Kp mode gelu outputs")


def call_flags(c):
    return c.mode | (ops.EPI_GELU if c.gelu else 0)


def call_form(c):
    return ops.gemm_form(c.M, c.N, c.Kp, call_flags(c), c.outputs != "split", c.outputs != "f32")


def _plain_letters(mode):
    s = "".join(ch for ch, b in zip("AWO", (ops.GEMM_A_PLAIN, ops.GEMM_W_PLAIN, ops.GEMM_OUT_PLAIN)) if mode & b)
    return s or "-"


def n_products(c, form):
    """the NPROD of the instantiation the call is meant to run: 3 without CRA5_GEMM_HI_ONLY, else 2 with 64-wide k-steps,
    else 1"""
    return 3 if not c.mode & ops.GEMM_HI_ONLY else 2 if form & ops.FORM_K64 else 1


def class_key(c):
    """the class of a call, as one line of text (the committed list of tests/test_gemm_classes_cpu.py holds these)"""
    form = call_form(c)
    if form < 0:
        assert form == ops.ERR_ARG
        # long K: would the fp32-accurate mode chain this call (an fp32 output alone, no GELU) or run it in one launch?
        chain = ops.gemm_form(c.M, c.N, c.Kp, ops.EPI_GELU if c.gelu else 0, c.outputs != "split", c.outputs != "f32") & ops.FORM_CHAINED
        longk = "short" if c.Kp <= 8192 else "chainable" if chain else "one-launch"
        return (f"refused hi={int(bool(c.mode & ops.GEMM_HI_ONLY))} wide={int(bool(c.mode & ops.GEMM_WIDE_K))} "
                f"plain={int(bool(c.mode & PLAIN_ANY))} K={longk} Kp%64={c.Kp % 64}")
    chained = bool(form & ops.FORM_CHAINED)
    kind = "chained" if chained else "longk" if c.Kp > 8192 else "short"
    return (f"tile={form & ops.FORM_TILE} prod={n_products(c, form)} K={kind} plain={_plain_letters(c.mode)} "
            f"wide={int(bool(c.mode & ops.GEMM_WIDE_K))} out={c.outputs} gelu={int(c.gelu)}")


def grid():
    for M, N, Kp, mode, gelu, outputs in itertools.product(MS, NS, KPS, MODES, (False, True), OUTPUTS):
        yield Call(M, N, Kp, mode, gelu, outputs)


def _order(c):
    return (c.M * c.N * c.Kp, c.M, c.N, c.Kp, c.mode, c.gelu, OUTPUTS.index(c.outputs))


@functools.lru_cache(maxsize=None)
def enumerate_classes():
    """-> ({class key: representative Call}, {class key: number of grid members}), keys in sorted order"""
    rep, count = {}, {}
    for c in grid():
        k = class_key(c)
        count[k] = count.get(k, 0) + 1
        if k not in rep or _order(c) < _order(rep[k]):
            rep[k] = c
    keys = sorted(rep)
    return {k: rep[k] for k in keys}, {k: count[k] for k in keys}


def accepted():
    return [(k, c) for k, c in enumerate_classes()[0].items() if not k.startswith("refused")]


def refused():
    return [(k, c) for k, c in enumerate_classes()[0].items() if k.startswith("refused")]


def is_hi(c):
    return bool(c.mode & ops.GEMM_HI_ONLY)


# ------------------------------------------------------------------------------------------------ operands


def density(K):
    """the density rule of tests/test_exact_gpu.py (imported there: the module holds GPU tests but starts no GPU)"""
    from test_exact_gpu import _density
    return _density(K)


W_SCALE = 4096.0        # what ops.split_f16(w, "auto") picks for max |w| in [1, 2): the weight's hi plane holds +-4096


def seed_of(M, N, Kp):
    return 7 * M + 3 * N + Kp


def operands(M, N, Kp):
    """(a [M, Kp], w [N, Kp], bias [N], res [M, N]) fp32 on the CPU: the operands of every launch of a representative of
    this shape (K = Kp: no K padding, so every lo half of an operand row is a real lo half)"""
    s = seed_of(M, N, Kp)
    d = density(Kp)
    return (X.grid_matrix(M, Kp, d, s, lo_shift=12), X.grid_matrix(N, Kp, d, s + 1, lo_shift=12),
            X.grid_vector(N, s + 2), X.grid_matrix(M, N, 1.0, s + 3, lo_shift=12))


def term_bound(pa, pw, scale_inv, hi_only, bias=None, res=None):
    """An upper bound of max sum_k |term| (+ |bias| + |res|) in granules of 2^-12, from the planes alone, for shapes whose
    full float64 evaluation is too slow without a GPU: (number of k at which both rows are non-zero - one fp32 matrix
    product of 0 / 1 matrices, exact below 2^24) times the largest |term| any k can give."""
    ha, la = pa
    hw, lw = pw
    common = ((ha != 0) | (la != 0)).float() @ ((hw != 0) | (lw != 0)).float().t()
    mha, mla, mhw, mlw = (float(t.abs().max()) for t in (ha, la, hw, lw))
    per = mha * mhw if hi_only else mha * (mhw + mlw) + mla * mhw
    top = float(common.max()) * per * scale_inv
    for t in (bias, res):
        if t is not None:
            top += float(t.abs().max())
    return top / 2.0 ** -12
