"""Operator-level GPU tests of the CNN codec kernels (cra5_amd/cnn.py) against float64 on the CPU, at the widths of the
production qualities (CNN_CFGS: N = 128 / 192, M = 192 / 320) and at the ragged shapes where gather kernels go wrong:
inputs smaller than the kernel, odd sizes, H != W, K not a multiple of 32, pixel counts off the GDN block size.

  conv2d            padded patch gather (conv_im2col_kernel) + split-f16 GEMM + transpose
  conv_transpose2d  transpose + split-f16 GEMM + gather overlap-add (deconv_col2im_kernel)
  gdn               gdn_kernel, forward and inverse, C up to the launcher's bound (512)
  unary             unary_kernel: relu / leaky_relu / abs bit-identical to torch, special values included
  transpose         transpose_kernel on row-strided views and degenerate shapes, bit-exact
  pixel_shuffle     p1 != p2 and an odd channel count, bit-exact

Every comparison prints one `ERR <family> ...` line (run with -s to collect them)."""
import math
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from cra5_amd import ops, synth
from cra5_amd._lib import Cra5Error, lib
from oracle import torch_ref as R

pytestmark = pytest.mark.gpu

# split-f16 GEMM accuracy class (tests/test_kernels_gpu.py::test_gemm_nt_split): operands carry ~22 bits (f16 hi + lo),
# products and sums are fp32; relative RMSE against float64 stays well below 2e-6 up to K = 29480
GEMM_REL_RMSE = 2e-6
U = 2.0 ** -24   # fp32 unit roundoff


def rel_rmse(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float(torch.sqrt(torch.mean((a - b) ** 2)) / max(float(torch.sqrt(torch.mean(b ** 2))), 1e-300))


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


# (Cin, Cout, k, stride, H, W, bias): the production layers (g_a / h_a / h_s convs of CNN_CFGS) and ragged ones.
# Cin = 3: K = 75 -> Kp = 96; Cin = 13: K odd; 1x1 and 2x3: the input is smaller than the kernel.
CONV_CASES = [
    (3, 192, 5, 2, 64, 96, True),      # g_a.0 at N = 192
    (3, 48, 5, 2, 33, 47, True),
    (13, 48, 5, 2, 5, 7, False),
    (13, 1, 3, 1, 2, 3, True),
    (13, 192, 3, 1, 64, 96, False),
    (192, 192, 5, 2, 33, 47, True),    # g_a.2 at N = 192: K = 4800
    (192, 320, 5, 2, 5, 7, True),      # g_a.6 at (192, 320)
    (192, 48, 5, 2, 1, 1, True),
    (320, 192, 3, 1, 5, 7, True),      # h_a.0 at (192, 320)
    (320, 1, 3, 1, 1, 1, False),
    (480, 640, 3, 1, 2, 3, True),      # mbt2018-mean h_s.4 at (192, 320): K = 4320, Cout = 2M
    (480, 13, 3, 1, 5, 7, False),
]


@pytest.mark.parametrize("cin,cout,k,s,H,W,bias", CONV_CASES)
def test_conv2d_vs_float64(dev, cin, cout, k, s, H, W, bias):
    g = _gen("conv", cin, cout, k, s, H, W, bias)
    x = torch.randn(cin, H, W, generator=g)
    w = torch.randn(cout, cin, k, k, generator=g) / math.sqrt(cin * k * k)
    b = torch.randn(cout, generator=g) if bias else None
    ws = ops.split_f16(w.reshape(cout, -1).contiguous().to(dev), "auto")
    out = ops.conv2d(x.to(dev), ws, b.to(dev) if bias else None, k, s)
    ref = F.conv2d(x[None].double(), w.double(), b.double() if bias else None, stride=s, padding=k // 2)[0]
    assert out.shape == ref.shape
    e = rel_rmse(out, ref)
    print(f"ERR conv2d Cin={cin} Cout={cout} k={k} s={s} {H}x{W} bias={bias}: rel rmse {e:.2e}")
    assert e < GEMM_REL_RMSE


# (Cin, Cout, k, stride, Hi, Wi, bias): Cout * k^2 = 75 (g_s.6), 4800 (g_s.0 / .2 / .4 at N = 192), 12000 (mbt2018-mean
# h_s.2 at M = 320); Hi or Wi = 1, odd sizes; one 3x3 stride-1 case (output_padding 0)
DECONV_CASES = [
    (192, 3, 5, 2, 33, 47, True),      # g_s.6 at N = 192
    (320, 192, 5, 2, 5, 7, True),      # g_s.0 at (192, 320)
    (192, 192, 5, 2, 1, 1, True),
    (320, 480, 5, 2, 2, 3, True),      # mbt2018-mean h_s.2 at (192, 320): N = 12000
    (192, 480, 5, 2, 1, 7, False),
    (13, 48, 5, 2, 7, 1, True),
    (3, 13, 5, 2, 5, 1, False),
    (48, 48, 5, 2, 64, 96, True),
    (13, 13, 3, 1, 5, 7, True),
]


@pytest.mark.parametrize("cin,cout,k,s,Hi,Wi,bias", DECONV_CASES)
def test_conv_transpose2d_vs_float64(dev, cin, cout, k, s, Hi, Wi, bias):
    g = _gen("deconv", cin, cout, k, s, Hi, Wi, bias)
    x = torch.randn(cin, Hi, Wi, generator=g)
    w = torch.randn(cin, cout, k, k, generator=g) / math.sqrt(cin)
    b = torch.randn(cout, generator=g) if bias else None
    ws = ops.split_f16(w.reshape(cin, -1).t().contiguous().to(dev), "auto")      # as cnn._Deconv
    out = ops.conv_transpose2d(x.to(dev), ws, b.to(dev) if bias else None, cout, k, s)
    ref = F.conv_transpose2d(x[None].double(), w.double(), b.double() if bias else None, stride=s, padding=k // 2,
                             output_padding=s - 1)[0]
    assert out.shape == ref.shape
    e = rel_rmse(out, ref)
    print(f"ERR conv_transpose2d Cin={cin} Cout={cout} k={k} s={s} {Hi}x{Wi} bias={bias}: rel rmse {e:.2e}")
    assert e < GEMM_REL_RMSE


# ---------------------------------------------------------------------------------------------------------- GDN

PED = (2.0 ** -18) ** 2


def _gdn_params(C, kind):
    """fp32 effective (beta, gamma) as cra5_amd.layers.GDN hands them to the kernel.  "init": the layer's own init
    (beta = 1, gamma = 0.1 I); "synth": the synthetic weights the golden fixtures use (beta in [1, 1.5), gamma =
    0.1 I + 0.02 |N(0, 1)|, every entry non-zero)."""
    if kind == "init":
        beta_p = torch.sqrt(torch.ones(C) + PED)
        gamma_p = torch.sqrt(torch.clamp(0.1 * torch.eye(C) + PED, min=PED))
    else:
        beta_p = synth.synth_tensor("g_a.1.beta", (C,), seed=C)
        gamma_p = synth.synth_tensor("g_a.1.gamma", (C, C), seed=C)
    beta = torch.clamp(beta_p, min=(1e-6 + PED) ** 0.5) ** 2 - PED        # NonNegativeParametrizer, in fp32
    gamma = torch.clamp(gamma_p, min=PED ** 0.5) ** 2 - PED
    return beta.contiguous(), gamma.contiguous()


def _gdn_ref(x, beta, gamma, inverse):
    """torch_ref.gdn in float64 on exactly the fp32 effective parameters: its re-parametrisation is undone in float64
    (p = sqrt(v + pedestal) -> p^2 - pedestal = v to ~1e-16)."""
    b64, g64 = beta.double(), gamma.double()
    return R.gdn(x.double(), torch.sqrt(b64 + PED), torch.sqrt(g64 + PED), inverse=inverse)


GDN_CHANNELS = [1, 3, 12, 63, 64, 65, 128, 192, 256, 257, 320, 512]
# (B, H, W, params): pixel counts 1, 63, 65 and 33 x 47 = 1551 (none a multiple of the kernel's 64-pixel block but 1551
# spans 25 blocks)
GDN_INPUTS = [(1, 1, 1, "init"), (3, 7, 9, "synth"), (1, 5, 13, "synth"), (3, 33, 47, "synth"), (1, 33, 47, "init")]


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("C", GDN_CHANNELS)
def test_gdn_vs_float64(dev, C, inverse):
    """Error model: per pixel the kernel forms n = beta + sum_j gamma[c, j] x_j^2 as a C-term fp32 chain of positive
    terms, then one sqrt (and a reciprocal and a product).  Each of the C additions rounds by at most u times the
    partial sum (<= n), the squares and products add one u each, so |dn| / n <= (C + 2) u; sqrt halves it, and the
    sqrt, reciprocal and final product add <= 5 u together (2 u of slack on sqrt / reciprocal):
        |y - y64| / |y64| <= ((C + 2) / 2 + 5) u  per element,  u = 2^-24.
    Rounding errors of a long chain are not all at their bound: their RMS stays far lower (~u sqrt(C) / 7); the
    RMS check below allows 1e-6, i.e. 16 u."""
    for B, H, W, kind in GDN_INPUTS:
        beta, gamma = _gdn_params(C, kind)
        x = torch.randn(B, C, H, W, generator=_gen("gdn", C, B, H, W, kind, inverse))
        y = ops.gdn(x.to(dev), beta.to(dev), gamma.to(dev), inverse=inverse).cpu()
        ref = _gdn_ref(x, beta, gamma, inverse)
        d = (y.double() - ref).abs()
        worst = float((d / ref.abs().clamp_min(1e-300)).max())
        e = rel_rmse(y, ref)
        bound = ((C + 2) / 2 + 5) * U
        print(f"ERR gdn C={C} inverse={inverse} B={B} {H}x{W} {kind}: rel rmse {e:.2e}, max rel {worst:.2e} "
              f"(bound {bound:.2e})")
        assert torch.all(d <= bound * ref.abs()), (B, H, W, kind, worst, bound)
        assert e < 1e-6, (B, H, W, kind, e)


def test_gdn_refuses_above_its_bound(dev):
    """C = 513 would need 64 px x 513 x 4 B = 131 KB of dynamic LDS per block: the launcher refuses it."""
    x = torch.ones(1, 513, 1, 1, device=dev)
    beta, gamma = torch.ones(513, device=dev), torch.eye(513, device=dev)
    with pytest.raises(Cra5Error) as e:
        ops.gdn(x, beta, gamma)
    assert e.value.status == -7          # CRA5_ERR_ARG
    assert lib().cra5_gdn_f32(x.data_ptr(), beta.data_ptr(), gamma.data_ptr(), x.data_ptr(), 1, 513, 1, 0, None) == -7


# ---------------------------------------------------------------------------------------------------------- unary

FLT_MAX = float(np.finfo(np.float32).max)
FLT_TRUE_MIN = float(np.finfo(np.float32).smallest_subnormal)


def _unary_input():
    """Random data around the special values: +-0, +-inf, NaN, +-FLT_MAX, +-denormals (smallest, mid, largest).  The
    length is not a multiple of 256 and exceeds the launcher's grid cap (4096 blocks x 256), so the grid-stride loop
    and the tail both run."""
    g = torch.Generator().manual_seed(31)
    x = torch.randn((1 << 20) + 4099, generator=g) * 3
    special = torch.tensor([0.0, -0.0, math.inf, -math.inf, math.nan, FLT_MAX, -FLT_MAX, FLT_TRUE_MIN, -FLT_TRUE_MIN,
                            1e-40, -1e-40, 1.1754942e-38, -1.1754942e-38, 1.1754944e-38, -1.1754944e-38, 1.0, -1.0],
                           dtype=torch.float32)
    idx = torch.randint(0, x.numel(), (4096,), generator=g)
    x[idx] = special[torch.arange(4096) % special.numel()]
    x[-special.numel():] = special          # and once at the very end
    return x


def _assert_bit_identical(got, ref, what):
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan), what
    assert torch.equal(got[~nan], ref[~nan]), what
    assert torch.equal(torch.signbit(got[~nan]), torch.signbit(ref[~nan])), what        # -0 vs +0
    zeros = (ref == 0)
    n_neg_zero = int(torch.signbit(ref[zeros]).sum())
    print(f"ERR unary {what}: bit-identical to torch on {got.numel()} values ({int(nan.sum())} NaN, "
          f"{int(zeros.sum())} zeros of which {n_neg_zero} negative)")


@pytest.mark.parametrize("op,slope", [("relu", None), ("leaky_relu", None), ("leaky_relu", 0.0), ("leaky_relu", 0.2),
                                      ("abs", None)])
def test_unary_bit_identical_to_torch(dev, op, slope):
    x = _unary_input()
    if op == "relu":
        ref = torch.relu(x)
    elif op == "abs":
        ref = torch.abs(x)
    else:
        ref = F.leaky_relu(x, 0.01 if slope is None else slope)
    got = (ops.unary(x.to(dev), op) if slope is None else ops.unary(x.to(dev), op, slope=slope)).cpu()
    _assert_bit_identical(got, ref, f"{op}(slope={slope})")


def test_relu_special_values(dev):
    """ReLU(-inf) = +0 (not -inf * 0 = NaN), ReLU(negative) = +0 (not -0), ReLU(-0) = -0, NaN propagates."""
    x = torch.tensor([-math.inf, -FLT_MAX, -1.0, -FLT_TRUE_MIN, -0.0, 0.0, math.nan, math.inf], device=dev)
    y = ops.unary(x, "relu").cpu()
    assert torch.equal(y[:4], torch.zeros(4)) and not torch.signbit(y[:4]).any()
    assert y[4] == 0 and torch.signbit(y[4]) and y[5] == 0 and not torch.signbit(y[5])
    assert torch.isnan(y[6]) and y[7] == math.inf
    # an explicit slope of 0 is honoured: torch.leaky_relu(x, 0.0) (-inf * 0 = NaN, negative * 0 = -0)
    z = ops.unary(x, "leaky_relu", slope=0.0).cpu()
    _assert_bit_identical(z, F.leaky_relu(x.cpu(), 0.0), "leaky_relu(slope=0.0) special values")


# ---------------------------------------------------------------------------------------------------------- layout


@pytest.mark.parametrize("R_,C_,pad_in,pad_out", [(1, 4097, 0, 0), (4097, 1, 3, 0), (1, 1, 5, 7), (33, 4097, 31, 0),
                                                  (33, 4097, 0, 1), (77, 45, 19, 13), (64, 32, 1, 32)])
def test_transpose_strided(dev, R_, C_, pad_in, pad_out):
    """out[c, r] = in[r, c] on row-strided views (ld = cols + pad) of both operands, bit-exact."""
    g = torch.Generator().manual_seed(R_ * 7 + C_ + pad_in)
    big = torch.randn(R_, C_ + pad_in, generator=g).to(dev)
    x = big[:, :C_]
    out_big = torch.full((C_, R_ + pad_out), 7.0, device=dev)
    out = out_big[:, :R_]
    ops.transpose(x, out=out)
    assert torch.equal(out.cpu(), x.cpu().t())
    if pad_out:
        assert torch.all(out_big[:, R_:] == 7.0)          # nothing written past the view's columns
    print(f"ERR transpose {R_}x{C_} ld_in={C_ + pad_in} ld_out={R_ + pad_out}: bit-exact")


@pytest.mark.parametrize("Hz,Wz,p1,p2,Cout", [(3, 5, 2, 4, 7), (5, 3, 4, 2, 3), (1, 1, 2, 4, 1), (18, 36, 2, 4, 33)])
def test_pixel_shuffle_rect(dev, Hz, Wz, p1, p2, Cout):
    from einops import rearrange
    g = torch.Generator().manual_seed(Hz * 100 + Wz * 10 + p1)
    lin = torch.randn(Hz * Wz, p1 * p2 * Cout, generator=g)
    ref = rearrange(lin.reshape(1, Hz, Wz, -1), "b h w (p1 p2 c) -> b c (h p1) (w p2)", p1=p1, p2=p2)[0]
    assert torch.equal(ops.pixel_shuffle(lin.to(dev), Hz, Wz, p1, p2).cpu(), ref)
    print(f"ERR pixel_shuffle {Hz}x{Wz} p=({p1},{p2}) Cout={Cout}: bit-exact")
