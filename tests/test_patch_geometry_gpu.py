"""The fused un-embed (cra5_gemm_nt_split_unembed, its side buffer, unembed_fixup_kernel), the overlap-add (col2im_kernel,
col2im_tiled_kernel) and the patch gather (im2col_kernel, im2col_tiled_kernel) on the superset geometries a subset,
thinned or coarsened decode launches them on - per element, away from the 72 x 144 grid the other tests fix
(geometries, inputs and references: tests/patch_geometry_helpers.py, checked by tests/test_patch_geometry_inputs_cpu.py).

Every image and side buffer starts as NaN and is followed by a sentinel tail: every pixel must be written, nothing past
the buffer.  An index error in these kernels is a wrong pixel, not a crash; the shapes are the smallest at which each
class of error shows (a few hundred tokens)."""
import numpy as np
import pytest
import torch

import exact_helpers as X
import patch_geometry_helpers as G
import split_helpers as S
from cra5_amd import ops
from cra5_amd._lib import Cra5Error, lib

pytestmark = pytest.mark.gpu

ERR_ARG = -7                       # CRA5_ERR_ARG (include/cra5_amd.h)
PATCH = (G.KH, G.KW, G.SH, G.SW)


def _split(a, w, dev):
    """the operands split on the device; the planes READ BACK from the SplitMats, checked"""
    a, w = a.to(dev), w.to(dev)
    sa, sw = ops.split_f16(a), ops.split_f16(w, "auto")
    pa, pw = sa.planes(), sw.planes()
    X.check_planes(a, pa[0], pa[1], 1.0, "A")
    X.check_planes(w, pw[0], pw[1], sw.scale_inv, "W")
    return sa, sw, pa, pw


def _fused(A_, W_, C, n_ti, n_tj, dev, mean, std, hi):
    """one fused launch pair into a NaN image with a side buffer of exactly unembed_side_bytes, both with sentinel tails"""
    H, W = G.image_shape(n_ti, n_tj)
    nb = ops.unembed_side_bytes(C, H, W, *PATCH)
    assert nb == C * n_ti * 2 * W * 4
    side, img = G.guarded(nb // 4, dev), G.guarded(C * H * W, dev)
    out = img[: C * H * W].view(C, H, W)
    ops.gemm_unembed(A_, W_, C, H, W, *PATCH, side[: nb // 4], mean=mean, std=std, out=out, hi_only=hi)
    torch.cuda.synchronize()
    assert G.tail_intact(side, nb // 4), "the un-embed wrote past the side buffer"
    assert G.tail_intact(img, C * H * W), "the un-embed wrote past the image"
    return out


# ------------------------------------------------------------------------------------------------ a. fused un-embed, exact


@pytest.mark.parametrize("n_ti,n_tj", G.GEOMETRIES)
def test_fused_unembed_exact_off_the_full_grid(dev, n_ti, n_tj):
    """Every geometry x C in {1, 3, 8} x the four instantiations of the launch (fp32-accurate; hi_only on split rows with
    Kp % 64 == 0 and != 0; hi_only on plain A and W) x raw / de-normalised: the exact overlap-add of the three-product
    model, every pixel, bit for bit."""
    H, W = G.image_shape(n_ti, n_tj)
    where = G.unembed_locator(H)
    for C in G.UNEMBED_CHANNELS:
        mean, std = (t.to(dev) for t in G.exact_stats(C))
        split, n, worst = {}, 0, 0.0
        for name, K, hi, plain in G.UNEMBED_FORMS:
            if K not in split:
                split[K] = _split(*G.unembed_operands(n_ti, n_tj, C, K), dev)
            sa, sw, pa, pw = split[K]
            e, g, w_ = X.three_product_expectation(pa, pw, sw.scale_inv, hi_only=hi)
            worst = max(worst, w_)
            A_, W_ = (X.plain_rows_of(sa), sw.plain_copy()) if plain else (sa, sw)
            if plain:
                assert A_.plain and W_.plain and torch.equal(A_.planes()[0], pa[0]) and torch.equal(W_.planes()[0], pw[0])
            assert float(pa[1].abs().max()) > 0 and float(pw[1].abs().max()) > 0      # hi_only must not read them
            for m_, s_ in ((None, None), (mean, std)):
                exp = X.unembed_expectation(e, C, n_ti, n_tj, G.KH, G.KW, mean=m_, std=s_)
                out = _fused(A_, W_, C, n_ti, n_tj, dev, m_, s_, hi)
                X.assert_exact(out.view(C * H, W), exp.view(C * H, W), g,
                               f"fused un-embed {n_ti} x {n_tj} tokens, C = {C}, K = {K}, {name}, de-normalised {m_ is not None}",
                               locate=where, gemm_tiles=False)
                assert bool(torch.isfinite(out).all())
                n += 1
        print(f"fused un-embed {n_ti} x {n_tj} tokens (M = {n_ti * n_tj}), C = {C}: 0 differing pixels of {C * H * W} in each of "
              f"{n} launches (4 forms x raw / de-normalised; max sum |term| {worst:.3g} granules)")


def test_fused_unembed_refusals_leave_the_image_untouched(dev):
    """odd n_tj (W % 4 != 0), M != Hp * Wp and a side buffer one byte short: CRA5_ERR_ARG, nothing written"""
    C, K = 3, 128
    a, w = G.unembed_operands(2, 6, C, K)
    sw = ops.split_f16(w.to(dev), "auto")
    sa = ops.split_f16(torch.cat([a, a[:4]]).to(dev))                  # 16 rows: every M tried below stays inside A

    def call(M, n_ti, n_tj, short=0):
        H, W = G.image_shape(n_ti, n_tj)
        nb = ops.unembed_side_bytes(C, H, W, *PATCH)
        assert nb == C * n_ti * 2 * W * 4
        side, img = G.guarded(nb // 4, dev), G.guarded(C * H * W, dev)
        rc = lib().cra5_gemm_nt_split_unembed(sa.data.data_ptr(), sa.pitch, sw.data.data_ptr(), sw.pitch, img.data_ptr(),
                                              side.data_ptr(), nb - short, None, None, M, sa.Kp, float(sw.scale_inv), C, H, W,
                                              *PATCH, 0, ops._stream())
        torch.cuda.synchronize()
        assert G.tail_intact(side, nb // 4) and G.tail_intact(img, C * H * W)
        return rc, img[: C * H * W], side[: nb // 4]

    rc, img, side = call(12, 2, 6)                                      # the control: the same call, valid
    assert rc == 0 and bool(torch.isfinite(img).all()) and bool(torch.isfinite(side).all())
    for what, args in (("odd n_tj", (10, 2, 5)), ("M < Hp * Wp", (11, 2, 6)), ("M = Hp * Wp / 2", (6, 2, 6)),
                       ("side buffer one byte short", (12, 2, 6, 1))):
        rc, img, side = call(*args)
        assert rc == ERR_ARG, (what, rc)
        assert bool(torch.isnan(img).all()) and bool(torch.isnan(side).all()), what
    # ... and through ops: the status arrives in the exception
    H, W = G.image_shape(2, 6)
    nb = ops.unembed_side_bytes(C, H, W, *PATCH)
    out = torch.full((C, H, W), G.NAN, device=dev)
    s12 = ops.SplitMat(sa.data[:12], 12, sa.K, sa.Kp)
    with pytest.raises(Cra5Error) as ei:
        ops.gemm_unembed(s12, sw, C, H, W, *PATCH, torch.full((nb // 4 - 1,), G.NAN, device=dev), out=out)
    assert ei.value.status == ERR_ARG and bool(torch.isnan(out).all())


# ------------------------------------------------------------------------------------------------ b. fused pair = two calls


@pytest.mark.parametrize("n_ti,n_tj", G.GEOMETRIES)
def test_fused_pair_equals_gemm_plus_col2im_on_random_data(dev, n_ti, n_tj):
    """Random operands, mean and std; C = 2 (the two-call form's col2im is the tiled kernel where n_tj % 16 == 0) and
    C = 5 (ldn = K = 550: the generic one).  The GEMM of the two-call form is whatever gemm_dispatch picks at this size,
    with hi_only / wide_k as VAEformer._unembed passes them (wide_k: the reduced-precision mode names the 64-wide k-step
    form of the full-size launch whenever Kp % 64 == 0) - the same accumulators in the same order as the fused launch's
    256 x 256 tiles, so the images are torch.equal."""
    M = n_ti * n_tj
    for C in (2, 5):
        N = C * G.KH * G.KW
        mean, std = (t.to(dev) for t in G.random_stats(C, seed=M + C))
        for K, hi, plain in ((128, False, False), (128, True, False), (96, True, False), (128, True, True)):
            g = torch.Generator().manual_seed(1000 * M + 10 * C + K)
            a = ops.split_f16(torch.randn(M, K, generator=g).to(dev))
            w = ops.split_f16((torch.randn(N, K, generator=g) / np.sqrt(K)).to(dev), "auto")
            if plain:
                a, w = X.plain_rows_of(a), w.plain_copy()
            cols = ops.gemm_nt_split(a, w, hi_only=hi, wide_k=hi and a.Kp % 64 == 0)
            assert cols.is_contiguous() and tuple(cols.shape) == (M, N)
            for m_, s_ in ((None, None), (mean, std)):
                H, W = G.image_shape(n_ti, n_tj)
                ref = G.guarded(C * H * W, dev)
                ops.col2im(cols, C, *PATCH, n_ti, n_tj, mean=m_, std=s_, out=ref[: C * H * W].view(C, H, W))
                out = _fused(a, w, C, n_ti, n_tj, dev, m_, s_, hi)
                assert G.tail_intact(ref, C * H * W) and bool(torch.isfinite(out).all())
                assert torch.equal(out, ref[: C * H * W].view(C, H, W)), (n_ti, n_tj, C, K, hi, plain, m_ is not None)


# ------------------------------------------------------------------------------------------------ c. col2im


def _col2im(cols, C, n_ti, n_tj, dev, mean=None, std=None):
    H, W = G.image_shape(n_ti, n_tj)
    img = G.guarded(C * H * W, dev)
    out = img[: C * H * W].view(C, H, W)
    ops.col2im(cols, C, *PATCH, n_ti, n_tj, mean=mean, std=std, out=out)
    torch.cuda.synchronize()
    assert G.tail_intact(img, C * H * W), "col2im wrote past the image"
    assert bool(torch.isfinite(out).all())
    return out


def _layouts(mats, K, dev, with_offset):
    """the same column matrices three ways: (name, views, ldn, byte offset of the matrix from a 16-byte boundary).  Pad
    columns and the floats around an offset matrix are NaN: a sum that reads one shows."""
    M = mats[0].shape[0]
    yield "ldn = K", [m.to(dev).contiguous() for m in mats], K, 0
    ld = G.padded_pitch(K)
    views = []
    for m in mats:
        big = torch.full((M, ld), G.NAN, device=dev)
        big[:, :K] = m.to(dev)
        views.append(big[:, :K])
    yield "ldn = K rounded up to 4, + 4", views, ld, 0
    if with_offset:
        views = []
        for m in mats:
            flat = torch.full((M * K + 4,), G.NAN, device=dev)
            v = flat[1: 1 + M * K].view(M, K)
            v.copy_(m.to(dev))
            assert v.data_ptr() % 16 == 4
            views.append(v)
        yield "4 bytes past a 16-byte boundary", views, K, 4


@pytest.mark.parametrize("n_ti,n_tj", G.GEOMETRIES)
def test_col2im_both_kernels_against_float64(dev, n_ti, n_tj):
    """Raw output: bit-equal to the fp32 fold (a two-term sum has one rounding in either order).  De-normalised, exact
    inputs: bit-equal to float64.  De-normalised, random std and mean on column data whose overlap sums are exact: within
    2 u (|s std| + |mean|) of float64 (patch_geometry_helpers.denorm_bound: derived, not measured).  Odd C reaches the
    tiled kernel through a padded pitch, even C the generic one through an unaligned matrix: where both kernels take the
    same problem their outputs are torch.equal."""
    worst, seen = 0.0, set()
    for C in G.COL2IM_CHANNELS:
        K = C * G.KH * G.KW
        r, x, q = G.random_cols(n_ti, n_tj, C), G.exact_cols(n_ti, n_tj, C), G.quantised_cols(n_ti, n_tj, C)
        me, se = G.exact_stats(C)
        mr, sr = G.random_stats(C, seed=C)
        raw_ref = G.col2im_reference(r, C, n_ti, n_tj)                                   # fp32 fold
        den_ref = G.col2im_reference(x.double(), C, n_ti, n_tj, mean=me, std=se)
        s64 = G.col2im_reference(q.double(), C, n_ti, n_tj)
        rnd_ref = s64 * sr.double()[:, None, None] + mr.double()[:, None, None]
        bound = G.denorm_bound(s64, sr, mr)
        outs = {}
        for name, (rv, xv, qv), ld, al in _layouts((r, x, q), K, dev, with_offset=C == 2):
            kern = G.classify(n_ti, n_tj, C, ld, (al, 0))["kernel"]
            label = f"col2im {n_ti} x {n_tj}, C = {C}, {name} ({kern})"
            raw = _col2im(rv, C, n_ti, n_tj, dev)
            assert torch.equal(raw.cpu(), raw_ref), label + ": raw output"
            de = _col2im(xv, C, n_ti, n_tj, dev, me.to(dev), se.to(dev))
            assert torch.equal(de.cpu().double(), den_ref), label + ": de-normalised, exact inputs"
            dr = _col2im(qv, C, n_ti, n_tj, dev, mr.to(dev), sr.to(dev))
            ratio = float(((dr.cpu().double() - rnd_ref).abs() / bound).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, (label, ratio)
            outs[name] = (kern, raw, de, dr)
        kerns = {k for k, *_ in outs.values()}
        seen |= kerns
        assert kerns == ({"tiled", "generic"} if n_tj % G.TILE_TOK == 0 else {"generic"}), (C, kerns)
        first = outs["ldn = K"]
        for name, o in outs.items():
            for a_, b_ in zip(first[1:], o[1:]):
                assert torch.equal(a_, b_), (n_ti, n_tj, C, first[0], "against", name, o[0])
    print(f"ERR col2im {n_ti} x {n_tj} tokens, C in {G.COL2IM_CHANNELS}, kernels {sorted(seen)}: raw and exact de-normalised "
          f"output 0 differing pixels; random std / mean: worst |err| / (2u(|s std| + |mean|)) = {worst:.3f}")


# ------------------------------------------------------------------------------------------------ d. im2col


def _hi_plane(sm):
    return sm.data.view(sm.rows, sm.Kp // 32, 2, 32)[:, :, 0].reshape(sm.rows, sm.Kp)


@pytest.mark.parametrize("Hp,Wp", G.IM2COL_GEOMETRIES)
def test_im2col_both_kernels(dev, Hp, Wp):
    """An image larger than the patches cover (the launcher allows >), aligned (the tiled kernel where Wp % 16 == 0 and
    W % 4 == 0) and offset by one float (the generic kernel): fp32 output with ldk > K bit-equal to the CPU's fp32
    (x - mean) / std unfold, the pad columns untouched; split output bit-equal, both planes and the padding, to the
    host split model; plain output = the hi plane, K .. Kp re-zeroed, nothing past the plain row; the generic kernel
    refuses plain rows with ldk != K."""
    M, n_cmp = Hp * Wp, 0
    for C in G.IM2COL_CHANNELS:
        x, mean, std = G.im2col_image(Hp, Wp, C)
        Himg, Wimg = x.shape[1:]
        K = C * G.KH * G.KW
        Kp = (K + 31) // 32 * 32
        ld = G.padded_pitch(K)
        ref = G.im2col_reference(x, Hp, Wp, mean, std)                                    # fp32, the CPU's IEEE operations
        flat = torch.zeros(x.numel() + 4, device=dev)
        xo = flat[1: 1 + x.numel()].view(x.shape)
        xo.copy_(x.to(dev))
        assert xo.data_ptr() % 16 == 4 and xo.is_contiguous()
        md, sd = mean.to(dev), std.to(dev)
        got = {}
        for img, al in ((x.to(dev), 0), (xo, 4)):
            kern = G.kernel_choice("im2col", Wp, ld, W=Wimg, alignment=al)
            assert kern == G.kernel_choice("im2col", Wp, Kp, W=Wimg, alignment=al)
            label = f"im2col {Hp} x {Wp}, image {Himg} x {Wimg}, C = {C} ({kern})"
            buf = G.guarded(M * ld, dev)
            buf[: M * ld] = -777.0
            out = buf[: M * ld].view(M, ld)
            ops.im2col(img, *PATCH, ldk=ld, mean=md, std=sd, out=out)
            torch.cuda.synchronize()
            assert G.tail_intact(buf, M * ld), label
            assert torch.equal(out[:, :K].cpu(), ref), label + ": fp32 output"
            assert bool((out[:, K:] == -777.0).all()), label + ": pad columns written"
            sm = ops.SplitMat.empty(M, K, dev, zero=True)
            ops.im2col(img, *PATCH, mean=md, std=sd, out_split=sm)
            n_cmp += S.compare_planes(sm.data.cpu().numpy(), ref.numpy(), K, Kp, label=label + ": split output")
            sp = ops.SplitMat.empty(M, K, dev)
            sp.data.fill_(0x3c00)
            if kern == "tiled":
                ops.im2col(img, *PATCH, mean=md, std=sd, out_split=sp, out_plain=True)
                n_cmp += S.compare_planes(sp.data.cpu().numpy(), ref.numpy(), K, Kp, plain=True, fill=0x3c00,
                                          label=label + ": plain output")
                assert sp.plain and torch.equal(sp.data[:, :K], _hi_plane(sm)[:, :K])
            else:
                with pytest.raises(Cra5Error) as ei:
                    ops.im2col(img, *PATCH, mean=md, std=sd, out_split=sp, out_plain=True)
                torch.cuda.synchronize()
                assert ei.value.status == ERR_ARG and Kp != K and bool((sp.data == 0x3c00).all()), label
            got[al] = (kern, out[:, :K].clone(), sm.data)
        assert got[4][0] == "generic" and got[0][0] == ("tiled" if Wp % G.TILE_TOK == 0 else "generic")
        assert torch.equal(got[0][1], got[4][1]) and torch.equal(got[0][2], got[4][2]), (Hp, Wp, C, "tiled against generic")
    print(f"ERR im2col {Hp} x {Wp} tokens, C in {G.IM2COL_CHANNELS}: fp32, split and plain output bit-equal to the host "
          f"reference: 0 differing of {n_cmp} stored halves, worst ratio 0")
