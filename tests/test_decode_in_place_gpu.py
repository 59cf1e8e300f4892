"""The reconstruction lands in its final place: decompress / decode_latent / forward allocate the batch result once and
every un-embed form stores into its frame (no stack copy).  Checked here: a batch equals its single-frame decodes bit for
bit under every un-embed form, the result is fresh per call, the range guard's re-run ends in the returned tensor - and
the two kernels the same change looked at: the split GEMM on a ragged last tile row (a wave group wholly past M issues
no MFMAs and stores nothing) and the tiled patch gather against the generic one, byte for byte."""
import pytest
import torch

import exact_helpers as X
from cra5_amd import ops, synth
from cra5_amd.vaeformer import VAEformer

pytestmark = pytest.mark.gpu


def _thin(dev, mod=None):
    net = VAEformer(0, **synth.thin_model_kwargs())
    synth.load_synthetic(net, seed=7)
    if mod is not None:
        with torch.no_grad():
            mod(net)
    return net.to(dev)


def _same_bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    return tuple(a.shape) == tuple(b.shape) and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.fixture(scope="module")
def thin(dev):
    return _thin(dev)


@pytest.fixture(scope="module")
def latent2(dev):
    """two different latents [2, 16, 72, 144]"""
    g = torch.Generator().manual_seed(23)
    y = torch.round(2.0 * torch.randn(2, 16, 72, 144, generator=g)) + torch.randn(2, 16, 72, 144, generator=g)
    return y.to(dev)


@pytest.fixture(scope="module")
def streams2(thin, dev):
    """compress() of two different frames: (strings, z_shape)"""
    x = torch.stack([synth.synth_frame(8, seed=2), synth.synth_frame(8, seed=3)]).to(dev)
    out = thin.compress(x)
    return out["strings"], out["z_shape"]


# the un-embed forms: full decode, a channel subset (exact superset: the fused pair / two-call form writes the frame
# itself), a box whose superset is not exact (superset workspace + crop), a stride (thinned path), and all three at once
SELECTIONS = {
    "full": {},
    "channels": dict(channels=[5, 1, 3]),
    "box": dict(box=(123, 456, 1437, 7)),
    "stride": dict(step=6),
    "channels_box_stride": dict(channels=[0, 7], box=(72, 221, 1340, 281), step=(2, 3)),
}
ENGINES = {
    "split": {},
    "split_unfused": dict(fused_unembed=False),
    "f32": dict(gemm_mode="f32", attn_mode="f32"),
}


@pytest.fixture(params=list(ENGINES))
def engine(request, thin):
    keep = {k: getattr(thin, k) for k in ("gemm_mode", "attn_mode", "fused_unembed")}
    for k, v in ENGINES[request.param].items():
        setattr(thin, k, v)
    yield request.param
    for k, v in keep.items():
        setattr(thin, k, v)


def test_decode_latent_batch_equals_single_frames(thin, latent2, engine):
    for name, sel in SELECTIONS.items():
        both = thin.decode_latent(latent2, **sel)
        assert both.shape[0] == 2 and both.is_contiguous() and both._base is None, (engine, name)
        for b in range(2):
            one = thin.decode_latent(latent2[b:b + 1], **sel)
            assert one.shape[0] == 1 and _same_bits(both[b], one[0]), (engine, name, b)
        assert not _same_bits(both[0], both[1]), (engine, name)      # (the two frames do differ)


def test_decompress_batch_equals_single_frames(thin, streams2, engine):
    strings, z_shape = streams2
    for name in ("full", "box", "channels_box_stride"):
        sel = SELECTIONS[name]
        both = thin.decompress(strings, z_shape, **sel)["x_hat"]
        assert both.shape[0] == 2 and both.is_contiguous() and both._base is None, (engine, name)
        for b in range(2):
            one = thin.decompress([[strings[0][b]], [strings[1][b]]], z_shape, **sel)["x_hat"]
            assert _same_bits(both[b], one[0]), (engine, name, b)
    # the stream's reconstruction is the decode of its latent (one path below the public methods)
    y_hat = thin.decompress(strings, z_shape, return_format="latent")
    assert tuple(y_hat.shape) == (2, 16, 72, 144)
    assert _same_bits(thin.decompress(strings, z_shape)["x_hat"], thin.decode_latent(y_hat))


def test_forward_batch_equals_decode_of_its_latents(thin, dev):
    x = torch.stack([synth.synth_frame(8, seed=2), synth.synth_frame(8, seed=3)]).to(dev)
    out = thin(x)
    assert tuple(out["x_hat"].shape) == (2, 8, 721, 1440) and out["x_hat"]._base is None
    for b in range(2):
        y_hat = thin.encode_latent(x[b:b + 1])[1]
        assert _same_bits(out["x_hat"][b], thin.decode_latent(y_hat)[0]), b


def test_result_is_fresh_per_call(thin, latent2, streams2):
    """Two consecutive calls on one thread return different storage (never a view of a per-thread workspace), and the
    first result keeps its bits through the second call - for the frame-writing forms and the crop / thinned ones."""
    strings, z_shape = streams2
    for name in ("full", "box", "stride"):
        sel = SELECTIONS[name]
        first = thin.decode_latent(latent2[:1], **sel)
        kept = first.clone()
        second = thin.decode_latent(latent2[1:], **sel)
        assert first.untyped_storage().data_ptr() != second.untyped_storage().data_ptr(), name
        assert _same_bits(first, kept) and not _same_bits(first, second), name
    first = thin.decompress([[strings[0][0]], [strings[1][0]]], z_shape)["x_hat"]
    kept = first.clone()
    second = thin.decompress([[strings[0][1]], [strings[1][1]]], z_shape)["x_hat"]
    assert first.untyped_storage().data_ptr() != second.untyped_storage().data_ptr()
    assert _same_bits(first, kept) and not _same_bits(first, second)
    # a caller's destination of the wrong shape / layout is refused before anything is written
    with pytest.raises(ValueError, match="destination"):
        thin._decode_guarded(latent2[0], out=torch.empty(8, 721, 1441, device=latent2.device))
    with pytest.raises(ValueError, match="destination"):
        thin._decode_guarded(latent2[0], out=torch.empty(8, 721, 2880, device=latent2.device)[:, :, ::2])


def test_range_guard_rerun_ends_in_the_returned_tensor(thin, streams2, dev):
    """Outlier rows in a g_s MLP (the construction of tests/test_model_gpu.py's decode-side range-guard test): the split
    engines poison the frame that was written into the batch result, the guard re-runs it on the exact-f32 engines INTO
    THE SAME DESTINATION.  The returned batch holds the pure exact-f32 run's bits, frame by frame."""
    strings, z_shape = streams2

    def mod_gs(net):
        net.g_s.blocks[2].mlp.fc1.weight[:4] *= 3e5
        net.g_s.blocks[2].mlp.fc1.bias[:4] *= 3e5
        net.g_s.blocks[2].mlp.fc2.weight[:, :4] /= 3e5
    net = _thin(dev, mod_gs)
    ref = _thin(dev, mod_gs)
    ref.gemm_mode, ref.attn_mode = "f32", "f32"
    want = ref.decompress(strings, z_shape)["x_hat"]
    want_box = ref.decompress(strings, z_shape, **SELECTIONS["box"])["x_hat"]
    assert ref.range_fallbacks == [0, 0] and bool(torch.isfinite(want).all())
    with pytest.warns(RuntimeWarning, match="exact-f32"):
        got = net.decompress(strings, z_shape)["x_hat"]
    assert net.range_fallbacks == [0, 2]
    assert bool(torch.isfinite(got).all()) and _same_bits(got, want)
    with pytest.warns(RuntimeWarning, match="exact-f32"):
        got_box = net.decompress(strings, z_shape, **SELECTIONS["box"])["x_hat"]
    assert net.range_fallbacks == [0, 4] and _same_bits(got_box, want_box)
    y_hat = net.decompress(strings, z_shape, return_format="latent")
    with pytest.warns(RuntimeWarning, match="exact-f32"):
        got_l = net.decode_latent(y_hat)
    assert net.range_fallbacks == [0, 6] and _same_bits(got_l, want)


# ------------------------------------------------------------------------------------------------ GEMM M edge

# N = 256, K = 64, M = 128 + 32 k: a half-empty last tile, a partly filled second wave row, a full tile.  The second
# family has the same M edges behind four full tile rows of a launch wide enough for the 256 x 256 instantiation
# (M >= 1024, N >= 2048, >= 256 tiles of 128 x 128), whose lower wave group skips its MFMAs when it lies wholly past M.
M_EDGE = [(128 + 32 * k, 256, 64) for k in range(5)] + [(1024 + 128 + 32 * k, 4096, 64) for k in range(5)]
SENTINEL = -7.25


@pytest.mark.parametrize("M,N,K", M_EDGE)
def test_gemm_split_m_edge_exact_and_padding_rows_untouched(dev, M, N, K):
    """Split engine against the float64 product of the split operands as stored, every element pinned (no epilogue and
    bias + residual: the generic edge epilogue); rows >= M of a padded output buffer keep their sentinel."""
    a = X.grid_matrix(M, K, 1.0, 7 * M + N, lo_shift=12).to(dev)
    w = X.grid_matrix(N, K, 1.0, 7 * M + N + 1, lo_shift=12).to(dev)
    sa, sw = ops.split_f16(a), ops.split_f16(w, "auto")
    pa, pw = sa.planes(), sw.planes()
    X.check_planes(a, pa[0], pa[1], 1.0, "A")
    X.check_planes(w, pw[0], pw[1], sw.scale_inv, "W")
    bias = X.grid_vector(N, M + 2).to(dev)
    res = X.grid_matrix(M, N, 1.0, M + 3, lo_shift=12).to(dev)
    Mpad = (M + 255) // 256 * 256 + 256
    for epi in ("none", "bias_res"):
        kw = dict(bias=bias, res=res) if epi == "bias_res" else {}
        e, g, _ = X.three_product_expectation(pa, pw, sw.scale_inv, **kw)
        buf = torch.full((Mpad, N), SENTINEL, device=dev)
        ops.gemm_nt_split(sa, sw, out=buf[:M], **kw)
        X.assert_exact(buf[:M], e, g, f"gemm_nt_split {M}x{N}x{K} {epi}")
        assert bool((buf[M:] == SENTINEL).all()), f"{M}x{N}x{K} {epi}: rows >= M of the padded output were written"
        # the split output of the same launch: rows >= M of a padded SplitMat stay as they were
        if epi == "none":
            out_s = ops.SplitMat.empty(Mpad, N, dev)
            out_s.data.fill_(0x5A5A)
            view = ops.SplitMat(out_s.data[:M], M, N, out_s.Kp)
            ops.gemm_nt_split(sa, sw, out_split=view, want_f32=False)
            err = float((view.to_float().double() - e).abs().max())
            assert err <= 2 ** -21 * float(e.abs().max()) + 2 ** -24, (M, N, K, err)     # (22 bits of a 24-bit result)
            assert bool((out_s.data[M:] == 0x5A5A).all()), f"{M}x{N}x{K}: split rows >= M were written"


# ------------------------------------------------------------------------------------------------ patch gather

KH, KW, S = 11, 10, 10


def _gather_pair(dev, C, Hp, norm, plain, fill):
    """(tiled result bytes, generic result bytes) of one gather: the same frame at a 16-byte aligned address (the
    LDS-tiled kernel's route) and 4 bytes further (the launcher then takes the generic kernel)."""
    Wp = 16
    H, W = (Hp - 1) * S + KH, Wp * KW
    g = torch.Generator().manual_seed(100 * C + Hp)
    frame = (torch.randn(C * H * W, generator=g) * 3.0).to(dev)
    base = torch.empty(C * H * W + 4, device=dev)
    assert base.data_ptr() % 16 == 0
    x_al, x_off = base[:C * H * W].view(C, H, W), base[1:1 + C * H * W].view(C, H, W)
    mean = std = None
    if norm:
        mean = torch.randn(C, generator=g).to(dev)
        std = (0.5 + torch.rand(C, generator=g)).to(dev)
    outs = []
    for x in (x_al, x_off):
        x.copy_(frame.view(C, H, W))
        sm = ops.SplitMat.empty(Hp * Wp, C * KH * KW, dev)
        sm.data.fill_(fill)
        ops.im2col(x, KH, KW, S, S, mean=mean, std=std, out_split=sm, out_plain=plain)
        outs.append(sm)
    return outs


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("C,Hp", [(2, 1), (3, 2), (19, 2)])
def test_tiled_gather_split_rows_equal_the_generic_kernel(dev, C, Hp, norm):
    """Smallest legal tiled geometry (kernel 11 x 10, stride 10, Wp = 16): 2 channels = one full chunk, 3 = a ragged
    second chunk, 19 = three blocks per token tile, the last one short with a ragged chunk.  Whole rows compared, the K
    padding included (zero-initialised, as the model's workspace: neither kernel writes it)."""
    tiled, generic = _gather_pair(dev, C, Hp, norm, plain=False, fill=0)
    assert torch.equal(tiled.data, generic.data)
    assert tiled.Kp > tiled.K or C % 16 == 0
    # the fp32 rows too (the exact-f32 engines' operand), padding columns included
    Wp, K = 16, C * KH * KW
    H, W = (Hp - 1) * S + KH, Wp * KW
    n, ldk = C * H * W, (K + 31) // 32 * 32
    frame = torch.randn(n, generator=torch.Generator().manual_seed(C)).to(dev)
    base = torch.empty(n + 4, device=dev)
    outs = []
    for off in (0, 1):
        base[off:off + n].copy_(frame)
        outs.append(ops.im2col(base[off:off + n].view(C, H, W), KH, KW, S, S, ldk=ldk,
                               out=torch.zeros(Hp * Wp, ldk, device=dev)))
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))


@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("C,Hp", [(2, 1), (3, 2), (19, 2), (16, 1)])
def test_tiled_gather_plain_rows_equal_the_generic_kernel(dev, C, Hp, norm):
    """Plain rows: element k at half k of the row, the halves K .. Kp re-zeroed by the tiled kernel every time, the rest
    of the row untouched.  The generic kernel writes plain rows only without K padding (16 channels: K = 1760 = Kp) -
    compared directly there; for the padded widths the expectation is the hi plane of the generic kernel's split rows
    (a plain element is the hi half of its split pair: csrc/split.h)."""
    fill = 0x5A5A
    K = C * KH * KW
    Kp = (K + 31) // 32 * 32
    if K == Kp:
        tiled, generic = _gather_pair(dev, C, Hp, norm, plain=True, fill=fill)
        assert torch.equal(tiled.data, generic.data)
        return
    Wp = 16
    H, W = (Hp - 1) * S + KH, Wp * KW
    g = torch.Generator().manual_seed(100 * C + Hp)
    frame = (torch.randn(C * H * W, generator=g) * 3.0).to(dev)
    mean = std = None
    if norm:
        mean = torch.randn(C, generator=g).to(dev)
        std = (0.5 + torch.rand(C, generator=g)).to(dev)
    base = torch.empty(C * H * W + 4, device=dev)
    base[:C * H * W].copy_(frame)
    tiled = ops.SplitMat.empty(Hp * Wp, K, dev)
    tiled.data.fill_(fill)
    ops.im2col(base[:C * H * W].view(C, H, W), KH, KW, S, S, mean=mean, std=std, out_split=tiled, out_plain=True)
    base[1:1 + C * H * W].copy_(frame)
    generic = ops.SplitMat.empty(Hp * Wp, K, dev, zero=True)
    ops.im2col(base[1:1 + C * H * W].view(C, H, W), KH, KW, S, S, mean=mean, std=std, out_split=generic)
    want = torch.full_like(tiled.data, fill)
    want[:, :Kp] = generic.data.view(Hp * Wp, Kp // 32, 2, 32)[:, :, 0].reshape(Hp * Wp, Kp)   # hi plane; padding zero
    assert bool((want[:, K:Kp] == 0).all())
    assert torch.equal(tiled.data, want)
