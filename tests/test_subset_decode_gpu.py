"""Subset decode on the GPU (VAEformer.decode_latent / decompress with channels / box, cra5_api variables / region): the
result is the slice of a full decode of the same latent, bit for bit, under every engine and precision the full decode
supports, and the two new layout kernels (cra5_gather_token_rows, cra5_crop_f32) equal their numpy restatement."""
import warnings

import numpy as np
import pytest
import torch

from cra5_amd import ops, synth
from cra5_amd.api import cra5_api
from cra5_amd.vaeformer import VAEformer

pytestmark = pytest.mark.gpu

H, W = 721, 1440


def _yhat(latent, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.round(2.0 * torch.randn(1, latent, 72, 144, generator=g)) + torch.randn(1, latent, 72, 144, generator=g)


def _thin(dev, mod=None):
    net = VAEformer(0, **synth.thin_model_kwargs())
    synth.load_synthetic(net, seed=7)
    if mod is not None:
        with torch.no_grad():
            mod(net)
    return net.to(dev)


def _slice(full, chans, box):
    """full [C, H, W] -> the channels / box slice (columns wrap at W)."""
    x = full if chans is None else full[list(chans)]
    if box is None:
        return x.contiguous()
    r0, r1, c0, nc = box
    cols = torch.tensor([(c0 + k) % full.shape[-1] for k in range(nc)], device=full.device)
    return x[:, r0:r1].index_select(2, cols).contiguous()


def _same_bits(a, b):
    a, b = a.contiguous(), b.contiguous()
    return tuple(a.shape) == tuple(b.shape) and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.fixture(scope="module")
def thin(dev):
    return _thin(dev)


@pytest.fixture(scope="module")
def latent(dev):
    return _yhat(16, seed=11).to(dev)


# ---- the two layout kernels against numpy ---------------------------------------------------------------------------


def test_gather_token_rows_matches_numpy(dev):
    g = torch.Generator().manual_seed(0)
    Hp, Wp, K = 6, 10, 36
    src = torch.randn(Hp * Wp, K, generator=g)
    for ti0, n_ti, tj0, n_tj in [(1, 3, 7, 6), (0, 6, 0, 10), (5, 1, 9, 1), (2, 2, 3, 10), (0, 1, 9, 2)]:
        out = ops.gather_token_rows(src.to(dev), torch.empty(n_ti * n_tj, K, device=dev), Hp, Wp, ti0, n_ti, tj0, n_tj)
        s = src.numpy().reshape(Hp, Wp, K)
        ref = s[ti0:ti0 + n_ti][:, [(tj0 + j) % Wp for j in range(n_tj)]].reshape(-1, K)
        assert np.array_equal(out.cpu().numpy(), ref), (ti0, n_ti, tj0, n_tj)
    # split-f16 rows (and plain rows) are copied verbatim, layout flag and scale included
    sm = ops.split_f16(src.to(dev), "auto")
    for plain in (False, True):
        m = sm.plain_copy() if plain else sm
        if plain:   # a plain row living in a split-layout buffer, as the LayerNorm writes it
            buf = ops.SplitMat.empty(Hp * Wp, K, dev, zero=True)
            buf.data[:, :m.Kp].copy_(m.data)
            m = ops.SplitMat(buf.data, Hp * Wp, K, m.Kp, m.scale_inv, plain=True)
        out = ops.gather_token_rows(m, ops.SplitMat.empty(2 * 4, K, dev, zero=True), Hp, Wp, 3, 2, 8, 4)
        assert out.plain == plain and out.scale_inv == m.scale_inv
        idx = [t * Wp + (8 + j) % Wp for t in (3, 4) for j in range(4)]
        n = m.Kp if plain else 2 * m.Kp
        assert torch.equal(out.data[:, :n], m.data[idx, :n])


def test_crop_matches_numpy_with_wrap_and_odd_offsets(dev):
    g = torch.Generator().manual_seed(1)
    C, Hs, Ws = 3, 17, 23
    base = torch.randn(C * Hs * Ws + 3, generator=g)
    for off in (0, 1, 3):                       # src / dst at 4-byte, not 16-byte, alignment
        src_d = base.to(dev)[off:off + C * Hs * Ws].view(C, Hs, Ws)
        s = src_d.cpu().numpy()
        for r0, Hb, c0, Wb in [(2, 5, 21, 23), (0, 17, 0, 23), (16, 1, 22, 1), (3, 4, 5, 9), (7, 3, 13, 17)]:
            dst_base = torch.full((C * Hb * Wb + 1,), -7.0, device=dev)
            dst = dst_base[1:].view(C, Hb, Wb)
            ops.crop(src_d, r0, Hb, c0, Wb, out=dst)
            ref = s[:, r0:r0 + Hb][:, :, [(c0 + j) % Ws for j in range(Wb)]]
            assert np.array_equal(dst.cpu().numpy(), ref), (off, r0, Hb, c0, Wb)
            assert float(dst_base[0]) == -7.0     # nothing written in front of the box


# ---- bit identity with the slice of a full decode --------------------------------------------------------------------

CHANNELS = [None, [0], [7], [0, 7], [5, 1, 3], list(range(8))]
BOXES = [
    (30, 31, 100, 50),       # r0 = r1 - 1 = 30: a single seam row
    (30, 41, 0, 40),         # both edges on seam rows
    (0, 5, 0, 40),           # row 0 (the grid's top edge)
    (715, 721, 200, 33),     # row 720 (the bottom edge)
    (357, 358, 713, 1),      # a single pixel
    (72, 221, 1340, 281),    # across 0 deg (Europe: 35-72 N, -25-45 E)
    (123, 456, 1437, 7),     # odd offsets across 0 deg
    (200, 260, 1, 1440),     # the full circle off a patch boundary
    (0, 721, 720, 1440),     # the whole globe centred on Greenwich
    (0, 721, 0, 1440),       # the whole globe
    # supersets that take the LDS-tiled col2im (n_tj % 16 == 0) or sit on a 256-row tile edge of the un-embed launch
    # (tests/patch_geometry_helpers.py MODEL_BOXES; tests/test_patch_geometry_inputs_cpu.py asserts each superset)
    (205, 236, 403, 150),    # 4 x 16 tokens, away from the east edge
    (301, 322, 1385, 155),   # 3 x 16 across the east edge
    (401, 560, 800, 160),    # 16 x 16: M = 256, exactly one tile
    (101, 130, 15, 850),     # 3 x 86: M = 258, the second tile holds two rows
    (0, 15, 640, 320),       # 2 x 32 on the top edge
    (700, 721, 1120, 160),   # 3 x 16 on the bottom edge
]
ENGINES = {
    "default": {},
    "f32": dict(gemm_mode="f32"),
    "unfused": dict(fused_unembed=False),
    "f16": dict(precision="f16"),
    "f16_unfused": dict(precision="f16", fused_unembed=False),
}


@pytest.mark.parametrize("engine", list(ENGINES))
def test_subset_equals_slice_of_full_decode(thin, latent, dev, engine):
    keep = (thin.precision, thin.gemm_mode, thin.fused_unembed)
    try:
        for k, v in ENGINES[engine].items():
            setattr(thin, k, v)
        mean = torch.linspace(-1, 1, 8, device=dev)
        std = torch.linspace(0.5, 2, 8, device=dev)
        full_n = thin.decode_latent(latent)[0]
        full_d = thin._decode_guarded(latent[0], mean=mean, std=std)
        cases = [(c, None) for c in CHANNELS] + [(None, b) for b in BOXES] + \
                [([5, 1, 3], BOXES[5]), ([7], BOXES[4]), ([0, 7], BOXES[7]), (list(range(8)), BOXES[1])]
        for chans, box in cases:
            got = thin.decode_latent(latent, channels=chans, box=box)[0]
            assert _same_bits(got, _slice(full_n, chans, box)), (engine, chans, box, "normalized")
        for chans, box in [([0], None), (None, BOXES[5]), ([5, 1, 3], BOXES[6]), ([7], BOXES[8])]:
            ch, bx = thin._subset_args(chans, box)
            got = thin._decode_guarded(latent[0], mean=mean, std=std, channels=ch, box=bx)
            assert _same_bits(got, _slice(full_d, chans, box)), (engine, chans, box, "de-normalised")
        assert thin.range_fallbacks == [0, 0]
    finally:
        thin.precision, thin.gemm_mode, thin.fused_unembed = keep


def test_subset_argument_errors(thin, latent):
    for bad in ([], [8], [-1], [1, 1]):
        with pytest.raises(ValueError, match="channels"):
            thin.decode_latent(latent, channels=bad)
    for bad in ((5, 5, 0, 10), (0, 722, 0, 10), (0, 10, 1440, 10), (0, 10, 0, 0), (0, 10, 0, 1441)):
        with pytest.raises(ValueError, match="box"):
            thin.decode_latent(latent, box=bad)


def test_bounded_subset_caches(thin, latent, dev):
    """A long run over many different subsets keeps the gathered-weight cache at its bound and device memory flat."""
    rng = np.random.default_rng(0)
    thin.decode_latent(latent, channels=[1, 2], box=(10, 50, 1400, 100))
    torch.cuda.synchronize()
    mem0 = torch.cuda.memory_allocated(dev)
    for i in range(3 * VAEformer.SUBSET_CACHE):
        chans = [int(c) for c in rng.permutation(8)[: 1 + i % 7]]
        thin.decode_latent(latent, channels=chans, box=(10, 50, 1400, 100))
        assert len(thin._sub_cache) <= VAEformer.SUBSET_CACHE
    torch.cuda.synchronize()
    # (gathered weights of the thin model: <= 7 x 110 rows x 256 halves each; the bound leaves room for the allocator)
    assert torch.cuda.memory_allocated(dev) - mem0 <= 8 << 20


# ---- range guard ------------------------------------------------------------------------------------------------------


def _mod_gs(net):      # outlier hidden units in a g_s MLP (tests/test_model_gpu.py, range guard on the decode side)
    net.g_s.blocks[2].mlp.fc1.weight[:4] *= 3e5
    net.g_s.blocks[2].mlp.fc1.bias[:4] *= 3e5
    net.g_s.blocks[2].mlp.fc2.weight[:, :4] /= 3e5


def test_range_guard_reruns_a_poisoned_subset(dev, latent):
    net = _thin(dev, _mod_gs)
    ref = _thin(dev, _mod_gs)
    ref.gemm_mode, ref.attn_mode = "f32", "f32"
    full = ref.decode_latent(latent)[0]
    assert ref.range_fallbacks == [0, 0]
    for chans, box in [([6, 2], (72, 221, 1340, 281)), (None, (357, 358, 713, 1))]:
        with pytest.warns(RuntimeWarning, match="exact-f32"):
            got = net.decode_latent(latent, channels=chans, box=box)[0]
        assert _same_bits(got, _slice(full, chans, box)), (chans, box)
    assert net.range_fallbacks == [0, 2]


def test_subset_itself_is_probed(thin, latent, dev):
    """A non-finite std of a chosen channel poisons only the decoded subset (the residual stream is finite): the probe
    of the subset catches it - the re-run gives the same, and the decode is an error, never a quietly bad subset."""
    mean = torch.zeros(8, device=dev)
    std = torch.ones(8, device=dev)
    std[5] = float("nan")
    before = list(thin.range_fallbacks)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        with pytest.raises(FloatingPointError, match="exact-f32 engines too"):
            thin._decode_guarded(latent[0], mean=mean, std=std, channels=(1, 5), box=(0, 3, 0, 2))
    thin.range_fallbacks[:] = before
    ok = thin._decode_guarded(latent[0], mean=mean, std=std, channels=(1, 4), box=(0, 3, 0, 2))
    assert torch.isfinite(ok).all()


# ---- the 268 model ----------------------------------------------------------------------------------------------------


def test_subset_268_model(dev):
    net = VAEformer(268)
    synth.load_synthetic(net, seed=0)
    net = net.to(dev)
    y = _yhat(256, seed=5).to(dev)
    api_map = cra5_api.resolve_variables
    from cra5_amd.api import variable_mapping
    _, v2c = variable_mapping()
    chans = api_map(["z_500", "q_500", "u_500", "v_500", "t_500", "w_500"], v2c)
    box = cra5_api.grid_box((35, 72, -25, 45))["box"]
    full = net.decode_latent(y)[0]
    got = net.decode_latent(y, channels=chans, box=box)[0]
    assert _same_bits(got, _slice(full, chans, box))
    got = net.decode_latent(y, channels=chans)[0]
    assert _same_bits(got, _slice(full, chans, None))


# ---- API ---------------------------------------------------------------------------------------------------------------


def _api(thin, dev, tmp_path):
    api = cra5_api(local_root=str(tmp_path), device="cuda", weights=thin)
    api._mean_flat = torch.linspace(-1, 1, 8, device=dev)      # (268-channel stats do not fit the 8-channel thin model)
    api._std_flat = torch.linspace(0.5, 2, 8, device=dev)
    api.mean, api.std = api._mean_flat.view(8, 1, 1), api._std_flat.view(8, 1, 1)
    return api


def test_api_decode_from_bin_subset(thin, dev, tmp_path):
    api = _api(thin, dev, tmp_path)
    frame = synth.synth_frame(8, seed=3) * api.std.cpu() + api.mean.cpu()
    ts = "2024-06-01T00:00:00"
    api.encode_era5_as_bin(ts, save_root=str(tmp_path / "CRA5"), data=frame)
    full = api.decode_from_bin(ts)
    assert set(full) == {"x_hat", "decoding_time"}
    names = ["z_850", "z_1000", "z_925"]        # the thin model's 8 channels carry the first 8 names (z at 1000..825)
    chans = [api.vname_to_channels[v] for v in names]
    region = (35, 72, -25, 45)
    g = cra5_api.grid_box(region)
    d = api.decode_from_bin(ts, variables=names, region=region, to_host=True)
    assert set(d) == {"x_hat", "decoding_time", "variables", "lat", "lon"}
    assert d["variables"] == names and isinstance(d["x_hat"], np.ndarray)
    assert d["lat"].dtype == np.float64 and np.array_equal(d["lat"], g["lat"]) and np.array_equal(d["lon"], g["lon"])
    assert d["lon"].min() >= 0 and d["lon"].max() < 360 and d["lat"][0] == 72.0 and d["lat"][-1] == 35.0
    ref = _slice(full["x_hat"].reshape(8, H, W), chans, g["box"]).cpu().numpy()
    assert d["x_hat"].shape == (3, 149, 281) and np.array_equal(d["x_hat"].view(np.int32), ref.view(np.int32))
    dn = api.decode_from_bin(ts, return_format="normalized", variables=names)
    full_n = api.decode_from_bin(ts, return_format="normalized")["x_hat"]
    assert _same_bits(dn["x_hat"][0], _slice(full_n[0], chans, None))
    assert len(dn["lat"]) == H and len(dn["lon"]) == W
    dr = api.decode_from_bin(ts, region=(-90, 90, -180, 180))
    assert dr["variables"] == [api.channels_to_vname[c] for c in range(8)] and dr["lon"][0] == 180.0
    assert _same_bits(dr["x_hat"], _slice(full["x_hat"].reshape(8, H, W), None, (0, H, 720, W)))
    xr = api.latent_to_reconstruction(api.bin_to_latent(time_stamp=ts), variables=names[:1], region=(0, 0, 0, 0))
    assert xr.shape == (1, 1, 1, 1) and _same_bits(xr[0], _slice(full_n[0], chans[:1], (360, 361, 0, 1)))
    with pytest.raises(ValueError, match="latent"):
        api.decode_from_bin(ts, return_format="latent", variables=names)
    with pytest.raises(ValueError, match="unknown"):
        api.decode_from_bin(ts, variables=["z_850", "nope"])
    with pytest.raises(ValueError, match="more than once"):
        api.decode_from_bin(ts, variables=["z_850", "z_850"])


def test_api_decode_batch_subset(thin, dev, tmp_path):
    api = _api(thin, dev, tmp_path)
    frames = [(synth.synth_frame(8, seed=s) * api.std.cpu() + api.mean.cpu()).numpy() for s in (3, 4, 5)]
    stamps = [f"2024-06-01T{h:02d}:00:00" for h in range(3)]
    api.encode_era5_batch(stamps, data=frames, save_root=str(tmp_path / "CRA5"), workers=3)
    names, region = ["z_825", "z_975"], (-10.3, 20.1, 350.2, 9.9)
    g = cra5_api.grid_box(region)
    chans = [api.vname_to_channels[v] for v in names]
    shape = (2, len(g["lat"]), len(g["lon"]))
    out = np.empty((3,) + shape, dtype=np.float32)
    rec = api.decode_batch(stamps, out=out, workers=3, variables=names, region=region)
    seen = {}
    api.decode_batch(stamps, workers=2, variables=names, region=region,
                     sink=lambda i, fr: seen.__setitem__(i, (fr.shape, fr.copy())))
    for i, ts in enumerate(stamps):
        full = api.decode_from_bin(ts)["x_hat"].reshape(8, H, W)
        ref = _slice(full, chans, g["box"]).cpu().numpy()
        assert np.array_equal(out[i].view(np.int32), ref.view(np.int32)) and rec[i] is not None
        assert seen[i][0] == shape and np.array_equal(seen[i][1].view(np.int32), ref.view(np.int32))
    with pytest.raises(ValueError, match="out"):
        api.decode_batch(stamps, out=np.empty((3, 8, H, W), dtype=np.float32), variables=names, region=region)
