"""Point decode on the GPU (points=: VAEformer.decode_latent / _decode_guarded, cra5_api.decode_from_bin / decode_batch /
series_batch, cra5_amd.points.sample): the three kernels of csrc/points.hip against numpy, and the decode at a point
list against the full decode of the same latent - "nearest" is the node's value bit for bit, "bilinear" a float64 numpy
restatement of the formula applied to the full decode and the bits of regrid=Grid([lat], [lon]) - under every engine and
precision, on the sparse and on the dense route.  All comparisons are on bit patterns."""
import math
import warnings

import numpy as np
import pytest
import torch

from cra5_amd import ops, synth
from cra5_amd import points as cpoints
from cra5_amd.api import cra5_api, variable_mapping
from cra5_amd.points import Points
from cra5_amd.regrid import Grid
from cra5_amd.vaeformer import VAEformer

pytestmark = pytest.mark.gpu

H, W = 721, 1440
TOL_DEG = 1e-9
ENGINES = {
    "default": {},
    "f32": dict(gemm_mode="f32"),
    "unfused": dict(fused_unembed=False),
    "f16": dict(precision="f16"),
    "f16_unfused": dict(precision="f16", fused_unembed=False),
}


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


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _same_bits(a, b):
    a, b = _bits(a), _bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


# ---- the numpy restatement ------------------------------------------------------------------------------------------------


def _taps(r, tol):
    """One axis of the bilinear rule: within tol of a lattice index one tap, else floor and floor + 1."""
    n = float(np.rint(r))
    if abs(r - n) <= tol:
        return [(int(n), 1.0)]
    h0 = math.floor(r)
    f = r - h0
    return [(h0, 1.0 - f), (h0 + 1, f)]


def _axes(lat, lon, Hg, Wg):
    dlat, dlon = 180.0 / (Hg - 1), 360.0 / Wg
    return ([_taps((90.0 - v) / dlat, TOL_DEG / dlat) for v in lat],
            [[(c % Wg, w) for c, w in _taps(v / dlon, TOL_DEG / dlon)] for v in lon])


def _ref_bilinear(img, lat, lon):
    """img float32 [C, H, W] -> [C, P]: float64, sums from 0.0, one rounding per product and per add, north to south over
    west to east."""
    C, Hg, Wg = img.shape
    rt, ct = _axes(lat, lon, Hg, Wg)
    out = np.empty((C, len(lat)), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for p in range(len(lat)):
            acc = np.zeros(C, dtype=np.float64)
            for h, w in rt[p]:
                inner = np.zeros(C, dtype=np.float64)
                for c, v in ct[p]:
                    inner = inner + v * img[:, h, c].astype(np.float64)
                acc = acc + w * inner
            out[:, p] = acc.astype(np.float32)
    return out


def _nearest_nodes(lat, lon, Hg=H, Wg=W):
    dlat, dlon = 180.0 / (Hg - 1), 360.0 / Wg
    rows = np.rint((90.0 - np.asarray(lat)) / dlat).astype(np.int64)
    cols = np.rint(np.mod(np.asarray(lon), 360.0) / dlon).astype(np.int64) % Wg
    return rows, cols


def _ref_points(full, lat, lon, method):
    img = full.detach().cpu().numpy()
    if method == "nearest":
        rows, cols = _nearest_nodes(lat, lon, img.shape[1], img.shape[2])
        return img[:, rows, cols]
    return _ref_bilinear(img, lat, lon)


def _same_where_finite(got, ref):
    """Bit-equal where the reference is not NaN, NaN exactly where it is (a NaN's payload is the arithmetic's own)."""
    got, ref = np.asarray(got), np.asarray(ref)
    nan = np.isnan(ref)
    return got.shape == ref.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got)[~nan], _bits(ref)[~nan])


# ---- gather_token_list ------------------------------------------------------------------------------------------------------


def test_gather_token_list_matches_numpy(dev):
    g = torch.Generator().manual_seed(0)
    n_src, K = 60, 36                                     # rows of 144 bytes
    alloc = torch.randn(n_src + 1, K + 12, generator=g).to(dev)     # one row more than declared, pitch 192 bytes
    tok = torch.tensor([5, 0, 59, 5, 17, n_src, 33, -1, 1], dtype=torch.int32, device=dev)
    for src in (alloc[:n_src, :K], alloc[:n_src, :K].contiguous()):
        dst_full = torch.full((len(tok), K + 4), -7.0, device=dev)
        out = ops.gather_token_list(src, dst_full[:, :K], tok)
        got, s = out.cpu().numpy(), src.cpu().numpy()
        for r, t in enumerate(tok.tolist()):
            if 0 <= t < n_src:
                assert np.array_equal(got[r].view(np.int32), s[t].view(np.int32)), (r, t)
            else:
                assert (got[r].view(np.int32) == -1).all(), (r, t)          # all 0xFF bytes
        assert (dst_full[:, K:] == -7.0).all()             # nothing written past the row
    # split-f16 rows and plain rows: verbatim, layout flag and scale included; the source one row longer than declared
    sm = ops.split_f16(alloc[:, :K].contiguous(), "auto")
    for plain in (False, True):
        m = sm
        if plain:   # a plain row living in a split-layout buffer, as the LayerNorm writes it
            pc = sm.plain_copy()
            buf = ops.SplitMat.empty(n_src + 1, K, dev, zero=True)
            buf.data[:, :pc.Kp].copy_(pc.data)
            m = ops.SplitMat(buf.data, n_src + 1, K, pc.Kp, pc.scale_inv, plain=True)
        decl = ops.SplitMat(m.data[:n_src], n_src, K, m.Kp, m.scale_inv, plain=plain)
        out = ops.gather_token_list(decl, ops.SplitMat.empty(len(tok), K, dev, zero=True), tok)
        assert out.plain == plain and out.scale_inv == m.scale_inv
        n = m.Kp if plain else 2 * m.Kp
        for r, t in enumerate(tok.tolist()):
            if 0 <= t < n_src:
                assert torch.equal(out.data[r, :n], m.data[t, :n]), (plain, r, t)
            else:
                assert (out.data[r, :n] == -1).all(), (plain, r, t)
                assert torch.isnan(out.data[r, :n].view(torch.float16)).all()
    with pytest.raises(ValueError, match="tok"):
        ops.gather_token_list(alloc[:n_src, :K], torch.empty(2, K, device=dev), torch.tensor([1, 2], device=dev))


# ---- points.sample ----------------------------------------------------------------------------------------------------------

HS, WS = 31, 40          # dlat = 6, dlon = 9


def _sample_points():
    rng = np.random.default_rng(1)
    lat = list(rng.uniform(-90, 90, 40)) + [90.0 - 6.0 * 5, 90.0, -90.0, 90.0, -90.0, 13.0, -44.0, 7.7, 60.0, 90.0 - 6.0 * 30]
    lon = list(rng.uniform(0, 360, 40)) + [9.0 * 7, 0.0, 200.0, 355.5, 123.4, 355.0, 359.999, -3.0, -9.0, 9.0 * 39 + 720]
    return np.array(lat), np.array(lon)


def test_sample_matches_numpy_restatement(dev):
    g = torch.Generator().manual_seed(2)
    img = torch.randn(3, HS, WS, generator=g)
    lat, lon = _sample_points()
    x = img.to(dev)
    got = cpoints.sample(x, Points(lat, lon))
    assert tuple(got.shape) == (3, len(lat)) and got.dtype == torch.float32
    assert _same_bits(got, _ref_bilinear(img.numpy(), lat, lon))
    assert _same_bits(cpoints.sample(x, np.stack([lat, lon], axis=1)), got)          # the [P, 2] form
    # on-lattice points copy the value: row 5 column 7, both poles, row 30 column 39 given as 39 * 9 + 720 degrees
    a = img.numpy()
    assert _same_bits(got[:, 40], a[:, 5, 7]) and _same_bits(got[:, 41], a[:, 0, 0]) and _same_bits(got[:, 49], a[:, 30, 39])
    # the last cell wraps to column 0, and so does a negative longitude
    rt, ct = _axes(lat, lon, HS, WS)
    assert [c for c, _ in ct[45]] == [39, 0] and [c for c, _ in ct[46]] == [39, 0] and [c for c, _ in ct[47]] == [39, 0]
    assert [c for c, _ in ct[48]] == [39]
    # nearest against plain indexing
    rows, cols = _nearest_nodes(lat, lon, HS, WS)
    assert _same_bits(cpoints.sample(x, Points(lat, lon, "nearest")), a[:, rows, cols])
    with pytest.raises(ValueError, match="sample"):
        cpoints.sample(x[0], Points(lat, lon))


def test_sample_nonfinite_nodes_reach_exactly_their_points(dev):
    g = torch.Generator().manual_seed(3)
    img = torch.randn(3, HS, WS, generator=g).numpy()
    planted = {(0, 10, 12): np.nan, (1, 20, 39): np.inf, (2, 3, 0): -np.inf, (1, 0, 5): np.nan}
    for k, v in planted.items():
        img[k] = v
    rng = np.random.default_rng(4)
    lat = np.concatenate([rng.uniform(-90, 90, 400), [90.0 - 6 * 10, 90.0 - 6 * 10.5, 90.0 - 6 * 20.2, 90.0 - 6 * 2.9, 90.0, 89.0]])
    lon = np.concatenate([rng.uniform(0, 360, 400), [9.0 * 12, 9.0 * 11.5, 9.0 * 39.5, 359.0, 9.0 * 5, 9.0 * 4.5]])
    got = cpoints.sample(torch.from_numpy(img).to(dev), Points(lat, lon)).cpu().numpy()
    assert _same_where_finite(got, _ref_bilinear(img, lat, lon))
    rt, ct = _axes(lat, lon, HS, WS)
    for c in range(3):
        touched = np.array([any((c, h, w) in planted for h, _ in rt[p] for w, _ in ct[p]) for p in range(len(lat))])
        assert np.array_equal(~np.isfinite(got[c]), touched), c
        assert touched[400:].sum() >= 1
    assert (~np.isfinite(got)).sum() >= 6


def test_sample_nearest_copies_bits(dev):
    img = np.zeros((2, HS, WS), dtype=np.float32)
    img[0, 4, 6] = -0.0
    img[1, 4, 6] = np.array([0x7FC12345], dtype=np.uint32).view(np.float32)[0]      # a NaN with a payload
    img[0, 30, 0] = np.array([0xFFA00001], dtype=np.uint32).view(np.float32)[0]      # a signalling one, negative
    got = cpoints.sample(torch.from_numpy(img).to(dev), Points([90.0 - 6 * 4.2, -90.0], [9 * 5.9, 358.0], "nearest"))
    b = _bits(got).view(np.uint32)
    assert b[0, 0] == 0x80000000 and b[1, 0] == 0x7FC12345 and b[0, 1] == 0xFFA00001 and b[1, 1] == 0


# ---- the model ----------------------------------------------------------------------------------------------------------------


def _model_points():
    rng = np.random.default_rng(5)
    lat = [90.0, -90.0, 0.0, 90.0 - 9.5 * 0.25, 23.4, 51.5, 51.5, 89.9, -89.9] + list(rng.uniform(-90, 90, 300))
    lon = [33.25, 100.1, 12.5, 9.5 * 0.25, 359.9, -0.12, -0.12, 181.0, 0.05] + list(rng.uniform(-180, 540, 300))
    return np.array(lat), np.array(lon)


@pytest.fixture(scope="module")
def thin(dev):
    return _thin(dev)


@pytest.fixture(scope="module")
def latent(dev):
    return _yhat(16, seed=11).to(dev)


def test_model_points_cover_the_edge_cases():
    lat, lon = _model_points()
    p = Points(lat, lon).plan(H, W)
    assert list(p["rows"][0]) == [0, -1] and list(p["rows"][1]) == [720, -1] and list(p["rows"][2]) == [360, -1]
    ms = p["contrib"][p["pnode"][3]][:, [0, 2]].ravel()
    assert sorted(set(p["tokens"][ms[ms >= 0]])) == [0, 1, 144, 145]
    assert list(p["cols"][4]) == [1439, 0] and np.array_equal(p["pnode"][5], p["pnode"][6])
    assert 100 < len(p["tokens"]) < VAEformer.POINT_DENSE_TOKENS


@pytest.mark.parametrize("engine", list(ENGINES))
def test_points_equal_the_full_decode(thin, latent, dev, engine, monkeypatch):
    calls = {"cols": 0, "image": 0}
    for name, fn in (("cols", ops.points_from_cols), ("image", ops.points_from_image)):
        def counted(*a, _n=name, _f=fn, **k):
            calls[_n] += 1
            return _f(*a, **k)
        monkeypatch.setattr(ops, "points_from_" + name, counted)
    keep = (thin.precision, thin.gemm_mode, thin.fused_unembed)
    lat, lon = _model_points()
    try:
        for k, v in ENGINES[engine].items():
            setattr(thin, k, v)
        mean = torch.linspace(-1, 1, 8, device=dev)
        std = torch.linspace(0.5, 2, 8, device=dev)
        full_n = thin.decode_latent(latent)[0]
        full_d = thin._decode_guarded(latent[0], mean=mean, std=std)
        ref = {(m, d): _ref_points(f, lat, lon, m) for m in ("nearest", "bilinear") for d, f in (("n", full_n), ("d", full_d))}
        one = {m: _ref_points(full_n, lat[300:301], lon[300:301], m) for m in ("nearest", "bilinear")}
        sparse = {}
        for dense in (False, True):
            if dense:
                thin.POINT_DENSE_TOKENS = 0
            before = dict(calls)
            for method in ("nearest", "bilinear"):
                pts = Points(lat, lon, method)
                for chans in (None, [5, 1, 3]):
                    sl = slice(None) if chans is None else chans
                    got = thin.decode_latent(latent, channels=chans, points=pts)[0]
                    assert tuple(got.shape) == (8 if chans is None else 3, len(lat))
                    assert _same_bits(got, ref[method, "n"][sl]), (engine, method, chans, dense, "normalized")
                    plan = thin._points_arg(pts)
                    ch = thin._subset_args(chans)[0]
                    got = thin._decode_guarded(latent[0], mean=mean, std=std, channels=ch, points=plan)
                    assert _same_bits(got, ref[method, "d"][sl]), (engine, method, chans, dense, "de-normalised")
                    if not dense:
                        sparse[method, None if chans is None else tuple(chans)] = got
                    else:
                        assert _same_bits(got, sparse[method, None if chans is None else tuple(chans)])
                # one point alone
                got = thin.decode_latent(latent, channels=[5, 1, 3], points=Points(lat[300:301], lon[300:301], method))[0]
                assert tuple(got.shape) == (3, 1) and _same_bits(got, one[method][[5, 1, 3]]), (engine, method, dense, "P = 1")
            used = {k: calls[k] - before[k] for k in calls}
            assert used == ({"cols": 0, "image": 10} if dense else {"cols": 10, "image": 0}), (dense, used)
        del thin.POINT_DENSE_TOKENS
        # the bits of regrid=Grid([lat], [lon]) at five of the points: a seam node, the four-node point, the wrap, two random
        got = thin.decode_latent(latent, channels=[5, 1, 3], points=Points(lat, lon))[0]
        for p in (2, 3, 4, 9, 200):
            r = thin.decode_latent(latent, channels=[5, 1, 3], regrid=Grid([lat[p]], [lon[p]]))[0]
            assert _same_bits(got[:, p], r[:, 0, 0]), (engine, p)
        # the [P, 2] array form is Points(lat, lon)
        assert _same_bits(thin.decode_latent(latent, channels=[5, 1, 3], points=np.stack([lat, lon], axis=1))[0], got)
        assert thin.range_fallbacks == [0, 0]
    finally:
        thin.precision, thin.gemm_mode, thin.fused_unembed = keep
        if "POINT_DENSE_TOKENS" in thin.__dict__:
            del thin.POINT_DENSE_TOKENS


def test_points_argument_errors(thin, latent):
    pts = Points([10.0], [20.0])
    for kw in (dict(box=(0, 10, 0, 10)), dict(step=2), dict(coarsen=2), dict(regrid=Grid([10.0], [20.0]))):
        with pytest.raises(ValueError, match=f"points and {list(kw)[0]}"):
            thin.decode_latent(latent, points=pts, **kw)
    with pytest.raises(ValueError, match="points"):
        thin.decode_latent(latent, points="stations")
    with pytest.raises(ValueError, match="plan was built"):
        thin.decode_latent(latent, points=pts.plan(31, 40, 11, 10, 10, 10))
    with pytest.raises(ValueError, match="destination"):
        thin._decode_guarded(latent[0], points=thin._points_arg(pts), out=torch.empty(8, 2, device=latent.device))


def _mod_gs(net):      # outlier hidden units in a g_s MLP (tests/test_subset_decode_gpu.py)
    net.g_s.blocks[2].mlp.fc1.weight[:4] *= 3e5
    net.g_s.blocks[2].mlp.fc1.bias[:4] *= 3e5
    net.g_s.blocks[2].mlp.fc2.weight[:, :4] /= 3e5


def test_range_guard_reruns_poisoned_points(dev, latent):
    net = _thin(dev, _mod_gs)
    ref = _thin(dev, _mod_gs)
    ref.gemm_mode, ref.attn_mode = "f32", "f32"
    full = ref.decode_latent(latent)[0]
    assert ref.range_fallbacks == [0, 0]
    lat, lon = _model_points()
    for n, (method, chans) in enumerate([("nearest", [6, 2]), ("bilinear", None)]):
        with pytest.warns(RuntimeWarning, match="exact-f32"):
            got = net.decode_latent(latent, channels=chans, points=Points(lat, lon, method))[0]
        assert _same_bits(got, _ref_points(full, lat, lon, method)[slice(None) if chans is None else chans]), method
        assert net.range_fallbacks == [0, n + 1]


def test_points_themselves_are_probed(thin, latent, dev):
    """A non-finite std of a chosen channel poisons only the point output (the residual stream is finite): the probe of
    the points catches it; a channel that is not chosen does not matter."""
    mean = torch.zeros(8, device=dev)
    std = torch.ones(8, device=dev)
    std[5] = float("nan")
    plan = thin._points_arg(Points([10.0, -20.0, 33.3], [5.0, 100.0, 359.95]))
    before = list(thin.range_fallbacks)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        with pytest.raises(FloatingPointError, match="exact-f32 engines too"):
            thin._decode_guarded(latent[0], mean=mean, std=std, channels=(1, 5), points=plan)
    thin.range_fallbacks[:] = before
    ok = thin._decode_guarded(latent[0], mean=mean, std=std, channels=(1, 4), points=plan)
    assert tuple(ok.shape) == (2, 3) and torch.isfinite(ok).all()


def test_bounded_point_caches(thin, latent):
    rng = np.random.default_rng(6)
    for i in range(24):
        n = 1 + i % 5
        thin.decode_latent(latent, channels=[int(c) for c in rng.permutation(8)[:1 + i % 3]],
                           points=Points(rng.uniform(-90, 90, n), rng.uniform(0, 360, n), ("nearest", "bilinear")[i % 2]))
        assert len(thin._sub_cache) <= VAEformer.SUBSET_CACHE


def test_points_268_model(dev):
    net = VAEformer(268)
    synth.load_synthetic(net, seed=0)
    net = net.to(dev)
    y = _yhat(256, seed=5).to(dev)
    _, v2c = variable_mapping()
    chans = cra5_api.resolve_variables(["z_500", "q_500", "u_500", "v_500", "t_500", "w_500"], v2c)
    rng = np.random.default_rng(7)
    lat, lon = rng.uniform(-90, 90, 50), rng.uniform(0, 360, 50)
    full = net.decode_latent(y)[0]
    for method in ("nearest", "bilinear"):
        got = net.decode_latent(y, channels=chans, points=Points(lat, lon, method))[0]
        assert _same_bits(got, _ref_points(full[chans], lat, lon, method)), method
    assert net.range_fallbacks == [0, 0]


# ---- API ------------------------------------------------------------------------------------------------------------------------

NAMES = ["z_850", "z_1000", "z_925"]     # the thin model's 8 channels carry the first 8 names (z at 1000 .. 825)
STAMPS = [f"2024-06-01T{h:02d}:00:00" for h in range(3)]


@pytest.fixture(scope="module")
def archive(thin, dev, tmp_path_factory):
    root = tmp_path_factory.mktemp("points_archive")
    api = cra5_api(local_root=str(root), device="cuda", weights=thin)
    api._mean_flat = torch.linspace(-1, 1, 8, device=dev)      # (268-channel stats do not fit the 8-channel thin model)
    api._std_flat = torch.linspace(0.5, 2, 8, device=dev)
    api.mean, api.std = api._mean_flat.view(8, 1, 1), api._std_flat.view(8, 1, 1)
    frames = [(synth.synth_frame(8, seed=s) * api.std.cpu() + api.mean.cpu()).numpy() for s in (3, 4, 5)]
    api.encode_era5_batch(STAMPS, data=frames, save_root=str(root / "CRA5"), workers=3)
    chans = [api.vname_to_channels[v] for v in NAMES]
    fulls = [api.decode_from_bin(ts)["x_hat"].reshape(8, H, W)[chans].clone() for ts in STAMPS]
    return api, fulls


def _api_points():
    rng = np.random.default_rng(8)
    return np.concatenate([[90.0, 0.0, -33.3], rng.uniform(-90, 90, 20)]), np.concatenate([[10.0, 359.9, -0.1], rng.uniform(0, 360, 20)])


def test_api_decode_from_bin_points(archive):
    api, fulls = archive
    lat, lon = _api_points()
    for method in ("bilinear", "nearest"):
        d = api.decode_from_bin(STAMPS[0], points=Points(lat, lon, method), variables=NAMES, to_host=True)
        keys = {"x_hat", "decoding_time", "variables", "lat", "lon", "points"}
        assert set(d) == (keys | {"node_lat", "node_lon"} if method == "nearest" else keys)
        assert d["variables"] == NAMES and d["points"] == method and isinstance(d["x_hat"], np.ndarray)
        assert d["lat"].dtype == np.float64 and np.array_equal(d["lat"], lat) and np.array_equal(d["lon"], np.mod(lon, 360.0))
        assert d["x_hat"].shape == (3, len(lat)) and _same_bits(d["x_hat"], _ref_points(fulls[0], lat, lon, method))
        if method == "nearest":
            rows, cols = _nearest_nodes(lat, lon)
            assert np.array_equal(d["node_lat"], 90.0 - rows * 0.25) and np.array_equal(d["node_lon"], cols * 0.25)
    # on the device, every variable, a [P, 2] array; the normalised format; latent_to_reconstruction
    d = api.decode_from_bin(STAMPS[1], points=np.stack([lat, lon], axis=1))
    assert isinstance(d["x_hat"], torch.Tensor) and tuple(d["x_hat"].shape) == (8, len(lat)) and len(d["variables"]) == 8
    chans = [api.vname_to_channels[v] for v in NAMES]
    assert _same_bits(d["x_hat"][chans], _ref_points(fulls[1], lat, lon, "bilinear"))
    dn = api.decode_from_bin(STAMPS[0], return_format="normalized", points=Points(lat, lon, "nearest"), variables=NAMES)
    full_n = api.decode_from_bin(STAMPS[0], return_format="normalized")["x_hat"][0][chans]
    assert tuple(dn["x_hat"].shape) == (3, len(lat)) and _same_bits(dn["x_hat"], _ref_points(full_n, lat, lon, "nearest"))
    xr = api.latent_to_reconstruction(api.bin_to_latent(time_stamp=STAMPS[0]), variables=NAMES, points=Points(lat, lon, "nearest"))
    assert tuple(xr.shape) == (1, 3, len(lat)) and _same_bits(xr[0], dn["x_hat"])
    out = np.empty((3, len(lat)), dtype=np.float32)
    d = api.decode_from_bin(STAMPS[0], points=Points(lat, lon), variables=NAMES, out=out)
    assert d["x_hat"] is out and _same_bits(out, _ref_points(fulls[0], lat, lon, "bilinear"))


def test_api_decode_batch_and_series(archive):
    api, fulls = archive
    lat, lon = _api_points()
    pts = Points(lat, lon)
    refs = [_ref_points(f, lat, lon, "bilinear") for f in fulls]
    out = np.empty((3, 3, len(lat)), dtype=np.float32)
    rec = api.decode_batch(STAMPS, out=out, workers=3, variables=NAMES, points=pts)
    seen = {}
    api.decode_batch(STAMPS, workers=2, variables=NAMES, points=pts, sink=lambda i, fr: seen.__setitem__(i, (fr.shape, fr.copy())))
    for i in range(3):
        assert _same_bits(out[i], refs[i]) and rec[i] is not None
        assert seen[i][0] == (3, len(lat)) and _same_bits(seen[i][1], refs[i])
    with pytest.raises(ValueError, match="out"):
        api.decode_batch(STAMPS, out=np.empty((3, 3, H, W), dtype=np.float32), variables=NAMES, points=pts)
    # series_batch: the stack of the per-frame decodes, on the device and on the host, whatever the workers
    s3 = api.series_batch(STAMPS, points=pts, variables=NAMES, workers=3)
    assert set(s3) == {"series", "time_stamps", "variables", "lat", "lon", "points"} and s3["time_stamps"] == STAMPS
    assert isinstance(s3["series"], np.ndarray) and s3["series"].shape == (3, 3, len(lat)) and s3["series"].dtype == np.float32
    assert _same_bits(s3["series"], np.stack(refs)) and _same_bits(s3["series"], out)
    s1 = api.series_batch(STAMPS, points=pts, variables=NAMES, workers=1)
    assert _same_bits(s1["series"], s3["series"])
    sd = api.series_batch(paths=[api._bin_path(ts) for ts in STAMPS], points=Points(lat, lon, "nearest"), variables=NAMES,
                          workers=2, to_host=False)
    assert isinstance(sd["series"], torch.Tensor) and "paths" in sd and "time_stamps" not in sd and "node_lat" in sd
    assert _same_bits(sd["series"], np.stack([_ref_points(f, lat, lon, "nearest") for f in fulls]))
    sn = api.series_batch(STAMPS[:1], points=pts, return_format="normalized")
    assert sn["series"].shape == (1, 8, len(lat))
    with pytest.raises(ValueError, match="points"):
        api.series_batch(STAMPS)
    with pytest.raises(ValueError, match="time_stamps or paths"):
        api.series_batch(points=pts)


def test_api_refused_combinations(archive):
    api, _ = archive
    pts = Points([10.0, 20.0], [30.0, 40.0])
    refused = dict(region=(0, 10, 0, 10), stride=2, coarsen=2, regrid=Grid([10.0], [20.0]), residual=True, pack="int16",
                   return_format="latent")
    for name, v in refused.items():
        word = "latent" if name == "return_format" else name
        with pytest.raises(ValueError, match=word):
            api.decode_from_bin(STAMPS[0], points=pts, **{name: v})
        with pytest.raises(ValueError, match=word):
            api.decode_batch(STAMPS, points=pts, **{name: v})
        if name in ("region", "stride", "coarsen", "regrid"):
            with pytest.raises(ValueError, match=word):
                api.latent_to_reconstruction(None, points=pts, **{name: v})
    with pytest.raises(ValueError, match="latent"):
        api.series_batch(STAMPS, points=pts, return_format="latent")
