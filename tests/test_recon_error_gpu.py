"""Per-variable reconstruction error on the GPU (csrc/metrics.hip, cra5_amd.metrics, cra5_api.evaluate_batch), every value
against float64 numpy computed here from the same fp32 frames."""
import os

import numpy as np
import pytest
import torch

from cra5_amd import metrics, synth
from cra5_amd.pipeline import FramePipeline
from cra5_amd.vaeformer import VAEformer
from cra5_amd.zoo import vaeformer_pretrained

pytestmark = pytest.mark.gpu

STATS = ("mse", "rmse", "wrmse", "bias", "mae", "max_abs", "nonfinite")


def ref_stats(xh, x, lat):
    """float64 reference of the metric's definition: d = x_hat - x in fp32, statistics in float64, per channel."""
    C = x.shape[0]
    r = {k: np.empty(C) for k in STATS}
    r["nonfinite"] = np.empty(C, dtype=np.int64)
    L = np.ones(x.shape[1]) if lat is None else np.asarray(lat, dtype=np.float64)
    for c in range(C):
        bad = ~(np.isfinite(xh[c]) & np.isfinite(x[c]))
        d32 = xh[c] - x[c]
        d = d32.astype(np.float64)
        nf = int(bad.sum())
        r["nonfinite"][c] = nf
        if nf:
            for k in ("mse", "rmse", "wrmse", "bias", "mae", "max_abs"):
                r[k][c] = np.nan
            continue
        r["mse"][c] = np.mean(d * d)
        r["rmse"][c] = np.sqrt(r["mse"][c])
        r["wrmse"][c] = np.sqrt(np.mean(L[:, None] * d * d))
        r["bias"][c] = np.mean(d)
        r["mae"][c] = np.mean(np.abs(d))
        r["max_abs"][c] = np.max(np.abs(d32))          # fp32, exact
    return r


def assert_matches(got, ref, rtol=1e-6):
    for k in STATS:
        assert got[k].shape == ref[k].shape, k
    assert got["nonfinite"].dtype == np.int64 and np.array_equal(got["nonfinite"], ref["nonfinite"])
    for k in ("mse", "rmse", "wrmse", "mae", "bias", "max_abs"):
        assert got[k].dtype == np.float64, k
        assert np.array_equal(np.isnan(got[k]), np.isnan(ref[k])), k
    ok = ~np.isnan(ref["mse"])
    for k in ("mse", "rmse", "wrmse", "mae"):
        np.testing.assert_allclose(got[k][ok], ref[k][ok], rtol=rtol, atol=0, err_msg=k)
    assert np.all(np.abs(got["bias"][ok] - ref["bias"][ok]) <= rtol * ref["mae"][ok])
    assert np.array_equal(got["max_abs"][ok], ref["max_abs"][ok])


def physical_pair(C, H, W, seed, dev):
    """x at physical scales (offset ~5e4, std ~1e4 per channel) and x_hat = x + an error of 10 .. 1000 per channel."""
    g = torch.Generator(device=dev).manual_seed(seed)
    u = torch.rand((3, C, 1, 1), generator=g, device=dev)
    x = 5e4 * (1 + 0.2 * u[0]) + 1e4 * (0.5 + u[1]) * torch.randn((C, H, W), generator=g, device=dev)
    xh = x + 10.0 ** (1 + 2 * u[2]) * torch.randn((C, H, W), generator=g, device=dev)
    return xh.contiguous(), x.contiguous()


@pytest.mark.parametrize("shape", [(268, 721, 1440), (3, 37, 44), (5, 721, 1439), (1, 1, 3)])
def test_kernel_matches_float64(shape, dev):
    C, H, W = shape
    xh, x = physical_pair(C, H, W, seed=C + H + W, dev=dev)
    lat = "era5" if H >= 2 else None
    got = metrics.reconstruction_error(xh, x, lat_weights=lat)
    xh_np, x_np = xh.cpu().numpy(), x.cpu().numpy()
    assert_matches(got, ref_stats(xh_np, x_np, metrics.latitude_weights(H) if lat else None))
    if H >= 2:
        # no weights: wrmse IS rmse; an explicit [H] array; the [1, C, H, W] form
        g0 = metrics.reconstruction_error(xh, x, lat_weights=None)
        assert np.array_equal(g0["wrmse"], g0["rmse"]) and np.array_equal(g0["mse"], got["mse"])
        lw = np.linspace(0.5, 1.5, H)
        assert_matches(metrics.reconstruction_error(xh, x, lat_weights=lw), ref_stats(xh_np, x_np, lw))
        g4 = metrics.reconstruction_error(xh.unsqueeze(0), x.unsqueeze(0), lat_weights=lat)
        assert all(np.array_equal(g4[k], got[k]) for k in STATS)


def test_unaligned_views(dev):
    """Frames that do not start on a 16-byte boundary take the element-wise path: same values."""
    C, H, W = 2, 37, 44
    xh, x = physical_pair(C, H, W, seed=11, dev=dev)
    n = C * H * W
    bh, bx = torch.empty(n + 1, device=dev), torch.empty(n + 3, device=dev)
    bh[1:].copy_(xh.reshape(-1))
    bx[3:].copy_(x.reshape(-1))
    vh, vx = bh[1:].view(C, H, W), bx[3:].view(C, H, W)
    assert vh.data_ptr() % 16 and vx.data_ptr() % 16
    got = metrics.reconstruction_error(vh, vx)
    assert_matches(got, ref_stats(xh.cpu().numpy(), x.cpu().numpy(), metrics.latitude_weights(H)))


def test_nonfinite_channels(dev):
    C, H, W = 6, 721, 1439
    xh, x = physical_pair(C, H, W, seed=5, dev=dev)
    xh[1, 0, 0] = float("nan")
    xh[1, 400, 1438] = float("nan")
    xh[1, 720, 7] = float("nan")
    x[4, 13, 3] = float("inf")
    x[4, 13, 4] = float("-inf")
    x[4, 700, 1000] = float("inf")
    xh[4, 700, 1000] = float("nan")          # one position, both frames bad: counted once
    got = metrics.reconstruction_error(xh, x)
    assert got["nonfinite"].tolist() == [0, 3, 0, 0, 3, 0]
    for k in ("mse", "rmse", "wrmse", "bias", "mae", "max_abs"):
        assert np.isnan(got[k]).tolist() == [False, True, False, False, True, False], k
    assert_matches(got, ref_stats(xh.cpu().numpy(), x.cpu().numpy(), metrics.latitude_weights(H)))


def test_deterministic_across_calls_and_workers(dev):
    pairs = [physical_pair(32, 721, 1440, seed=s, dev=dev) for s in range(5)]
    one = [metrics.reconstruction_error(*p) for p in pairs]
    again = [metrics.reconstruction_error(*p) for p in pairs]
    runs = []
    for w in (1, 3):
        pipe = FramePipeline(None, workers=w, device=dev)
        try:
            runs.append(pipe.map(lambda p: metrics.reconstruction_error(*p), pairs))
        finally:
            pipe.close()
    for res in (again, runs[0], runs[1]):
        for a, b in zip(one, res):
            assert all(np.array_equal(a[k], b[k]) for k in STATS)


# ---- cra5_api.evaluate_batch ------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def thin(dev):
    net = VAEformer(0, **synth.thin_model_kwargs())
    synth.load_synthetic(net, seed=7)
    return net.to(dev)


def thin_api(thin, dev, root):
    """The 8-channel thin model with unit-style statistics (the 268-channel ones do not apply)."""
    from cra5_amd.api import cra5_api
    api = cra5_api(local_root=str(root), device="cuda", weights=thin)
    api._mean_flat = torch.linspace(-1, 1, 8, device=dev)
    api._std_flat = torch.linspace(0.5, 2, 8, device=dev)
    api.mean, api.std = api._mean_flat.view(8, 1, 1), api._std_flat.view(8, 1, 1)
    return api


def check_report(api, rep, ts, frame, bin_path):
    C, H, W = frame.shape
    x_hat = api.decode_from_bin(custom_path=bin_path, return_format="de_normalized", to_host=True)["x_hat"]
    assert_matches(rep, ref_stats(x_hat.reshape(C, H, W), frame, metrics.latitude_weights(H)))
    std = api._std_flat.cpu().numpy().astype(np.float64)
    np.testing.assert_allclose(rep["rmse_norm"], rep["rmse"] / std, rtol=1e-15, atol=0)
    assert rep["time_stamp"] == ts
    assert rep["variables"] == [api.channels_to_vname[c] for c in range(C)]
    assert rep["bin_bytes"] == os.path.getsize(bin_path)
    assert rep["compression_ratio"] == C * H * W * 4 / rep["bin_bytes"]


def test_evaluate_batch_codec_and_dataset_modes(thin, dev, tmp_path):
    api = thin_api(thin, dev, tmp_path)
    frames = [(synth.synth_frame(8, seed=s) * api.std.cpu() + api.mean.cpu()).numpy() for s in (3, 4, 5)]
    stamps = [f"2024-06-01T{h:02d}:00:00" for h in range(3)]
    api.phase_log = []
    reps = api.evaluate_batch(stamps, data=frames, save_root=str(tmp_path / "EV"), workers=3)
    log, api.phase_log = api.phase_log, None
    assert not [p for p in log if p[1].startswith("d2h")]       # no reconstruction crossed to the host
    assert [p for p in log if p[1] == "metrics"]
    paths = [str(tmp_path / "EV" / "2024" / f"{ts}.bin") for ts in stamps]
    for i, ts in enumerate(stamps):
        one = api.encode_era5_as_bin(ts, save_root=str(tmp_path / "single"), data=frames[i])
        assert open(paths[i], "rb").read() == open(one["save_path"], "rb").read()
        check_report(api, reps[i], ts, frames[i], paths[i])
    # dataset check on the files just written: the same reports, bit for bit
    api.phase_log = []
    ds = api.evaluate_batch(stamps, data=frames, bins=paths, workers=2)
    log, api.phase_log = api.phase_log, None
    assert not [p for p in log if p[1].startswith("d2h")]
    # no save_root: nothing written; one worker: the same numbers
    solo = api.evaluate_batch(stamps, data=frames, workers=1)
    for a in (ds, solo):
        for r, q in zip(reps, a):
            assert set(q) == set(r)
            for k in set(STATS) | {"rmse_norm"}:
                assert np.array_equal(r[k], q[k], equal_nan=True), k
            assert (q["bin_bytes"], q["compression_ratio"], q["variables"]) == \
                (r["bin_bytes"], r["compression_ratio"], r["variables"])
    assert sorted(os.listdir(tmp_path / "EV" / "2024")) == sorted(f"{ts}.bin" for ts in stamps)
    with pytest.raises(ValueError):
        api.evaluate_batch(stamps, data=frames, bins=paths[:2])


def test_evaluate_batch_full_size(dev, tmp_path):
    from cra5_amd.api import cra5_api
    net = vaeformer_pretrained(quality=268, pretrained=False)
    synth.load_synthetic(net, seed=7)
    api = cra5_api(local_root=str(tmp_path), device="cuda", weights=net.to(dev))
    mean, std = api.get_mean_std()
    frame = (synth.synth_frame(268, seed=2).numpy() * std[:, None, None] + mean[:, None, None]).astype(np.float32)
    ts = "2024-06-01T00:00:00"
    rep = api.evaluate_batch([ts], data=[frame], save_root=str(tmp_path / "EV"), workers=1)[0]
    check_report(api, rep, ts, frame, str(tmp_path / "EV" / "2024" / f"{ts}.bin"))
    assert "z_500" in rep["variables"] and "t2m" in rep["variables"]
    np.testing.assert_allclose(rep["rmse_norm"], rep["rmse"] / std.astype(np.float64), rtol=1e-15)
