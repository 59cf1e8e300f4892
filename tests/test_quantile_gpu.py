"""Exact quantiles on the GPU (csrc/quantile.hip, cra5_amd.metrics.frame_quantiles, cra5_api.evaluate_batch(quantiles=)):
every result against the numpy reference of quantile_helpers.ref_quantiles, bit for bit (only the sign of a zero is free)."""
import threading

import numpy as np
import pytest
import torch

from cra5_amd import metrics, ops, synth
from cra5_amd.vaeformer import VAEformer
from quantile_helpers import FAMILIES, FIELDS, Q8, Q16, assert_same_bits, bits, interior_zero_weights, ref_quantiles, smooth

pytestmark = pytest.mark.gpu

SHAPES = [(3, 40, 1440), (2, 9, 45), (2, 5, 7), (1, 1, 1), (1, 2, 2), (2, 721, 8)]
KEYS = tuple("quantile_" + k for k in FIELDS) + ("quantile", "quantile_shift", "nonfinite")


def weight_cases(H):
    """(name, lat_weights argument) - "era5" needs two rows from pole to pole."""
    cases = [("none", None), ("zero-rows", interior_zero_weights(H))]
    if H >= 2:
        cases.append(("era5", "era5"))
    return cases


def same_bytes(a, b, keys=KEYS):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in keys)


def to_dev(pair, dev):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in pair)


@pytest.mark.parametrize("family", sorted(FAMILIES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_matches_numpy_bit_for_bit(shape, family, dev):
    C, H, W = shape
    xh_np, x_np = FAMILIES[family](shape, seed=C + H + W)
    xh, x = to_dev((xh_np, x_np), dev)
    for name, lat in weight_cases(H):
        row_w = metrics.quantile_weights(lat, H)
        got = metrics.frame_quantiles(xh, x, Q8, lat_weights=lat)
        ref, nf = ref_quantiles(xh_np, x_np, Q8, row_w)
        assert got["nonfinite"].tolist() == nf.tolist() == [0] * C
        assert got["quantile"].tolist() == list(Q8) and got["quantile_truth"].shape == (C, len(Q8))
        assert_same_bits(got, ref, f"{shape} {family} {name}")
        assert np.array_equal(got["quantile_shift"], got["quantile_recon"] - got["quantile_truth"])
        assert np.array_equal(got["quantile_truth"][:, 3], got["quantile_truth"][:, 4])     # p = 0.5 asked twice


@pytest.mark.parametrize("q", [(0.37,), Q16], ids=["Q1", "Q16"])
@pytest.mark.parametrize("family", ["smooth", "random_bits"])
def test_one_and_sixteen_probabilities(q, family, dev):
    shape = (3, 40, 1440)
    xh_np, x_np = FAMILIES[family](shape, seed=9)
    xh, x = to_dev((xh_np, x_np), dev)
    for name, lat in weight_cases(shape[1]):
        got = metrics.frame_quantiles(xh, x, q, lat_weights=lat)
        ref, _ = ref_quantiles(xh_np, x_np, q, metrics.quantile_weights(lat, shape[1]))
        assert_same_bits(got, ref, f"Q={len(q)} {family} {name}")
    # [1, C, H, W] frames are the same frames
    assert same_bytes(metrics.frame_quantiles(xh.unsqueeze(0), x.unsqueeze(0), q), metrics.frame_quantiles(xh, x, q))


def test_cross_checks_with_the_metric_and_the_extremes(dev):
    shape = (3, 40, 1440)
    xh_np, x_np = smooth(shape, seed=21)
    xh, x = to_dev((xh_np, x_np), dev)
    for lat in (None, "era5"):
        got = metrics.frame_quantiles(xh, x, Q8, lat_weights=lat)
        err = metrics.reconstruction_error(xh, x, lat_weights=lat)
        if lat is None:                       # with "era5" the poles do not count here, but they do in max_abs
            assert bits(got["quantile_abs_error"][:, -1]) == bits(err["max_abs"])
            assert bits(got["quantile_truth"][:, 0]) == bits(x.amin(dim=(1, 2)).cpu().numpy())
            assert bits(got["quantile_truth"][:, -1]) == bits(x.amax(dim=(1, 2)).cpu().numpy())
            assert bits(got["quantile_recon"][:, 0]) == bits(xh.amin(dim=(1, 2)).cpu().numpy())
        else:
            rows = metrics.quantile_weights(lat, shape[1]) > 0
            assert bits(got["quantile_abs_error"][:, -1]) == bits(np.abs(xh_np - x_np)[:, rows].max(axis=(1, 2)))
            assert bits(got["quantile_truth"][:, 0]) == bits(x_np[:, rows].min(axis=(1, 2)))
            assert bits(got["quantile_truth"][:, -1]) == bits(x_np[:, rows].max(axis=(1, 2)))
    # a frame without zero-weight rows: max_abs under any weights
    got = metrics.frame_quantiles(xh, x, [1.0], lat_weights=np.linspace(0.5, 1.5, shape[1]))
    assert bits(got["quantile_abs_error"][:, 0]) == bits(metrics.reconstruction_error(xh, x)["max_abs"])


@pytest.mark.parametrize("shape", [(3, 40, 1440), (2, 9, 45)], ids=lambda s: "x".join(map(str, s)))
def test_unaligned_views_give_the_same_bits(shape, dev):
    C, H, W = shape
    xh_np, x_np = smooth(shape, seed=11)
    n = C * H * W
    bh, bx = torch.empty(n + 1, device=dev), torch.empty(n + 1, device=dev)
    bh[1:].copy_(torch.from_numpy(xh_np).reshape(-1))
    bx[1:].copy_(torch.from_numpy(x_np).reshape(-1))
    vh, vx = bh[1:].view(C, H, W), bx[1:].view(C, H, W)
    assert vh.data_ptr() % 16 == 4 and vx.data_ptr() % 16 == 4
    got = metrics.frame_quantiles(vh, vx, Q8)
    assert_same_bits(got, ref_quantiles(xh_np, x_np, Q8, metrics.quantile_weights("era5", H))[0], f"unaligned {shape}")
    assert same_bytes(got, metrics.frame_quantiles(*to_dev((xh_np, x_np), dev), Q8))


def test_nonfinite_channels(dev):
    shape = (3, 40, 1440)
    xh_np, x_np = smooth(shape, seed=5)
    xh, x = to_dev((xh_np, x_np), dev)
    clean = metrics.frame_quantiles(xh, x, Q8)
    x[0, 17, 33] = float("nan")
    xh[2, 39, 1439] = float("inf")
    got = metrics.frame_quantiles(xh, x, Q8)
    assert got["nonfinite"].tolist() == [1, 0, 1]
    assert np.array_equal(got["nonfinite"], metrics.reconstruction_error(xh, x)["nonfinite"])
    for k in KEYS[:3] + ("quantile_shift",):
        assert np.isnan(got[k][[0, 2]]).all(), k
        assert got[k][1].tobytes() == clean[k][1].tobytes(), k
    assert_same_bits(got, ref_quantiles(xh.cpu().numpy(), x.cpu().numpy(), Q8, metrics.quantile_weights("era5", 40))[0],
                     "nonfinite")
    # a non-finite point in a row of weight 0 is still a non-finite point of the channel
    xh, x = to_dev((xh_np, x_np), dev)
    x[1, 0, 5] = float("-inf")
    got = metrics.frame_quantiles(xh, x, Q8)
    assert got["nonfinite"].tolist() == [0, 1, 0] and np.isnan(got["quantile_truth"][1]).all()
    assert got["quantile_truth"][[0, 2]].tobytes() == clean["quantile_truth"][[0, 2]].tobytes()


def test_deterministic_across_calls_and_streams(dev):
    pairs = [to_dev(smooth((3, 40, 1440), seed=s), dev) for s in (1, 2)]
    torch.cuda.synchronize()
    one = [metrics.frame_quantiles(*p, Q8) for p in pairs]
    again = [metrics.frame_quantiles(*p, Q8) for p in pairs]
    assert all(same_bytes(a, b) for a, b in zip(one, again))
    res, errs = [None, None], []

    def run(i):
        try:
            with torch.cuda.stream(torch.cuda.Stream(device=dev)):
                for _ in range(3):
                    res[i] = metrics.frame_quantiles(*pairs[i], Q8)
        except Exception as e:       # noqa: BLE001 - reported below, on the test's thread
            errs.append(e)
    threads = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs
    assert all(same_bytes(a, b) for a, b in zip(one, res))


def test_a_column_does_not_depend_on_the_other_probabilities(dev):
    xh_np, x_np = smooth((3, 40, 1440), seed=8)
    xh, x = to_dev((xh_np, x_np), dev)
    alone = metrics.frame_quantiles(xh, x, [0.99])
    many = metrics.frame_quantiles(xh, x, Q16)
    j = Q16.index(0.99)
    for k in KEYS[:3]:
        assert alone[k][:, 0].tobytes() == many[k][:, j].tobytes(), k


def test_ops_argument_checks(dev):
    x = torch.zeros((1, 2, 8), device=dev)
    t = torch.ones(2, device=dev, dtype=torch.int64)
    with pytest.raises(TypeError):
        ops.frame_quantiles(x, x, None, t.int())                                     # int32 targets
    with pytest.raises(TypeError):
        ops.frame_quantiles(x, x, torch.ones(2, device=dev), t)                      # fp32 weights
    with pytest.raises(ValueError):
        ops.frame_quantiles(x, x, torch.ones(3, device=dev, dtype=torch.int32), t)   # [H] is 2
    with pytest.raises(ValueError, match="16"):
        ops.frame_quantiles(x, x, None, torch.ones(17, device=dev, dtype=torch.int64))
    with pytest.raises(TypeError):
        ops.frame_quantiles(x, x, None, t, out=torch.empty(3 * 2 + 1, device=dev))   # fp32 out
    q, nf = ops.frame_quantiles(x, x, None, t)
    assert tuple(q.shape) == (3, 1, 2) and tuple(nf.shape) == (1,) and not q.cpu().numpy().any()


# ---- cra5_api.evaluate_batch(quantiles=...) -------------------------------------------------------------------------------


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


QKEYS = ("quantile", "quantile_truth", "quantile_recon", "quantile_abs_error", "quantile_shift")


def test_evaluate_batch_quantiles(thin, dev, tmp_path):
    api = thin_api(thin, dev, tmp_path)
    frames = [(synth.synth_frame(8, seed=s) * api.std.cpu() + api.mean.cpu()).numpy() for s in (3, 4)]
    stamps = [f"2024-06-01T{h:02d}:00:00" for h in range(2)]
    C, H, W = frames[0].shape
    q = (0.001, 0.5, 0.999, 1.0)
    api.phase_log = []
    reps = api.evaluate_batch(stamps, data=frames, save_root=str(tmp_path / "EV"), workers=2, quantiles=q)
    log, api.phase_log = api.phase_log, None
    assert not [p for p in log if p[1].startswith("d2h")]       # no reconstruction crossed to the host
    assert len([p for p in log if p[1] == "quantiles"]) == 2
    paths = [str(tmp_path / "EV" / "2024" / f"{ts}.bin") for ts in stamps]
    for rep, frame, path in zip(reps, frames, paths):
        x_hat = api.decode_from_bin(custom_path=path, return_format="de_normalized", to_host=False)["x_hat"]
        x = torch.from_numpy(np.ascontiguousarray(frame, dtype=np.float32)).to(dev)
        want = metrics.frame_quantiles(x_hat.reshape(C, H, W).contiguous(), x, q)
        assert rep["quantile_truth"].shape == (C, len(q)) and rep["quantile"].tolist() == list(q)
        for k in QKEYS:
            assert rep[k].tobytes() == want[k].tobytes(), k
        assert bits(rep["quantile_abs_error"][:, -1]) != bits(np.zeros(C))

    # without quantiles=: today's reports - the same keys, and the same values as the statistics of the call above
    api.phase_log = []
    plain = api.evaluate_batch(stamps, data=frames, workers=2)
    log, api.phase_log = api.phase_log, None
    assert not [p for p in log if p[1] == "quantiles"]
    want_keys = {"time_stamp", "variables", "mse", "rmse", "wrmse", "bias", "mae", "max_abs", "nonfinite", "rmse_norm",
                 "bin_bytes", "compression_ratio"}
    for r, p in zip(reps, plain):
        assert set(p) == want_keys and set(r) == want_keys | set(QKEYS)
        for k in want_keys:
            assert np.array_equal(r[k], p[k]) if isinstance(p[k], np.ndarray) else r[k] == p[k], k

    # the dataset mode on the files just written: the same quantiles, bit for bit
    ds = api.evaluate_batch(stamps, data=frames, bins=paths, workers=1, quantiles=q)
    for r, d in zip(reps, ds):
        assert set(d) == set(r) and all(r[k].tobytes() == d[k].tobytes() for k in QKEYS)

    # coarsen=6: the quantiles of the coarse pair under the integer weights of latitude_weights(121)
    coarse = api.evaluate_batch(stamps, data=frames, workers=2, coarsen=6, quantiles=q)
    for rep, frame, path in zip(coarse, frames, paths):
        xh_c = api.decode_from_bin(custom_path=path, return_format="de_normalized", to_host=False, coarsen=6)["x_hat"]
        Ho, Wo = xh_c.shape[-2:]
        x_c = api.net.coarsen_frame(torch.from_numpy(frame).to(dev).contiguous(), 6)
        want = metrics.frame_quantiles(xh_c.reshape(C, Ho, Wo).contiguous(), x_c.reshape(C, Ho, Wo).contiguous(), q)
        assert (Ho, Wo) == (121, 240) and rep["quantile_recon"].shape == (C, len(q))
        for k in QKEYS:
            assert rep[k].tobytes() == want[k].tobytes(), k


@pytest.mark.parametrize("bad", [(), (0.5, 1.5), 0.5, (float("nan"),), (0.5,) * 17],
                         ids=["empty", "above-1", "bare-float", "nan", "17"])
def test_evaluate_batch_refuses_bad_quantiles_before_any_frame(thin, dev, tmp_path, monkeypatch, bad):
    api = thin_api(thin, dev, tmp_path)
    frame = (synth.synth_frame(8, seed=3) * api.std.cpu() + api.mean.cpu()).numpy()

    def reached(*a, **k):
        raise AssertionError("a frame was staged")
    monkeypatch.setattr(api, "_stage_in", reached)
    api.phase_log = []
    with pytest.raises(ValueError, match="16"):
        api.evaluate_batch(["2024-06-01T00:00:00"], data=[frame], workers=1, quantiles=bad)
    assert api.phase_log == []
    api.phase_log = None
