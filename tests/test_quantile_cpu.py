"""Quantiles without a GPU: the host side of cra5_amd.metrics.frame_quantiles (weights, targets, validation), the C ABI's
argument checks, and the numpy reference of tests/quantile_helpers.py checked against hand values and np.quantile."""
import numpy as np
import pytest
import torch

from cra5_amd import _lib, metrics, ops
from quantile_helpers import ref_field_quantiles, ref_quantiles, targets


def test_targets_hand_values():
    ones = np.ones(10, dtype=np.int64)
    t = metrics.quantile_targets([0, 0.1, 0.5, 0.999, 1], ones, 1)
    assert t.dtype == np.int64 and t.tolist() == [1, 1, 5, 10, 10]
    assert targets([0, 0.1, 0.5, 0.999, 1], ones, 1).tolist() == [1, 1, 5, 10, 10]
    # any order, duplicates; the width multiplies the total
    assert metrics.quantile_targets((1.0, 0.5, 0.5, 0.0), ones, 3).tolist() == [30, 15, 15, 1]
    # weighted: Wtot = 4 * (3 + 0 + 5) = 32
    assert metrics.quantile_targets([0.25, 0.26], np.array([3, 0, 5]), 4).tolist() == [8, 9]
    w = metrics.quantile_weights("era5", 721)
    q = (0.0, 1e-4, 0.01, 0.5, 0.99, 0.9999, 1.0)
    assert np.array_equal(metrics.quantile_targets(q, w, 1440), targets(q, w, 1440))
    assert 1440 * int(w.sum()) < 1 << 53


def test_reference_is_numpy_inverted_cdf_for_unit_weights():
    rng = np.random.default_rng(0)
    p = [0, 0.1, 0.5, 0.999, 1]
    for n in (10, 97, 1000):
        v = rng.standard_normal(n).astype(np.float32)
        v[: n // 5] = v[0]                                # ties
        got = ref_field_quantiles(v.reshape(1, n), np.ones(1, dtype=np.int64), targets(p, np.ones(1), n))
        want = np.quantile(v, p, method="inverted_cdf")
        assert got.dtype == np.float32 and got.tobytes() == want.astype(np.float32).tobytes()
        assert np.array_equal(got, np.sort(v)[targets(p, np.ones(1), n) - 1])


def test_quantile_weights():
    w = metrics.quantile_weights("era5", 721)
    assert w.dtype == np.int64 and w.shape == (721,)
    assert (w == 0).sum() == 2 and w[0] == 0 and w[-1] == 0           # the poles do not count
    assert w.max() == 103087 and np.array_equal(w, w[::-1])
    assert np.array_equal(w, np.rint(metrics.latitude_weights(721) * 65536.0).astype(np.int64))
    ones = metrics.quantile_weights(None, 5)
    assert ones.dtype == np.int64 and ones.tolist() == [1] * 5
    assert metrics.quantile_weights(np.array([0.0, 1.0, 16.0]), 3).tolist() == [0, 65536, 1 << 20]
    assert metrics.quantile_weights(torch.tensor([0.5, 0.25]), 2).tolist() == [32768, 16384]
    with pytest.raises(ValueError, match="2\\^20"):
        metrics.quantile_weights(np.array([1.0, 16.001]), 2)           # above 2^20 / 2^16
    with pytest.raises(ValueError, match="weight 0"):
        metrics.quantile_weights(np.zeros(4), 4)
    with pytest.raises(ValueError, match="weight 0"):
        metrics.quantile_weights(np.full(4, 1e-6), 4)                  # rounds to all zero
    with pytest.raises(ValueError):
        metrics.quantile_weights(np.ones(3), 4)
    with pytest.raises(ValueError):
        metrics.quantile_weights(np.array([1.0, -1.0]), 2)
    with pytest.raises(ValueError):
        metrics.quantile_weights("cos", 4)


@pytest.mark.parametrize("bad", [[], [0.5] * 17, [0.5, float("nan")], [-0.1], [1.5], 0.5, [float("inf")], "0.5"],
                         ids=["empty", "17", "nan", "negative", "above-1", "bare-float", "inf", "string"])
def test_q_validation_names_the_limit(bad):
    with pytest.raises(ValueError, match="16"):
        metrics.quantile_targets(bad, np.ones(10, dtype=np.int64), 4)
    assert ops.QUANTILE_MAX_Q == 16 and ops.QUANTILE_FIELDS == ("truth", "recon", "abs_error")


def test_abi_validates_arguments_without_a_gpu():
    L = _lib.lib()
    f = L.cra5_frame_quantiles_f32
    nb = L.cra5_frame_quantiles_ws_bytes(268, 721, 1440, 16)
    assert nb > 0 and nb % 8 == 0
    assert L.cra5_frame_quantiles_ws_bytes(268, 721, 1440, 1) < nb
    ok = 4096                                                    # stands for a device address: never dereferenced here
    assert f(None, None, 1, 1, 1, None, None, 1, None, 0, None, None) == -7
    assert f(None, ok, 268, 721, 1440, None, ok, 8, ok, nb, ok, None) == -7
    assert f(ok, ok, 268, 721, 1440, None, None, 8, ok, nb, ok, None) == -7
    assert f(ok, ok, 268, 721, 1440, None, ok, 8, None, nb, ok, None) == -7
    assert f(ok, ok, 268, 721, 1440, None, ok, 8, ok, nb, None, None) == -7
    assert f(ok, ok, 268, 721, 1440, None, ok, 0, ok, nb, ok, None) == -7        # Q = 0
    assert f(ok, ok, 268, 721, 1440, None, ok, 17, ok, nb, ok, None) == -7       # Q = 17
    assert f(ok, ok, 268, 721, 1440, None, ok, 16, ok, nb - 8, ok, None) == -7   # short workspace
    assert f(ok, ok, 268, 721, 1440, None, ok, 16, ok + 4, nb, ok, None) == -7   # misaligned workspace
    for C, H, W in [(0, 721, 1440), (268, 0, 1440), (268, 721, 0), (1, 1 << 16, 1 << 16)]:
        assert L.cra5_frame_quantiles_ws_bytes(C, H, W, 1) == 0, (C, H, W)
        assert f(ok, ok, C, H, W, None, ok, 1, ok, nb, ok, None) == -7, (C, H, W)
    assert L.cra5_frame_quantiles_ws_bytes(1, 1 << 16, 1 << 16, 1) == 0
    assert L.cra5_frame_quantiles_ws_bytes(2, 5, 7, 0) == 0 and L.cra5_frame_quantiles_ws_bytes(2, 5, 7, 17) == 0
    assert L.cra5_abi_version() == 1


def test_frame_quantiles_refuses_host_tensors_and_mismatched_shapes():
    x = torch.zeros((2, 3, 8))
    with pytest.raises(TypeError):
        metrics.frame_quantiles(x, x, [0.5])                     # host tensors: the GPU is the only path
    with pytest.raises(TypeError):
        metrics.frame_quantiles(x.numpy(), x.numpy(), [0.5])
    with pytest.raises(TypeError):
        ops.frame_quantiles(x, x, None, torch.ones(1, dtype=torch.int64))
    with pytest.raises(ValueError):
        metrics.frame_quantiles(x, torch.zeros((2, 3, 9)), [0.5])


def test_reference_hand_values_with_ties_and_a_zero_weight_row():
    # rows:   w = 2            w = 0 (left out)      w = 1
    f = np.array([[3.0, 1.0, 1.0, -0.0], [-9.0, 9.0, 9.0, 9.0], [1.0, 2.0, 0.0, 3.0]], dtype=np.float32)
    w = np.array([2, 0, 1])
    # sorted values and weights: 0 (2), 0 (1), 1 (2), 1 (2), 1 (1), 2 (1), 3 (2), 3 (1)  -> cumulative 2 3 5 7 8 9 11 12
    assert 4 * int(w.sum()) == 12
    for T, want in [(1, 0.0), (3, 0.0), (4, 1.0), (8, 1.0), (9, 2.0), (10, 3.0), (12, 3.0)]:
        got = ref_field_quantiles(f, w, [T])
        assert got.tolist() == [want], (T, got)
    assert not np.signbit(ref_field_quantiles(f, w, [1]))[0]             # zeros are canonical
    # through the probabilities: T(0) = 1, T(0.5) = 6, T(0.75) = 9, T(1) = 12
    out, nf = ref_quantiles(f[None] + 1, f[None], [0, 0.5, 0.75, 1], w)
    assert nf.tolist() == [0]
    assert out["truth"].tolist() == [[0.0, 1.0, 2.0, 3.0]] and out["recon"].tolist() == [[1.0, 2.0, 3.0, 4.0]]
    assert out["abs_error"].tolist() == [[1.0] * 4]
    bad = f[None].copy()
    bad[0, 1, 0] = np.inf                                               # a zero-weight row still counts as non-finite
    out, nf = ref_quantiles(bad, f[None], [0.5], w)
    assert nf.tolist() == [1] and np.isnan(out["truth"]).all() and np.isnan(out["abs_error"]).all()


def test_weighted_reference_equals_unit_reference_on_repeated_rows():
    rng = np.random.default_rng(3)
    H, W = 7, 5
    f = rng.integers(-4, 5, size=(H, W)).astype(np.float32)             # many ties
    w = np.array([2, 0, 3, 1, 0, 4, 1])
    rep = np.repeat(f, w, axis=0)                                       # each row w_h times
    assert rep.shape == (int(w.sum()), W)
    T = np.arange(1, W * int(w.sum()) + 1)
    a = ref_field_quantiles(f, w, T)
    b = ref_field_quantiles(rep, np.ones(rep.shape[0], dtype=np.int64), T)
    assert a.tobytes() == b.tobytes()
    assert np.array_equal(b, np.sort(rep.reshape(-1)))
