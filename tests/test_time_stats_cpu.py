"""Per-grid-point time statistics without a GPU: the C ABI's argument validation (CRA5_ERR_ARG before any device work), the
refusals of ops.time_accumulate / TimeStats / cra5_api.aggregate_batch, and the numpy reference of the GPU tests against
numpy's own mean / std / min / max."""
import ctypes

import numpy as np
import pytest
import torch

from cra5_amd import _lib, ops, synth
from cra5_amd.vaeformer import VAEformer
from time_stats_helpers import RefTimeStats, ref_time_stats, within_one_ulp

ERR_ARG = -7


def test_time_launchers_validate_arguments_without_gpu():
    L = _lib.lib()
    acc, fin = L.cra5_time_accumulate_f32, L.cra5_time_finish_f32
    a = ctypes.c_void_p(1 << 20)      # never dereferenced: every call below is refused before a launch
    assert acc(None, 0, 1, None, None, None, None, None) == ERR_ARG
    assert acc(a, 0, 1, a, a, a, a, None) == ERR_ARG                  # n == 0
    assert acc(a, 16, 1, None, None, None, None, None) == ERR_ARG     # no accumulator
    assert acc(a, 16, 0, None, None, None, None, None) == ERR_ARG
    assert acc(None, 16, 1, a, a, a, a, None) == ERR_ARG              # no frame
    assert fin(0, 5, 0, a, a, a, a, None) == ERR_ARG                  # n == 0
    assert fin(16, 5, 0, None, None, a, a, None) == ERR_ARG           # no accumulator
    assert fin(16, 5, 0, None, a, a, None, None) == ERR_ARG           # mean without sum
    assert fin(16, 5, 0, a, a, None, None, None) == ERR_ARG           # no output
    assert fin(16, 5, 0, a, None, a, a, None) == ERR_ARG              # std without sumsq
    assert fin(16, 5, 0, a, None, None, a, None) == ERR_ARG
    assert fin(16, 1, 1, a, a, a, a, None) == ERR_ARG                 # count - ddof < 1
    assert fin(16, 5, 5, a, a, None, a, None) == ERR_ARG
    assert fin(16, 0, 0, a, a, a, None, None) == ERR_ARG
    assert fin(16, 5, -1, a, a, a, a, None) == ERR_ARG


def test_ops_and_time_stats_refuse_host_tensors_dtypes_and_shapes():
    from cra5_amd.timestats import TimeStats
    x = torch.zeros((2, 3, 8))
    acc = dict(sum=torch.zeros((2, 3, 8), dtype=torch.float64))
    with pytest.raises(TypeError):
        ops.time_accumulate(x, acc, True)                     # host tensors: the GPU is the only path
    with pytest.raises(TypeError):
        ops.time_accumulate(x.double(), acc, True)
    with pytest.raises(TypeError):
        ops.time_accumulate(x.numpy(), acc, True)
    with pytest.raises(TypeError):
        ops.time_finish(acc, 3, 0, ("mean",))
    with pytest.raises(ValueError):
        ops.time_finish(acc, 3, 0, ("std",))                  # std without sumsq
    with pytest.raises(ValueError):
        ops.time_finish(acc, 1, 1, ("mean",))                 # count - ddof < 1
    with pytest.raises(ValueError):
        ops.time_finish(acc, 3, 0, ("median",))
    ts = TimeStats((2, 3, 8), stats=("mean", "max"), device="cpu")
    assert sorted(ts.acc) == ["max", "sum"]
    with pytest.raises(TypeError):
        ts.add(x)
    with pytest.raises(TypeError):
        ts.add(x.double())
    with pytest.raises(TypeError):
        ts.add(x.numpy())
    with pytest.raises(ValueError, match=r"\(2, 3, 9\)"):
        ts.add(torch.zeros((2, 3, 9)))
    with pytest.raises(ValueError, match=r"\(1, 2, 3, 8\)"):
        ts.add(x.unsqueeze(0))
    with pytest.raises(ValueError, match="no frame"):
        ts.result()
    for bad in ((), ("mean", "median"), "mean"):
        with pytest.raises(ValueError):
            TimeStats((2, 3), stats=bad, device="cpu")
    for bad in (-1, 1.0, True, None):
        with pytest.raises(ValueError):
            TimeStats((2, 3), device="cpu", ddof=bad)
    with pytest.raises(ValueError):
        TimeStats((2, 0), device="cpu")


def test_time_stats_skip_and_abort_without_gpu():
    """The turn protocol is host logic: a skipped turn is passed over, an aborted object raises the first error given, and
    an add with a seq that is refused aborts the object (nobody may be left waiting for that turn)."""
    from cra5_amd.timestats import TimeStats
    ts = TimeStats((4,), stats=("min",), device="cpu")
    ts.skip(1)
    assert ts._next == 0
    ts.skip(0)
    assert ts._next == 2
    with pytest.raises(ValueError):
        ts.skip(1)
    ts.abort(FileNotFoundError("frame 2"))
    ts.abort(RuntimeError("later"))
    with pytest.raises(FileNotFoundError):
        ts.result()
    ts = TimeStats((4,), stats=("min",), device="cpu")
    with pytest.raises(TypeError):
        ts.add(torch.zeros(4), seq=3)           # a host frame
    with pytest.raises(TypeError):
        ts.result()


@pytest.fixture(scope="module")
def cpu_api(tmp_path_factory):
    from cra5_amd.api import cra5_api
    return cra5_api(local_root=str(tmp_path_factory.mktemp("agg")), device="cpu",
                    weights=VAEformer(0, **synth.thin_model_kwargs()))


@pytest.mark.parametrize("kw", [
    dict(stats=("mean", "median")),
    dict(stats=()),
    dict(stats="mean"),
    dict(groups=[0, 0, 1]),
    dict(groups=[0, 0, 1, 1, 1]),
    dict(ddof=-1),
    dict(ddof=1.5),
    dict(ddof=True),
    dict(return_format="latent"),
    dict(return_format="physical"),
    dict(stats=("std",), ddof=1, groups=[0, 0, 1, 0]),     # group 1 holds one frame
    dict(stats=("mean", "std"), ddof=4),                   # four frames, no group
    dict(stride=7),
    dict(variables=["no_such_variable"]),
])
def test_aggregate_batch_refuses_bad_arguments_before_requiring_a_gpu(cpu_api, kw):
    paths = [f"/nonexistent/{i}.bin" for i in range(4)]
    with pytest.raises(ValueError):
        cpu_api.aggregate_batch(paths=paths, **kw)


def test_aggregate_batch_needs_frames_and_then_a_gpu(cpu_api):
    with pytest.raises(ValueError):
        cpu_api.aggregate_batch()
    with pytest.raises(ValueError):
        cpu_api.aggregate_batch(paths=[])
    # good arguments: the next thing it needs is the GPU (no CPU fallback), not the files
    with pytest.raises(RuntimeError, match="MI355X"):
        cpu_api.aggregate_batch(paths=["/nonexistent/0.bin", "/nonexistent/1.bin"], stats=("std",), ddof=1,
                                groups=["a", "a"], variables=["z_1000"], region=(35, 72, -25, 45), stride=6)


def test_reference_of_the_gpu_tests_against_numpy():
    rng = np.random.default_rng(3)
    stack = (5e4 + 1e4 * rng.standard_normal((7, 3, 5, 11))).astype(np.float32)
    r = ref_time_stats(stack, ddof=0)
    assert r["n"] == 7
    s64 = stack.astype(np.float64)
    for k in ("mean", "std", "min", "max"):
        assert r[k].dtype == np.float32 and r[k].shape == stack.shape[1:]
    assert np.array_equal(r["min"], stack.min(axis=0)) and np.array_equal(r["max"], stack.max(axis=0))
    # (np.mean sums pairwise, the reference in order: equal to the last float32 bit at most)
    assert within_one_ulp(r["mean"], s64.mean(axis=0).astype(np.float32))
    for ddof in (0, 1):
        assert within_one_ulp(ref_time_stats(stack, ddof)["std"], s64.std(axis=0, ddof=ddof).astype(np.float32))
    # the sums themselves: an exact-arithmetic check on small integers, where every order gives the same float64
    ints = rng.integers(-1000, 1001, size=(6, 4, 9)).astype(np.float32)
    acc = RefTimeStats()
    for x in ints:
        acc.add(x)
    assert np.array_equal(acc.s, ints.astype(np.int64).sum(axis=0).astype(np.float64))
    assert np.array_equal(acc.q, (ints.astype(np.int64) ** 2).sum(axis=0).astype(np.float64))
    assert np.array_equal(acc.mean(), (ints.astype(np.float64).sum(axis=0) / 6).astype(np.float32))
    # a constant series has zero spread exactly; NaN and inf propagate as numpy's own reductions do
    assert np.array_equal(ref_time_stats(np.full((5, 2, 3), 3.0, dtype=np.float32))["std"], np.zeros((2, 3), np.float32))
    bad = stack.copy()
    bad[2, 0, 0, 0] = np.nan
    bad[3, 0, 0, 1] = np.inf
    bad[3, 0, 0, 2], bad[4, 0, 0, 2] = np.inf, -np.inf
    rb = ref_time_stats(bad)
    with np.errstate(invalid="ignore"):
        b64 = bad.astype(np.float64)
        assert within_one_ulp(rb["mean"], b64.mean(axis=0).astype(np.float32))
        assert np.array_equal(rb["min"], bad.min(axis=0), equal_nan=True)
        assert np.array_equal(rb["max"], bad.max(axis=0), equal_nan=True)
    assert np.isnan(rb["mean"][0, 0, 0]) and np.isnan(rb["std"][0, 0, 0]) and np.isnan(rb["min"][0, 0, 0])
    assert rb["max"][0, 0, 1] == np.inf and rb["mean"][0, 0, 1] == np.inf and np.isnan(rb["std"][0, 0, 1])
    assert np.isnan(rb["mean"][0, 0, 2]) and rb["min"][0, 0, 2] == -np.inf and rb["max"][0, 0, 2] == np.inf
    assert np.array_equal(rb["mean"][1:], r["mean"][1:]) and np.array_equal(rb["std"][1:], r["std"][1:])
