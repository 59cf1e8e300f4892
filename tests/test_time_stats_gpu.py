"""Per-grid-point time statistics on the GPU (csrc/timestats.hip, cra5_amd.timestats.TimeStats, cra5_api.aggregate_batch)
against the sequential float64 numpy reference of time_stats_helpers: sums, mean, min and max bit for bit, std to one
fp32 ulp (the device's double sqrt need not be correctly rounded; everything else is)."""
import itertools
import threading

import numpy as np
import pytest
import torch

from cra5_amd import ops, synth
from cra5_amd.pipeline import FramePipeline
from cra5_amd.timestats import STATS, TimeStats
from cra5_amd.vaeformer import VAEformer
from cra5_amd.zoo import vaeformer_pretrained
from time_stats_helpers import RefTimeStats, ref_time_stats, within_one_ulp

pytestmark = pytest.mark.gpu

ACC = {"sum": torch.float64, "sumsq": torch.float64, "min": torch.float32, "max": torch.float32}


def physical_frames(T, shape, seed, dev):
    """T frames at physical scales (offset ~5e4, std ~1e4 per leading index): |mean| / std of a point is ~10."""
    g = torch.Generator(device=dev).manual_seed(seed)
    lead = (shape[0],) + (1,) * (len(shape) - 1)
    u = torch.rand((2,) + lead, generator=g, device=dev)
    return [(5e4 * (1 + 0.2 * u[0]) + 1e4 * (0.5 + u[1]) * torch.randn(shape, generator=g, device=dev)).contiguous()
            for _ in range(T)]


def fresh_acc(shape, dev, keys=tuple(ACC)):
    return {k: torch.empty(shape, device=dev, dtype=ACC[k]) for k in keys}


def run_ops(frames, acc):
    for t, x in enumerate(frames):
        ops.time_accumulate(x, acc, first=t == 0)
    return acc


def assert_stats_equal(got, ref, exact_std=False):
    """got: dict of device tensors / host arrays, ref: dict of host arrays - mean / min / max bit for bit, std to one ulp."""
    for k in STATS:
        if k not in ref or k not in got:
            continue
        g = got[k].cpu().numpy() if isinstance(got[k], torch.Tensor) else got[k]
        assert g.dtype == np.float32 and g.shape == ref[k].shape, k
        if k == "std" and not exact_std:
            assert within_one_ulp(g, ref[k]), k
        else:
            assert np.array_equal(g, ref[k], equal_nan=True), k


SHAPES = [(1, 1, 1), (1, 1, 3), (2, 37, 43), (3, 37, 44), (1, 5, 1439)]


@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_bit_for_bit(shape, dev):
    frames = physical_frames(5, shape, seed=sum(shape), dev=dev)
    host = [x.cpu().numpy() for x in frames]
    acc, ref = fresh_acc(shape, dev), RefTimeStats()
    for t, x in enumerate(frames):
        ops.time_accumulate(x, acc, first=t == 0)
        ref.add(host[t])
        for k, r in (("sum", ref.s), ("sumsq", ref.q), ("min", ref.mn), ("max", ref.mx)):
            assert np.array_equal(acc[k].cpu().numpy(), r), (k, t)
    stack = np.stack(host).astype(np.float64)
    for ddof in (0, 1):
        fin = ops.time_finish(acc, 5, ddof, ("mean", "std"))
        assert np.array_equal(fin["mean"].cpu().numpy(), ref.mean())
        std = fin["std"].cpu().numpy()
        assert within_one_ulp(std, ref.std(ddof))
        # the two-pass definition: the one-pass formula's relative error here is ~T * 2**-53 * mean**2 / var <~ 1e-11
        assert within_one_ulp(std, np.std(stack, axis=0, ddof=ddof).astype(np.float32))
    only = ops.time_finish(acc, 5, 0, ("std",))
    assert set(only) == {"std"} and torch.equal(only["std"], ops.time_finish(acc, 5, 0)["std"])


def test_constant_series_has_zero_std(dev):
    x = torch.full((3, 7, 9), 3.0, device=dev)
    for ddof in (0, 1):
        ts = TimeStats((3, 7, 9), device=dev, ddof=ddof)
        for _ in range(5):
            ts.add(x)
        r = ts.result()
        assert torch.equal(r["std"], torch.zeros((3, 7, 9), device=dev))
        assert r["n"] == 5 and all(torch.equal(r[k], x) for k in ("mean", "min", "max"))
    one = TimeStats((3, 7, 9), stats=("std", "mean"), device=dev, ddof=1)
    one.add(x)
    with pytest.raises(ValueError, match="ddof"):
        one.result()                                # n - ddof < 1


def test_stat_selection(dev):
    shape = (2, 37, 43)
    frames = physical_frames(5, shape, seed=9, dev=dev)
    full = TimeStats(shape, device=dev)
    for x in frames:
        full.add(x)
    want = full.result()
    assert list(want) == ["n", "mean", "std", "min", "max"] and sorted(full.acc) == ["max", "min", "sum", "sumsq"]
    needs = {"mean": {"sum"}, "std": {"sum", "sumsq"}, "min": {"min"}, "max": {"max"}}
    for sel in [(s,) for s in STATS] + list(itertools.combinations(STATS, 2)):
        ts = TimeStats(shape, stats=sel[::-1], device=dev)
        assert set(ts.acc) == set().union(*(needs[s] for s in sel)), sel       # nothing else is allocated
        for x in frames:
            ts.add(x)
        got = ts.result()
        assert list(got) == ["n"] + [s for s in STATS if s in sel] and got["n"] == 5
        for s in sel:
            assert torch.equal(got[s], want[s]), (sel, s)


def test_first_needs_no_memset(dev):
    shape = (3, 37, 44)
    frames = physical_frames(5, shape, seed=4, dev=dev)
    clean = run_ops(frames, fresh_acc(shape, dev))
    for fill in (float("nan"), -1e30, float("inf")):
        dirty = fresh_acc(shape, dev)
        for t in dirty.values():
            t.fill_(fill)
        run_ops(frames, dirty)
        assert all(torch.equal(dirty[k], clean[k]) for k in ACC), fill


@pytest.mark.parametrize("off", [1, 3])
def test_unaligned_views(off, dev):
    """x and every accumulator start `off` elements past a 16-byte boundary: the element-wise path, same values."""
    shape = (2, 37, 44)
    n = 2 * 37 * 44
    frames = physical_frames(5, shape, seed=11, dev=dev)
    clean = run_ops(frames, fresh_acc(shape, dev))
    acc = {k: torch.empty(n + off, device=dev, dtype=dt)[off:].view(shape) for k, dt in ACC.items()}
    for t, x in enumerate(frames):
        v = torch.empty(n + off, device=dev)[off:].view(shape)
        v.copy_(x)
        assert v.data_ptr() % 16 and all(a.data_ptr() % 16 for a in acc.values())
        ops.time_accumulate(v, acc, first=t == 0)
    assert all(torch.equal(acc[k], clean[k]) for k in ACC)
    # one unaligned base among aligned ones is enough to leave the vector path
    for lone in ACC:
        mixed = fresh_acc(shape, dev)
        mixed[lone] = torch.empty(n + off, device=dev, dtype=ACC[lone])[off:].view(shape)
        assert mixed[lone].data_ptr() % 16
        run_ops(frames, mixed)
        assert all(torch.equal(mixed[k], clean[k]) for k in ACC), lone
    fin_c, fin_u = ops.time_finish(clean, 5, 1), ops.time_finish(acc, 5, 1)
    assert torch.equal(fin_c["mean"], fin_u["mean"]) and torch.equal(fin_c["std"], fin_u["std"])


def test_nonfinite_samples(dev):
    shape = (2, 37, 43)
    frames = physical_frames(5, shape, seed=21, dev=dev)
    base = TimeStats(shape, device=dev)
    for x in frames:
        base.add(x)
    want = {k: v.cpu().numpy() for k, v in base.result().items() if k != "n"}
    bad = [x.clone() for x in frames]
    bad[2][0, 0, 0] = float("nan")
    bad[3][1, 36, 42] = float("inf")
    bad[3][0, 5, 7], bad[4][0, 5, 7] = float("inf"), float("-inf")
    ts = TimeStats(shape, device=dev)
    for x in bad:
        ts.add(x)
    got = {k: v.cpu().numpy() for k, v in ts.result().items() if k != "n"}
    ref = ref_time_stats([x.cpu().numpy() for x in bad])
    assert_stats_equal(got, ref)
    assert all(np.isnan(got[k][0, 0, 0]) for k in STATS)
    assert got["max"][1, 36, 42] == np.inf and got["mean"][1, 36, 42] == np.inf and np.isnan(got["std"][1, 36, 42])
    assert got["min"][0, 5, 7] == -np.inf and got["max"][0, 5, 7] == np.inf and np.isnan(got["mean"][0, 5, 7])
    touched = np.zeros(shape, dtype=bool)
    touched[0, 0, 0] = touched[1, 36, 42] = touched[0, 5, 7] = True
    for k in STATS:
        assert np.array_equal(got[k][~touched], want[k][~touched]), k      # every other point: bit-identical


def test_full_size_indices(dev):
    """268 x 721 x 1440: the fp64 accumulators pass 2^31 bytes - 32-bit element or byte offsets would show here."""
    shape = (268, 721, 1440)
    x0, x1 = physical_frames(2, shape, seed=1, dev=dev)
    ts = TimeStats(shape, device=dev)
    ts.add(x0)
    ts.add(x1)
    r = ts.result()
    d0, d1 = x0.double(), x1.double()
    s = d0 + d1
    assert torch.equal(ts.acc["sum"], s)
    assert torch.equal(r["mean"], (s / 2).float())
    del s
    assert torch.equal(ts.acc["sumsq"], d0 * d0 + d1 * d1)
    del d0, d1
    assert torch.equal(r["min"], torch.minimum(x0, x1)) and torch.equal(r["max"], torch.maximum(x0, x1))
    assert r["n"] == 2 and bool(torch.isfinite(r["std"]).all())


def test_order_does_not_depend_on_threads(dev):
    shape = (8, 721, 1440)
    frames = physical_frames(6, shape, seed=2, dev=dev)
    solo = TimeStats(shape, device=dev)
    for x in frames:
        solo.add(x)
    want = solo.result()
    torch.cuda.synchronize()

    def run(workers, order):
        ts = TimeStats(shape, device=dev)
        pipe = FramePipeline(None, workers=workers, device=dev)
        try:
            pipe.map(lambda i: ts.add(frames[i], seq=i), order)
        finally:
            pipe.close()
        got = ts.result()
        assert got["n"] == 6
        for k in STATS:
            assert torch.equal(got[k], want[k]), (workers, order, k)
        for k in ACC:
            assert torch.equal(ts.acc[k], solo.acc[k]), (workers, order, k)

    for w in (1, 3, 6):
        run(w, list(range(6)))
    # later seqs are called first, inside the pool's window (every item of a window has started before one must wait)
    run(3, [2, 1, 0, 5, 4, 3])
    run(6, [5, 4, 3, 2, 1, 0])


# ---- cra5_api.aggregate_batch -------------------------------------------------------------------------------------------


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


@pytest.fixture(scope="module")
def archive(thin, dev, tmp_path_factory):
    """Six .bin files of the thin model, decode_batch's host frames of them (the reference's input, computed once) and
    the full-grid aggregate."""
    root = tmp_path_factory.mktemp("agg")
    api = thin_api(thin, dev, root)
    frames = [(synth.synth_frame(8, seed=s) * api.std.cpu() + api.mean.cpu()).numpy() for s in range(3, 9)]
    stamps = [f"2024-06-{1 + h // 3:02d}T{h % 3:02d}:00:00" for h in range(6)]
    res = api.encode_era5_batch(stamps, data=frames, save_root=str(root / "CRA5"), workers=3)
    paths = [r["save_path"] for r in res]
    decoded = api.decode_batch(paths=paths, workers=3)
    return dict(api=api, paths=paths, stamps=stamps, decoded=decoded, full=api.aggregate_batch(paths=paths, workers=3))


def test_aggregate_batch_matches_numpy_over_decode_batch(archive):
    api, paths, full = archive["api"], archive["paths"], archive["full"]
    ref = ref_time_stats(archive["decoded"])
    assert full["n"] == 6 and isinstance(full["n"], int) and "groups" not in full
    assert_stats_equal(full, ref)
    assert full["variables"] == [api.channels_to_vname[c] for c in range(8)]
    g = api.grid_box((-90, 90, 0, 360))
    assert np.array_equal(full["lat"], g["lat"]) and np.array_equal(full["lon"], g["lon"])
    assert full["mean"].shape == (8, 721, 1440) and len(full["lat"]) == 721 and len(full["lon"]) == 1440
    for w in (1, 4):
        again = api.aggregate_batch(paths=paths, workers=w)
        for k in STATS:
            assert np.array_equal(again[k], full[k]), (w, k)
    # time stamps and the default path layout name the same files
    by_ts = api.aggregate_batch(time_stamps=archive["stamps"], stats=("max",), workers=3)
    assert list(by_ts) == ["variables", "lat", "lon", "n", "max"] and np.array_equal(by_ts["max"], full["max"])
    r1 = api.aggregate_batch(paths=paths, stats=("std", "mean"), ddof=1, workers=3)
    assert_stats_equal(r1, ref_time_stats(archive["decoded"], ddof=1))
    assert "min" not in r1 and np.array_equal(r1["mean"], full["mean"])


def test_aggregate_batch_groups(archive):
    api, paths = archive["api"], archive["paths"]
    labels = [0, 0, 1, 1, 0, 2]
    stats = ("mean", "min", "max")
    got = api.aggregate_batch(paths=paths, groups=labels, stats=stats, workers=3)
    assert got["groups"] == [0, 1, 2]
    assert got["n"].dtype == np.int64 and got["n"].tolist() == [3, 2, 1]
    for g in range(3):
        own = [p for p, lab in zip(paths, labels) if lab == g]
        solo = api.aggregate_batch(paths=own, stats=stats, workers=2)
        assert solo["n"] == len(own)
        for k in stats:
            assert got[k].shape == (3, 8, 721, 1440) and np.array_equal(got[k][g], solo[k]), (g, k)
        assert_stats_equal(solo, ref_time_stats([d for d, lab in zip(archive["decoded"], labels) if lab == g]))
    # labels are any hashable value, reported in order of first appearance
    days = api.aggregate_batch(paths=paths, groups=[ts[:10] for ts in archive["stamps"]][::-1], stats=("std",), workers=3)
    assert days["groups"] == ["2024-06-02", "2024-06-01"] and days["n"].tolist() == [3, 3]
    assert within_one_ulp(days["std"][1], ref_time_stats(archive["decoded"][3:])["std"])
    with pytest.raises(ValueError, match="ddof"):
        api.aggregate_batch(paths=paths, groups=labels, stats=("std",), ddof=1, workers=3)


def test_aggregate_batch_subset_is_the_slice_of_the_full_grid(archive):
    api, paths, full = archive["api"], archive["paths"], archive["full"]
    names = [api.channels_to_vname[5], api.channels_to_vname[2]]
    region, stride = (35, 72, -25, 45), (6, 4)                  # crosses 0 deg
    got = api.aggregate_batch(paths=paths, variables=names, region=region, stride=stride, workers=3)
    g = api.grid_box(region, stride=stride)
    assert got["variables"] == names and np.array_equal(got["lat"], g["lat"]) and np.array_equal(got["lon"], g["lon"])
    assert 0.0 in got["lon"] and got["lon"][0] == 335.0
    for k in STATS:
        want = full[k][[5, 2]][:, g["kept_rows"]][:, :, g["kept_cols"]]
        assert got[k].shape == want.shape == (2, len(g["lat"]), len(g["lon"])) and np.array_equal(got[k], want), k


def test_aggregate_batch_normalized_and_device_results(archive):
    api, paths, full = archive["api"], archive["paths"], archive["full"]
    norm = api.aggregate_batch(paths=paths, return_format="normalized", workers=3)
    assert_stats_equal(norm, ref_time_stats(api.decode_batch(paths=paths, return_format="normalized", workers=3)))
    assert not np.array_equal(norm["mean"], full["mean"])
    on_dev = api.aggregate_batch(paths=paths, to_host=False, workers=3)
    grouped = api.aggregate_batch(paths=paths, to_host=False, groups=[0, 1, 0, 1, 0, 1], stats=("max",), workers=3)
    assert on_dev["n"] == 6 and tuple(grouped["max"].shape) == (2, 8, 721, 1440) and grouped["max"].is_cuda
    for k in STATS:
        assert isinstance(on_dev[k], torch.Tensor) and on_dev[k].is_cuda and on_dev[k].dtype == torch.float32
        assert np.array_equal(on_dev[k].cpu().numpy(), full[k]), k
    assert np.array_equal(grouped["max"].max(dim=0).values.cpu().numpy(), full["max"])


def test_aggregate_batch_phase_log(archive):
    api, paths = archive["api"], archive["paths"]
    api.phase_log = []
    try:
        api.aggregate_batch(paths=paths, workers=3)
    finally:
        log, api.phase_log = api.phase_log, None
    phases = [p[1] for p in log]
    assert phases.count("accumulate") == 6 and phases.count("decompress") == 6
    last_acc = max(i for i, p in enumerate(phases) if p == "accumulate")
    assert not [p for p in phases[:last_acc] if p.startswith("d2h")]     # no reconstruction crossed to the host
    assert phases[last_acc + 1:] == ["d2h"]                             # the statistics, once


def test_a_failing_frame_ends_the_call_without_a_hang(archive):
    """A host-side failure (a missing file) in the middle: the frames behind it must not wait for its turn for ever."""
    api, paths = archive["api"], list(archive["paths"])
    paths[3] = paths[3] + ".missing"
    seen = []

    def call():
        try:
            api.aggregate_batch(paths=paths, workers=3)
        except BaseException as e:        # noqa: BLE001
            seen.append(e)
    t = threading.Thread(target=call, daemon=True)
    t.start()
    t.join(120)
    assert not t.is_alive(), "aggregate_batch hangs after a frame failed"
    assert len(seen) == 1 and isinstance(seen[0], FileNotFoundError)
    # and the API is usable afterwards
    again = api.aggregate_batch(paths=archive["paths"], stats=("min",), workers=3)
    assert np.array_equal(again["min"], archive["full"]["min"])


def test_aggregate_batch_full_size_model(dev, tmp_path):
    from cra5_amd.api import cra5_api
    net = vaeformer_pretrained(quality=268, pretrained=False)
    synth.load_synthetic(net, seed=7)
    api = cra5_api(local_root=str(tmp_path), device="cuda", weights=net.to(dev))
    mean, std = api.get_mean_std()
    frames = [(synth.synth_frame(268, seed=s).numpy() * std[:, None, None] + mean[:, None, None]).astype(np.float32)
              for s in (2, 3)]
    stamps = ["2024-06-01T00:00:00", "2024-06-01T01:00:00"]
    api.encode_era5_batch(stamps, data=frames, save_root=str(tmp_path / "CRA5"), workers=2)
    kw = dict(variables=["z_500", "t2m"], stride=6)
    got = api.aggregate_batch(time_stamps=stamps, stats=("mean", "max"), workers=2, **kw)
    assert got["mean"].shape == got["max"].shape == (2, 121, 240) and got["n"] == 2
    assert got["variables"] == ["z_500", "t2m"] and len(got["lat"]) == 121 and len(got["lon"]) == 240
    assert_stats_equal(got, ref_time_stats(api.decode_batch(time_stamps=stamps, workers=2, **kw)))
