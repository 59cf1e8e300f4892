"""Packed int16 input on the host ("Packed int16 input"): the helper's own self-check, pack.unpack_f32
against the definition, PackedFrame, and read_era5_nc_packed against cra5_api.read_data_from_nc bit for bit.  No GPU."""
import warnings

import numpy as np
import pytest

import pack_helpers as ph
import unpack_helpers as uh
from cra5_amd import pack, synth
from cra5_amd.vaeformer import VAEformer

ALL_SHAPES = uh.SHAPES + [uh.FULL_SHAPE]


def _frame(q, table, swapped=False):
    fill = table[:, 2]
    q = q.astype(q.dtype.newbyteorder()) if swapped else q
    return pack.PackedFrame(q, table[:, 0], table[:, 1], fill, table[:, 3])


@pytest.mark.parametrize("shape", ALL_SHAPES)
def test_inputs_separate_the_definition_from_its_mutants(shape):
    seen = uh.self_check(shape)
    assert set(seen) == set(uh.INPUT_NAMES)
    if shape == uh.FULL_SHAPE:
        q, _ = uh.unpack_inputs(shape)["random"]
        assert all(len(np.unique(q[c])) == 65536 for c in range(shape[0]))      # every code value in every channel


def test_tie_construction_rate_and_tp_share():
    rng = np.random.default_rng(1)
    kept = sum(uh.tie_channel(rng) is not None for _ in range(400))
    assert kept >= 80, kept                       # roughly two in five constructions separate the fused multiply-add
    _, t = uh.unpack_inputs((3, 7, 13))["tp_like"]
    assert t[-1, 3] == 1000.0 and uh.tp_share(t[-1])[0] > 0.05


@pytest.mark.parametrize("shape", ALL_SHAPES)
def test_unpack_f32_is_the_definition(shape):
    for name, (q, table) in uh.unpack_inputs(shape).items():
        ref = uh.bits(uh.ref_unpack(q, table))
        for swapped in (False, True):
            got = pack.unpack_f32(_frame(q, table, swapped))
            assert got.dtype == np.float32 and np.array_equal(uh.bits(got), ref), (shape, name, swapped)
        if q.shape[0] > 1:          # the same frame as blocks
            f = pack.PackedFrame([q[:1].copy(), q[1:].copy()], table[:, 0], table[:, 1], table[:, 2], table[:, 3])
            assert f.shape == q.shape and np.array_equal(uh.bits(pack.unpack_f32(f)), ref)
    nan = pack.unpack_f32(pack.PackedFrame(np.full((1, 1, 2), uh.FILL, dtype=np.int16), [1.0], [0.0]))
    assert (uh.bits(nan) == uh.QNAN).all()


def test_packed_frame_validation():
    q = np.zeros((3, 4, 5), dtype=np.int16)
    sf, ao = np.ones(3), np.zeros(3)
    f = pack.PackedFrame(q, sf, ao)
    assert f.shape == (3, 4, 5) and not f.swapped and f.nbytes == 120 and (f.fill == -32768).all() and (f.multiplier == 1).all()
    assert f.table().shape == (3, 4) and f.table().dtype == np.float64
    assert np.isnan(pack.PackedFrame(q, sf, ao, None).fill).all()
    assert pack.PackedFrame(q.astype(">i2"), sf, ao).swapped != pack.PackedFrame(q.astype("<i2"), sf, ao).swapped
    assert pack.PackedFrame([q[:2], q[2:]], sf, ao, [1, np.nan, -5], [1, 1000, 0.5]).shape == (3, 4, 5)
    bad = [
        lambda: pack.PackedFrame(q.astype(np.int32), sf, ao),
        lambda: pack.PackedFrame(q.astype(np.float32), sf, ao),
        lambda: pack.PackedFrame(q[0], sf, ao),
        lambda: pack.PackedFrame([], sf, ao),
        lambda: pack.PackedFrame([q[:2], q[2:, :3]], sf, ao),
        lambda: pack.PackedFrame([q[:2], q[2:].astype(q.dtype.newbyteorder())], sf, ao),
        lambda: pack.PackedFrame([q[:2], q[:, :, ::2][2:]], sf, ao),
        lambda: pack.PackedFrame(q, sf[:2], ao),
        lambda: pack.PackedFrame(q, sf, np.zeros((3, 1))),
        lambda: pack.PackedFrame(q, [1.0, np.inf, 1.0], ao),
        lambda: pack.PackedFrame(q, sf, [0.0, 0.0, np.nan]),
        lambda: pack.PackedFrame(q, sf, ao, fill_value=[1, 2]),
        lambda: pack.PackedFrame(q, sf, ao, fill_value=0.5),
        lambda: pack.PackedFrame(q, sf, ao, fill_value=40000),
        lambda: pack.PackedFrame(q, sf, ao, multiplier=[1, 1]),
        lambda: pack.PackedFrame(q, sf, ao, multiplier=[1, 0.1, 1]),
        lambda: pack.PackedFrame(q, sf, ao, multiplier=[1, np.inf, 1]),
        lambda: pack.PackedFrame("q", sf, ao),
    ]
    for i, make in enumerate(bad):
        with pytest.raises(ValueError, match="PackedFrame"):
            make()
            pytest.fail(f"case {i} was accepted")


def test_from_decode():
    rng = np.random.default_rng(3)
    q = rng.integers(-32768, 32768, size=(4, 6, 7)).astype(np.int16)
    sf, ao = rng.uniform(0.1, 2, 4), rng.uniform(-5, 5, 4)
    stats = dict(scale_factor=sf, add_offset=ao, fill_value=-32768, vmin=None, vmax=None, nonfinite=None, saturated=None)
    table = np.stack([sf, ao, np.full(4, -32768.0), np.ones(4)], 1)
    ref = uh.bits(uh.ref_unpack(q, table))
    for d in (dict(stats, x_hat=q, decoding_time=0.1), dict(stats, q=q), dict(stats, x_hat=q[None])):
        f = pack.PackedFrame.from_decode(d)
        assert f.shape == (4, 6, 7) and np.array_equal(uh.bits(pack.unpack_f32(f)), ref)


# ---- the NetCDF files ----------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def api268(tmp_path_factory):
    from cra5_amd.api import cra5_api
    root = tmp_path_factory.mktemp("unpack_nc")
    return cra5_api(local_root=str(root), device="cpu", weights=VAEformer(0, **synth.thin_model_kwargs()))


LAT, LON = np.linspace(90, 89, 5), np.linspace(0, 1.75, 8)


def _packed_268(api, seed=5):
    """All 268 channels on a 5 x 8 grid, the levels of a pressure variable under one shared range, one NaN in t2m."""
    rng = np.random.default_rng(seed)
    names = [api.channels_to_vname[c] for c in range(268)]
    x = np.stack([rng.standard_normal((5, 8)) * (1 + c % 9) + 10.0 * (c % 5) for c in range(268)]).astype(np.float32)
    x[names.index("t2m"), 1, 2] = np.nan
    fixed = np.full((268, 2), np.nan)
    for v in api.vnames["pressure"]:
        rows = [i for i, n in enumerate(names) if n.startswith(v + "_")]
        fixed[rows] = (float(x[rows].min()), float(x[rows].max()))
    q, scale, offset, *_ = ph.ref_pack(x, fixed)
    return names, dict(q=q, scale_factor=scale, add_offset=offset)


def _read_both(api, ts):
    """(the packed frame's unpack_f32, its block count / dtypes, read_data_from_nc) with no mapping left open."""
    with warnings.catch_warnings():
        warnings.simplefilter("error")                  # closing a mapping that still has views warns
        frame = pack.read_era5_nc_packed(api.local_root, ts, api.vnames, api.pressure_level)
        assert isinstance(frame, pack.PackedFrame)
        info = dict(blocks=len(frame.blocks), dtypes={b.dtype.str for b in frame.blocks}, shape=frame.shape,
                    views=all(b.base is not None and not b.flags["OWNDATA"] and not b.flags["WRITEABLE"] for b in frame.blocks),
                    swapped=frame.swapped, multiplier=frame.multiplier.copy(), fill=frame.fill.copy())
        got = pack.unpack_f32(frame)
        frame.close()
        assert frame.blocks is None
    return got, info, api.read_data_from_nc(ts)


def test_read_era5_nc_packed_equals_the_host_reader(api268):
    api = api268
    ts = "2024-06-01T06:00:00"
    names, packed = _packed_268(api)
    pack.write_era5_nc(api.local_root, ts, packed, names, LAT, LON, api.vnames)
    got, info, host = _read_both(api, ts)
    n_vars = len(api.vnames["pressure"]) + len(api.vnames["single"])
    assert info["shape"] == (268, 5, 8) and info["dtypes"] == {">i2"} and info["swapped"] == (np.little_endian)
    assert info["blocks"] == n_vars and info["views"]              # one view per file variable: nothing concatenated
    tp = names.index("tp")
    assert info["multiplier"][tp] == 1000.0 and info["multiplier"].sum() == 1267.0 and (info["fill"] == -32768).all()
    assert host.dtype == np.float32 and host.shape == (268, 5, 8)
    assert np.array_equal(uh.bits(got), uh.bits(host))              # bit for bit: tp and the NaN included
    assert np.isnan(got[names.index("t2m"), 1, 2]) and np.isnan(got).sum() == 1


def _write_pressure(path, levels, variables, lat=LAT, lon=LON, single=False):
    """A test-written file: variables = {name: (dtype, codes or values [L, H, W] / [H, W], attributes)}."""
    from scipy.io import netcdf_file
    f = netcdf_file(path, "w", version=2)
    f.createDimension("time", 1)
    if not single:
        f.createDimension("level", len(levels))
    f.createDimension("latitude", len(lat))
    f.createDimension("longitude", len(lon))
    if not single:
        v = f.createVariable("level", "f4", ("level",))
        v[:] = np.asarray(levels, dtype=np.float32)
    dims = ("time", "latitude", "longitude") if single else ("time", "level", "latitude", "longitude")
    for name, (dtype, data, att) in variables.items():
        v = f.createVariable(name, dtype, dims)
        v[:] = data[None]
        for k, a in att.items():
            setattr(v, k, a)
    f.close()


def test_reversed_superset_of_levels(api268, tmp_path):
    """The file's level axis holds every model level in reverse order, with two foreign levels in between."""
    api = api268
    ts = "2023-03-01T00:00:00"
    rng = np.random.default_rng(11)
    levels = [float(v) for v in api.pressure_level][::-1]
    levels[5:5] = [3.5, 1234.0]
    folder = tmp_path / "ERA5" / "2023"
    folder.mkdir(parents=True)
    att = lambda s, o: dict(scale_factor=np.float64(s), add_offset=np.float64(o), _FillValue=np.int16(-32768),   # noqa: E731
                            missing_value=np.int16(-32768))
    pv = {}
    for i, name in enumerate(api.vnames["pressure"]):
        codes = rng.integers(-32768, 32768, size=(len(levels), 5, 8)).astype(np.int16)
        codes[-1, 0, i] = -32768                        # a fill code on the model's first level
        pv[name] = ("i2", codes, att(rng.uniform(1e-3, 2.0), rng.uniform(-100, 5e4)))
    _write_pressure(str(folder / f"{ts}_pressure.nc"), levels, pv)
    sv = {name: ("i2", rng.integers(-32768, 32768, size=(5, 8)).astype(np.int16),
                 att(rng.uniform(1e-7, 2.0), rng.uniform(-1, 300))) for name in api.vnames["single"]}
    _write_pressure(str(folder / f"{ts}_single.nc"), None, sv, single=True)
    root, api.local_root = api.local_root, str(tmp_path)
    try:
        got, info, host = _read_both(api, ts)
    finally:
        api.local_root = root
    assert info["blocks"] == 37 * len(api.vnames["pressure"]) + len(api.vnames["single"]) and info["views"]
    assert np.array_equal(uh.bits(got), uh.bits(host)) and np.isnan(got).any()
    # channel 0 is the model's first level, the LAST of the file's axis
    z = pv[api.vnames["pressure"][0]]
    assert levels[-1] == float(api.pressure_level[0])
    t = np.array([[z[2]["scale_factor"], z[2]["add_offset"], -32768.0, 1.0]])
    assert np.array_equal(uh.bits(got[0]), uh.bits(uh.ref_unpack(z[1][-1:], t)[0]))


def test_none_for_files_that_are_not_plain_packed_int16(api268, tmp_path):
    ts = "2022-01-01T00:00:00"
    folder = tmp_path / "ERA5" / "2022"
    folder.mkdir(parents=True)
    vn = dict(pressure=["z"], single=["t2m"])
    levels = [1000.0, 850.0]
    good = dict(scale_factor=np.float64(0.5), add_offset=np.float64(3.0), _FillValue=np.int16(-32768), missing_value=np.int16(-32768))
    codes = np.arange(80, dtype=np.int16).reshape(2, 5, 8)

    def attempt(z_var, t_var=("i2", codes[0], good)):
        _write_pressure(str(folder / f"{ts}_pressure.nc"), levels, dict(z=z_var))
        _write_pressure(str(folder / f"{ts}_single.nc"), None, dict(t2m=t_var), single=True)
        why = []
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            f = pack.read_era5_nc_packed(str(tmp_path), ts, vn, levels, reason=why)
        return f, why

    f, why = attempt(("i2", codes, good))
    assert f is not None and f.shape == (3, 5, 8) and why == []
    f.close()
    f, why = attempt(("i2", codes, {k: v for k, v in good.items() if k != "_FillValue"}))      # one of the two: fine
    assert f is not None and (f.fill == -32768).all()
    f.close()
    f, why = attempt(("i2", codes, dict(scale_factor=np.float64(0.5), add_offset=np.float64(3.0))))
    assert f is not None and np.isnan(f.fill[:2]).all() and f.fill[2] == -32768                 # no fill code at all
    f.close()
    for z_var, t_var, word in (
            (("f4", codes.astype(np.float32), {}), ("i2", codes[0], good), "float32"),
            (("i2", codes, good), ("f8", codes[0].astype(np.float64), {}), "float64"),
            (("i2", codes, {k: v for k, v in good.items() if k != "scale_factor"}), ("i2", codes[0], good), "scale_factor"),
            (("i2", codes, {k: v for k, v in good.items() if k != "add_offset"}), ("i2", codes[0], good), "add_offset"),
            (("i2", codes, dict(good, missing_value=np.int16(-999))), ("i2", codes[0], good), "missing_value"),
            (("i2", codes, good), ("i2", codes[0], dict(good, _FillValue=np.int16(7))), "_FillValue")):
        f, why = attempt(z_var, t_var)
        assert f is None and len(why) == 1 and word in why[0] and f"{ts}_" in why[0], (word, why)
    # a level of the model that the file lacks, and a file that is not NetCDF-3
    _write_pressure(str(folder / f"{ts}_pressure.nc"), levels, dict(z=("i2", codes, good)))
    why = []
    assert pack.read_era5_nc_packed(str(tmp_path), ts, vn, [1000.0, 500.0], reason=why) is None and "level" in why[0]
    with open(folder / f"{ts}_pressure.nc", "r+b") as fh:
        fh.write(b"\x89HDF")
    why = []
    assert pack.read_era5_nc_packed(str(tmp_path), ts, vn, levels, reason=why) is None and "NetCDF-3" in why[0]
    assert pack.read_era5_nc_packed(str(tmp_path), ts, vn, levels) is None


def test_api_ingest_argument_and_cpu_frame(api268):
    """The keyword is checked before anything is read; on a CPU net _frame unpacks a PackedFrame on the host."""
    api = api268
    with pytest.raises(ValueError, match="ingest"):
        api.encode_era5_as_bin("2024-06-01T06:00:00", ingest="int16")
    with pytest.raises(ValueError, match="ingest"):
        api.encode_to_latent("2024-06-01T06:00:00", ingest=None)
    q, table = uh.unpack_inputs((3, 7, 13))["tp_like"]
    x = api._frame(None, _frame(q, table, swapped=True))
    assert x.dtype.is_floating_point and np.array_equal(uh.bits(x.numpy()), uh.bits(uh.ref_unpack(q, table)))
    # a float variable: "packed" names the file, "auto" reads it as "host" does
    ts = "2021-01-01T00:00:00"
    keep = api.vnames, api.pressure_level
    api.vnames, api.pressure_level = dict(pressure=["z"], single=["t2m"]), [1000.0, 850.0]
    try:
        import os
        os.makedirs(f"{api.local_root}/ERA5/2021", exist_ok=True)
        good = dict(scale_factor=np.float64(0.5), add_offset=np.float64(3.0), _FillValue=np.int16(-32768))
        vals = np.arange(80, dtype=np.float32).reshape(2, 5, 8)
        _write_pressure(f"{api.local_root}/ERA5/2021/{ts}_pressure.nc", [1000.0, 850.0], dict(z=("f4", vals, {})))
        _write_pressure(f"{api.local_root}/ERA5/2021/{ts}_single.nc", None,
                        dict(t2m=("i2", vals[0].astype(np.int16), good)), single=True)
        with pytest.raises(ValueError, match=f"ingest='packed'.*{ts}_pressure.nc.*'z'"):
            api._ingest(ts, "packed")
        auto = api._ingest(ts, "auto")
        assert isinstance(auto, np.ndarray) and np.array_equal(auto, api._ingest(ts, "host")) and auto.shape == (3, 5, 8)
    finally:
        api.vnames, api.pressure_level = keep


def test_launcher_refuses_bad_arguments_before_any_device_work():
    """CRA5_ERR_ARG (-7) without a GPU; the pointers are never followed."""
    from cra5_amd._lib import lib
    L, p = lib(), 1 << 20
    ok = (p, 3, 91, p, 0, p)
    cases = [(None, 3, 91, p, 0, p), (p, 3, 91, None, 0, p), (p, 3, 91, p, 0, None),          # NULL
             (p + 1, 3, 91, p, 0, p), (p, 3, 91, p + 4, 0, p), (p, 3, 91, p, 0, p + 2),        # misaligned
             (p, 0, 91, p, 0, p), (p, -1, 91, p, 0, p), (p, 3, 0, p, 0, p), (p, 3, 1 << 31, p, 0, p),
             (p, 3, 91, p, 2, p), (p, 3, 91, p, 3, p), (p, 3, 91, p, 1 << 31, p)]               # unknown flag bits
    assert len(ok) == 6
    for q, C, plane, table, flags, x in cases:
        assert L.cra5_unpack_i16_f32(q, C, plane, table, flags, x, None) == -7, (q, C, plane, table, flags, x)
