"""Packed int16 output, the host side (cra5_amd/pack.py) and the definition itself (tests/pack_helpers.py): the unpack
bound, the inputs' power to tell a wrong kernel from a right one, the range resolver and the NetCDF writer read back by
cra5_api.read_data_from_nc.  No GPU."""
import numpy as np
import pytest

import pack_helpers as ph
from cra5_amd import pack, synth
from cra5_amd.vaeformer import VAEformer

SHAPES = [(3, 7, 13), (1, 1, 1), (2, 70, 1440), (5, 25, 40)]


@pytest.fixture(scope="module")
def cases():
    """(shape, name, x, fixed, ref_pack(x, fixed)) of every named input at every shape, computed once."""
    out = []
    for shape in SHAPES:
        for name, (x, fixed) in ph.pack_inputs(shape).items():
            out.append((shape, name, x, fixed, ph.ref_pack(x, fixed)))
    return out


def test_reference_meets_the_unpack_bound_and_the_code_range(cases):
    worst = 0.0
    for shape, name, x, fixed, (q, scale, offset, vmin, vmax, nonfinite, saturated) in cases:
        fin = ph.finite_mask(x)
        assert np.array_equal(q == ph.FILL, ~fin), (shape, name)
        assert (np.abs(q[fin].astype(np.int32)) <= 32767).all(), (shape, name)
        assert np.array_equal(nonfinite, (~fin).reshape(len(x), -1).sum(1))
        back = ph.unpack(q, scale, offset)
        assert np.isnan(back[~fin]).all()
        for c in range(len(x)):
            if not fin[c].any():
                assert np.isnan(vmin[c]) and np.isnan(vmax[c])
                assert (scale[c], offset[c]) == (1.0, 0.0) or (fixed is not None and not np.isnan(fixed[c, 0]))
                continue
            given = fixed is not None and not np.isnan(fixed[c, 0])
            lo, hi = (fixed[c, 0], fixed[c, 1]) if given else (float(vmin[c]), float(vmax[c]))
            xc = x[c].astype(np.float64)
            inside = fin[c] & (xc >= lo) & (xc <= hi)
            assert saturated[c] == bool(given and (~inside & fin[c]).any()), (shape, name, c)
            err = np.abs(back[c][inside] - xc[inside])
            b = ph.bound(scale[c], lo, hi)
            assert (err <= b).all(), (shape, name, c, err.max(), b)
            worst = max(worst, float(err.max() / b))
            # outside a fixed range: the end codes
            assert (q[c][fin[c] & (xc > hi)] == 32767).all() and (q[c][fin[c] & (xc < lo)] == -32767).all()
    assert 0.9 < worst <= 1.0, worst       # the bound is met and is not slack


def test_exact_values_of_the_definition():
    # the tie ranges: scale and offset exact, ties to the even code
    for rng, scale in ((ph.TIE_RANGE, 0.25), (ph.TIE2_RANGE, 15.375)):
        k = np.arange(-6, 6)
        x = (scale * (k + 0.5)).astype(np.float32).reshape(1, 1, -1)
        q, s, o, *_ = ph.ref_pack(x, np.array([rng]))
        assert s[0] == scale and o[0] == 0.0
        assert q[0, 0].tolist() == [-6, -4, -4, -2, -2, 0, 0, 2, 2, 4, 4, 6]
    # a constant channel, a channel without a finite value, the per-frame range's end codes
    x = np.array([[[2.5, 2.5]], [[np.nan, np.inf]], [[-1.0, 3.0]]], dtype=np.float32)
    q, s, o, vmin, vmax, nf, sat = ph.ref_pack(x)
    assert (s[0], o[0], s[1], o[1]) == (1.0, 2.5, 1.0, 0.0) and s[2] == 4.0 / 65534.0 and o[2] == 1.0
    assert q.tolist() == [[[0, 0]], [[ph.FILL, ph.FILL]], [[-32767, 32767]]]
    assert np.isnan(vmin[1]) and np.isnan(vmax[1]) and nf.tolist() == [0, 2, 0] and not sat.any()
    assert np.array_equal(pack.unpack(q, s, o), ph.unpack(q, s, o), equal_nan=True)
    assert np.isnan(pack.unpack(q, s, o)[1]).all() and pack.FILL == ph.FILL == -32768


@pytest.mark.parametrize("mutant", ph.MUTANTS)
def test_every_mutant_differs_from_the_reference_on_the_inputs(cases, mutant):
    """The inputs can tell a wrong kernel from a right one - at the small shape alone, too."""
    for only in ((3, 7, 13), None):
        differs = [name for shape, name, x, fixed, ref in cases if only in (None, shape)
                   and not np.array_equal(ph.ref_pack(x, fixed, mutant)[0], ref[0])]
        assert differs, (mutant, only)


def test_resolve_ranges_and_check_fixed():
    names = ["z_850", "z_1000", "t_850", "t2m", "tp"]
    assert np.isnan(pack.resolve_ranges("int16", names)).all() and pack.resolve_ranges(True, names).shape == (5, 2)
    got = pack.resolve_ranges({"z": (-1e3, 6e4), "t2m": (200, 330.5)}, names)
    assert got.dtype == np.float64 and got[0].tolist() == got[1].tolist() == [-1e3, 6e4] and got[3].tolist() == [200.0, 330.5]
    assert np.isnan(got[[2, 4]]).all()
    assert pack.resolve_ranges({"z_1000": (0, 1)}, names)[1].tolist() == [0.0, 1.0]
    for bad in ({"q": (0, 1)}, {"t": (0, 1), "t_850": (0, 2)}, {"tp": (0, np.inf)}, {"tp": (np.nan, 1)}, {"tp": (1, 1)},
                {"tp": (2, 1)}, {"tp": 3}, {"tp": (1, 2, 3)}, "int8", None, False, 16, [("tp", (0, 1))], {"t2": (0, 1)}):
        with pytest.raises(ValueError):
            pack.resolve_ranges(bad, names)
    assert pack.check_fixed([[0, 1], [np.nan, np.nan]], 2).dtype == np.float64
    for bad, C in (([[0, 1]], 2), ([[1, 0]], 1), ([[0, np.inf]], 1), ([[0, np.nan]], 1), ([0, 1], 1)):
        with pytest.raises(ValueError):
            pack.check_fixed(bad, C)
    st = pack.frame_stats(np.array([[-7.0, 9.0, 2.0, 0.5, 1.0], [np.nan, np.nan, 12.0, 1.0, 0.0], [0.0, 1.0, 0.0, 1.0, 0.0]]),
                          np.array([[-5.0, 10.0], [0.0, 1.0], [np.nan, np.nan]]))
    assert st["saturated"].tolist() == [True, False, False] and st["nonfinite"].tolist() == [2, 12, 0]
    assert st["vmin"].dtype == np.float32 and st["scale_factor"].tolist() == [0.5, 1.0, 1.0] and st["fill_value"] == -32768
    assert pack.hours_since_1900("1900-01-02T03:00:00") == 27


# ---- the NetCDF writer -------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def api268(tmp_path_factory):
    from cra5_amd.api import cra5_api
    root = tmp_path_factory.mktemp("pack_nc")
    return cra5_api(local_root=str(root), device="cpu", weights=VAEformer(0, **synth.thin_model_kwargs()))


def _packed_268(api, Hg=3, Wg=4, seed=5):
    """All 268 channels on a tiny grid, the levels of a pressure variable under one shared range."""
    rng = np.random.default_rng(seed)
    names = [api.channels_to_vname[c] for c in range(268)]
    x = np.stack([rng.standard_normal((Hg, Wg)) * (1 + c % 9) + 10.0 * (c % 5) for c in range(268)]).astype(np.float32)
    x[names.index("t2m"), 1, 2] = np.nan
    x[names.index("q_500"), 0, 0] = np.inf
    fixed = np.full((268, 2), np.nan)
    for v in api.vnames["pressure"]:
        rows = [i for i, n in enumerate(names) if n.startswith(v + "_")]
        assert len(rows) == 37
        vals = x[rows][np.isfinite(x[rows])]
        fixed[rows] = (float(vals.min()), float(vals.max()))
    q, scale, offset, *_ = ph.ref_pack(x, fixed)
    return names, x, dict(q=q, scale_factor=scale, add_offset=offset)


def test_writer_files_are_read_back_by_read_data_from_nc(api268):
    from scipy.io import netcdf_file
    api = api268
    ts = "2024-06-01T06:00:00"
    names, x, packed = _packed_268(api)
    lat, lon = np.array([90.0, 89.75, 89.5]), np.array([0.0, 0.25, 0.5, 0.75])
    paths = pack.write_era5_nc(api.local_root, ts, packed, names, lat, lon, api.vnames)
    assert paths == [f"{api.local_root}/ERA5/2024/{ts}_pressure.nc", f"{api.local_root}/ERA5/2024/{ts}_single.nc"]
    want = pack.unpack(packed["q"], packed["scale_factor"], packed["add_offset"])
    # the files open with scipy, masked and scaled
    f = netcdf_file(paths[0], "r", mmap=False, maskandscale=True)
    assert f.version_byte == 2 and f.dimensions == dict(time=1, level=37, latitude=3, longitude=4)
    assert f.variables["level"][:].tolist() == [float(v) for v in api.pressure_level]
    assert f.variables["time"][:].tolist() == [pack.hours_since_1900(ts)] and f.variables["time"].units.startswith(b"hours since 1900")
    assert np.array_equal(f.variables["latitude"][:], lat.astype(np.float32))
    z = f.variables["z"]
    assert z.dimensions == ("time", "level", "latitude", "longitude") and z.data.dtype.kind == "i" and z.data.dtype.itemsize == 2
    assert np.asarray(z.scale_factor).dtype == np.float64 and float(z.scale_factor) == packed["scale_factor"][0]
    assert int(z._FillValue) == -32768 and int(z.missing_value) == -32768
    assert np.array_equal(np.ma.filled(z[:], np.nan)[0], want[:37])
    qv = f.variables["q"][:]
    assert np.ma.is_masked(qv) and qv.mask.sum() == 1
    f.close()
    f = netcdf_file(paths[1], "r", mmap=False, maskandscale=True)
    assert "level" not in f.dimensions and f.variables["t2m"].dimensions == ("time", "latitude", "longitude")
    tp = names.index("tp")
    assert float(f.variables["tp"].scale_factor) == packed["scale_factor"][tp] / 1000.0
    assert float(f.variables["tp"].add_offset) == packed["add_offset"][tp] / 1000.0
    f.close()
    # ... and come back through the project's own reader (fp32, tp x 1000 again): every channel is unpack(q)
    got = api.read_data_from_nc(ts)
    assert got.shape == (268, 3, 4) and got.dtype == np.float32
    for c, name in enumerate(names):
        # the reader works in fp32: 1e-6 of the value, and of the range's magnitude where scale * q and offset cancel
        atol = 1e-6 * (abs(packed["add_offset"][c]) + 32767 * packed["scale_factor"][c])
        assert np.allclose(got[c], want[c], rtol=1e-6, atol=atol, equal_nan=True), name
    assert np.isnan(got[names.index("t2m"), 1, 2]) and np.isnan(got[names.index("q_500"), 0, 0])
    assert np.isnan(got).sum() == 2


def test_writer_selections(api268, tmp_path):
    api = api268
    names, x, packed = _packed_268(api)
    lat, lon = np.array([90.0, 89.75, 89.5]), np.array([0.0, 0.25, 0.5, 0.75])

    def sub(sel):
        rows = [names.index(n) for n in sel]
        return dict(q=packed["q"][rows], scale_factor=packed["scale_factor"][rows], add_offset=packed["add_offset"][rows])

    # pressure levels in the order selected; no single-level variable: no _single.nc
    sel = ["z_850", "z_1000", "z_925", "t_850", "t_1000", "t_925"]
    ts = "2023-01-01T00:00:00"
    paths = pack.write_era5_nc(str(tmp_path), ts, sub(sel), sel, lat, lon, api.vnames)
    assert paths == [f"{tmp_path}/ERA5/2023/{ts}_pressure.nc"]
    assert sorted(p.name for p in (tmp_path / "ERA5" / "2023").iterdir()) == [f"{ts}_pressure.nc"]
    from scipy.io import netcdf_file
    f = netcdf_file(paths[0], "r", mmap=False, maskandscale=True)
    assert f.variables["level"][:].tolist() == [850.0, 1000.0, 925.0] and f.variables["t"].shape == (1, 3, 3, 4)
    want = pack.unpack(sub(sel)["q"], sub(sel)["scale_factor"], sub(sel)["add_offset"])
    assert np.array_equal(np.ma.filled(f.variables["t"][:], np.nan)[0], want[3:])
    f.close()
    # singles only: no _pressure.nc
    paths = pack.write_era5_nc(str(tmp_path), "2022-01-01T00:00:00", sub(["tp", "t2m"]), ["tp", "t2m"], lat, lon, api.vnames)
    assert paths == [f"{tmp_path}/ERA5/2022/2022-01-01T00:00:00_single.nc"]
    # not rectangular: the odd variable is named
    for bad in (["z_850", "z_1000", "t_850"], ["z_850", "z_1000", "t_1000", "t_850"]):
        with pytest.raises(ValueError, match="'t'"):
            pack.write_era5_nc(str(tmp_path), ts, sub(bad), bad, lat, lon, api.vnames)
    # levels of one variable under two packings, an unknown name, a wrong shape
    with pytest.raises(ValueError, match="share one"):
        pack.write_era5_nc(str(tmp_path), ts, sub(["z_850", "t2m"]) | dict(q=sub(["z_850", "z_500"])["q"]),
                           ["z_850", "z_500"], lat, lon, api.vnames)
    with pytest.raises(ValueError, match="neither"):
        pack.write_era5_nc(str(tmp_path), ts, sub(["t2m"]), ["sst"], lat, lon, api.vnames)
    with pytest.raises(ValueError, match="int16"):
        pack.write_era5_nc(str(tmp_path), ts, sub(["t2m"]), ["t2m"], lat[:2], lon, api.vnames)


def test_launchers_refuse_bad_arguments_before_any_device_work():
    """CRA5_ERR_ARG (-7) without a GPU; the pointers are never followed."""
    from cra5_amd._lib import lib
    L, p = lib(), 1 << 20
    assert L.cra5_pack_range_slab_bytes(0, 5) == 0 and L.cra5_pack_range_slab_bytes(1, 0) == 0
    assert L.cra5_pack_range_slab_bytes(1, 1 << 31) == 0 and L.cra5_pack_range_slab_bytes(3, 91) == 3 * 16
    assert L.cra5_pack_range_slab_bytes(268, 721 * 1440) == 268 * 43 * 16
    for C, plane, x, slab, nb, out in ((0, 91, p, p, 128, p), (3, 0, p, p, 128, p), (3, 1 << 31, p, p, 1 << 40, p),
                                       (3, 91, None, p, 128, p), (3, 91, p, None, 128, p), (3, 91, p, p, 128, None),
                                       (3, 91, p, p, 47, p), (3, 91, p + 2, p, 128, p), (3, 91, p, p + 8, 128, p)):
        assert L.cra5_pack_range_f32(x, C, plane, None, slab, nb, out, None) == -7, (C, plane, nb)
    for C, plane, x, table, q in ((0, 91, p, p, p), (3, 0, p, p, p), (3, 1 << 31, p, p, p), (3, 91, None, p, p),
                                  (3, 91, p, None, p), (3, 91, p, p, None), (3, 91, p, p, p + 1), (3, 91, p + 1, p, p)):
        assert L.cra5_pack_i16_f32(x, C, plane, table, q, None) == -7, (C, plane)
