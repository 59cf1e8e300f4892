"""Subset decode, host side (no GPU): the lat/lon box -> grid rows / columns rules (cra5_api.grid_box), variable names ->
channel indices for the 268- and a 159-variable configuration, the token range of the un-embed superset, the C ABI's
argument validation of the two new kernels, and the Selection record cra5_api._select makes of the decode arguments."""
import ctypes

import numpy as np
import pytest

from cra5_amd import _lib, subset, synth
from cra5_amd.api import cra5_api, variable_mapping
from cra5_amd.vaeformer import VAEformer

H, W = 721, 1440
ERR_ARG = -7


def box(region):
    return cra5_api.grid_box(region)["box"]


# ---- grid_box --------------------------------------------------------------------------------------------------------


def test_bounds_on_and_between_grid_points():
    assert box((35, 72, 0, 10)) == (72, 221, 0, 41)                  # on grid points: both ends included
    assert box((35.1, 71.9, 0.1, 9.9)) == (73, 220, 1, 39)           # between: the inner points
    assert box((35 - 1e-12, 72 + 1e-12, 1e-12, 10 - 1e-12)) == (72, 221, 0, 41)   # snapped within 1e-9 deg
    assert box((35 + 1e-12, 72 - 1e-12, -1e-12, 10 + 1e-12)) == (72, 221, 0, 41)
    g = cra5_api.grid_box((35, 72, 0, 10))
    assert g["rows"] == (72, 221) and g["col0"] == 0 and g["ncols"] == 41
    assert g["lat"].dtype == np.float64 and g["lat"][0] == 72.0 and g["lat"][-1] == 35.0
    assert np.all(np.diff(g["lat"]) < 0)                             # north to south
    assert g["lon"].dtype == np.float64 and g["lon"][0] == 0.0 and g["lon"][-1] == 10.0


def test_poles_and_last_meridian():
    assert box((90, 90, 0, 0)) == (0, 1, 0, 1)
    assert box((-90, -90, 0, 0)) == (720, 721, 0, 1)
    assert box((-90, 90, 0, 0))[:2] == (0, 721)
    g = cra5_api.grid_box((0, 0, 359.75, 359.75))
    assert g["box"] == (360, 361, 1439, 1) and g["lon"][0] == 359.75
    assert box((0, 0, -0.25, -0.25)) == (360, 361, 1439, 1)


def test_crossing_zero_degrees():
    europe = box((35, 72, -25, 45))
    assert europe == box((35, 72, 335, 45)) == (72, 221, 1340, 281)
    g = cra5_api.grid_box((35, 72, -25, 45))
    assert g["lon"][0] == 335.0 and g["lon"][-1] == 45.0 and np.all((g["lon"] >= 0) & (g["lon"] < 360))
    assert 0.0 in g["lon"] and len(set(g["lon"])) == 281
    assert box((0, 1, 359.9, 0.1)) == (356, 361, 0, 1)               # only lon 0 lies in [359.9, 360.1]


def test_full_circle():
    g = cra5_api.grid_box((-90, 90, -180, 180))
    assert g["box"] == (0, 721, 720, 1440) and g["lon"][0] == 180.0 and g["lon"][-1] == 179.75
    assert sorted(g["lon"]) == list(np.arange(1440) * 0.25)
    g = cra5_api.grid_box((-90, 90, 0.25, 360.25))
    assert g["box"] == (0, 721, 1, 1440) and g["lon"][0] == 0.25 and g["lon"][-1] == 0.0
    assert box((-90, 90, 0, 360)) == (0, 721, 0, 1440)
    assert box((-10, 10, 0.1, 360.1))[2:] == (1, 1440)               # never W + 1 columns
    assert box((-10, 10, 5, 725))[3] == 1440


def test_single_points():
    assert box((10, 10, 20, 20)) == (320, 321, 80, 1)
    assert box((-89.75, -89.75, 180.25, 180.25)) == (719, 720, 721, 1)


@pytest.mark.parametrize("region, msg", [
    ((10.1, 10.2, 0, 10), "no grid row"),
    ((0, 10, 20.1, 20.2), "no grid column"),
    ((-91, 0, 0, 10), r"\[-90, 90\]"),
    ((0, 90.5, 0, 10), r"\[-90, 90\]"),
    ((20, 10, 0, 10), "lat_min > lat_max"),
    ((0, 10, 0), "lat_min, lat_max, lon_min, lon_max"),
    ((0, float("nan"), 0, 10), "finite"),
])
def test_grid_box_errors(region, msg):
    with pytest.raises(ValueError, match=msg):
        cra5_api.grid_box(region)


# ---- variable names --------------------------------------------------------------------------------------------------


def test_resolve_variables_268():
    c2v, v2c = variable_mapping()
    assert len(c2v) == 268 and c2v[0] == "z_1000" and c2v[267] == "msl"
    assert cra5_api.resolve_variables(["z_500", "t_850", "t2m"], v2c) == [15, 154, 263]
    assert cra5_api.resolve_variables(["t2m", "z_500"], v2c) == [263, 15]          # the order given
    assert cra5_api.resolve_variables(None, v2c) is None
    with pytest.raises(ValueError, match="empty"):
        cra5_api.resolve_variables([], v2c)
    with pytest.raises(ValueError, match=r"unknown.*'z_501'"):
        cra5_api.resolve_variables(["z_500", "z_501"], v2c)
    with pytest.raises(ValueError, match=r"more than once.*'t2m'"):
        cra5_api.resolve_variables(["t2m", "z_500", "t2m"], v2c)
    with pytest.raises(ValueError, match="list of names"):
        cra5_api.resolve_variables("t2m", v2c)


def test_resolve_variables_159_from_a_config(tmp_path):
    cfg = tmp_path / "era5_159v.py"
    levels = [1000.0, 925.0, 850.0, 700.0, 600.0, 500.0, 400.0, 300.0, 250.0, 200.0, 150.0, 100.0, 50.0]
    cfg.write_text("vnames = dict(pressure=['z', 'q', 'u', 'v', 't', 'r', 'w', 'x', 'y', 'o', 'p', 's'],\n"
                   "              single=['v10', 'u10', 'tp'])\n"
                   f"pressure_level = {levels!r}\n")
    c2v, v2c = variable_mapping(str(cfg))
    assert len(c2v) == 159 and c2v[0] == "z_1000" and c2v[158] == "tp"
    assert cra5_api.resolve_variables(["tp", "z_500", "s_50"], v2c) == [158, 5, 155]
    with pytest.raises(ValueError, match="unknown"):
        cra5_api.resolve_variables(["z_975"], v2c)                # a level the 159 set does not carry
    with pytest.raises(ValueError, match="unknown"):
        cra5_api.resolve_variables(["t2m"], v2c)


# ---- token range of the un-embed superset ----------------------------------------------------------------------------


def test_token_range_covers_every_box_row():
    """numpy restatement: image row r receives token rows ti with 0 <= r - 10 ti <= 10.  For every box r0 .. r1 - 1
    (all 721 x 722 / 2 row ranges) every contributing token row of every box row lies in the superset, and the
    superset's own edge rows that lack a partner are outside the box or on the grid's edge."""
    Hp = 72
    r = np.arange(H)
    lo_c = np.maximum(0, -(-(r - 10) // 10))       # first contributing token row of image row r
    hi_c = np.minimum(Hp - 1, r // 10)             # last
    for r0 in range(H):
        r1 = np.arange(r0 + 1, H + 1)
        ti0 = max(0, -(-r0 // 10) - 1)
        ti1 = np.minimum(Hp - 1, (r1 - 1) // 10)
        # every box row's contributors: the first is >= ti0 (top rows) and the last <= ti1 (bottom rows)
        assert lo_c[r0] >= ti0 and hi_c[r0] <= ti1.min()
        assert np.all(hi_c[r1 - 1] <= ti1) and np.all(lo_c[r1 - 1] >= ti0)
        # edge rows of the superset (10 ti0 and 10 (ti1 + 1)) with one contribution: outside the box or a grid edge
        top, bot = 10 * ti0, 10 * (ti1 + 1)
        assert top < r0 or top == 0
        assert np.all((bot > r1 - 1) | (bot == 720))
        for a in (0, len(r1) // 2, len(r1) - 1):   # the product's plan agrees
            p = subset.token_plan((r0, int(r1[a]), 0, 40), H, W)
            assert (p["ti0"], p["ti0"] + p["n_ti"] - 1) == (ti0, int(ti1[a]))
            assert p["r_off"] == r0 - 10 * ti0 and p["Hs"] == 10 * p["n_ti"] + 1


def test_token_columns_wrap_even_and_cap():
    p = subset.token_plan((72, 221, 1340, 281), H, W)              # Europe, across 0 deg
    assert (p["tj0"], p["n_tj"], p["Ws"], p["c_off"]) == (134, 30, 300, 0) and p["n_tj"] % 2 == 0
    p = subset.token_plan((0, 10, 13, 1), H, W)                     # one column: two tokens (even count)
    assert (p["tj0"], p["n_tj"], p["c_off"]) == (1, 2, 3)
    p = subset.token_plan((0, 721, 1, 1440), H, W)                  # full circle off a patch boundary: wraps in the crop
    assert (p["tj0"], p["n_tj"], p["c_off"], p["exact"]) == (0, 144, 1, False)
    p = subset.token_plan((0, 10, 5, 1431), H, W)                   # 144 tokens needed: capped, the whole circle
    assert (p["tj0"], p["n_tj"], p["c_off"]) == (0, 144, 5)
    assert subset.token_plan((0, 721, 0, 1440), H, W)["exact"]
    assert subset.token_plan((10, 31, 20, 40), H, W)["exact"] is False
    with pytest.raises(ValueError, match="box"):
        subset.token_plan((5, 5, 0, 10), H, W)


# ---- C ABI: argument validation before any device work ---------------------------------------------------------------


def test_new_kernels_validate_arguments_without_gpu():
    L = _lib.lib()
    fake_a, fake_b = ctypes.c_void_p(1 << 20), ctypes.c_void_p(2 << 20)   # never dereferenced: every call is refused
    assert L.cra5_gather_token_rows(None, 64, fake_b, 64, 64, 2, 2, 0, 1, 0, 1, None) == ERR_ARG
    assert L.cra5_gather_token_rows(fake_a, 64, fake_b, 64, 60, 2, 2, 0, 1, 0, 1, None) == ERR_ARG    # row % 16
    assert L.cra5_gather_token_rows(fake_a, 48, fake_b, 64, 64, 2, 2, 0, 1, 0, 1, None) == ERR_ARG    # pitch < row
    assert L.cra5_gather_token_rows(fake_a, 64, fake_b, 64, 64, 2, 2, 1, 2, 0, 1, None) == ERR_ARG    # rows past Hp
    assert L.cra5_gather_token_rows(fake_a, 64, fake_b, 64, 64, 2, 2, 0, 1, 2, 1, None) == ERR_ARG    # tj0 >= Wp
    assert L.cra5_gather_token_rows(fake_a, 64, fake_b, 64, 64, 2, 2, 0, 1, 0, 3, None) == ERR_ARG    # n_tj > Wp
    assert L.cra5_crop_f32(None, 1, 4, 4, fake_b, 0, 1, 0, 1, None) == ERR_ARG
    assert L.cra5_crop_f32(fake_a, 1, 4, 4, fake_b, 2, 3, 0, 1, None) == ERR_ARG                      # rows past Hs
    assert L.cra5_crop_f32(fake_a, 1, 4, 4, fake_b, 0, 1, 4, 1, None) == ERR_ARG                      # c0 >= Ws
    assert L.cra5_crop_f32(fake_a, 1, 4, 4, fake_b, 0, 1, 0, 5, None) == ERR_ARG                      # Wb > Ws
    assert L.cra5_crop_f32(fake_a, 0, 4, 4, fake_b, 0, 1, 0, 1, None) == ERR_ARG
    # CRA5_GEMM_WIDE_K exists with CRA5_GEMM_HI_ONLY only
    assert L.cra5_gemm_nt_split(fake_a, 64, fake_b, 64, fake_b, 64, None, 0, None, None, 0, 1, 1, 64, 1.0, 128,
                                None) == ERR_ARG


# ---- the Selection record of the decode methods ------------------------------------------------------------------------


@pytest.fixture(scope="module")
def thin_api():
    return cra5_api(device="cpu", weights=VAEformer(0, **synth.thin_model_kwargs()))


GLOBE = (-90, 90, 0, 360)
ALL_8 = ["z_1000", "z_975", "z_950", "z_925", "z_900", "z_875", "z_850", "z_825"]     # the thin model's channels, in order
# (variables, region, stride, coarsen), every argument canonical-None, whole
SELECTIONS = [
    (None, None, None, None, True, True),
    (["z_850", "z_1000", "z_925"], None, None, None, False, False),       # not sorted: the order given
    (None, (35, 72, 0, 10), None, None, False, False),
    (None, (-10.3, 20.1, 350.2, 9.9), None, None, False, False),          # across 0 deg: the columns wrap at W
    (None, (-60, 60, 170, -170), None, None, False, False),               # across the date line
    (None, None, 6, None, False, False),
    (None, (35, 72, -25, 45), (6, 4), None, False, False),
    (None, None, None, 6, False, False),
    (["z_825", "z_975"], (-30, 30, 350, 20), None, (6, 4), False, False),
    # the no-op spellings: the model takes the whole-frame path for each of them
    (None, None, 1, None, True, True),
    (None, None, None, (1, 1), True, True),
    # ... and these two name a region / variables: decode_from_bin's dict carries variables, lat and lon for them
    (None, GLOBE, None, None, True, False),
    (ALL_8, None, None, None, True, False),
]


@pytest.mark.parametrize("variables, region, stride, coarsen, noop, whole", SELECTIONS)
def test_select_record(thin_api, variables, region, stride, coarsen, noop, whole):
    """_select against the pieces composed by hand: subset.resolve_variables and subset.grid_box for the request, the
    model's _subset_args / _step_arg / _coarsen_arg for the canonical arguments, _decoded_shape for the frame."""
    api, net = thin_api, thin_api.net
    sel = api._select(variables, region, stride, coarsen)
    chans = subset.resolve_variables(variables, api.vname_to_channels)
    g = subset.grid_box(region if region is not None else GLOBE, H, W, stride=stride, coarsen=coarsen)
    channels, box = net._subset_args(chans, g["box"] if region is not None else None)
    step = net._step_arg(stride, box)
    k = net._coarsen_arg(coarsen, box, step)
    assert (sel.channels, sel.box, sel.step, sel.coarsen) == (channels, box, step, k)
    assert sel.model == dict(channels=channels, box=box, step=step, coarsen=k)
    assert ((channels, box, step, k) == (None, None, None, None)) == noop
    assert sel.shape == net._decoded_shape(channels, box, step, k)
    assert sel.names == (list(variables) if variables is not None else ALL_8)
    assert sel.lat.dtype == sel.lon.dtype == np.float64
    assert np.array_equal(sel.lat, g["lat"]) and np.array_equal(sel.lon, g["lon"])
    assert sel.shape == (len(sel.names), len(g["lat"]), len(g["lon"]))
    meta = sel.meta
    if k is None:
        assert sel.lat_bnds is None and sel.lon_bnds is None
        assert list(meta) == ["variables", "lat", "lon"]
    else:
        assert np.array_equal(sel.lat_bnds, g["lat_bnds"]) and np.array_equal(sel.lon_bnds, g["lon_bnds"])
        assert sel.lat_bnds.shape == (sel.shape[1], 2) and sel.lon_bnds.shape == (sel.shape[2], 2)
        assert list(meta) == ["variables", "lat", "lon", "coarsen", "lat_bnds", "lon_bnds"]
        assert meta["coarsen"] == k and meta["lat_bnds"] is sel.lat_bnds and meta["lon_bnds"] is sel.lon_bnds
    assert meta["variables"] is sel.names and meta["lat"] is sel.lat and meta["lon"] is sel.lon
    assert sel.whole is whole
    if whole:
        assert sel.shape == (8, H, W) and sel.lat[0] == 90.0 and sel.lat[-1] == -90.0 and sel.lon[-1] == 359.75


@pytest.mark.parametrize("kw, msg", [
    (dict(stride=6, coarsen=6), "pass one of the two"),
    (dict(stride=(1, 2), coarsen=(6, 1)), "pass one of the two"),
    (dict(stride=7), r"1440 % s_lon \(7\)"),
    (dict(coarsen=7), r"\(721 - 1\) % k_lat \(7\)"),
    (dict(variables=["z_850", "z_501"]), r"unknown.*'z_501'"),
    (dict(variables=["t2m"]), r"indices \[263\] outside \[0, 8\)"),            # a name of the 268 set the thin model lacks
    (dict(variables=[]), "empty"),
    (dict(region=(9.25, 10.25, 0, 10), stride=6), "hold no row"),               # rows 319 .. 323: none with row % 6 == 0
    (dict(region=(0, 10, 0.25, 1), stride=6), "hold no column"),
    (dict(region=(9.25, 10.25, 0, 10), coarsen=6), "hold no row"),
    (dict(region=(20, 10, 0, 10)), "lat_min > lat_max"),
])
def test_select_refusals(thin_api, kw, msg):
    with pytest.raises(ValueError, match=msg):
        thin_api._select(**kw)
