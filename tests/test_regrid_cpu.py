"""The host side of regridding (cra5_amd/regrid.py: Grid, Grid.plan, tile_table) against definitions written here: np.interp,
exact rational overlaps, the area integral, and coarsen_plan's own cells.  No GPU."""
from fractions import Fraction

import numpy as np
import pytest

import coarsen_helpers as ch
import regrid_helpers as rh
from cra5_amd import subset
from cra5_amd.regrid import Grid, as_plan, tile_table

GRIDS = [(13, 24), (721, 1440)]


def _random_targets(Hg, Wg, seed, Ho=9, Wo=11):
    rng = np.random.default_rng(seed)
    lat = np.sort(rng.uniform(-90, 90, Ho))[::-1].copy()
    lon0 = rng.uniform(-400, 400)
    lon = lon0 + np.sort(rng.uniform(0, 359.0, Wo))
    return lat, lon


# ---- bilinear ----------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("grid", GRIDS)
def test_bilinear_equals_np_interp_along_each_axis(grid):
    Hg, Wg = grid
    full = rh.field(2, Hg, Wg, seed=Hg)
    lat, lon = _random_targets(Hg, Wg, seed=Wg)
    plan = Grid(lat, lon).plan(Hg, Wg)
    _, got = rh.ref_regrid(full, plan)
    slat, slon = rh.source_lat(Hg), rh.source_lon(Wg)
    lon_pad = np.concatenate([slon, [360.0]])
    x = full.astype(np.float64)
    ref = np.empty_like(got)
    for c in range(2):
        rows = np.stack([np.interp(lon % 360.0, lon_pad, np.concatenate([x[c, h], x[c, h, :1]])) for h in range(Hg)])
        for j in range(len(lon)):
            ref[c, :, j] = np.interp(lat, slat[::-1], rows[::-1, j])
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(x).max()
    assert plan["ntap"].max() <= 2 and plan["ctap"].max() <= 2 and plan["method"] == "bilinear"
    assert np.array_equal(plan["lat"], lat) and np.array_equal(plan["lon"], lon)


@pytest.mark.parametrize("grid", GRIDS)
def test_bilinear_points_on_the_lattice_have_one_tap_of_weight_one(grid):
    Hg, Wg = grid
    slat, slon = rh.source_lat(Hg), rh.source_lon(Wg)
    rows, cols = [0, 3, Hg // 2, Hg - 1], [Wg - 2, Wg - 1, Wg, Wg + 5]          # the poles; columns across the east edge
    g = Grid(slat[rows], slon[np.array(cols) % Wg] + 360.0 * (np.array(cols) // Wg))
    p = g.plan(Hg, Wg)
    assert p["ntap"].tolist() == [1] * 4 and p["ctap"].tolist() == [1] * 4
    assert p["row0"].tolist() == rows and p["col0"].tolist() == [c % Wg for c in cols]
    assert (p["rw"] == 1.0).all() and (p["cw"] == 1.0).all() and p["rw"].shape == (4, 1)
    full = rh.field(1, Hg, Wg, seed=3)
    got, _ = rh.ref_regrid(full, p)
    assert rh.same_bits(got, full[:, rows][:, :, np.array(cols) % Wg])          # the source value, exactly
    # a point within TOL_DEG of the lattice snaps; one well off it does not
    p2 = Grid([slat[3] + 0.5 * subset.TOL_DEG, slat[5] - 0.3 * (180.0 / (Hg - 1))], [slon[2] - 0.5 * subset.TOL_DEG]).plan(Hg, Wg)
    assert p2["ntap"].tolist() == [1, 2] and p2["row0"].tolist() == [3, 5] and p2["ctap"].tolist() == [1]
    assert p2["col0"].tolist() == [2] and abs(p2["rw"][1, 1] - 0.3) < 1e-12 and abs(p2["rw"][1, 0] - 0.7) < 1e-12


def test_a_south_to_north_grid_gives_the_row_reversed_result():
    Hg, Wg = 25, 40
    full = rh.field(2, Hg, Wg, seed=5, physical=False)
    lat, lon = _random_targets(Hg, Wg, seed=8)
    for method, kw in (("bilinear", {}), ("conservative", {})):
        a = Grid(lat, lon, method, **kw).plan(Hg, Wg)
        b = Grid(lat[::-1].copy(), lon, method, **kw).plan(Hg, Wg)
        ga, gb = rh.ref_regrid(full, a)[0], rh.ref_regrid(full, b)[0]
        assert rh.same_bits(gb, ga[:, ::-1]), method
        assert a["order"].tolist() == list(range(len(lat))) and b["order"].tolist() == list(range(len(lat)))[::-1]
        assert np.array_equal(b["lat_bnds"], a["lat_bnds"][::-1]) and np.array_equal(b["area_weights"], a["area_weights"][::-1])
        # the walk runs north to south: the windows' first rows do not decrease along it
        assert (np.diff(b["row0"][b["order"]]) >= 0).all() and (np.diff(a["row0"][a["order"]]) >= 0).all()


# ---- conservative ------------------------------------------------------------------------------------------------------


CONS = [("eq32", lambda: Grid.equiangular(32, 64, method="conservative"), (721, 1440)),
        ("eq8", lambda: Grid.equiangular(8, 12, method="conservative"), (25, 40)),
        ("reg1.5", lambda: Grid.regular(1.5, 1.5, method="conservative"), (721, 1440)),
        ("gauss", lambda: Grid.gaussian(32, 64, method="conservative"), (721, 1440)),
        ("fine", lambda: Grid.regular(0.1, 0.1, region=(40, 44, -3, 5), method="conservative"), (721, 1440)),
        ("random", lambda: Grid(*_random_targets(25, 40, seed=4), method="conservative"), (25, 40))]


@pytest.mark.parametrize("name, make, grid", CONS, ids=[c[0] for c in CONS])
def test_conservative_weights_are_positive_and_sum_to_one(name, make, grid):
    p = make().plan(*grid)
    for w, n in ((p["rw"], p["ntap"]), (p["cw"], p["ctap"])):
        for i in range(len(n)):
            row = w[i, :n[i]]
            assert n[i] >= 1 and (row > 0).all() and (w[i, n[i]:] == 0).all()
            total = 0.0
            for v in row:
                total = total + v
            assert abs(total - 1.0) <= 4 * 2.0 ** -52, (name, i, total)
    assert p["method"] == "conservative" and p["rw"].dtype == p["cw"].dtype == np.float64
    assert p["row0"].dtype == p["ntap"].dtype == p["col0"].dtype == p["ctap"].dtype == np.int32
    assert p["row0"].min() >= 0 and (p["row0"] + p["ntap"]).max() <= grid[0]
    assert p["col0"].min() >= 0 and p["col0"].max() < grid[1]


@pytest.mark.parametrize("cell, n", [(Fraction(45, 8), 64), (Fraction(3, 2), 240)])
def test_conservative_column_overlaps_are_the_exact_rational_overlaps(cell, n):
    """5.625 deg and 1.5 deg cells against the 0.25 deg source: every edge is a binary fraction, so the float64 overlaps
    must be the exact ones."""
    W = 1440
    g = Grid.regular(float(cell), float(cell), method="conservative")
    assert g.shape == (int(180 / cell), n)
    p = g.plan(721, W)
    d = Fraction(360, W)
    for j in range(n):
        west, east = j * cell, (j + 1) * cell
        exact = []
        for c in range(-2, W + 2):
            ov = min(east, (c + Fraction(1, 2)) * d) - max(west, (c - Fraction(1, 2)) * d)
            if ov > 0:
                exact.append((c % W, ov))
        assert p["ctap"][j] == len(exact)
        assert [(int(p["col0"][j]) + u) % W for u in range(len(exact))] == [c for c, _ in exact]
        assert [Fraction(float(v)) for v in p["cl"][j, :len(exact)]] == [ov for _, ov in exact]
        total = 0.0
        for _, ov in exact:
            total = total + float(ov)
        assert np.array_equal(p["cw"][j, :len(exact)], np.array([float(ov) for _, ov in exact]) / total)
    assert np.array_equal(p["lon_bnds"], np.stack([np.arange(n) * float(cell), (np.arange(n) + 1) * float(cell)], axis=1))


def test_gaussian_cells_tile_pole_to_pole():
    g = Grid.gaussian(32, 64, method="conservative")
    x, w = np.polynomial.legendre.leggauss(32)
    assert np.allclose(g.lat, np.rad2deg(np.arcsin(x))[::-1], rtol=0, atol=1e-12) and (np.diff(g.lat) < 0).all()
    b = g.lat_bnds
    assert b[0, 0] == 90.0 and b[-1, 1] == -90.0 and np.array_equal(b[1:, 0], b[:-1, 1])            # no gap, no overlap
    assert (b[:, 0] > g.lat).all() and (g.lat > b[:, 1]).all()
    area = np.sin(np.deg2rad(b[:, 0])) - np.sin(np.deg2rad(b[:, 1]))
    assert np.allclose(area, w[::-1], rtol=0, atol=1e-14)                                             # the quadrature weights
    p = g.plan()
    assert np.allclose(p["area_weights"], area / area.mean(), rtol=1e-14) and abs(p["area_weights"].mean() - 1) < 1e-15
    assert np.array_equal(g.lon, np.arange(64) * 5.625) and p["src_box"] == (0, 721, 0, 1440)


@pytest.mark.parametrize("name, make, grid", [c for c in CONS if c[0] in ("eq32", "eq8", "reg1.5", "gauss")],
                         ids=["eq32", "eq8", "reg1.5", "gauss"])
def test_conservative_keeps_the_area_integral_on_a_global_target(name, make, grid):
    Hg, Wg = grid
    full = rh.field(1, Hg, Wg, seed=2)
    p = make().plan(Hg, Wg)
    _, got = rh.ref_regrid(full, p)
    A = np.sin(np.deg2rad(p["lat_bnds"][:, 0])) - np.sin(np.deg2rad(p["lat_bnds"][:, 1]))
    L = p["lon_bnds"][:, 1] - p["lon_bnds"][:, 0]
    a = np.array([ch.band_area(*ch.fine_band(h, Hg)) for h in range(Hg)])
    assert abs(A.sum() - 2.0) < 1e-14 and abs(L.sum() - 360.0) < 1e-11
    target = (A[:, None] * L[None, :] * got[0]).sum()
    source = (a[:, None] * (360.0 / Wg) * full[0].astype(np.float64)).sum()
    assert abs(target - source) <= 1e-12 * abs(source), (target, source)


@pytest.mark.parametrize("grid, k, box", [((25, 40), (4, 4), None), ((25, 40), (6, 5), (3, 22, 30, 25)), ((13, 24), (3, 8), None),
                                          ((721, 1440), (6, 6), (100, 160, 1400, 90))])
def test_conservative_on_coarsen_plans_own_cells_equals_the_coarsening(grid, k, box):
    """Two float64 evaluations of one real number: |a - b| <= (ntap + ctap + 3) 2^-52 sum |w| |x| per point."""
    Hg, Wg = grid
    full = rh.field(2, Hg, Wg, seed=11, physical=False)
    cp = subset.coarsen_plan(box, k, Hg, Wg)
    lat = 90.0 - cp["rows"] * (180.0 / (Hg - 1))
    lon = cp["cols"].astype(np.float64) * (360.0 / Wg)
    lon = lon + 360.0 * (np.cumsum(np.concatenate([[0], np.diff(lon) < 0])))             # eastward, not wrapped
    lb = cp["lon_bnds"] + (lon - cp["lon_bnds"].mean(axis=1)).round()[:, None]
    p = Grid(lat, lon, "conservative", cp["lat_bnds"], lb).plan(Hg, Wg)
    assert np.array_equal(p["row0"], cp["row0"]) and np.array_equal(p["ntap"], cp["ntap"]) and p["src_box"] == cp["src_box"]
    _, got = rh.ref_regrid(full, p)
    # the coarsening from the helper's own inputs (coarsen_helpers.rw_table and the half-weight edge columns), in float64
    rows, cols = ch.kept(box, k, Hg, Wg)
    row0, ntap, rw = ch.rw_table(rows, k[0], k[1], Hg)
    half = k[1] // 2
    ov = np.ones(2 * half + 1)
    if k[1] % 2 == 0 and half:
        ov[0] = ov[-1] = 0.5
    x = full.astype(np.float64)
    ref = np.zeros_like(got)
    for i in range(len(rows)):
        for t in range(ntap[i]):
            inner = np.zeros((2, len(cols)))
            for j in range(-half, half + 1):
                inner = inner + ov[j + half] * x[:, row0[i] + t, (cols + j) % Wg]
            ref[:, i] = ref[:, i] + rw[i, t] * inner
    bound = (p["ntap"][None, :, None] + p["ctap"][None, None, :] + 3) * 2.0 ** -52 * rh.abs_regrid(full, p)
    assert (np.abs(got - ref) <= bound).all(), float((np.abs(got - ref) / bound).max())
    assert rh.same_bits(ch.ref_coarsen(full, k, box), ref.astype(np.float32))               # (the helper's own result)


# ---- the constructors, the plan's geometry, the refusals ----------------------------------------------------------------


def test_constructors():
    g = Grid.equiangular(32, 64)
    assert g.shape == (32, 64) and g.lat[0] == -87.1875 and g.lat[-1] == 87.1875 and g.lon[0] == 2.8125 and g.method == "bilinear"
    assert Grid.equiangular(64, 128).lat[0] == -88.59375
    gp = Grid.equiangular(121, 240, poles=True)
    assert gp.lat[0] == -90.0 and gp.lat[-1] == 90.0 and gp.lat[1] == -88.5 and gp.lon[1] == 1.5
    r = Grid.regular(0.5, 0.5, method="conservative")
    assert r.shape == (360, 720) and r.lat[0] == 89.75 and r.lat[-1] == -89.75 and r.lon[0] == 0.25 and r.lon[-1] == 359.75
    assert r.lat_bnds[0].tolist() == [90.0, 89.5] and r.lat_bnds[-1].tolist() == [-89.5, -90.0]
    b = Grid.regular(0.1, 0.1, region=(40, 50, -5, 10))
    assert b.shape == (100, 150) and abs(b.lat[0] - 49.95) < 1e-12 and abs(b.lon[0] + 4.95) < 1e-12
    assert Grid.regular(1, 1, region=(-10, 10, 350, 10)).shape == (20, 20)                   # across 0 deg
    # default cells: midpoints, the end cells mirrored, clipped at the poles; a uniform closed circle wraps
    d = Grid([80.0, 60.0, 50.0], [0.0, 120.0, 240.0], "conservative")
    assert d.lat_bnds.tolist() == [[90.0, 70.0], [70.0, 55.0], [55.0, 45.0]]
    assert d.lon_bnds.tolist() == [[-60.0, 60.0], [60.0, 180.0], [180.0, 300.0]] and d.closes_circle
    e = Grid([0.0, -10.0], [10.0, 20.0, 40.0], "conservative")
    assert e.lon_bnds.tolist() == [[5.0, 15.0], [15.0, 30.0], [30.0, 50.0]] and not e.closes_circle
    assert Grid([89.0, 80.0], [0.0, 1.0]).lat_bnds[0].tolist() == [90.0, 84.5]
    assert g == Grid.equiangular(32, 64) and g != Grid.equiangular(32, 64, method="conservative") and hash(g) == hash(Grid.equiangular(32, 64))
    assert g.plan() is g.plan(721, 1440) and as_plan(g, 721, 1440) is g.plan() and as_plan(g.plan(), 721, 1440) is g.plan()


@pytest.mark.parametrize("kw", [
    dict(lat=[0.0, np.nan], lon=[0.0]), dict(lat=[0.0], lon=[np.inf]), dict(lat=[[0.0]], lon=[0.0]), dict(lat=0.0, lon=[0.0]),
    dict(lat=[True, False], lon=[0.0]), dict(lat="12", lon=[0.0]), dict(lat=["a"], lon=[0.0]), dict(lat=[], lon=[0.0]),
    dict(lat=[0.0], lon=[]), dict(lat=[0.0, 1.0, 0.5], lon=[0.0]), dict(lat=[0.0, 0.0], lon=[0.0]), dict(lat=[91.0], lon=[0.0]),
    dict(lat=[0.0], lon=[10.0, 5.0]), dict(lat=[0.0], lon=[0.0, 0.0]), dict(lat=[0.0], lon=[0.0, 200.0, 360.0]),
    dict(lat=[0.0], lon=[0.0, 361.0]), dict(lat=[0.0], lon=[0.0], method="nearest"), dict(lat=[0.0], lon=[0.0], method=None),
    dict(lat=[1.0, 0.0], lon=[0.0, 1.0], lat_bnds=np.zeros((3, 2))), dict(lat=[1.0, 0.0], lon=[0.0, 1.0], lon_bnds=np.zeros(2)),
    dict(lat=[1.0, 0.0], lon=[0.0, 1.0], lat_bnds=[[2, 0.5], [0.5, np.nan]]),
    dict(lat=[1.0], lon=[0.0, 1.0], method="conservative"), dict(lat=[1.0, 0.0], lon=[0.0], method="conservative"),
    dict(lat=[0.0], lon=[0.0], method="conservative", lat_bnds=[[1, -1]], lon_bnds=[[-200.0, 200.0]]),       # wider than 360
    dict(lat=[0.0], lon=[0.0], method="conservative", lat_bnds=[[3, 1]], lon_bnds=[[-1.0, 1.0]]),           # centre outside
])
def test_grid_refuses(kw):
    with pytest.raises(ValueError):
        Grid(**kw)


def test_constructors_and_plans_refuse():
    for bad in [(0, 4), (4, 0), (2.5, 4), (True, 4), ("4", 4)]:
        with pytest.raises(ValueError):
            Grid.equiangular(*bad)
        with pytest.raises(ValueError):
            Grid.gaussian(*bad)
    for args in [(0.7, 1.0), (1.0, 0.7), (0, 1), (1, -1), (1, 1, (10, 5, 0, 10)), (1, 1, (0, 100, 0, 10)), ("x", 1)]:
        with pytest.raises(ValueError):
            Grid.regular(*args)
    with pytest.raises(ValueError):
        Grid.equiangular(1, 4, poles=True)
    g = Grid.equiangular(4, 8)
    with pytest.raises(ValueError, match="source grid"):
        g.plan(1, 8)
    with pytest.raises(ValueError, match="regrid must be"):
        as_plan((4, 8), 13, 24)
    with pytest.raises(ValueError, match="built for"):
        as_plan(g.plan(13, 24), 25, 40)
    # a column whose window is wider than the kernel's column-weight budget
    wide = Grid([0.0], [0.0], "conservative", lat_bnds=[[10, -10]], lon_bnds=[[-30.0, 30.0]]).plan(721, 1440)
    assert wide["ctap"].tolist() == [241]
    with pytest.raises(ValueError, match="at most 64"):
        tile_table(wide)


def test_src_box_is_the_hull_and_the_whole_circle_when_the_span_closes():
    Hg, Wg = 25, 40                                     # 7.5 deg rows, 9 deg columns
    p = Grid([40.0, 10.0], [350.0, 365.0, 380.0]).plan(Hg, Wg)           # rows 6.67 .. 10.67; columns 38.9 .. 42.2
    assert p["src_box"] == (6, 12, 38, 6) and p["col0"].tolist() == [38, 0, 2] and p["ucol0"].tolist() == [38, 40, 42]
    assert p["row0"].tolist() == [6, 10] and p["ntap"].tolist() == [2, 2]
    c = Grid([40.0, 10.0], [350.0, 380.0], "conservative").plan(Hg, Wg)  # cells 335 .. 365 .. 395, 55 .. 25 .. -5
    # rows: cell edges 93.75 - 7.5 h -> rows 5 .. 9 and 9 .. 13; columns: cell edges 9 c - 4.5 -> columns 37 .. 41 and 41 .. 44
    assert c["src_box"] == (5, 14, 37, 8) and c["ctap"].tolist() == [5, 4] and c["ntap"].tolist() == [5, 5]
    assert c["row0"].tolist() == [5, 9] and c["col0"].tolist() == [37, 1]
    one = Grid([90.0], [0.0]).plan(Hg, Wg)
    assert one["src_box"] == (0, 1, 0, 1) and one["Ho"] == one["Wo"] == 1
    for g in (Grid.equiangular(8, 12, method="conservative"), Grid([0.0], np.arange(40) * 9.0 + 4.0),
              Grid([0.0], np.arange(40) * 9.0 - 100.0)):
        assert g.plan(Hg, Wg)["src_box"][2:] == (0, Wg), g
    assert Grid.equiangular(8, 12).plan(Hg, Wg)["src_box"][2:] == (1, 39)                    # 15 .. 345 deg: columns 1 .. 39
    assert Grid([0.0], np.arange(39) * 9.0).plan(Hg, Wg)["src_box"][2:] == (0, 39)          # one column short of the circle
    assert Grid.equiangular(8, 12).plan(Hg, Wg)["src_box"][:2] == (1, 24) and Grid.equiangular(8, 12, method="conservative").plan(Hg, Wg)["src_box"][:2] == (0, 25)


def test_tile_table_covers_every_column_within_the_budgets():
    for g, grid in [(Grid.equiangular(32, 64, method="conservative"), (721, 1440)), (Grid.regular(0.1, 0.1, region=(40, 44, -3, 50)), (721, 1440)),
                    (Grid.equiangular(721, 1440, poles=True), (721, 1440)), (Grid(*_random_targets(7, 1440, seed=1, Wo=700)), (7, 1440))]:
        p = g.plan(*grid)
        for kw in ({}, dict(max_cols=7, span_max=100)):
            tiles, tc, ms = tile_table(p, **kw)
            assert tiles.dtype == np.int32 and tiles[0, 0] == 0 and tiles[:, 1].sum() == p["Wo"]
            assert np.array_equal(tiles[1:, 0], np.cumsum(tiles[:-1, 1])) and tc == tiles[:, 1].max() and ms == tiles[:, 3].max()
            assert tc <= kw.get("max_cols", 256) and tc * p["cw"].shape[1] <= 4096 and ms <= kw.get("span_max", 7936) and ms <= 2 * grid[1]
            for j0, n, first, span in tiles:
                off = (p["col0"][j0:j0 + n] - first) % grid[1]
                assert (off + p["ctap"][j0:j0 + n] <= span).all() and off.min() == 0


# ---- the Selection record of the decode methods (no GPU: cra5_api._select is host logic) -------------------------------


def test_select_record_with_regrid():
    from cra5_amd import synth
    from cra5_amd.api import cra5_api
    from cra5_amd.vaeformer import VAEformer
    api = cra5_api(device="cpu", weights=VAEformer(0, **synth.thin_model_kwargs()))
    g = Grid.equiangular(32, 64, method="conservative")
    plan = g.plan(721, 1440)
    for arg in (g, plan):
        sel = api._select(["z_850", "z_1000"], regrid=arg)
        assert sel.regrid is plan and (sel.box, sel.step, sel.coarsen) == (None, None, None) and sel.channels == (6, 0)
        assert sel.model == dict(channels=(6, 0), box=None, step=None, coarsen=None, regrid=plan)
        assert sel.shape == (2, 32, 64) == api.net._decoded_shape(sel.channels, regrid=plan) and not sel.whole
        assert list(sel.meta) == ["variables", "lat", "lon", "regrid", "lat_bnds", "lon_bnds"]
        assert sel.meta["regrid"] == "conservative" and sel.meta["lat"] is plan["lat"] and sel.meta["lon_bnds"] is plan["lon_bnds"]
    # without regrid= nothing changes: no key in the model's arguments, none in the result dicts
    assert api._select().regrid is None and "regrid" not in api._select().model and "regrid" not in api._select(coarsen=6).meta
    for kw, msg in ((dict(region=(35, 72, -25, 45)), "regrid and region"), (dict(stride=6), "regrid and stride"),
                    (dict(coarsen=(6, 4)), "regrid and coarsen")):
        with pytest.raises(ValueError, match=msg):
            api._select(regrid=g, **kw)
    for kw, msg in ((dict(box=(0, 100, 0, 100)), "regrid and box"), (dict(step=6), "regrid and step"), (dict(coarsen=6), "regrid and coarsen")):
        with pytest.raises(ValueError, match=msg):
            api.net._selection_args(regrid=g, **kw)
    for bad in ((32, 64), "wb", g.plan(13, 24)):
        with pytest.raises(ValueError, match="regrid"):
            api._select(regrid=bad)
    assert api._select(regrid=g, stride=1, coarsen=(1, 1)).regrid is plan            # the no-op spellings are no conflict
    with pytest.raises(ValueError, match="residual= with regrid="):
        api._residual_arg("decode_batch", True, ["x.bin"], "de_normalized", None, plan)
