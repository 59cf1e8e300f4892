"""Point decode, host geometry (cra5_amd/points.py): validation, the taps against regrid.Grid, the node -> (token, ky, kx)
mapping against a brute-force footprint, the token list, nearest's rounding.  No GPU."""
import numpy as np
import pytest

from cra5_amd.points import Points, as_plan, as_points
from cra5_amd.regrid import Grid

H, W = 721, 1440
HP, WP = 72, 144


def _special():
    """(lat, lon): on-lattice, both poles, a seam row, the last cell, negative and large longitudes, within TOL_DEG."""
    return np.array([(90.0, 0.0), (-90.0, 123.4), (0.0, 0.0), (0.0, 359.9), (45.0, -0.1), (12.3456, 359.99), (89.999, 720.3),
                     (-89.876, -359.875), (10.0, 10.0 + 5e-10), (10.0 - 5e-10, 250.0), (87.625, 2.375), (0.125, 359.875),
                     (33.3, 180.0), (-45.25, 1e-12)])


def test_validation_errors():
    ok = ([10.0, 20.0], [5.0, 6.0])
    Points(*ok)
    Points([10], [5], "nearest")           # integers are real numbers
    for lat, lon in [([], []), ([10.0], [5.0, 6.0]), ([91.0], [0.0]), ([-90.0001], [0.0]), ([np.nan], [0.0]),
                     ([0.0], [np.inf]), ([[0.0]], [[0.0]]), ("ab", [0.0, 1.0]), ([True], [0.0]), (None, [0.0]),
                     ([0.0], ["x"]), ([0j], [0.0])]:
        with pytest.raises(ValueError, match="Points"):
            Points(lat, lon)
    for m in ("linear", None, 1, "conservative"):
        with pytest.raises(ValueError, match="method"):
            Points(*ok, method=m)
    for bad in ("abc", None, [1.0, 2.0], [[1.0, 2.0, 3.0]], [[True, False]], {"lat": 1}):
        with pytest.raises(ValueError, match="points"):
            as_points(bad)
    with pytest.raises(ValueError, match="lat must lie"):
        as_points([[100.0, 0.0]])
    with pytest.raises(ValueError, match="geometry"):
        Points(*ok).plan(H, W, 10, 10, 10, 10)
    with pytest.raises(ValueError, match="tile"):
        Points(*ok).plan(720, W)


def test_key_hash_and_array_form():
    a, b = Points([1.0, 2.0], [3.0, 4.0]), Points(np.array([1.0, 2.0]), (3.0, 4.0))
    assert a == b and hash(a) == hash(b) and len({a, b}) == 1
    assert a != Points([1.0, 2.0], [3.0, 4.0], "nearest") and a != Points([2.0, 1.0], [4.0, 3.0])
    c = as_points([[1.0, 3.0], [2.0, 4.0]])
    assert c == a and c.method == "bilinear" and as_points(a) is a
    p = as_plan([[1.0, 3.0], [2.0, 4.0]], H, W)
    assert p["key"] == a.plan()["key"] and as_plan(p, H, W) is p
    with pytest.raises(ValueError, match="plan was built"):
        as_plan(a.plan(31, 1440), H, W)
    lon = Points([0.0, 0.0, 0.0], [-0.1, 720.5, -1e-17]).lon
    assert np.array_equal(lon, np.mod([-0.1, 720.5, 0.0], 360.0)) and (lon >= 0).all() and (lon < 360).all()


def test_bilinear_taps_are_grids():
    rng = np.random.default_rng(0)
    pts = np.concatenate([_special(), np.stack([rng.uniform(-90, 90, 300), rng.uniform(-400, 800, 300)], axis=1)])
    for Hg, Wg in ((H, W), (31, 40)):
        t = Points(pts[:, 0], pts[:, 1]).taps(Hg, Wg)
        assert t["P"] == len(pts) and t["rows"].dtype == np.int32 and t["rw"].dtype == np.float64
        for p, (lat, lon) in enumerate(pts):
            g = Grid([lat], [lon], "bilinear").plan(Hg, Wg)
            nt, nu = int(g["ntap"][0]), int(g["ctap"][0])
            assert (t["row0"][p], t["ntap"][p], t["col0"][p], t["ctap"][p]) == (g["row0"][0], nt, g["col0"][0], nu), (lat, lon)
            assert np.array_equal(t["rw"][p, :nt].view(np.int64), g["rw"][0, :nt].view(np.int64)) and (t["rw"][p, nt:] == 0).all()
            assert np.array_equal(t["cw"][p, :nu].view(np.int64), g["cw"][0, :nu].view(np.int64)) and (t["cw"][p, nu:] == 0).all()
            assert list(t["rows"][p]) == [g["row0"][0], g["row0"][0] + 1 if nt == 2 else -1]
            assert list(t["cols"][p]) == [g["col0"][0], (g["col0"][0] + 1) % Wg if nu == 2 else -1]
    # the special points do what their names say
    t = Points(_special()[:, 0], _special()[:, 1]).taps(H, W)
    assert list(t["rows"][0]) == [0, -1] and list(t["rows"][1]) == [720, -1] and list(t["rows"][2]) == [360, -1]
    assert list(t["cols"][3]) == [1439, 0] and list(t["cols"][4]) == [1439, 0] and list(t["cols"][7]) == [0, 1]
    assert list(t["rows"][8]) == [320, -1] and list(t["cols"][8]) == [40, -1] and list(t["rows"][9]) == [320, -1]


def test_node_to_token_mapping_against_brute_force():
    """All 721 rows x columns {0, 9, 10, 1439}: token row ti covers rows 10 ti .. 10 ti + 10, token column tj covers columns
    10 tj .. 10 tj + 9."""
    cols = [0, 9, 10, 1439]
    rr, cc = np.meshgrid(np.arange(H), cols, indexing="ij")
    pts = Points(90.0 - rr.ravel() * 0.25, cc.ravel() * 0.25, "nearest")
    p = pts.plan(H, W)
    assert p["tokens_grid"] == (HP, WP) and p["patch"] == (11, 10, 10, 10)
    assert np.array_equal(p["rows"][:, 0], rr.ravel()) and np.array_equal(p["cols"][:, 0], cc.ravel())
    assert len(p["nodes"]) == H * len(cols) and np.array_equal(p["pnode"][:, 0], np.arange(H * len(cols)))
    assert (p["pnode"][:, 1:] == -1).all()
    tok = p["tokens"]
    assert tok.dtype == np.int32 and np.array_equal(tok, np.unique(tok))
    assert np.array_equal(tok, np.array([ti * WP + tj for ti in range(HP) for tj in (0, 1, 143)]))
    for n, (r, c) in enumerate(p["nodes"]):
        cover = [(ti, r - 10 * ti) for ti in range(HP) if 10 * ti <= r <= 10 * ti + 10]       # north to south
        tj = [t for t in range(WP) if 10 * t <= c <= 10 * t + 9]
        assert len(tj) == 1 and len(cover) == (2 if r % 10 == 0 and 0 < r < 720 else 1), (r, c)
        m0, tap0, m1, tap1 = (int(v) for v in p["contrib"][n])
        kx = c - 10 * tj[0]
        assert (tok[m0], tap0) == (cover[0][0] * WP + tj[0], cover[0][1] * 10 + kx), (r, c)
        if len(cover) == 2:
            assert cover[0][1] == 10 and (tok[m1], tap1) == (cover[1][0] * WP + tj[0], kx), (r, c)    # the upper partner first
        else:
            assert m1 == -1, (r, c)
    # rows 0 and 720: one contribution
    first, last = p["contrib"][0], p["contrib"][-1]
    assert first[2] == -1 and first[1] // 10 == 0 and last[2] == -1 and last[1] // 10 == 10


def test_duplicates_share_nodes_and_order_is_kept():
    lat = [10.1, -33.3, 10.1, 90.0, 10.1]
    lon = [20.2, 100.0, 20.2, 5.0, 380.2]
    p = Points(lat, lon).plan(H, W)
    assert np.array_equal(p["lat"], lat) and np.allclose(p["lon"], [20.2, 100.0, 20.2, 5.0, 20.2])
    assert np.array_equal(p["pnode"][0], p["pnode"][2]) and (p["pnode"][0] >= 0).all()
    assert np.array_equal(p["rows"][0], p["rows"][4])
    nodes = [tuple(v) for v in p["nodes"]]
    assert nodes == sorted(set(nodes)) and len(nodes) == len(set(p["pnode"][p["pnode"] >= 0]))
    assert list(p["pnode"][3]) == [nodes.index((0, 20)), -1, -1, -1]
    assert np.array_equal(p["tokens"], np.unique(p["tokens"]))
    for q in range(len(lat)):
        for e, n in enumerate(p["pnode"][q]):
            if n >= 0:
                assert tuple(p["nodes"][n]) == (p["rows"][q, e // 2], p["cols"][q, e % 2])
    # a bilinear point at grid coordinates (9.5, 9.5): four nodes, two token rows (row 10 is a seam), two token columns
    q = Points([90.0 - 9.5 * 0.25], [9.5 * 0.25]).plan(H, W)
    assert [tuple(v) for v in q["nodes"]] == [(9, 9), (9, 10), (10, 9), (10, 10)]
    assert list(q["tokens"]) == [0, 1, WP, WP + 1]
    assert [list(v) for v in q["contrib"]] == [[0, 99, -1, 0], [1, 90, -1, 0], [0, 109, 2, 9], [1, 100, 3, 0]]
    assert np.array_equal(q["rw"], [[0.5, 0.5]]) and np.array_equal(q["cw"], [[0.5, 0.5]])


def test_nearest_ties_and_wrap():
    lat = 90.0 - np.array([0.5, 1.5, 2.5, 3.49, 719.5]) * 0.25      # ties go to the even row
    lon = np.array([0.5, 1.5, 2.5, 1439.5, 1438.5]) * 0.25
    t = Points(lat, lon, "nearest").taps(H, W)
    assert list(t["rows"][:, 0]) == [0, 2, 2, 3, 720] and list(t["cols"][:, 0]) == [0, 2, 2, 0, 1438]
    assert list(t["rows"][:, 0]) == [int(v) for v in np.rint((90.0 - lat) / 0.25)]
    t = Points([0.0, 0.0, 0.0], [359.9, -0.1, 359.8], "nearest").taps(H, W)
    assert list(t["cols"][:, 0]) == [0, 0, 1439] and (t["cols"][:, 1] == -1).all() and (t["rw"][:, 0] == 1).all()
    assert np.array_equal(t["node_lon"], [0.0, 0.0, 359.75]) and np.array_equal(t["node_lat"], [0.0, 0.0, 0.0])
    assert "node_lat" not in Points([0.0], [0.0]).taps(H, W)
