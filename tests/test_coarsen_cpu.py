"""Geometry of the area-weighted coarsening (cra5_amd.subset: resolve_coarsen, coarsen_plan, grid_box(coarsen=)), host
only, against the independent numpy restatement of the definition in tests/coarsen_helpers.py."""
import numpy as np
import pytest

import coarsen_helpers as ch
from cra5_amd import _lib, subset

H, W = 721, 1440
KS = [(2, 2), (3, 3), (4, 4), (5, 5), (6, 6), (8, 8), (10, 10), (24, 24), (12, 8), (2, 3)]
GRIDS = [(13, 24), (25, 40), (7, 1440), (721, 1440)]


def _ks(Hg, Wg):
    return [k for k in KS + [(1, 4), (6, 1)] if (Hg - 1) % k[0] == 0 and Wg % k[1] == 0]


@pytest.mark.parametrize("grid", GRIDS)
def test_plan_tables_equal_the_helper_bit_for_bit(grid):
    Hg, Wg = grid
    for k in _ks(Hg, Wg):
        p = subset.coarsen_plan(None, k, Hg, Wg)
        rows, cols = ch.kept(None, k, Hg, Wg)
        row0, ntap, rw = ch.rw_table(rows, k[0], k[1], Hg)
        assert np.array_equal(p["rows"], rows) and np.array_equal(p["cols"], cols)
        assert np.array_equal(p["row0"], row0) and np.array_equal(p["ntap"], ntap)
        assert p["rw"].dtype == np.float64 and p["rw"].shape == (len(rows), k[0] + 1)
        assert np.array_equal(p["rw"].view(np.int64), rw.view(np.int64)), (grid, k)
        # k_lat + 1 rows for an even k_lat, k_lat for an odd one; fewer at the poles
        n_full = k[0] + 1 if k[0] % 2 == 0 else k[0]
        assert (ntap[1:-1] == n_full).all() and ntap[0] == ntap[-1] == k[0] // 2 + 1
        assert p["row0"].dtype == np.int32 and p["ntap"].dtype == np.int32


@pytest.mark.parametrize("k", KS)
def test_weights_partition_the_fine_cells_and_conserve_the_integral(k):
    p = subset.coarsen_plan(None, k, H, W)
    ky, kx = k
    # un-normalised row weights V[R, h]: every fine band is split among the coarse bands without loss
    share = np.zeros(H)
    A = np.array([ch.band_area(*b) for b in p["lat_bnds"]])
    a = np.array([ch.band_area(*ch.fine_band(h, H)) for h in range(H)])
    for i in range(p["Ho"]):
        n = p["ntap"][i]
        V = p["rw"][i, :n] * kx
        assert abs(V.sum() - 1.0) <= 4e-16 * n                    # normalised: a constant field is preserved
        share[p["row0"][i]:p["row0"][i] + n] += V * A[i]
    assert np.abs(share - a).max() <= 1e-15
    # column overlaps: every fine column is shared out exactly
    half = kx // 2
    ov = np.ones(2 * half + 1)
    if kx % 2 == 0 and half:
        ov[0] = ov[-1] = 0.5
    tot = np.zeros(W)
    for c in p["cols"]:
        tot[(c + np.arange(-half, half + 1)) % W] += ov
    assert np.array_equal(tot, np.ones(W))
    # the global integral: sum_R A_R sum_c out[R, c] k_lon == sum_h a_h sum_w x[h, w]
    rng = np.random.default_rng(k[0] * 100 + k[1])
    x = (5e4 + 1e4 * rng.standard_normal((1, H, W))).astype(np.float32)
    out = ch.ref_coarsen(x, k)
    lhs = float((A[:, None] * out[0].astype(np.float64)).sum() * kx)
    rhs = float((a[:, None] * x[0].astype(np.float64)).sum())
    assert abs(lhs - rhs) <= 2e-7 * abs(rhs)          # out is rounded to fp32 per point: 6e-8 relative each, same sign at worst
    # in float64 (before the final rounding) the identity holds to rounding
    o64 = np.zeros((p["Ho"], p["Wo"]))
    for i in range(p["Ho"]):
        for t in range(p["ntap"][i]):
            row = x[0, p["row0"][i] + t].astype(np.float64)
            inner = sum(ov[j + half] * row[(p["cols"] + j) % W] for j in range(-half, half + 1))
            o64[i] += p["rw"][i, t] * inner
    assert abs(float((A[:, None] * o64).sum() * kx) - rhs) <= 1e-14 * abs(rhs)
    const = np.full((1, H, W), 287.65, dtype=np.float32)
    got = ch.ref_coarsen(const, k)
    assert np.abs(got.astype(np.float64) - np.float64(const[0, 0, 0])).max() <= np.spacing(np.float32(287.65))


@pytest.mark.parametrize("k", [(2, 2), (3, 3), (6, 6), (24, 24), (12, 8)])
def test_bounds_tile_the_sphere(k):
    p = subset.coarsen_plan(None, k, H, W)
    lb, ob = p["lat_bnds"], p["lon_bnds"]
    assert lb[0, 0] == 90.0 and lb[-1, 1] == -90.0 and np.array_equal(lb[1:, 0], lb[:-1, 1]) and (lb[:, 0] > lb[:, 1]).all()
    assert np.array_equal(ob[1:, 0], ob[:-1, 1]) and ob[-1, 1] - ob[0, 0] == 360.0
    lat = 90.0 - p["rows"] * (180.0 / (H - 1))
    assert np.allclose(lat[1:-1], lb[1:-1].mean(axis=1), atol=1e-12) and lb[0, 1] == 90.0 - k[0] * 0.125
    assert np.array_equal(ob.mean(axis=1), p["cols"] * 0.25)


BOXES = [(72, 221, 1340, 281), (0, 40, 100, 300), (650, 721, 7, 90), (123, 456, 1437, 7), (360, 361, 720, 1),
         (200, 260, 1, 1440), (0, 721, 720, 1440)]


@pytest.mark.parametrize("k", [(2, 2), (5, 5), (6, 6), (8, 10), (6, 1), (1, 6)])
def test_region_plan_is_the_sub_block_of_the_globes_and_source_box_is_the_hull(k):
    g = subset.coarsen_plan(None, k, H, W)
    gi = {int(r): i for i, r in enumerate(g["rows"])}
    gj = {int(c): j for j, c in enumerate(g["cols"])}
    assert g["src_box"] == (0, H, 0, W)
    for box in BOXES:
        try:
            rows, cols = subset.kept_points(box, k, W)
        except ValueError:
            with pytest.raises(ValueError):
                subset.coarsen_plan(box, k, H, W)
            continue
        p = subset.coarsen_plan(box, k, H, W)
        assert np.array_equal(p["rows"], rows) and np.array_equal(p["cols"], cols)
        ii, jj = [gi[int(r)] for r in rows], [gj[int(c)] for c in cols]
        for key in ("row0", "ntap", "rw", "lat_bnds"):
            assert np.array_equal(p[key], g[key][ii]), (k, box, key)
        assert np.array_equal(p["lon_bnds"], g["lon_bnds"][jj])
        sr0, sr1, sc0, snc = p["src_box"]
        assert sr0 == max(0, rows[0] - k[0] // 2) and sr1 == min(H - 1, rows[-1] + k[0] // 2) + 1
        assert sr0 == p["row0"].min() and sr1 == (p["row0"] + p["ntap"]).max()
        span = (len(cols) - 1) * k[1] + 2 * (k[1] // 2) + 1
        if span >= W:
            assert (sc0, snc) == (0, W)
        else:
            assert (sc0, snc) == ((cols[0] - k[1] // 2) % W, span)
            assert (sc0 + snc - 1) % W == (cols[-1] + k[1] // 2) % W
    # clipped at the poles, wrapped across 0 deg, whole circle when the hull closes
    assert subset.coarsen_plan((0, 40, 100, 300), (6, 6), H, W)["src_box"][:2] == (0, 40)
    assert subset.coarsen_plan((650, 721, 7, 90), (6, 6), H, W)["src_box"][:2] == (651, 721)
    assert subset.coarsen_plan((72, 221, 1340, 281), (6, 6), H, W)["src_box"] == (69, 220, 1341, 283)
    assert subset.coarsen_plan((200, 260, 1, 1440), (6, 6), H, W)["src_box"] == (201, 262, 0, W)
    assert subset.coarsen_plan((100, 130, 4, 1436), (6, 6), H, W)["src_box"][2:] == (3, 1435)   # 239 cells: not closed


def test_identity_in_one_dimension():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, 13, 24)).astype(np.float32)
    lon_only = ch.ref_coarsen(x, (1, 6))
    p = subset.coarsen_plan(None, (1, 6), 13, 24)
    assert (p["ntap"] == 1).all() and np.array_equal(p["row0"], np.arange(13)) and np.allclose(p["rw"][:, 0], 1 / 6, rtol=4e-16, atol=0)
    ref = np.zeros((2, 13, 4))
    for j in range(-3, 4):
        ref = ref + (0.5 if abs(j) == 3 else 1.0) * x[:, :, (np.arange(0, 24, 6) + j) % 24].astype(np.float64)
    assert np.array_equal(lon_only, (p["rw"][:, 0][None, :, None] * ref).astype(np.float32))
    # (6, 1): the identity in longitude - every column is its own row-weighted sum, one column in, weight 1
    lat_only = ch.ref_coarsen(x, (6, 1))
    q = subset.coarsen_plan(None, (6, 1), 13, 24)
    assert lat_only.shape == (2, 3, 24) and np.array_equal(q["cols"], np.arange(24)) and q["src_box"] == (0, 13, 0, 24)
    assert np.array_equal(q["row0"], [0, 3, 9]) and np.array_equal(q["ntap"], [4, 7, 4])
    x64 = x.astype(np.float64)
    for i in range(3):
        acc = np.zeros((2, 24))
        for t in range(q["ntap"][i]):
            acc = acc + q["rw"][i, t] * (0.0 + 1.0 * x64[:, q["row0"][i] + t, :])
        assert np.array_equal(lat_only[:, i], acc.astype(np.float32)), i
        assert abs(q["rw"][i, :q["ntap"][i]].sum() - 1.0) <= 4e-16 * q["ntap"][i]       # k_lon = 1: the weights alone sum to 1
    both = ch.ref_coarsen(x, (6, 6))
    assert both.shape == (2, 3, 4)
    assert subset.coarsen_plan(None, (6, 1), 13, 24)["lon_bnds"][1].tolist() == [7.5, 22.5]


def test_resolve_coarsen():
    assert subset.resolve_coarsen(None) is None and subset.resolve_coarsen(1) is None and subset.resolve_coarsen((1, 1)) is None
    assert subset.resolve_coarsen(6) == (6, 6) and subset.resolve_coarsen((6, 1)) == (6, 1)
    assert subset.resolve_coarsen(np.int64(4)) == (4, 4) and subset.resolve_coarsen([2, 3]) == (2, 3)
    assert subset.resolve_coarsen(12, 13, 24) == (12, 12)
    for bad in (0, -1, (2, 0), 2.5, "2", (2, 2, 2), True, (2, False), (6,)):
        with pytest.raises(ValueError, match="coarsen"):
            subset.resolve_coarsen(bad)
    with pytest.raises(ValueError, match=r"\(721 - 1\) % k_lat \(7\)"):
        subset.resolve_coarsen(7)
    with pytest.raises(ValueError, match=r"1440 % k_lon \(7\)"):
        subset.resolve_coarsen((6, 7))
    with pytest.raises(ValueError, match=r"k_lat \(32\)"):
        subset.resolve_coarsen((32, 32))          # 1440 % 32 == 0 but 720 % 32 != 0
    with pytest.raises(ValueError, match="coarsen"):
        subset.coarsen_plan(None, (7, 6), H, W)
    with pytest.raises(ValueError, match="no row"):
        subset.coarsen_plan((1, 5, 0, 40), (6, 6), H, W)


def test_grid_box_coarsen_and_stride_are_exclusive():
    g = subset.grid_box((-90, 90, 0, 360), coarsen=6)
    s = subset.grid_box((-90, 90, 0, 360), stride=6)
    assert len(g["lat"]) == 121 and len(g["lon"]) == 240 and g["lat"][0] == 90.0 and g["lat"][-1] == -90.0
    assert np.array_equal(g["lat"], s["lat"]) and np.array_equal(g["lon"], s["lon"]) and g["box"] == s["box"]
    assert g["coarsen"] == (6, 6) and "stride" not in g
    assert g["lat_bnds"].shape == (121, 2) and g["lon_bnds"].shape == (240, 2)
    assert g["lat_bnds"][1].tolist() == [89.25, 87.75] and g["lon_bnds"][0].tolist() == [-0.75, 0.75]
    assert np.array_equal(g["kept_rows"], s["kept_rows"]) and np.array_equal(g["kept_cols"], s["kept_cols"])
    r = subset.grid_box((35, 72, -25, 45), coarsen=(6, 4))
    rs = subset.grid_box((35, 72, -25, 45), stride=(6, 4))
    assert np.array_equal(r["lat"], rs["lat"]) and np.array_equal(r["lon"], rs["lon"]) and r["lon_bnds"][0].tolist() == [334.5, 335.5]
    assert "coarsen" not in subset.grid_box((35, 72, -25, 45), coarsen=1)
    with pytest.raises(ValueError, match="one of the two"):
        subset.grid_box((-90, 90, 0, 360), stride=6, coarsen=6)
    with pytest.raises(ValueError, match="one of the two"):
        subset.grid_box((-90, 90, 0, 360), stride=(1, 2), coarsen=(6, 1))
    assert "stride" in subset.grid_box((-90, 90, 0, 360), stride=6, coarsen=1)       # an identity is no second selector
    with pytest.raises(ValueError, match="no row"):
        subset.grid_box((89.0, 89.75, 0, 10), coarsen=6)


def test_launcher_validates_arguments_without_a_gpu():
    L = _lib.lib()
    assert L.cra5_coarsen_f32(None, 1, 1, 1, 0, 0, 1, 1, 1, 0, 1, 1, 0, 1, 1, None, None, None, 1, None, 1, None, None) == -7
    # the pointer and size checks come first and return before any device work (the addresses are never dereferenced)
    ok = [64, 1, 1, 1, 0, 0, 1, 1, 1, 0, 1, 1, 0, 1, 1, 64, 64, 64, 1, None, 1, 64, None]
    for pos, val in ((0, 66), (21, 66), (15, 65), (16, 66), (17, 68), (19, 66),      # misaligned src, dst, row0, ntap, rw, chan_map
                     (0, None), (21, None), (15, None), (16, None), (17, None),     # NULL
                     (1, 0), (2, 0), (3, 0), (6, 0), (7, 0), (10, 0), (11, 0), (13, 0), (14, 0), (18, 0), (20, 0)):   # zero sizes
        args = list(ok)
        args[pos] = val
        assert L.cra5_coarsen_f32(*args) == -7, (pos, val)
