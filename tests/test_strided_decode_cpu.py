"""Thinned (strided) decode, host side (no GPU): subset.stride_plan / scatter_tables against a brute-force numpy
restatement of the un-embed, the seam partners of every row range, the economy condition of the class design, the
stride rules of grid_box / resolve_stride, and the C ABI's argument validation of the two new kernels."""
import ctypes

import numpy as np
import pytest

from cra5_amd import _lib, subset
from cra5_amd.api import cra5_api

H, W = 721, 1440
KH, KW, SH, SW = 11, 10, 10, 10
HP, WP = 72, 144
ERR_ARG = -7
C = 2

LON_STRIDES = [s for s in range(1, 13) if W % s == 0]          # 1 2 3 4 5 6 8 9 10 12
BOXES = [
    (30, 31, 100, 50),       # a single seam row
    (30, 41, 0, 40),         # starts and ends on seam rows
    (0, 5, 0, 40),           # row 0
    (715, 721, 200, 33),     # row 720
    (360, 361, 720, 1),      # a single point (kept by every stride that divides 360 / 720)
    (72, 221, 1340, 281),    # across 0 deg
    (123, 456, 1437, 7),     # odd offsets across 0 deg
    (200, 260, 1, 1440),     # the whole circle from a column off a patch boundary
    (0, 721, 720, 1440),     # the globe from 180 deg
    None,                    # the globe
]
BOX_STRIDES = [(2, 2), (4, 4), (5, 5), (6, 6), (10, 10), (6, 4), (7, 6), (1, 6), (6, 1), (12, 12), (11, 9), (3, 8), (1, 1)]


@pytest.fixture(scope="module")
def products():
    """Y[ti, tj, c, ky, kx]: small-integer "GEMM outputs" (every sum below is exact) and the full image they overlap-add
    to: image row 10 ti + ky, column 10 tj + kx."""
    rng = np.random.default_rng(0)
    Y = rng.integers(-50, 51, size=(HP, WP, C, KH, KW)).astype(np.float32)
    full = np.zeros((C, H, W), dtype=np.float32)
    for ky in range(KH):
        # (token rows at one ky never collide: a strided view takes them all at once)
        full[:, ky:ky + SH * HP:SH, :] += Y[:, :, :, ky, :].transpose(2, 0, 1, 3).reshape(C, HP, W)
    return Y, full


def kept_slice(full, box, stride):
    r0, r1, c0, nc = box if box is not None else (0, H, 0, W)
    rows = [r for r in range(r0, r1) if r % stride[0] == 0]
    cols = [(c0 + k) % W for k in range(nc) if ((c0 + k) % W) % stride[1] == 0]
    return full[:, rows][:, :, cols], rows, cols


def class_matrices(plan, Y):
    """What the class GEMMs compute: per class pair [n_ti * n_tj, C * n_ky * n_kx], columns (c, ky, kx)."""
    G = {}
    for i, rc in enumerate(plan["row_classes"]):
        tis = [rc["t0"] + k * rc["step"] for k in range(rc["n"])]
        for j, cc in enumerate(plan["col_classes"]):
            tjs = [(cc["t0"] + k * cc["step"]) % WP for k in range(cc["n"])]
            g = Y[np.ix_(tis, tjs, range(C), rc["taps"], cc["taps"])]
            G[i, j] = g.reshape(len(tis) * len(tjs), -1)
    return G


def assemble_from_plan(plan, G):
    """The thinned image from the plan's own landing sites: direct rows, and seam slots added upper (slot 0) first."""
    out = np.full((C, plan["Ho"], plan["Wo"]), np.nan, dtype=np.float32)
    side = np.full((C, len(plan["seams"]), 2, plan["Wo"]), np.nan, dtype=np.float32)
    for i, rc in enumerate(plan["row_classes"]):
        for j, cc in enumerate(plan["col_classes"]):
            g = G[i, j].reshape(rc["n"], cc["n"], C, len(rc["taps"]), len(cc["taps"]))
            for (a, ka), lr in np.ndenumerate(rc["land"]):
                if lr == -1:
                    continue
                for (b, kb), lc in np.ndenumerate(cc["land"]):
                    if lc < 0:
                        continue
                    if lr >= 0:
                        assert np.isnan(out[0, lr, lc])          # written once
                        out[:, lr, lc] = g[a, b, :, ka, kb]
                    else:
                        s, slot = divmod(-2 - int(lr), 2)
                        assert np.isnan(side[0, s, slot, lc])
                        side[:, s, slot, lc] = g[a, b, :, ka, kb]
    for s, orow in enumerate(plan["seams"]):
        assert np.isnan(out[:, orow]).all()
        out[:, orow] = side[:, s, 0] + side[:, s, 1]
    return out


def assemble_from_tables(plan, G):
    """numpy restatement of cra5_strided_scatter_f32 on the tables of subset.scatter_tables."""
    tb = subset.scatter_tables(plan, C)
    g = np.full(tb["elems"], np.nan, dtype=np.float32)
    for i, j, off, M, N in tb["gemms"]:
        assert G[i, j].shape == (M, N) and off % subset.SCATTER_ALIGN == 0
        g[off:off + M * N] = G[i, j].reshape(-1)
    rows, cols, cls, n_cc = tb["rows"], tb["cols"], tb["cls"], tb["n_cc"]
    cc, tj, kx = cols[:, 0], cols[:, 1], cols[:, 2]
    out = np.empty((C, plan["Ho"], plan["Wo"]), dtype=np.float32)
    for i in range(plan["Ho"]):
        for c in range(C):
            acc = None
            for rc, ti, ky in (rows[i, :3], rows[i, 3:]):
                if rc < 0:
                    continue
                k = cls[rc * n_cc + cc]
                v = g[k[:, 0] + (ti * k[:, 2] + tj) * k[:, 1] + c * k[:, 4] + ky * k[:, 3] + kx]
                acc = v if acc is None else acc + v
            out[c, i] = acc
    return out


def check(box, stride, products):
    Y, full = products
    ref, rows, cols = kept_slice(full, box, stride)
    plan = subset.stride_plan(box, stride, H, W, KH, KW, SH, SW, C=C)
    assert list(plan["rows"]) == rows and list(plan["cols"]) == cols and (plan["Ho"], plan["Wo"]) == ref.shape[1:]
    G = class_matrices(plan, Y)
    assert np.array_equal(assemble_from_plan(plan, G), ref), (box, stride, "plan")
    assert np.array_equal(assemble_from_tables(plan, G), ref), (box, stride, "tables")
    assert plan["gemm_elems"] == sum(g.size for g in G.values())
    return plan


@pytest.mark.parametrize("sx", LON_STRIDES)
def test_plan_equals_brute_force_on_the_globe(products, sx):
    for sy in range(1, 13):
        plan = check(None, (sy, sx), products)
        # the globe needs every product a class computes
        assert plan["gemm_elems"] == plan["needed_elems"]


@pytest.mark.parametrize("stride", BOX_STRIDES)
def test_plan_equals_brute_force_on_boxes(products, stride):
    n = 0
    for box in BOXES:
        try:
            subset.kept_points(box if box is not None else (0, H, 0, W), stride, W)
        except ValueError:
            continue            # (this box holds no kept point at this stride: test_stride_errors covers the refusal)
        check(box, stride, products)
        n += 1
    assert n >= 6               # every stride of the sweep keeps points in most boxes


def test_issue_table_of_classes_and_products():
    """The counts of the design table: output grid, (token, tap) products per channel, whole globe."""
    want = {(2, 2): (1, 1, 361, 720, 311040), (4, 4): (2, 2, 181, 360, 77760), (5, 5): (1, 1, 145, 288, 62208),
            (6, 6): (3, 3, 121, 240, 34560), (10, 10): (1, 1, 73, 144, 20736), (12, 12): (6, 5, 61, 120, 8640)}
    for st, (n_rc, n_cc, Ho, Wo, need) in want.items():
        p = subset.stride_plan(None, st, H, W)
        # ((12, 12): the sixth column class would need kx = 10, which a 10-wide patch does not have - it is empty)
        assert (len(p["row_classes"]), len(p["col_classes"]), p["Ho"], p["Wo"], p["needed_elems"]) == (n_rc, n_cc, Ho, Wo, need)
    assert subset.stride_plan(None, (1, 1), H, W)["needed_elems"] == HP * WP * KH * KW == 1140480


@pytest.mark.parametrize("s", [2, 5, 6, 10])
def test_every_kept_seam_row_has_both_partners_upper_first(s):
    """For every row range [r0, r1): each kept seam row (image row 10 t, 0 < t < 72) has exactly two contributions in
    the plan - slot 0 from token row t - 1 at ky = 10 (the upper partner, added first), slot 1 from token row t at
    ky = 0 -, every other kept row exactly one, and no token row of the plan is outside the grid."""
    for r0 in range(H):
        for r1 in list(range(r0 + 1, min(H, r0 + 24) + 1)) + [min(H, r0 + 101), H]:
            if not any(r % s == 0 for r in range(r0, min(r1, r0 + s))):
                continue
            p = subset.stride_plan((r0, r1, 0, 40), (s, s), H, W)
            kept = [r for r in range(r0, r1) if r % s == 0]
            seams = [r for r in kept if r % SH == 0 and 0 < r < H - 1]
            assert [int(p["rows"][o]) for o in p["seams"]] == seams
            slots, direct = {}, {}
            for rc in p["row_classes"]:
                assert 0 <= rc["t0"] and rc["t0"] + (rc["n"] - 1) * rc["step"] < HP
                for (i, a), v in np.ndenumerate(rc["land"]):
                    ti, ky = rc["t0"] + i * rc["step"], rc["taps"][a]
                    if v >= 0:
                        assert v not in direct
                        direct[int(v)] = (ti, ky)
                    elif v <= -2:
                        assert -2 - int(v) not in slots
                        slots[-2 - int(v)] = (ti, ky)
            for k, r in enumerate(seams):
                assert slots[2 * k] == (r // SH - 1, KH - 1) and slots[2 * k + 1] == (r // SH, 0), (r0, r1, r)
            assert len(slots) == 2 * len(seams)
            want = {o: (min(r // SH, HP - 1), r - SH * min(r // SH, HP - 1)) for o, r in enumerate(kept) if r not in seams}
            assert direct == want, (r0, r1)


def test_economy_of_the_class_design():
    """A condition on the design, not a measurement: for the 268 model, all channels, whole globe, the class GEMMs
    compute at most 2 x the needed products.  (Running every token over the union of taps costs 4 x at (4, 4) and 9 x at
    (6, 6).)"""
    for st in [(2, 2), (4, 4), (5, 5), (6, 6), (10, 10)]:
        p = subset.stride_plan(None, st, H, W, C=268)
        assert p["needed_elems"] == 268 * subset.stride_plan(None, st, H, W)["needed_elems"]
        assert p["gemm_elems"] <= 2 * p["needed_elems"], st
        tb = subset.scatter_tables(p, 268)
        assert sum(M * N for *_, M, N in tb["gemms"]) == p["gemm_elems"]
        # and the workspace of the class matrices is a small part of the full column matrix (1 140 480 x 268)
        assert tb["elems"] <= 2 * p["needed_elems"] + subset.SCATTER_ALIGN * len(tb["gemms"])


# ---- the stride rules -----------------------------------------------------------------------------------------------


def test_no_stride_forms():
    for s in (None, 1, (1, 1), [1, 1], np.int64(1)):
        assert subset.resolve_stride(s) is None
    assert subset.resolve_stride(6) == (6, 6) and subset.resolve_stride((7, 6)) == (7, 6)
    assert subset.resolve_stride(np.int32(4)) == (4, 4) and subset.resolve_stride([1, 6]) == (1, 6)
    g0, g1 = cra5_api.grid_box((35, 72, -25, 45)), cra5_api.grid_box((35, 72, -25, 45), stride=1)
    assert g0["box"] == g1["box"] and np.array_equal(g0["lat"], g1["lat"]) and np.array_equal(g0["lon"], g1["lon"])
    assert "stride" not in g1


def test_grid_box_with_a_stride_is_anchored_to_the_global_grid():
    g = cra5_api.grid_box((-90, 90, 0, 360), stride=6)                    # the 1.5 deg grid, poles included
    assert len(g["lat"]) == 121 and len(g["lon"]) == 240 and g["box"] == (0, 721, 0, 1440) and g["stride"] == (6, 6)
    assert g["lat"][0] == 90.0 and g["lat"][-1] == -90.0 and g["lat"][1] == 88.5
    assert g["lon"][0] == 0.0 and g["lon"][1] == 1.5 and g["lon"][-1] == 358.5
    assert len(cra5_api.grid_box((-90, 90, 0, 360), stride=4)["lat"]) == 181                # 1 deg
    e = cra5_api.grid_box((35, 72, -25, 45), stride=(6, 4))               # rows 72 .. 220, columns 1340 .. 180
    assert e["box"] == (72, 221, 1340, 281)                               # the box itself is unthinned
    assert list(e["kept_rows"]) == list(range(72, 221, 6)) and e["lat"][0] == 72.0 and e["lat"][-1] == 36.0
    assert list(e["kept_cols"]) == list(range(1340, 1440, 4)) + list(range(0, 181, 4))
    assert e["lon"][0] == 335.0 and e["lon"][-1] == 45.0 and 0.0 in e["lon"]
    # a region's thinned points are a sub-block of the globe's, whatever its bounds: 35.1 N is not on the lattice
    o = cra5_api.grid_box((35.1, 71.9, -24.9, 44.9), stride=(6, 4))
    assert set(o["lat"]) <= set(g["lat"]) and list(o["kept_rows"]) == list(range(78, 217, 6))
    assert list(o["kept_cols"]) == list(range(1344, 1440, 4)) + list(range(0, 177, 4))
    # the whole circle from a column off the lattice: starts at the next kept column, ends just before the first
    c = cra5_api.grid_box((0, 0, 0.25, 360.25), stride=6)
    assert list(c["kept_cols"]) == list(range(6, 1440, 6)) + [0] and list(c["kept_rows"]) == [360]


@pytest.mark.parametrize("stride, msg", [
    (0, "0"), (-2, "-2"), ((2, 0), r"\(2, 0\)"), (2.0, r"2\.0"), ((2, 2.5), r"2\.5"), ("2", "'2'"), (True, "True"),
    ((2, 3, 4), r"\(2, 3, 4\)"), ((2,), r"\(2,\)"),
    (7, r"1440 % s_lon \(7\)"), ((2, 11), r"1440 % s_lon \(11\)"),
])
def test_stride_errors(stride, msg):
    with pytest.raises(ValueError, match=msg):
        subset.resolve_stride(stride)
    with pytest.raises(ValueError, match=msg):
        cra5_api.grid_box((-90, 90, 0, 360), stride=stride)


def test_a_box_without_a_kept_point_is_refused():
    with pytest.raises(ValueError, match=r"\(6, 6\).*no row"):
        cra5_api.grid_box((89.0, 89.75, 0, 10), stride=6)                 # rows 1 .. 4
    with pytest.raises(ValueError, match=r"\(6, 6\).*no column"):
        cra5_api.grid_box((0, 10, 0.25, 1.25), stride=6)                  # columns 1 .. 5
    with pytest.raises(ValueError, match="no row"):
        subset.stride_plan((1, 5, 0, 40), (6, 6), H, W)
    with pytest.raises(ValueError, match="no column"):
        subset.kept_points((0, 10, 1435, 5), (2, 12), W)                  # columns 1435 .. 1439
    with pytest.raises(ValueError, match="box"):
        subset.stride_plan((5, 5, 0, 10), (2, 2), H, W)
    with pytest.raises(ValueError, match="stride"):
        subset.stride_plan(None, (2, 7), H, W)


# ---- C ABI: argument validation before any device work ---------------------------------------------------------------


def test_new_kernels_validate_arguments_without_gpu():
    L = _lib.lib()
    a, b = ctypes.c_void_p(1 << 20), ctypes.c_void_p(2 << 20)     # never dereferenced: every call is refused
    lat = L.cra5_gather_token_lattice
    assert lat(None, 64, b, 64, 64, 4, 6, 0, 1, 1, 0, 1, 1, None) == ERR_ARG
    assert lat(a, 64, None, 64, 64, 4, 6, 0, 1, 1, 0, 1, 1, None) == ERR_ARG
    assert lat(a, 64, b, 64, 60, 4, 6, 0, 1, 1, 0, 1, 1, None) == ERR_ARG      # row % 16
    assert lat(a, 48, b, 64, 64, 4, 6, 0, 1, 1, 0, 1, 1, None) == ERR_ARG      # pitch < row
    assert lat(ctypes.c_void_p((1 << 20) + 8), 64, b, 64, 64, 4, 6, 0, 1, 1, 0, 1, 1, None) == ERR_ARG   # alignment
    assert lat(a, 64, b, 64, 64, 4, 6, 1, 2, 3, 0, 1, 1, None) == ERR_ARG      # last token row 1 + 2 * 2 = 5 >= Hp
    assert lat(a, 64, b, 64, 64, 4, 6, 4, 1, 1, 0, 1, 1, None) == ERR_ARG      # ti0 >= Hp
    assert lat(a, 64, b, 64, 64, 4, 6, 0, 0, 1, 0, 1, 1, None) == ERR_ARG      # ti_step < 1
    assert lat(a, 64, b, 64, 64, 4, 6, 0, 1, 1, 6, 1, 1, None) == ERR_ARG      # tj0 >= Wp
    assert lat(a, 64, b, 64, 64, 4, 6, 0, 1, 1, 0, 3, 3, None) == ERR_ARG      # (3 - 1) * 3 >= Wp: a token twice
    assert lat(a, 64, b, 64, 64, 4, 6, 0, 1, 1, 0, 0, 1, None) == ERR_ARG      # tj_step < 1
    assert lat(a, 64, b, 64, 64, 4, 6, 0, 1, 0, 0, 1, 1, None) == ERR_ARG      # n_ti < 1
    sc = L.cra5_strided_scatter_f32
    assert sc(None, 16, a, a, a, 1, 1, None, None, b, 1, 1, 1, None) == ERR_ARG
    assert sc(a, 0, a, a, a, 1, 1, None, None, b, 1, 1, 1, None) == ERR_ARG    # an empty workspace
    assert sc(a, 16, None, a, a, 1, 1, None, None, b, 1, 1, 1, None) == ERR_ARG
    assert sc(a, 16, a, None, a, 1, 1, None, None, b, 1, 1, 1, None) == ERR_ARG
    assert sc(a, 16, a, a, None, 1, 1, None, None, b, 1, 1, 1, None) == ERR_ARG
    assert sc(a, 16, a, a, a, 1, 1, None, None, None, 1, 1, 1, None) == ERR_ARG
    assert sc(a, 16, a, a, a, 0, 1, None, None, b, 1, 1, 1, None) == ERR_ARG   # no row class
    assert sc(a, 16, a, a, a, 1, 1, None, None, b, 0, 1, 1, None) == ERR_ARG   # C
    assert sc(a, 16, a, a, a, 1, 1, None, None, b, 1, 0, 1, None) == ERR_ARG   # Ho
    assert sc(a, 16, a, a, a, 1, 1, None, None, b, 1, 1, 0, None) == ERR_ARG   # Wo
    assert sc(a, 16, a, a, a, 1, 1, a, None, b, 1, 1, 1, None) == ERR_ARG      # mean without std
    assert sc(a, 16, a, a, ctypes.c_void_p((1 << 20) + 4), 1, 1, None, None, b, 1, 1, 1, None) == ERR_ARG   # int64 table
