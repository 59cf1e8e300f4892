"""Point decode: the host-side geometry of csrc/points.hip ("Point sampling", and section 10.7).
numpy only - no model, no GPU (`sample` alone runs a kernel).

`Points` is a list of (lat, lon) positions - stations, a track - and a method; `Points.taps(H, W)` turns it into the grid
nodes each point reads and their float64 weights, `Points.plan(H, W, kh, kw, sh, sw)` adds what the decoder's un-embed
needs to produce those nodes and nothing else: the sorted list of tokens whose patches hold a node, and per node its one
or two (token, tap) products.

  bilinear  row taps and column taps are regrid.Grid._bilinear_taps of (90 - lat) / dlat and lon / dlon with the TOL_DEG
            rule, columns modulo W: 1 or 2 taps each way, 1, 2 or 4 nodes - what Grid([lat], [lon], "bilinear") reads.
  nearest   row rint((90 - lat) / dlat), column rint((lon mod 360) / dlon) mod W, np.rint (ties to even): one node.
"""
import numpy as np

from .regrid import Grid
from .subset import TOL_DEG

METHODS = ("bilinear", "nearest")


def _coords(name, v):
    if isinstance(v, (str, bytes)) or v is None:
        raise ValueError(f"Points: {name} must be a 1-D array of degrees, got {v!r}")
    try:
        a = np.asarray(v)
    except Exception:
        raise ValueError(f"Points: {name} must be a 1-D array of degrees") from None
    if a.dtype == np.bool_ or a.dtype.kind not in "iuf":
        raise ValueError(f"Points: {name} must hold real numbers, got dtype {a.dtype}")
    if a.ndim != 1:
        raise ValueError(f"Points: {name} must have rank 1, got shape {a.shape}")
    if a.size == 0:
        raise ValueError(f"Points: {name} is empty")
    a = np.array(a, dtype=np.float64)
    if not np.isfinite(a).all():
        raise ValueError(f"Points: {name} holds non-finite values")
    return a


class Points:
    """P positions.  lat: float64 [P] inside [-90, 90]; lon: float64 [P], any real values (taken modulo 360); duplicates
    and any order are fine - the output keeps the order given.  method: "bilinear" | "nearest".  ValueError for anything
    else.  Hashable and comparable through `key` (the arrays' bytes and the method)."""

    def __init__(self, lat, lon, method="bilinear"):
        if not isinstance(method, str) or method not in METHODS:
            raise ValueError(f"Points: unknown method {method!r} (one of {METHODS})")
        lat, lon = _coords("lat", lat), _coords("lon", lon)
        if len(lat) != len(lon):
            raise ValueError(f"Points: lat holds {len(lat)} values, lon {len(lon)}")
        if (lat < -90.0).any() or (lat > 90.0).any():
            raise ValueError("Points: lat must lie in [-90, 90]")
        self.lat, self.lon_given, self.method = lat, lon, method
        self.lon = np.mod(lon, 360.0)
        self.lon[self.lon >= 360.0] = 0.0            # (-1e-17 mod 360 rounds to 360.0)
        for a in (self.lat, self.lon_given, self.lon):
            a.setflags(write=False)
        self.key = (method, self.lat.tobytes(), self.lon_given.tobytes())
        self._plans = {}

    def __eq__(self, other):
        return isinstance(other, Points) and self.key == other.key

    def __hash__(self):
        return hash(self.key)

    def __len__(self):
        return len(self.lat)

    def __repr__(self):
        return f"Points({len(self.lat)}, {self.method!r})"

    # ---- taps ------------------------------------------------------------------------------------------------------------
    def taps(self, H=721, W=1440):
        """The nodes of an H x W grid every point reads (built once per (H, W), then shared).  dict(
          P, grid = (H, W), method, key (hashable: these points and (H, W)), lat, lon (as given, lon in [0, 360));
          rows, cols int32 [P, 2]: the point's first and second row / column tap, -1 where there is no second one (nearest:
            never); rw, cw float64 [P, 2]: their weights, zero-padded (nearest: 1.0, 0.0);
          row0, ntap, col0, ctap int32 [P]: the same as Grid.plan's tables;
          nearest only - node_lat, node_lon float64 [P]: the grid point that is taken)."""
        H, W = int(H), int(W)
        if H < 2 or W < 1:
            raise ValueError(f"Points.taps: need a grid of at least 2 rows and 1 column, got {(H, W)}")
        t = self._plans.get((H, W))
        if t is None:
            t = self._plans[(H, W)] = self._make_taps(H, W)
        return t

    def _make_taps(self, H, W):
        P = len(self.lat)
        dlat, dlon = 180.0 / (H - 1), 360.0 / W
        rows = np.full((P, 2), -1, dtype=np.int32)
        cols = np.full((P, 2), -1, dtype=np.int32)
        rw = np.zeros((P, 2), dtype=np.float64)
        cw = np.zeros((P, 2), dtype=np.float64)
        extra = {}
        if self.method == "bilinear":
            for p in range(P):
                h0, w = Grid._bilinear_taps((90.0 - self.lat[p]) / dlat, TOL_DEG / dlat)
                if h0 < 0 or h0 + len(w) > H:
                    raise AssertionError(f"points plan: point {p} leaves the grid")
                c0, v = Grid._bilinear_taps(self.lon_given[p] / dlon, TOL_DEG / dlon)
                for t in range(len(w)):
                    rows[p, t], rw[p, t] = h0 + t, w[t]
                for u in range(len(v)):
                    cols[p, u], cw[p, u] = (c0 + u) % W, v[u]
        else:
            rows[:, 0] = np.clip(np.rint((90.0 - self.lat) / dlat), 0, H - 1).astype(np.int32)
            cols[:, 0] = (np.rint(self.lon / dlon).astype(np.int64) % W).astype(np.int32)
            rw[:, 0] = cw[:, 0] = 1.0
            extra = dict(node_lat=90.0 - rows[:, 0].astype(np.float64) * dlat, node_lon=cols[:, 0].astype(np.float64) * dlon)
        return dict(P=P, grid=(H, W), method=self.method, key=(self.key, H, W), lat=self.lat, lon=self.lon, rows=rows,
                    cols=cols, rw=rw, cw=cw, row0=rows[:, 0].copy(), ntap=(1 + (rows[:, 1] >= 0)).astype(np.int32),
                    col0=cols[:, 0].copy(), ctap=(1 + (cols[:, 1] >= 0)).astype(np.int32), **extra)

    # ---- the plan --------------------------------------------------------------------------------------------------------
    def plan(self, H=721, W=1440, kh=11, kw=10, sh=10, sw=10):
        """taps(H, W) plus the un-embed products behind them, for patches of kh x kw pixels at stride (sh, sw) (the ERA5
        geometry of subset.token_plan: kh = sh + 1, one shared row between vertically adjacent patches; kw = sw).  dict(
          **taps, patch = (kh, kw, sh, sw), tokens_grid = (Hp, Wp), key (hashable: the points, the grid, the patches);
          nodes int32 [n_nodes, 2]: the unique (row, col) pairs, sorted by (row, col);
          pnode int32 [P, 4]: the point's node at (row tap t, column tap u) in entry 2 t + u, -1 where there is none;
          tokens int32 [M]: the sorted unique token indexes ti * Wp + tj whose patches hold a node;
          contrib int32 [n_nodes, 4] = (m0, tap0, m1, tap1): the node is product `tap` = ky * kw + kx of row m of the token
            list - row r belongs to token row ti = min(r // sh, Hp - 1) at ky = r - sh * ti, column c to tj = c // sw at kx
            = c % sw; a seam row (r % sh == 0, 0 < r < sh * Hp) is token row ti - 1 at ky = sh, the UPPER partner, FIRST
            (m0, tap0), plus token row ti at ky = 0 (m1, tap1); every other row has m1 = -1)."""
        H, W, kh, kw, sh, sw = (int(v) for v in (H, W, kh, kw, sh, sw))
        k = (H, W, kh, kw, sh, sw)
        p = self._plans.get(k)
        if p is None:
            p = self._plans[k] = self._make_plan(*k)
        return p

    def _make_plan(self, H, W, kh, kw, sh, sw):
        if kh != sh + 1 or kw != sw or sh < 1 or sw < 1:
            raise ValueError("point decode needs the ERA5 un-embed geometry (kh = sh + 1, kw = sw)")
        Hp, Wp = (H - kh) // sh + 1, (W - kw) // sw + 1
        if Hp < 1 or Wp < 1 or H != sh * Hp + 1 or W != sw * Wp:
            raise ValueError(f"point decode: the patches ({kh} x {kw}, stride ({sh}, {sw})) do not tile the {H} x {W} grid")
        t = self.taps(H, W)
        rows, cols = t["rows"].astype(np.int64), t["cols"].astype(np.int64)
        # the (row tap, column tap) pairs of every point, -1 where a tap is absent
        pr = np.stack([rows[:, 0], rows[:, 0], rows[:, 1], rows[:, 1]], axis=1)
        pc = np.stack([cols[:, 0], cols[:, 1], cols[:, 0], cols[:, 1]], axis=1)
        have = (pr >= 0) & (pc >= 0)
        flat = np.where(have, pr * W + pc, -1)
        uniq = np.unique(flat[have])                               # sorted by (row, col)
        pnode = np.full(flat.shape, -1, dtype=np.int32)
        pnode[have] = np.searchsorted(uniq, flat[have]).astype(np.int32)
        nr, nc = uniq // W, uniq % W
        ti = np.minimum(nr // sh, Hp - 1)
        ky = nr - sh * ti
        tj, kx = nc // sw, nc % sw
        seam = (nr % sh == 0) & (nr > 0) & (nr < sh * Hp)
        lower = ti * Wp + tj                                        # the token that holds the row at ky (a seam: ky = 0)
        upper = np.where(seam, (ti - 1) * Wp + tj, -1)
        tokens = np.unique(np.concatenate([lower, upper[seam]]))
        contrib = np.full((len(uniq), 4), -1, dtype=np.int32)
        m_lower = np.searchsorted(tokens, lower)
        m_upper = np.searchsorted(tokens, np.where(seam, upper, lower))
        contrib[:, 0] = np.where(seam, m_upper, m_lower)
        contrib[:, 1] = np.where(seam, sh * kw + kx, ky * kw + kx)
        contrib[seam, 2] = m_lower[seam]
        contrib[seam, 3] = kx[seam]                                 # ky = 0
        contrib[~seam, 3] = 0
        return dict(t, key=(self.key,) + (H, W, kh, kw, sh, sw), patch=(kh, kw, sh, sw), tokens_grid=(Hp, Wp),
                    nodes=np.stack([nr, nc], axis=1).astype(np.int32), pnode=pnode, tokens=tokens.astype(np.int32),
                    contrib=contrib)


def as_points(points):
    """points= of the decode methods -> a Points: a Points itself, or a plain [P, 2] array-like of (lat, lon) rows
    (bilinear)."""
    if isinstance(points, Points):
        return points
    if isinstance(points, (str, bytes, dict)) or points is None:
        raise ValueError(f"points must be a cra5_amd.points.Points or a [P, 2] array of (lat, lon), got {type(points).__name__}")
    try:
        a = np.asarray(points)
    except Exception:
        raise ValueError("points must be a cra5_amd.points.Points or a [P, 2] array of (lat, lon)") from None
    if a.ndim != 2 or a.shape[1] != 2 or a.dtype == np.bool_ or a.dtype.kind not in "iuf":
        raise ValueError(f"points must be a cra5_amd.points.Points or a real [P, 2] array of (lat, lon), got {a.dtype} "
                         f"{a.shape}")
    return Points(a[:, 0], a[:, 1])


def as_plan(points, H, W, kh=11, kw=10, sh=10, sw=10):
    """points= of the decode methods -> its plan for the H x W grid and the patch geometry: a Points, a [P, 2] array-like,
    or a plan Points.plan returned."""
    if isinstance(points, dict) and all(k in points for k in ("key", "pnode", "tokens", "contrib", "rows", "cw")):
        if tuple(points["grid"]) != (H, W) or tuple(points["patch"]) != (kh, kw, sh, sw):
            raise ValueError(f"points: the plan was built for a {tuple(points['grid'])} grid and patches "
                             f"{tuple(points['patch'])}, the model's are {(H, W)} and {(kh, kw, sh, sw)}")
        return points
    return as_points(points).plan(H, W, kh, kw, sh, sw)


def sample(x, points, out=None):
    """A device frame x (contiguous fp32 [C, H, W]: row 0 = 90 N, dlat = 180 / (H - 1); column 0 = 0 E, dlon = 360 / W - a
    truth frame, a decoded one) at the points (Points | [P, 2] array-like) -> fp32 device [C, P]: what a decode with
    points= returns, applied to a frame that is already there (cra5_points_from_image)."""
    from . import ops
    if not hasattr(x, "dim") or x.dim() != 3:
        raise ValueError("points.sample: x must be a [C, H, W] device tensor")
    t = as_points(points).taps(int(x.shape[1]), int(x.shape[2]))
    return ops.points_from_image(x, ops.points_tables(t, x.device), out=out)
