"""Regridding onto any rectilinear lat/lon grid: the host-side geometry of cra5_regrid_f32 (csrc/window_reduce.hip; DESIGN.md
section 4, "Regridding").  numpy only - no model, no GPU.

`Grid` is a target grid (cell centres, optional cell bounds, a method); `Grid.plan(H, W)` turns it into the separable
weight tables the kernel walks: per target row a contiguous run of source rows with float64 weights, per target column a
contiguous run of source columns (wrapping modulo W) with float64 weights.

Source geometry (subset.coarsen_plan's): row h is latitude 90 - h * 180 / (H - 1) and owns the band between the half-row
edges of subset._edge_lat (the pole rows own half cells); column c is longitude c * 360 / W and owns -+ half a column.

  bilinear      r = (90 - lat) / dlat; within TOL_DEG of a source row: ONE tap (rint(r), 1.0) - a target point on the
                source lattice copies the source value exactly; otherwise (floor(r), 1 - f), (floor(r) + 1, f).  The
                same along the columns, modulo W.
  conservative  first-order: rw[i][t] = V_t / S, V_t = sin(north) - sin(south) of the overlap of source row row0[i] + t's
                band with the target band, S the sum of the V_t added north to south; cw[j][u] = L_u / T, L_u the overlap
                in degrees of the source cell with the target interval, T their sum added west to east.  Taps without a
                positive overlap are not in the tables.
"""
import math

import numpy as np

from .subset import TOL_DEG, _edge_lat

METHODS = ("bilinear", "conservative")
# the kernel's LDS budget (csrc/window_reduce.hip): one staged source row of a tile, and the tile's column weights
SPAN_MAX = 7936            # floats of one staged row
CW_LDS_DOUBLES = 4096      # tile columns x cw pitch
MAX_TILE_COLS = 256
MAX_CTAP = 64


def _axis(name, v):
    if isinstance(v, (str, bytes)) or v is None:
        raise ValueError(f"Grid: {name} must be a 1-D array of degrees, got {v!r}")
    try:
        a = np.asarray(v)
    except Exception:
        raise ValueError(f"Grid: {name} must be a 1-D array of degrees") from None
    if a.dtype == np.bool_ or a.dtype.kind not in "iuf":
        raise ValueError(f"Grid: {name} must hold real numbers, got dtype {a.dtype}")
    if a.ndim != 1:
        raise ValueError(f"Grid: {name} must have rank 1, got shape {a.shape}")
    if a.size == 0:
        raise ValueError(f"Grid: {name} is empty")
    a = np.ascontiguousarray(a, dtype=np.float64)
    if not np.isfinite(a).all():
        raise ValueError(f"Grid: {name} holds non-finite values")
    return a


def _bounds(name, b, n):
    if b is None:
        return None
    if isinstance(b, (str, bytes)):
        raise ValueError(f"Grid: {name} must be a [{n}, 2] array of degrees, got {b!r}")
    try:
        a = np.asarray(b)
    except Exception:
        raise ValueError(f"Grid: {name} must be a [{n}, 2] array of degrees") from None
    if a.dtype == np.bool_ or a.dtype.kind not in "iuf" or a.shape != (n, 2):
        raise ValueError(f"Grid: {name} must be a real [{n}, 2] array, got {a.dtype} {a.shape}")
    a = np.ascontiguousarray(a, dtype=np.float64)
    if not np.isfinite(a).all():
        raise ValueError(f"Grid: {name} holds non-finite values")
    return a


def _sind(deg):
    return float(np.sin(np.deg2rad(deg)))


class Grid:
    """A rectilinear target grid.  lat: float64 [Ho], strictly monotone (either direction; output rows come back in this
    order), inside [-90, 90].  lon: float64 [Wo], strictly increasing eastward (0 < lon[j + 1] - lon[j] < 360, lon[-1] -
    lon[0] < 360), any real values - columns wrap modulo 360.  method: "bilinear" | "conservative".  lat_bnds [Ho, 2] /
    lon_bnds [Wo, 2]: the cells' edges in degrees (either order per row; a longitude cell may be given shifted by a
    multiple of 360); default: the midpoints between neighbouring centres, an end cell mirrored about its centre,
    latitudes clipped to -+90; a uniform lon that closes the circle within TOL_DEG wraps.  A one-row / one-column
    conservative grid must bring its bounds.  ValueError for anything else."""

    def __init__(self, lat, lon, method="bilinear", lat_bnds=None, lon_bnds=None):
        if not isinstance(method, str) or method not in METHODS:
            raise ValueError(f"Grid: unknown method {method!r} (one of {METHODS})")
        lat, lon = _axis("lat", lat), _axis("lon", lon)
        if (lat < -90.0).any() or (lat > 90.0).any():
            raise ValueError("Grid: lat must lie in [-90, 90]")
        d = np.diff(lat)
        if len(d) and not ((d > 0).all() or (d < 0).all()):
            raise ValueError("Grid: lat must be strictly monotone")
        d = np.diff(lon)
        if len(d) and not ((d > 0).all() and (d < 360.0).all() and lon[-1] - lon[0] < 360.0):
            raise ValueError("Grid: lon must increase eastward, 0 < lon[j + 1] - lon[j] < 360 and lon[-1] - lon[0] < 360")
        lat_bnds, lon_bnds = _bounds("lat_bnds", lat_bnds, len(lat)), _bounds("lon_bnds", lon_bnds, len(lon))
        if method == "conservative":
            if len(lat) == 1 and lat_bnds is None:
                raise ValueError("Grid: a one-row conservative grid must bring lat_bnds")
            if len(lon) == 1 and lon_bnds is None:
                raise ValueError("Grid: a one-column conservative grid must bring lon_bnds")
        self.lat, self.lon, self.method = lat, lon, method
        self.lat_bnds = self._lat_cells(lat, lat_bnds)
        self.lon_bnds = self._lon_cells(lon, lon_bnds)
        for a in (self.lat, self.lon, self.lat_bnds, self.lon_bnds):
            a.setflags(write=False)
        self.key = (method, self.lat.tobytes(), self.lon.tobytes(), self.lat_bnds.tobytes(), self.lon_bnds.tobytes())
        self._plans = {}

    def __eq__(self, other):
        return isinstance(other, Grid) and self.key == other.key

    def __hash__(self):
        return hash(self.key)

    def __repr__(self):
        return f"Grid({len(self.lat)} x {len(self.lon)}, {self.method!r})"

    @property
    def shape(self):
        return len(self.lat), len(self.lon)

    # ---- cells ---------------------------------------------------------------------------------------------------------
    @staticmethod
    def _lat_cells(lat, bnds):
        """-> [Ho, 2] (north, south), clipped to the poles."""
        n = len(lat)
        if bnds is not None:
            out = np.stack([bnds.max(axis=1), bnds.min(axis=1)], axis=1)
            if (out[:, 0] > 90.0 + TOL_DEG).any() or (out[:, 1] < -90.0 - TOL_DEG).any():
                raise ValueError("Grid: lat_bnds must lie in [-90, 90]")
            out = np.clip(out, -90.0, 90.0)
            if (out[:, 0] <= out[:, 1]).any():
                raise ValueError("Grid: every lat_bnds row must span a band of positive height")
            if (lat > out[:, 0] + TOL_DEG).any() or (lat < out[:, 1] - TOL_DEG).any():
                raise ValueError("Grid: every lat must lie inside its lat_bnds")
            return out
        if n == 1:
            return np.clip(np.array([[lat[0] + 0.5, lat[0] - 0.5]]), -90.0, 90.0)     # (bilinear only: area weights)
        mid = 0.5 * (lat[:-1] + lat[1:])
        first, last = lat[0] - (mid[0] - lat[0]), lat[-1] + (lat[-1] - mid[-1])
        e = np.concatenate([[first], mid, [last]])                    # edge i between cell i - 1 and cell i
        a, b = e[:-1], e[1:]
        return np.clip(np.stack([np.maximum(a, b), np.minimum(a, b)], axis=1), -90.0, 90.0)

    @staticmethod
    def _lon_cells(lon, bnds):
        """-> [Wo, 2] (west, east), not wrapped: west <= lon <= east."""
        n = len(lon)
        if bnds is not None:
            w, e = bnds.min(axis=1), bnds.max(axis=1)
            if (e - w <= 0.0).any():
                raise ValueError("Grid: every lon_bnds row must span an interval of positive width")
            if (e - w > 360.0 + TOL_DEG).any():
                raise ValueError("Grid: a target cell wider than 360 degrees is refused")
            shift = 360.0 * np.floor((lon - w + TOL_DEG) / 360.0)
            w, e = w + shift, e + shift
            if (lon > e + TOL_DEG).any():
                raise ValueError("Grid: every lon must lie inside its lon_bnds (modulo 360)")
            return np.stack([w, e], axis=1)
        if n == 1:
            return np.array([[lon[0] - 0.5, lon[0] + 0.5]])                            # (bilinear only)
        d = np.diff(lon)
        mid = 0.5 * (lon[:-1] + lon[1:])
        if np.abs(d - d[0]).max() <= TOL_DEG and abs(n * d[0] - 360.0) <= TOL_DEG:      # closes the circle: wraps
            east = 0.5 * (lon[-1] + (lon[0] + 360.0))
            first, last = east - 360.0, east
        else:
            first, last = lon[0] - (mid[0] - lon[0]), lon[-1] + (lon[-1] - mid[-1])
        e = np.concatenate([[first], mid, [last]])
        if (e[1:] - e[:-1] > 360.0).any():
            raise ValueError("Grid: a target cell wider than 360 degrees is refused")
        return np.stack([e[:-1], e[1:]], axis=1)

    @property
    def closes_circle(self):
        """The longitudes are uniform and close the circle (within TOL_DEG): a zonal spectrum of the rows makes sense."""
        n = len(self.lon)
        if n < 2:
            return False
        d = np.diff(self.lon)
        return bool(np.abs(d - d[0]).max() <= TOL_DEG and abs(n * d[0] - 360.0) <= TOL_DEG)

    # ---- constructors --------------------------------------------------------------------------------------------------
    @classmethod
    def equiangular(cls, nlat, nlon, poles=False, method="bilinear"):
        """nlat x nlon equiangular, south to north (WeatherBench's order), lon from 0 eastward.  poles=False: cell-centred,
        lat = -90 + (i + 1/2) * 180 / nlat, lon = (j + 1/2) * 360 / nlon - (32, 64) is the 5.625 deg WeatherBench grid, its
        cells tile the sphere.  poles=True: lat = -90 + i * 180 / (nlat - 1) with both poles as rows, lon = j * 360 / nlon."""
        nlat, nlon = cls._count(nlat, "nlat"), cls._count(nlon, "nlon")
        if poles:
            if nlat < 2:
                raise ValueError("Grid.equiangular: poles=True needs nlat >= 2")
            lat = -90.0 + np.arange(nlat) * (180.0 / (nlat - 1))
            lat[-1] = 90.0
            lon = np.arange(nlon) * (360.0 / nlon)
            half = 180.0 / nlon
            return cls(lat, lon, method, lon_bnds=np.stack([lon - half, lon + half], axis=1))
        dlat, dlon = 180.0 / nlat, 360.0 / nlon
        es = -90.0 + np.arange(nlat + 1) * dlat
        es[-1] = 90.0
        ew = np.arange(nlon + 1) * dlon
        return cls(-90.0 + (np.arange(nlat) + 0.5) * dlat, (np.arange(nlon) + 0.5) * dlon, method,
                   lat_bnds=np.stack([es[1:], es[:-1]], axis=1), lon_bnds=np.stack([ew[:-1], ew[1:]], axis=1))

    @classmethod
    def regular(cls, dlat, dlon, region=None, method="bilinear"):
        """Cell-centred dlat x dlon cells tiling region = (lat_min, lat_max, lon_min, lon_max) (default: the globe, lon from
        0), north to south: lat = lat_max - (i + 1/2) * dlat, lon = lon_min + (j + 1/2) * dlon - regular(0.5, 0.5) runs
        89.75 .. -89.75.  The region must hold a whole number of cells (within TOL_DEG)."""
        try:
            dlat, dlon = float(dlat), float(dlon)
            lat_min, lat_max, lon_min, lon_max = (float(v) for v in (region if region is not None else (-90, 90, 0, 360)))
        except (TypeError, ValueError):
            raise ValueError(f"Grid.regular: need numbers dlat, dlon and region = (lat_min, lat_max, lon_min, lon_max), got "
                             f"{dlat!r}, {dlon!r}, {region!r}") from None
        if not all(math.isfinite(v) for v in (dlat, dlon, lat_min, lat_max, lon_min, lon_max)) or dlat <= 0 or dlon <= 0:
            raise ValueError("Grid.regular: dlat and dlon must be positive, the region finite")
        if not -90.0 <= lat_min < lat_max <= 90.0:
            raise ValueError(f"Grid.regular: region {region!r}: need -90 <= lat_min < lat_max <= 90")
        span = lon_max - lon_min
        if span <= 0.0 or span > 360.0:
            span = span % 360.0 or 360.0
        nlat, nlon = round((lat_max - lat_min) / dlat), round(span / dlon)
        if nlat < 1 or nlon < 1 or abs(nlat * dlat - (lat_max - lat_min)) > TOL_DEG or abs(nlon * dlon - span) > TOL_DEG:
            raise ValueError(f"Grid.regular: the region does not hold a whole number of {dlat} x {dlon} degree cells")
        en = lat_max - np.arange(nlat + 1) * dlat
        en[-1] = lat_min
        ew = lon_min + np.arange(nlon + 1) * dlon
        return cls(lat_max - (np.arange(nlat) + 0.5) * dlat, lon_min + (np.arange(nlon) + 0.5) * dlon, method,
                   lat_bnds=np.stack([en[:-1], en[1:]], axis=1), lon_bnds=np.stack([ew[:-1], ew[1:]], axis=1))

    @classmethod
    def gaussian(cls, nlat, nlon, method="bilinear"):
        """The nlat Gaussian latitudes (numpy.polynomial.legendre.leggauss), north to south, x nlon uniform longitudes from
        0.  The cell edges are asin of the running sum of the quadrature weights: the cells tile pole to pole."""
        nlat, nlon = cls._count(nlat, "nlat"), cls._count(nlon, "nlon")
        x, w = np.polynomial.legendre.leggauss(nlat)
        lat = np.rad2deg(np.arcsin(x[::-1]))
        s = 1.0 - np.concatenate([[0.0], np.cumsum(w[::-1])])         # sin of the edges, from the north pole
        edge = np.rad2deg(np.arcsin(np.clip(s, -1.0, 1.0)))
        edge[0], edge[-1] = 90.0, -90.0
        lon = np.arange(nlon) * (360.0 / nlon)
        half = 180.0 / nlon
        return cls(lat, lon, method, lat_bnds=np.stack([edge[:-1], edge[1:]], axis=1),
                   lon_bnds=np.stack([lon - half, lon + half], axis=1))

    @staticmethod
    def _count(n, name):
        if isinstance(n, (bool, np.bool_)) or not isinstance(n, (int, np.integer)) or n < 1:
            raise ValueError(f"Grid: {name} must be a positive int, got {n!r}")
        return int(n)

    # ---- the plan --------------------------------------------------------------------------------------------------------
    def plan(self, H=721, W=1440):
        """The tables of cra5_regrid_f32 for an H x W source grid (built once per (H, W), then shared).  dict(
          Ho, Wo, grid = (H, W), method, key (hashable: this grid and (H, W));
          row0, ntap int32 [Ho]: the first GLOBAL source row and the row count of target row i's window; rw float64
            [Ho, Tmax], zero-padded: its weights, north to south;  rv: the conservative V_t before normalisation (bilinear:
            rw itself);
          order int32 [Ho]: the target rows from north to south - the kernel walks the source in this order and writes
            row order[k] (the caller's order);
          col0, ctap int32 [Wo], cw float64 [Wo, Umax]: the same along the columns, window column u is source column
            (col0[j] + u) mod W, west to east;  cl: the conservative overlaps L_u in degrees (bilinear: cw itself);
            ucol0 int64 [Wo]: col0 before the wrap (non-decreasing: the columns are one eastward run);
          src_box (r0, r1, c0, nc): the hull of all windows, (0, W) in columns when the span reaches the whole circle;
          lat, lon: as given;  lat_bnds [Ho, 2] (north, south), lon_bnds [Wo, 2] (west, east, not wrapped) in degrees (for
            bilinear: the midpoint cells, serving only the area weights);
          area_weights float64 [Ho]: sin(north) - sin(south), normalised to mean 1;  closes_circle: the property)."""
        H, W = int(H), int(W)
        if H < 2 or W < 1:
            raise ValueError(f"Grid.plan: need a source grid of at least 2 rows and 1 column, got {(H, W)}")
        p = self._plans.get((H, W))
        if p is None:
            p = self._plans[(H, W)] = self._make_plan(H, W)
        return p

    def _make_plan(self, H, W):
        Ho, Wo = self.shape
        if self.method == "bilinear":
            rows = [self._bilinear_taps((90.0 - v) / (180.0 / (H - 1)), TOL_DEG / (180.0 / (H - 1))) for v in self.lat]
            cols = [self._bilinear_taps(v / (360.0 / W), TOL_DEG / (360.0 / W)) for v in self.lon]
            for i, (h0, w) in enumerate(rows):
                if h0 < 0 or h0 + len(w) > H:
                    raise AssertionError(f"regrid plan: row {i} leaves the grid")
            rraw, craw = rows, cols
        else:
            rraw = [self._band_taps(n, s, H) for n, s in self.lat_bnds]
            craw = [self._interval_taps(w, e, W) for w, e in self.lon_bnds]
            rows = [(h0, self._normalised(v)) for h0, v in rraw]
            cols = [(c0, self._normalised(v)) for c0, v in craw]
        row0, ntap, rw = self._table(rows)
        ucol0, ctap, cw = self._table(cols, np.int64)
        _, _, rv = self._table(rraw)
        _, _, cl = self._table(craw, np.int64)
        order = np.arange(Ho, dtype=np.int32)
        if self.lat[0] < self.lat[-1]:
            order = np.ascontiguousarray(order[::-1])
        sr0, sr1 = int(row0.min()), int((row0 + ntap).max())
        u0, u1 = int(ucol0.min()), int((ucol0 + ctap).max())
        sc0, snc = (u0 % W, u1 - u0) if u1 - u0 < W else (0, W)
        area = np.array([_sind(n) - _sind(s) for n, s in self.lat_bnds], dtype=np.float64)
        return dict(Ho=Ho, Wo=Wo, grid=(H, W), method=self.method, key=(self.key, H, W), row0=row0, ntap=ntap, rw=rw, rv=rv,
                    order=order, col0=(ucol0 % W).astype(np.int32), ucol0=ucol0, ctap=ctap, cw=cw, cl=cl,
                    src_box=(sr0, sr1, sc0, snc), lat=self.lat, lon=self.lon, lat_bnds=self.lat_bnds, lon_bnds=self.lon_bnds,
                    area_weights=area / area.mean(), closes_circle=self.closes_circle)

    @staticmethod
    def _bilinear_taps(r, tol):
        n = float(np.rint(r))
        if abs(r - n) <= tol:
            return int(n), [1.0]
        h0 = math.floor(r)
        f = r - h0
        return int(h0), [1.0 - f, f]

    @staticmethod
    def _normalised(v):
        total = 0.0
        for x in v:                       # in window order, one rounding per add
            total = total + x
        return [x / total for x in v]

    @staticmethod
    def _band_taps(north, south, H):
        """-> (first source row, [V_t]) of the target band: the rows whose own band overlaps it with V > 0."""
        d = 180.0 / (H - 1)
        lo = max(0, int(math.floor((90.0 - north) / d - 0.5)) - 1)
        hi = min(H - 1, int(math.ceil((90.0 - south) / d + 0.5)) + 1)
        hs, vs = [], []
        for h in range(lo, hi + 1):
            n = min(north, float(_edge_lat(2 * h - 1, H)))
            s = max(south, float(_edge_lat(2 * h + 1, H)))
            v = _sind(n) - _sind(s) if n > s else 0.0
            if v > 0.0:
                hs.append(h)
                vs.append(v)
        if not hs or hs != list(range(hs[0], hs[0] + len(hs))):
            raise ValueError(f"Grid.plan: the target band {south} .. {north} has no contiguous window of source rows")
        return hs[0], vs

    @staticmethod
    def _interval_taps(west, east, W):
        """-> (first source column, not wrapped, [L_u]) of the target interval: the columns whose cell overlaps it."""
        if east - west > 360.0:
            raise ValueError("Grid.plan: a target cell wider than 360 degrees is refused")
        hd = 180.0 / W                                    # half a column: cell c spans (2 c - 1) hd .. (2 c + 1) hd
        lo = int(math.floor(west / (2 * hd) + 0.5)) - 1
        hi = int(math.ceil(east / (2 * hd) - 0.5)) + 1
        cs, ls = [], []
        for c in range(lo, hi + 1):
            ov = min(east, (2 * c + 1) * hd) - max(west, (2 * c - 1) * hd)
            if ov > 0.0:
                cs.append(c)
                ls.append(ov)
        if not cs or cs != list(range(cs[0], cs[0] + len(cs))):
            raise ValueError(f"Grid.plan: the target interval {west} .. {east} has no contiguous window of source columns")
        return cs[0], ls

    @staticmethod
    def _table(taps, first_dtype=np.int32):
        n = len(taps)
        first = np.array([t[0] for t in taps], dtype=first_dtype)
        count = np.array([len(t[1]) for t in taps], dtype=np.int32)
        w = np.zeros((n, int(count.max())), dtype=np.float64)
        for i, (_, v) in enumerate(taps):
            w[i, :len(v)] = v
        return first, count, w


def as_plan(regrid, H, W):
    """regrid= of the decode methods -> its plan for the H x W grid: a Grid, or a plan Grid.plan(H, W) returned."""
    if isinstance(regrid, Grid):
        return regrid.plan(H, W)
    if isinstance(regrid, dict) and all(k in regrid for k in ("key", "row0", "rw", "col0", "cw", "src_box", "closes_circle")):
        if tuple(regrid["grid"]) != (H, W):
            raise ValueError(f"regrid: the plan was built for a {tuple(regrid['grid'])} source grid, the model's is {(H, W)}")
        return regrid
    raise ValueError(f"regrid must be a cra5_amd.regrid.Grid or the plan of one, got {type(regrid).__name__}")


def tile_table(plan, max_cols=None, span_max=None):
    """The column tiles of cra5_regrid_f32 -> (tiles int32 [n, 4]: first target column, column count, first GLOBAL source
    column of the tile's span (mod W), the span's length; max columns; max span).  Greedy, west to east: a tile grows
    while it holds <= max_cols columns and its source span - one eastward run, the columns are monotone - fits span_max
    floats, the part past the source's east edge at most one row.  ValueError when one column alone does not fit."""
    W = int(plan["grid"][1])
    pitch = int(plan["cw"].shape[1])
    if pitch > MAX_CTAP:
        raise ValueError(f"regrid: a target column takes {pitch} source columns, the kernel at most {MAX_CTAP}")
    if max_cols is None:
        max_cols = min(MAX_TILE_COLS, CW_LDS_DOUBLES // pitch)
    span_max = SPAN_MAX if span_max is None else span_max
    u0, u1 = plan["ucol0"].astype(np.int64), plan["ucol0"].astype(np.int64) + plan["ctap"]
    tiles, j, Wo = [], 0, len(u0)
    while j < Wo:
        lo, hi, n = int(u0[j]), int(u1[j]), 0
        while j + n < Wo and n < max_cols:
            nlo, nhi = min(lo, int(u0[j + n])), max(hi, int(u1[j + n]))
            # the span is staged in two pieces: up to the source's east edge, then from column 0 for at most one row
            if nhi - nlo > span_max or (nhi - nlo) - (W - nlo % W) > W:
                break
            lo, hi, n = nlo, nhi, n + 1
        if n == 0:
            raise ValueError(f"regrid: target column {j} spans {hi - lo} source columns, the kernel stages at most {span_max}")
        tiles.append((j, n, lo % W, hi - lo))
        j += n
    t = np.array(tiles, dtype=np.int32)
    return t, int(t[:, 1].max()), int(t[:, 3].max())
