"""Subset decode: which grid points and channels a request names, and which tokens of the decoder's un-embed reach them.

Host-side geometry only (no model, no GPU): `grid_box` turns a lat/lon box in degrees into grid rows / columns,
`resolve_variables` turns variable names into channel indices, `token_plan` gives the patch-aligned superset of tokens the
un-embed runs on for a box (VAEformer._decode_frame; DESIGN.md, "Subset decode").  `resolve_stride`, `kept_points`,
`stride_plan` and `scatter_tables` are the geometry of a thinned grid (every s_lat-th row, every s_lon-th column of the
global grid): which (token, tap) products of the un-embed a thinned box needs and where each lands.  `resolve_coarsen`
and `coarsen_plan` are the geometry of the area-weighted (first-order conservative) regrid onto those same points: the
source box the windows need and the float64 row-weight table of cra5_coarsen_f32 ("Coarsening").

Grid convention (metrics.latitude_weights): row h is latitude 90 - h * 180 / (H - 1) (row 0 = 90 N), column w is longitude
w * 360 / W (column 0 = Greenwich, eastward).
"""
import math
import operator

import numpy as np

TOL_DEG = 1e-9        # a bound within this many degrees of a grid point is on it


def resolve_stride(stride, W=1440):
    """stride: None | a positive int | a pair (s_lat, s_lon) of positive ints -> (s_lat, s_lon), or None for "no
    stride" (None, 1, (1, 1): the unthinned decode).  Raises ValueError for anything that is not an integer (a float, a
    bool, a string), for a value < 1, and for W % s_lon != 0: the thinned columns are those of the GLOBAL grid with
    column % s_lon == 0, a lattice that closes round the circle only when s_lon divides W."""
    if stride is None:
        return None
    parts = stride if isinstance(stride, (tuple, list, np.ndarray)) else (stride, stride)
    try:
        if len(parts) != 2 or any(isinstance(v, (bool, np.bool_)) for v in parts):
            raise TypeError
        sy, sx = (operator.index(v) for v in parts)
    except TypeError:
        raise ValueError(f"stride must be a positive int or a pair (s_lat, s_lon) of positive ints, got {stride!r}") from None
    if sy < 1 or sx < 1:
        raise ValueError(f"stride {stride!r}: strides must be >= 1")
    if W % sx:
        raise ValueError(f"stride {stride!r}: {W} % s_lon ({sx}) = {W % sx} != 0 - the thinned columns are the global "
                         f"columns with column % s_lon == 0, which must close round the circle")
    return None if (sy, sx) == (1, 1) else (sy, sx)


def kept_points(box, stride, W=1440):
    """The grid points of the box (r0, r1, c0, nc) that a stride (s_lat, s_lon) keeps -> (rows, cols), int64 arrays of
    GLOBAL indices: the rows r of [r0, r1) with r % s_lat == 0, north to south, and the columns c of the box with
    c % s_lon == 0, in the box's eastward order (wrapping at W).  The thinned grid is anchored to the global grid, not to
    the box: a region's thinned decode is a sub-block of the globe's.  Raises ValueError when no row / column is kept."""
    r0, r1, c0, nc = (int(v) for v in box)
    sy, sx = (int(v) for v in stride)
    rows = np.arange(-(-r0 // sy) * sy, r1, sy, dtype=np.int64)
    cols = (c0 + np.arange(nc, dtype=np.int64)) % W
    cols = cols[cols % sx == 0]
    if not len(rows):
        raise ValueError(f"stride {(sy, sx)!r}: the box rows [{r0}, {r1}) hold no row with row % {sy} == 0")
    if not len(cols):
        raise ValueError(f"stride {(sy, sx)!r}: the {nc} box columns from {c0} hold no column with column % {sx} == 0")
    return rows, cols


def resolve_coarsen(coarsen, H=721, W=1440):
    """coarsen: None | a positive int | a pair (k_lat, k_lon) of positive ints -> (k_lat, k_lon), or None for "no
    coarsening" (None, 1, (1, 1)).  resolve_stride's rules: ValueError for anything that is not an integer (a float, a
    bool, a string), for a value < 1, and for (H - 1) % k_lat != 0 or W % k_lon != 0 - the coarse cells tile the sphere
    and both poles stay output rows only then."""
    if coarsen is None:
        return None
    parts = coarsen if isinstance(coarsen, (tuple, list, np.ndarray)) else (coarsen, coarsen)
    try:
        if len(parts) != 2 or any(isinstance(v, (bool, np.bool_)) for v in parts):
            raise TypeError
        ky, kx = (operator.index(v) for v in parts)
    except TypeError:
        raise ValueError(f"coarsen must be a positive int or a pair (k_lat, k_lon) of positive ints, got {coarsen!r}") from None
    if ky < 1 or kx < 1:
        raise ValueError(f"coarsen {coarsen!r}: factors must be >= 1")
    if (H - 1) % ky:
        raise ValueError(f"coarsen {coarsen!r}: ({H} - 1) % k_lat ({ky}) = {(H - 1) % ky} != 0 - the coarse latitude bands "
                         f"must tile pole to pole with both poles as output rows")
    if W % kx:
        raise ValueError(f"coarsen {coarsen!r}: {W} % k_lon ({kx}) = {W % kx} != 0 - the coarse cells must close round the "
                         f"circle")
    return None if (ky, kx) == (1, 1) else (ky, kx)


def _stride_or_coarsen(stride, coarsen, H, W):
    """-> (stride (s_lat, s_lon) | None, coarsen (k_lat, k_lon) | None); both given (neither the identity) is refused."""
    step, k = resolve_stride(stride, W), resolve_coarsen(coarsen, H, W)
    if step is not None and k is not None:
        raise ValueError(f"stride {stride!r} and coarsen {coarsen!r}: pass one of the two - coarsen=k returns the grid "
                         f"points of stride=k, area-averaged instead of sampled")
    return step, k


def _edge_lat(u, H):
    """Latitude in degrees of the cell edge u half-rows south of the north pole (u = 2 h - 1: the northern edge of row
    h's cell), clipped to the poles.  ONE expression, monotone in u: min / max of edges commute with it exactly."""
    return np.clip(90.0 - np.asarray(u, dtype=np.float64) * (90.0 / (H - 1)), -90.0, 90.0)


def coarsen_plan(box, k, H=721, W=1440):
    """The area-weighted mean onto the points a stride k = (k_lat, k_lon) keeps in the box (r0, r1, c0, nc) | None (the
    globe).  Fine cell of row h: the latitude band between the edges 2 h - 1 and 2 h + 1 (in half-rows from the north
    pole, clipped to [0, 2 (H - 1)]: the pole rows own half cells); coarse cell of output row R: the band 2 R - k_lat ..
    2 R + k_lat, clipped; columns c - k_lon / 2 .. c + k_lon / 2 (mod W), the two edge columns of an even k_lon shared
    half and half with the neighbour cells.  Returns dict(
      rows, cols: the output points (kept_points: GLOBAL indices), Ho, Wo, k = (k_lat, k_lon), grid = (H, W);
      src_box (r0, r1, c0, nc): the hull of the windows - rows[0] - k_lat // 2 .. rows[-1] + k_lat // 2 clipped at the
        poles, columns cols[0] - k_lon // 2 .. cols[-1] + k_lon // 2 eastward, (0, W) - the whole circle from column 0 -
        when that span reaches W columns;
      row0, ntap int32 [Ho]: the first GLOBAL source row and the row count of each window;
      rw float64 [Ho, k_lat + 1], zero-padded: rw[i, t] = V / (S * k_lon) with V = sin(north edge) - sin(south edge) of
        the overlap of fine row row0[i] + t with the coarse band and S the sum of the window's V, added north to south;
      lat_bnds float64 [Ho, 2] (north, south edge) and lon_bnds [Wo, 2] (west, east edge: lon -+ k_lon * 180 / W, not
        wrapped into [0, 360)) in degrees)."""
    ky, kx = (int(v) for v in k)
    if ky < 1 or kx < 1 or (H - 1) % ky or W % kx:
        raise ValueError(f"coarsen {k!r}: need k_lat >= 1 dividing {H} - 1 and k_lon >= 1 dividing {W}")
    r0, r1, c0, nc = (0, H, 0, W) if box is None else (int(v) for v in box)
    if not (0 <= r0 < r1 <= H and 0 <= c0 < W and 1 <= nc <= W):
        raise ValueError(f"box {box!r}: need 0 <= r0 < r1 <= {H}, 0 <= c0 < {W}, 1 <= nc <= {W}")
    rows, cols = kept_points((r0, r1, c0, nc), (ky, kx), W)
    Ho, Wo = len(rows), len(cols)
    umax = 2 * (H - 1)
    row0 = np.zeros(Ho, dtype=np.int32)
    ntap = np.zeros(Ho, dtype=np.int32)
    rw = np.zeros((Ho, ky + 1), dtype=np.float64)
    lat_bnds = np.zeros((Ho, 2), dtype=np.float64)
    for i, R in enumerate(int(r) for r in rows):
        un, us = max(0, 2 * R - ky), min(umax, 2 * R + ky)              # the coarse band's edges, in half-rows
        hs = [h for h in range(max(0, R - ky // 2 - 1), min(H - 1, R + ky // 2 + 1) + 1)
              if min(us, 2 * h + 1, umax) > max(un, 2 * h - 1, 0)]       # fine rows with a strip inside it
        v = [float(np.sin(np.deg2rad(_edge_lat(max(un, 2 * h - 1, 0), H))) -
                   np.sin(np.deg2rad(_edge_lat(min(us, 2 * h + 1, umax), H)))) for h in hs]
        if hs != list(range(hs[0], hs[0] + len(hs))) or len(hs) > ky + 1 or min(v) <= 0.0:
            raise AssertionError(f"coarsen plan: output row {R} has no contiguous window of positive weights")
        total = 0.0
        for x in v:                                                       # north to south, one rounding per add
            total = total + x
        row0[i], ntap[i] = hs[0], len(hs)
        rw[i, :len(hs)] = np.array(v, dtype=np.float64) / (total * kx)
        lat_bnds[i] = (_edge_lat(un, H), _edge_lat(us, H))
    sr0, sr1 = int(row0[0]), int(row0[-1] + ntap[-1])
    span = (Wo - 1) * kx + 2 * (kx // 2) + 1
    sc0, snc = ((int(cols[0]) - kx // 2) % W, span) if span < W else (0, W)
    lon = cols.astype(np.float64) * (360.0 / W)
    half = kx * (180.0 / W)
    return dict(rows=rows, cols=cols, Ho=Ho, Wo=Wo, k=(ky, kx), grid=(H, W), src_box=(sr0, sr1, sc0, snc), row0=row0, ntap=ntap, rw=rw,
                lat_bnds=lat_bnds, lon_bnds=np.stack([lon - half, lon + half], axis=1))


def grid_box(region, H=721, W=1440, stride=None, coarsen=None):
    """region = (lat_min, lat_max, lon_min, lon_max) in degrees -> dict(rows=(r0, r1), col0, ncols, box, lat, lon).

    The box holds the grid points with lat in [lat_min, lat_max] and lon in the closed eastward interval from lon_min to
    lon_max (longitudes modulo 360: lon_max < lon_min crosses 0 deg, (-25, 45) and (335, 45) are one box).  A span of
    360 deg or more is the whole circle - W columns, the first one at lon_min.  Rows run north to south (r1 exclusive),
    columns eastward from col0 (wrapping at W).  `box` = (r0, r1, col0, ncols) is what VAEformer.decompress /
    decode_latent take; lat / lon (float64, lon in [0, 360)) are the coordinates of the rows / columns.
    stride (resolve_stride): lat / lon are those of the kept rows / columns only (kept_points; `box` stays the unthinned
    box) and the dict also carries stride = (s_lat, s_lon) and kept_rows / kept_cols (global indices).
    coarsen (resolve_coarsen; not together with a stride): lat / lon, kept_rows / kept_cols are those of stride=coarsen -
    the points the area-weighted mean is returned at - and the dict carries coarsen = (k_lat, k_lon), lat_bnds [Ho, 2]
    (north, south) and lon_bnds [Wo, 2] (west, east), the edges of the coarse cells in degrees (coarsen_plan).
    Raises ValueError for an empty box, a latitude outside [-90, 90] or lat_min > lat_max, a bad stride / coarsen, both
    of them, or a box in which the stride keeps no row / no column."""
    step, coarse = _stride_or_coarsen(stride, coarsen, H, W)
    try:
        lat_min, lat_max, lon_min, lon_max = (float(v) for v in region)
    except (TypeError, ValueError):
        raise ValueError(f"region must be (lat_min, lat_max, lon_min, lon_max) in degrees, got {region!r}") from None
    if not all(math.isfinite(v) for v in (lat_min, lat_max, lon_min, lon_max)):
        raise ValueError(f"region {region!r}: bounds must be finite")
    if not (-90.0 <= lat_min <= 90.0 and -90.0 <= lat_max <= 90.0):
        raise ValueError(f"region {region!r}: latitudes must lie in [-90, 90]")
    if lat_min > lat_max:
        raise ValueError(f"region {region!r}: lat_min > lat_max")
    dlat, dlon = 180.0 / (H - 1), 360.0 / W
    eps_r, eps_c = TOL_DEG / dlat, TOL_DEG / dlon
    r0 = max(0, math.ceil((90.0 - lat_max) / dlat - eps_r))
    r_last = min(H - 1, math.floor((90.0 - lat_min) / dlat + eps_r))
    if r0 > r_last:
        raise ValueError(f"region {region!r}: no grid row lies between latitudes {lat_min} and {lat_max}")
    a = lon_min % 360.0
    first = math.ceil(a / dlon - eps_c)
    if lon_max - lon_min >= 360.0 - TOL_DEG:
        nc = W
    else:
        span = (lon_max - lon_min) % 360.0
        last = math.floor((a + span) / dlon + eps_c)
        nc = min(W, last - first + 1)
        if nc <= 0:
            raise ValueError(f"region {region!r}: no grid column lies between longitudes {lon_min} and {lon_max}")
    c0 = first % W
    rows = np.arange(r0, r_last + 1, dtype=np.float64)
    cols = (c0 + np.arange(nc)) % W
    extra = {}
    if step is not None:
        try:
            kr, cols = kept_points((r0, r_last + 1, c0, nc), step, W)
        except ValueError as e:
            raise ValueError(f"region {region!r}: {e}") from None
        rows = kr.astype(np.float64)
        extra = dict(stride=step, kept_rows=kr, kept_cols=cols)
    if coarse is not None:
        try:
            p = coarsen_plan((r0, r_last + 1, c0, nc), coarse, H, W)
        except ValueError as e:
            raise ValueError(f"region {region!r}: {e}") from None
        cols = p["cols"]
        rows = p["rows"].astype(np.float64)
        extra = dict(coarsen=coarse, kept_rows=p["rows"], kept_cols=cols, lat_bnds=p["lat_bnds"], lon_bnds=p["lon_bnds"])
    return dict(rows=(r0, r_last + 1), col0=c0, ncols=nc, box=(r0, r_last + 1, c0, nc),
                lat=90.0 - rows * (180.0 / (H - 1)), lon=cols.astype(np.float64) * (360.0 / W), **extra)


def resolve_variables(variables, vname_to_channels):
    """Variable names (e.g. ["z_500", "t_850", "t2m"]) -> their channel indices, in the order given.  None -> None.
    Raises ValueError for an empty list, an unknown name or a name given twice."""
    if variables is None:
        return None
    if isinstance(variables, (str, bytes)):
        raise ValueError(f"variables must be a list of names, got the string {variables!r}")
    names = list(variables)
    if not names:
        raise ValueError("variables: the list is empty - pass None for every variable")
    unknown = [v for v in names if v not in vname_to_channels]
    if unknown:
        raise ValueError(f"variables: unknown name(s) {unknown} (known names look like "
                         f"{list(vname_to_channels)[:3]} ... {list(vname_to_channels)[-2:]})")
    dup = sorted({v for v in names if names.count(v) > 1})
    if dup:
        raise ValueError(f"variables: name(s) given more than once: {dup}")
    return [int(vname_to_channels[v]) for v in names]


def token_plan(box, H, W, kh=11, kw=10, sh=10, sw=10):
    """The patch-aligned superset of tokens whose un-embed patches reach the box (r0, r1, c0, nc) (rows [r0, r1), columns
    c0 .. c0 + nc - 1 mod W).  Geometry of the ERA5 un-embed: kh = sh + 1 (one shared row between vertically adjacent
    patches), kw = sw (no column overlap).  Returns dict(ti0, n_ti, tj0, n_tj, Hs, Ws, r_off, c_off, Hb, Wb, exact):
      token rows ti0 .. ti0 + n_ti - 1 = every token whose kh-row footprint meets the box; the superset's own top / bottom
        row then lacks its seam partner only where that row lies outside the box or on the grid's edge;
      token columns tj0 .. tj0 + n_tj - 1 mod Wp cover the box, n_tj rounded up to even (the fused un-embed wants the
        superset width % 4 == 0) and capped at Wp - a capped superset is the whole circle from column 0;
      the superset image is [Hs = sh * n_ti + 1, Ws = sw * n_tj]; the box is its rows r_off .. r_off + Hb - 1 and columns
        c_off .. c_off + Wb - 1 mod Ws; exact: the superset IS the box (no crop)."""
    if kh != sh + 1 or kw != sw:
        raise ValueError("subset decode needs the ERA5 un-embed geometry (kh = sh + 1, kw = sw)")
    Hp, Wp = (H - kh) // sh + 1, (W - kw) // sw + 1
    r0, r1, c0, nc = (int(v) for v in box)
    if not (0 <= r0 < r1 <= H and 0 <= c0 < W and 1 <= nc <= W):
        raise ValueError(f"box {box!r}: need 0 <= r0 < r1 <= {H}, 0 <= c0 < {W}, 1 <= nc <= {W}")
    ti0 = max(0, -(-r0 // sh) - 1)
    ti1 = min(Hp - 1, (r1 - 1) // sh)
    tj0 = c0 // sw
    n_tj = (c0 + nc - 1) // sw - tj0 + 1
    n_tj += n_tj % 2
    if n_tj >= Wp:
        tj0, n_tj = 0, Wp
    n_ti = ti1 - ti0 + 1
    Hs, Ws = sh * n_ti + 1, sw * n_tj
    r_off, c_off = r0 - sh * ti0, (c0 - sw * tj0) % Ws
    return dict(ti0=ti0, n_ti=n_ti, tj0=tj0, n_tj=n_tj, Hs=Hs, Ws=Ws, r_off=r_off, c_off=c_off, Hb=r1 - r0, Wb=nc,
                exact=(r_off == 0 and r1 - r0 == Hs and c_off == 0 and nc == Ws))


def stride_plan(box, stride, H, W, kh=11, kw=10, sh=10, sw=10, C=1):
    """The un-embed products a thinned box needs.  box = (r0, r1, c0, nc) | None (the globe); stride = (s_lat, s_lon)
    (kept_points: anchored to the global grid; (1, 1) is allowed here and gives one class with every tap).

    Token row ti writes image rows sh * ti + ky (ky < kh), so its kept taps are {ky : (sh * ti + ky) % s_lat == 0}; that
    set depends on ti % P_r only (P_r = s_lat / gcd(sh, s_lat)): the token rows fall into at most P_r ROW CLASSES, the
    token columns likewise into at most P_c = s_lon / gcd(sw, s_lon) COLUMN CLASSES of taps {kx : (sw * tj + kx) % s_lon
    == 0} (W % s_lon == 0 makes the classes survive the wrap at the east edge).  A class pair (row class, column class)
    is one small GEMM: its tokens x (channels x its ky taps x its kx taps).  Returns dict(
      rows, cols: the kept global rows / columns (kept_points); Ho, Wo: their counts - the thinned image is [C, Ho, Wo];
      row_classes: [dict(t0, step, n, taps, land)]: token rows t0, t0 + step, .. (n of them: those with a tap inside the
        box - a kept seam row's partner outside the box's own token range included), taps = the class's ky, land int32
        [n, len(taps)]: where (token row, ky) lands -  >= 0: that row of the thinned image (its only contribution);
        -1: outside the box (computed, not used);  <= -2: seam slot -2 - (2 * s + slot) of seam s;
      col_classes: the same along the columns (t0 + i * step mod Wp, eastward from the box's first token column; land
        >= 0 | -1; kw == sw: no seams);
      seams: int32 [n_seam], the thinned-image row of each kept seam row (image row sh * t, 0 < t < Hp: the sum of token
        row t - 1 at ky = kh - 1 - slot 0, the UPPER partner, added first - and token row t at ky = 0 - slot 1);
      needed_elems: C x the (token, tap) products that land in the thinned box (a seam row counts twice);
      gemm_elems: the sum of M x N over the class GEMMs (M = n_ti * n_tj tokens, N = C * n_ky * n_kx columns; the GEMM
        launchers bound-check their edge tiles and need no padded operand or output, so this is what is computed))."""
    if kh != sh + 1 or kw != sw:
        raise ValueError("subset decode needs the ERA5 un-embed geometry (kh = sh + 1, kw = sw)")
    Hp, Wp = (H - kh) // sh + 1, (W - kw) // sw + 1
    r0, r1, c0, nc = (0, H, 0, W) if box is None else (int(v) for v in box)
    if not (0 <= r0 < r1 <= H and 0 <= c0 < W and 1 <= nc <= W):
        raise ValueError(f"box {box!r}: need 0 <= r0 < r1 <= {H}, 0 <= c0 < {W}, 1 <= nc <= {W}")
    sy, sx = (int(v) for v in stride)
    if sy < 1 or sx < 1 or W % sx:
        raise ValueError(f"stride {stride!r}: need s_lat >= 1, s_lon >= 1 and {W} % s_lon == 0")
    rows, cols = kept_points((r0, r1, c0, nc), (sy, sx), W)
    Ho, Wo = len(rows), len(cols)
    out_row = np.full(H, -1, dtype=np.int64)
    out_row[rows] = np.arange(Ho)
    out_col = np.full(W, -1, dtype=np.int64)
    out_col[cols] = np.arange(Wo)
    seam_rows = [int(r) for r in rows if r % sh == 0 and 0 < r < H - 1]
    seam_of = {r: s for s, r in enumerate(seam_rows)}

    row_classes = []
    Pr = sy // math.gcd(sh, sy)
    for k in range(Pr):
        taps = tuple(ky for ky in range(kh) if (sh * k + ky) % sy == 0)
        tis = [ti for ti in range(k, Hp, Pr) if any(r0 <= sh * ti + ky < r1 for ky in taps)]
        if not taps or not tis:
            continue
        land = np.full((len(tis), len(taps)), -1, dtype=np.int32)
        for i, ti in enumerate(tis):
            for a, ky in enumerate(taps):
                r = sh * ti + ky
                if not r0 <= r < r1:
                    continue
                if r in seam_of:     # ky == kh - 1: this token row is the one above the seam (upper, slot 0)
                    land[i, a] = -2 - (2 * seam_of[r] + (0 if ky == kh - 1 else 1))
                else:
                    land[i, a] = out_row[r]
        assert tis == list(range(tis[0], tis[0] + Pr * len(tis), Pr))
        row_classes.append(dict(t0=tis[0], step=Pr, n=len(tis), taps=taps, land=land))

    col_classes = []
    Pc = sx // math.gcd(sw, sx)
    u0 = c0 // sw
    for k in range(Pc):
        taps = tuple(kx for kx in range(kw) if (sw * k + kx) % sx == 0)
        qs = [q for q in range(Wp) if (u0 + q) % Wp % Pc == k
              and any(out_col[sw * ((u0 + q) % Wp) + kx] >= 0 for kx in taps)]
        if not taps or not qs:
            continue
        assert qs == list(range(qs[0], qs[0] + Pc * len(qs), Pc))
        tjs = [(u0 + q) % Wp for q in qs]
        land = np.array([[out_col[sw * tj + kx] for kx in taps] for tj in tjs], dtype=np.int32)
        col_classes.append(dict(t0=tjs[0], step=Pc, n=len(tjs), taps=taps, land=land))

    n_r = sum(int((rc["land"] != -1).sum()) for rc in row_classes)
    n_c = sum(int((cc["land"] != -1).sum()) for cc in col_classes)
    gemm = sum(rc["n"] * cc["n"] * C * len(rc["taps"]) * len(cc["taps"]) for rc in row_classes for cc in col_classes)
    return dict(rows=rows, cols=cols, Ho=Ho, Wo=Wo, row_classes=row_classes, col_classes=col_classes,
                seams=np.array([out_row[r] for r in seam_rows], dtype=np.int32), needed_elems=C * n_r * n_c,
                gemm_elems=gemm)


SCATTER_ALIGN = 64      # class matrices start at multiples of this many floats in the workspace (256 bytes)


def scatter_tables(plan, C):
    """The lookup tables of ops.strided_scatter (cra5_strided_scatter_f32) for a stride_plan and C channels.  The class
    matrices G[rc][cc] = [n_ti * n_tj tokens, C * n_ky * n_kx columns (c, ky, kx)] lie in ONE fp32 workspace; -> dict(
      rows int32 [Ho, 6]: per thinned row its contributions (row class, token-row index, ky index) x 2 - a seam row has
        two, UPPER first; every other row one, the second triple is (-1, 0, 0);
      cols int32 [Wo, 3]: per thinned column (column class, token-column index, kx index);
      cls int64 [n_rc * n_cc, 5]: per class pair (element offset of its matrix in the workspace, row pitch, n_tj, n_kx,
        n_ky * n_kx);
      n_cc, elems: workspace size in floats;  gemms: [(rc, cc, offset, M, N)] in launch order)."""
    rcs, ccs = plan["row_classes"], plan["col_classes"]
    Ho, Wo = plan["Ho"], plan["Wo"]
    rows = np.zeros((Ho, 6), dtype=np.int32)
    rows[:, 0] = rows[:, 3] = -1
    for k, rc in enumerate(rcs):
        for (i, a), v in np.ndenumerate(rc["land"]):
            if v >= 0:
                rows[v, 0:3] = (k, i, a)
            elif v <= -2:
                s, slot = divmod(-2 - int(v), 2)
                rows[plan["seams"][s], 3 * slot:3 * slot + 3] = (k, i, a)
    cols = np.full((Wo, 3), -1, dtype=np.int32)
    for k, cc in enumerate(ccs):
        for (i, a), v in np.ndenumerate(cc["land"]):
            if v >= 0:
                cols[v] = (k, i, a)
    seam = np.zeros(Ho, dtype=bool)
    seam[plan["seams"]] = True
    if (rows[:, 0] < 0).any() or (cols[:, 0] < 0).any() or ((rows[:, 3] >= 0) != seam).any():
        raise AssertionError("stride plan: a kept row / column has no source, or a seam row lacks a partner")
    cls = np.zeros((len(rcs) * len(ccs), 5), dtype=np.int64)
    gemms, off = [], 0
    for i, rc in enumerate(rcs):
        for j, cc in enumerate(ccs):
            M, N = rc["n"] * cc["n"], C * len(rc["taps"]) * len(cc["taps"])
            cls[i * len(ccs) + j] = (off, N, cc["n"], len(cc["taps"]), len(rc["taps"]) * len(cc["taps"]))
            gemms.append((i, j, off, M, N))
            off += -(-M * N // SCATTER_ALIGN) * SCATTER_ALIGN
    return dict(rows=rows, cols=cols, cls=cls, n_cc=len(ccs), elems=off, gemms=gemms)
