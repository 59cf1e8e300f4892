"""Subset decode: which grid points and channels a request names, and which tokens of the decoder's un-embed reach them.

Host-side geometry only (no model, no GPU): `grid_box` turns a lat/lon box in degrees into grid rows / columns,
`resolve_variables` turns variable names into channel indices, `token_plan` gives the patch-aligned superset of tokens the
un-embed runs on for a box (VAEformer._decode_frame; DESIGN.md, "Subset decode").

Grid convention (metrics.latitude_weights): row h is latitude 90 - h * 180 / (H - 1) (row 0 = 90 N), column w is longitude
w * 360 / W (column 0 = Greenwich, eastward).
"""
import math

import numpy as np

TOL_DEG = 1e-9        # a bound within this many degrees of a grid point is on it


def grid_box(region, H=721, W=1440):
    """region = (lat_min, lat_max, lon_min, lon_max) in degrees -> dict(rows=(r0, r1), col0, ncols, box, lat, lon).

    The box holds the grid points with lat in [lat_min, lat_max] and lon in the closed eastward interval from lon_min to
    lon_max (longitudes modulo 360: lon_max < lon_min crosses 0 deg, (-25, 45) and (335, 45) are one box).  A span of
    360 deg or more is the whole circle - W columns, the first one at lon_min.  Rows run north to south (r1 exclusive),
    columns eastward from col0 (wrapping at W).  `box` = (r0, r1, col0, ncols) is what VAEformer.decompress /
    decode_latent take; lat / lon (float64, lon in [0, 360)) are the coordinates of the rows / columns.
    Raises ValueError for an empty box, a latitude outside [-90, 90] or lat_min > lat_max."""
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
    return dict(rows=(r0, r_last + 1), col0=c0, ncols=nc, box=(r0, r_last + 1, c0, nc),
                lat=90.0 - rows * (180.0 / (H - 1)), lon=cols.astype(np.float64) * (360.0 / W))


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
