"""The numpy reference of the area-weighted coarsening ("Coarsening"), shared by the CPU and the GPU
tests.  Written from the definition, not from subset.coarsen_plan: the row weights come from the sin formula on the cell
edges, the value from the sequential float64 loop in the stated order - vectorised over output points, never over taps."""
import numpy as np


def edge_lat(u, H):
    """Latitude (degrees) of the cell edge u half-rows south of the north pole, clipped to the poles."""
    return min(90.0, max(-90.0, 90.0 - u * (90.0 / (H - 1))))


def fine_band(h, H):
    """(north, south) edge of grid row h's own cell: halfway to its neighbours, the pole rows half cells."""
    return edge_lat(2 * h - 1, H), edge_lat(2 * h + 1, H)


def coarse_band(R, k_lat, H):
    return edge_lat(2 * R - k_lat, H), edge_lat(2 * R + k_lat, H)


def sind(deg):
    return float(np.sin(np.deg2rad(deg)))


def row_weights(R, k_lat, H):
    """-> (first row, [V[R, h]] for the rows h with V > 0): V = sin(min(top_R, top_h)) - sin(max(bot_R, bot_h))."""
    top_R, bot_R = coarse_band(R, k_lat, H)
    hs, vs = [], []
    for h in range(H):
        top_h, bot_h = fine_band(h, H)
        v = sind(min(top_R, top_h)) - sind(max(bot_R, bot_h))
        if v > 0.0:
            hs.append(h)
            vs.append(v)
    assert hs == list(range(hs[0], hs[0] + len(hs)))
    return hs[0], vs


def rw_table(rows, k_lat, k_lon, H):
    """-> (row0 [Ho], ntap [Ho], rw [Ho, k_lat + 1] zero-padded): rw = V / (sum of the window's V, north to south, * k_lon)."""
    row0, ntap, rw = [], [], np.zeros((len(rows), k_lat + 1))
    for i, R in enumerate(rows):
        h0, vs = row_weights(int(R), k_lat, H)
        total = 0.0
        for v in vs:
            total = total + v
        row0.append(h0)
        ntap.append(len(vs))
        for t, v in enumerate(vs):
            rw[i, t] = v / (total * k_lon)
    return np.array(row0), np.array(ntap), rw


def kept(box, k, H, W):
    """The output points of the box (r0, r1, c0, nc) | None: global rows % k_lat == 0, columns % k_lon == 0, eastward."""
    r0, r1, c0, nc = box if box is not None else (0, H, 0, W)
    rows = [r for r in range(r0, r1) if r % k[0] == 0]
    cols = [(c0 + j) % W for j in range(nc) if ((c0 + j) % W) % k[1] == 0]
    return np.array(rows), np.array(cols)


def ref_coarsen(full, k, box=None, chans=None):
    """full: float32 [C, H, W], the GLOBAL field -> float32 [C', Ho, Wo], the coarsened box, by the sequential loop:
        acc = 0;  for h north to south:  inner = 0;  for w west to east:  inner = inner + ov * x[h, w];
        acc = acc + rw[R, h] * inner;   out = float32(acc)."""
    full = np.asarray(full)
    assert full.dtype == np.float32
    x = full if chans is None else full[list(chans)]
    C, H, W = x.shape
    k_lat, k_lon = k
    rows, cols = kept(box, k, H, W)
    row0, ntap, rw = rw_table(rows, k_lat, k_lon, H)
    half = k_lon // 2
    ov = np.ones(2 * half + 1)
    if k_lon % 2 == 0 and half:
        ov[0] = ov[-1] = 0.5
    out = np.empty((C, len(rows), len(cols)), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for i in range(len(rows)):
            acc = np.zeros((C, len(cols)))
            for t in range(ntap[i]):
                h = row0[i] + t
                inner = np.zeros((C, len(cols)))
                for j in range(-half, half + 1):
                    inner = inner + ov[j + half] * x[:, h, (cols + j) % W].astype(np.float64)
                acc = acc + rw[i, t] * inner
            out[:, i] = acc.astype(np.float32)
    return out


def band_area(north, south):
    return sind(north) - sind(south)
