"""Error-bounded residual layer, host side: tolerances, the `.res` sidecar container and its errors (no GPU needed).

A sidecar holds, for one frame, the quantised corrections that bring every point of the corrected channels within tol[c] of
the truth once they are added to the plain decode of the `.bin` beside it ("Residual layer"; the
kernels are csrc/residual.hip, their launchers ops.residual_quantize / residual_apply / residual_gather).

Container (little-endian), `pack` / `unpack`:
  magic    8 bytes  b"CRA5RES1"
  header   <IIIQQI  C, H, W, n (records), m (escapes), nw (witnesses)
  tol      float32 [C]      (+inf: the channel is not corrected)
  widx     uint32 [nw]      witness points: flat global indexes floor(i * C*H*W / nw), nw = min(1024, C*H*W)
  wbits    uint32 [nw]      the bits of the UNCORRECTED decode there, taken on the encoder
  payload  four arrays - idx as first differences (uint32 [n]), q (int16 [n]), eidx as first differences (uint32 [m]), ebits
           (uint32 [m]) - each split into its byte planes, every plane as <I length + zlib stream
  crc      <I  CRC-32 of everything before it
A better entropy coder for the payload is out of scope: byte planes + deflate is the standard library, vectorised numpy.
"""
import numbers
import struct
import zlib

import numpy as np

MAGIC = b"CRA5RES1"
HEADER = struct.Struct("<IIIQQI")
WITNESSES = 1024
MAX_TOL = 1e30           # ops.RESIDUAL_MAX_TOL: step = 2 * tol stays finite in fp32


class ResidualFormatError(ValueError):
    """The bytes are not a residual sidecar: bad magic, truncated, CRC mismatch, or indexes that do not ascend inside the
    frame."""


class ResidualMismatchError(RuntimeError):
    """A witness differs: the plain decode the corrections would be added to is not the one the encoder saw."""


class ResidualBudgetError(ValueError):
    """Records + escapes exceed max_fraction of the points of the corrected channels."""


def _bound(what, v):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (numbers.Real, np.floating, np.integer)):
        raise ValueError(f"max_error: {what} must be a positive number, got {v!r}")
    v = float(v)
    if not (np.isfinite(v) and v > 0):
        raise ValueError(f"max_error: {what} must be finite and > 0, got {v!r}")
    return v


def resolve_tolerance(max_error, vname_to_channels, std):
    """max_error -> the per-channel tolerance, float32 [C] (C = len(std)), in PHYSICAL units.
      a positive number e: tol[c] = float32(e * std[c]) - a bound of e in the codec's normalised units, every channel
        corrected;
      a dict {variable name: bound in physical units}: those channels get their bound, every other channel +inf (not
        corrected, no records).
    ValueError for a non-positive or non-finite value, an unknown name, an empty dict, a bool, a string, or a tolerance
    above 1e30."""
    std = np.asarray(std, dtype=np.float64).reshape(-1)
    C = len(std)
    if isinstance(max_error, dict):
        if not max_error:
            raise ValueError("max_error: the dict is empty - pass None for no residual layer")
        tol = np.full(C, np.inf, dtype=np.float32)
        unknown = [v for v in max_error if not (v in vname_to_channels and 0 <= int(vname_to_channels[v]) < C)]
        if unknown:
            raise ValueError(f"max_error: unknown variable name(s) {unknown}")
        for v, e in max_error.items():
            tol[int(vname_to_channels[v])] = np.float32(_bound(f"the bound of {v!r}", e))
    else:
        if isinstance(max_error, (str, bytes)):
            raise ValueError(f"max_error must be a positive number or a dict {{variable: bound}}, got the string {max_error!r}")
        tol = (_bound("the bound", max_error) * std).astype(np.float32)
    bad = ~(np.isposinf(tol) | (np.isfinite(tol) & (tol > 0) & (tol <= np.float32(MAX_TOL))))
    if bad.any():
        c = int(np.flatnonzero(bad)[0])
        raise ValueError(f"max_error: the tolerance of channel {c} is {tol[c]!r} in float32; it must lie in (0, {MAX_TOL:g}]")
    return tol


def witness_indices(C, H, W):
    """The flat global indexes of the witness points: uint32 [min(1024, C*H*W)], floor(i * C*H*W / count)."""
    N = int(C) * int(H) * int(W)
    nw = min(WITNESSES, N)
    return ((np.arange(nw, dtype=np.uint64) * np.uint64(N)) // np.uint64(nw)).astype(np.uint32)


def check_budget(per_channel, tol, points_per_channel, max_fraction, names=None):
    """ResidualBudgetError when records + escapes exceed max_fraction of the points of the corrected channels; the message
    names the three densest channels and their share.  per_channel int [C, 2]; max_fraction None: no check."""
    if max_fraction is None:
        return
    per = np.asarray(per_channel, dtype=np.int64).sum(axis=1)
    on = np.isfinite(np.asarray(tol, dtype=np.float32))
    total = int(on.sum()) * int(points_per_channel)
    if total == 0 or per.sum() <= float(max_fraction) * total:
        return
    share = per / float(points_per_channel)
    top = np.argsort(-share, kind="stable")[:3]
    worst = ", ".join(f"{names[c] if names is not None else c} {100.0 * share[c]:.1f} %" for c in top)
    raise ResidualBudgetError(
        f"the residual layer would store {int(per.sum())} corrections for {total} points of the corrected channels "
        f"({100.0 * per.sum() / total:.1f} %, max_fraction = {100.0 * float(max_fraction):.1f} %); densest channels: {worst}. "
        "The tolerance lies far below the codec's own error there: loosen it, or raise max_fraction on purpose")


def _planes(a, level):
    b = np.ascontiguousarray(a).view(np.uint8).reshape(len(a), a.dtype.itemsize)
    out = []
    for p in range(a.dtype.itemsize):
        z = zlib.compress(np.ascontiguousarray(b[:, p]).tobytes(), level)
        out += [struct.pack("<I", len(z)), z]
    return out


def _diffs(idx):
    idx = np.ascontiguousarray(idx, dtype=np.uint32)
    d = idx.copy()
    d[1:] -= idx[:-1]
    return d


def pack(C, H, W, tol, widx, wbits, idx, q, eidx, ebits, level=6):
    """-> the sidecar's bytes.  tol float32 [C]; widx / wbits uint32 [nw]; idx uint32 [n] and eidx uint32 [m] strictly
    ascending and below C*H*W; q int16 [n]; ebits uint32 [m]."""
    tol = np.ascontiguousarray(tol, dtype=np.float32)
    widx, wbits = np.ascontiguousarray(widx, dtype=np.uint32), np.ascontiguousarray(wbits, dtype=np.uint32)
    idx, eidx = np.ascontiguousarray(idx, dtype=np.uint32), np.ascontiguousarray(eidx, dtype=np.uint32)
    q, ebits = np.ascontiguousarray(q, dtype=np.int16), np.ascontiguousarray(ebits, dtype=np.uint32)
    N = int(C) * int(H) * int(W)
    if tol.shape != (C,) or widx.shape != wbits.shape or idx.shape != q.shape or eidx.shape != ebits.shape or N >= 1 << 32:
        raise ValueError("residual.pack: array lengths do not fit the header (tol [C], widx / wbits, idx / q, eidx / ebits), "
                         "or C*H*W >= 2^32")
    for name, a in (("idx", idx), ("eidx", eidx)):
        if len(a) and (int(a[-1]) >= N or (len(a) > 1 and not (a[1:] > a[:-1]).all())):
            raise ValueError(f"residual.pack: {name} must ascend strictly and stay below C*H*W")
    parts = [MAGIC, HEADER.pack(C, H, W, len(idx), len(eidx), len(widx)), tol.tobytes(), widx.tobytes(), wbits.tobytes()]
    for a in (_diffs(idx), q, _diffs(eidx), ebits):
        parts += _planes(a, level)
    body = b"".join(parts)
    return body + struct.pack("<I", zlib.crc32(body) & 0xffffffff)


def unpack(blob):
    """The sidecar's bytes -> dict(C, H, W, tol, widx, wbits, idx, q, eidx, ebits) (numpy arrays of pack's dtypes).
    ResidualFormatError for a bad magic, truncated bytes, a CRC mismatch, or indexes that do not ascend below C*H*W."""
    blob = bytes(blob)
    if len(blob) < len(MAGIC) or blob[:len(MAGIC)] != MAGIC:
        raise ResidualFormatError(f"not a residual sidecar: the bytes start with {blob[:8]!r}, not {MAGIC!r}")
    if len(blob) < len(MAGIC) + HEADER.size + 4:
        raise ResidualFormatError(f"residual sidecar truncated: {len(blob)} bytes hold no header")
    if zlib.crc32(blob[:-4]) & 0xffffffff != struct.unpack("<I", blob[-4:])[0]:
        raise ResidualFormatError("residual sidecar: CRC mismatch - the file is truncated or damaged")
    end = len(blob) - 4
    pos = len(MAGIC)
    C, H, W, n, m, nw = HEADER.unpack_from(blob, pos)
    pos += HEADER.size
    N = C * H * W
    if not (C > 0 and H > 0 and W > 0 and N < 1 << 32 and n <= N and m <= N and nw <= N):
        raise ResidualFormatError(f"residual sidecar: header (C, H, W, n, m, witnesses) = {(C, H, W, n, m, nw)} is inconsistent")

    def take(count, dtype):
        nonlocal pos
        nb = count * np.dtype(dtype).itemsize
        if pos + nb > end:
            raise ResidualFormatError("residual sidecar truncated inside its tables")
        a = np.frombuffer(blob, dtype=dtype, count=count, offset=pos).copy()
        pos += nb
        return a

    def planes(count, dtype):
        nonlocal pos
        size = np.dtype(dtype).itemsize
        b = np.empty((count, size), dtype=np.uint8)
        for p in range(size):
            if pos + 4 > end:
                raise ResidualFormatError("residual sidecar truncated inside its payload")
            (nz,) = struct.unpack_from("<I", blob, pos)
            pos += 4
            if pos + nz > end:
                raise ResidualFormatError("residual sidecar truncated inside its payload")
            try:
                raw = zlib.decompress(blob[pos:pos + nz])
            except zlib.error as e:
                raise ResidualFormatError(f"residual sidecar: a payload plane does not inflate ({e})") from None
            pos += nz
            if len(raw) != count:
                raise ResidualFormatError(f"residual sidecar: a payload plane holds {len(raw)} bytes for {count} entries")
            b[:, p] = np.frombuffer(raw, dtype=np.uint8)
        return b.view(dtype).reshape(count)

    tol = take(C, np.float32)
    widx, wbits = take(nw, np.uint32), take(nw, np.uint32)
    didx, q = planes(n, np.uint32), planes(n, np.int16)
    deidx, ebits = planes(m, np.uint32), planes(m, np.uint32)
    if pos != end:
        raise ResidualFormatError(f"residual sidecar: {end - pos} stray bytes after the payload")
    out = []
    for name, d in (("idx", didx), ("eidx", deidx)):
        full = np.cumsum(d, dtype=np.uint64)
        if len(d) and ((d[1:] == 0).any() or int(full[-1]) >= N):
            raise ResidualFormatError(f"residual sidecar: {name} does not ascend strictly below C*H*W = {N}")
        out.append(full.astype(np.uint32))
    if len(widx) and int(widx.max()) >= N:
        raise ResidualFormatError(f"residual sidecar: a witness index lies outside C*H*W = {N}")
    return dict(C=C, H=H, W=W, tol=tol, widx=widx, wbits=wbits, idx=out[0], q=q, eidx=out[1], ebits=ebits)


def sidecar_path(bin_path):
    """The `.res` beside a `.bin`: the same path with the extension replaced ({save_root}/{yyyy}/{ts}.res)."""
    p = str(bin_path)
    return (p[:-4] if p.endswith(".bin") else p) + ".res"


def check_witnesses(inside, got_bits, wbits, what="residual"):
    """ResidualMismatchError when a witness inside the decoded subset differs from the stored bits.  inside: bool [nw];
    got_bits / wbits: uint32 [nw].  Witnesses outside the subset are not checked."""
    inside = np.asarray(inside, dtype=bool)
    bad = inside & (np.asarray(got_bits, dtype=np.uint32) != np.asarray(wbits, dtype=np.uint32))
    if bad.any():
        raise ResidualMismatchError(
            f"{what}: {int(bad.sum())} of {int(inside.sum())} witness points of the plain decode differ from the bits the "
            "encoder stored: this decoder's x_hat is not the encoder's (other weights, engine or precision settings), so "
            "applying the corrections would be wrong; nothing was corrected")
