"""Packed int16 output and the way back to NetCDF ("Packed int16 output").

The packing itself runs on the GPU (csrc/pack.hip through ops.pack_range / ops.pack_i16); this module is the host side:
the ranges a caller may fix, the per-frame result dict, the inverse, and the writer of the ERA5 NetCDF layout that
cra5_api.read_data_from_nc reads.  Importing it needs no GPU.
"""
import datetime
import math
import os

import numpy as np

FILL = -32768      # CRA5_PACK_FILL: the code of a non-finite value, written as _FillValue / missing_value
QMAX = 32767


def _level_of(name, base):
    """"z_500", "z" -> "500"; None when `name` is not a level of the variable `base`."""
    if name.startswith(base + "_") and name[len(base) + 1:].isdigit():
        return name[len(base) + 1:]
    return None


def resolve_ranges(pack, names):
    """pack= of the decode methods -> float64 numpy [C', 2] of fixed (lo, hi) per channel of `names` (the decoded
    channels' names, in order); a NaN row: that channel takes each frame's own range.
      "int16" / True: every channel per frame.
      {variable: (lo, hi)}: a fixed PHYSICAL range for those variables, per frame for the rest.  A key is a channel name
        ("t2m", "z_500") or the name of a pressure variable ("z": every decoded level z_<level>).
    ValueError for any other type, an unknown name, a channel named twice (as itself and through its variable), a
    non-finite bound and lo >= hi."""
    names = list(names)
    fixed = np.full((len(names), 2), np.nan, dtype=np.float64)
    if pack is True or (isinstance(pack, str) and pack == "int16"):
        return fixed
    if not isinstance(pack, dict):
        raise ValueError(f"pack must be 'int16', True or a dict {{variable: (lo, hi)}}, got {pack!r}")
    for key, rng in pack.items():
        rows = [i for i, n in enumerate(names) if n == key or (isinstance(key, str) and _level_of(n, key) is not None)]
        if not rows:
            raise ValueError(f"pack: unknown variable {key!r} (the decoded channels are {names[:3]} ... {names[-2:]})")
        try:
            lo, hi = (float(v) for v in rng)
        except (TypeError, ValueError):
            raise ValueError(f"pack[{key!r}] must be (lo, hi), got {rng!r}") from None
        if not (math.isfinite(lo) and math.isfinite(hi)):
            raise ValueError(f"pack[{key!r}] = {rng!r}: the bounds must be finite")
        if not lo < hi:
            raise ValueError(f"pack[{key!r}] = {rng!r}: need lo < hi")
        for i in rows:
            if not np.isnan(fixed[i, 0]):
                raise ValueError(f"pack: channel {names[i]!r} is given a range twice")
            fixed[i] = (lo, hi)
    return fixed


def check_fixed(fixed, C):
    """A caller's [C, 2] table of fixed ranges (host values) -> float64 numpy [C, 2], checked as resolve_ranges checks."""
    fixed = np.array(fixed, dtype=np.float64)
    if fixed.shape != (C, 2):
        raise ValueError(f"fixed must be [{C}, 2] (lo, hi) per channel, NaN rows for per-frame channels; got {fixed.shape}")
    given = ~np.isnan(fixed[:, 0])
    if not (np.isfinite(fixed[given]).all() and (fixed[given, 0] < fixed[given, 1]).all()):
        raise ValueError("fixed: every given range must be finite with lo < hi")
    return fixed


def frame_stats(table, fixed=None):
    """The host view of one frame's device table (ops.pack_range: float64 [C, 5]) and of the fixed ranges it was made
    with (float64 [C, 2] | None) -> dict(scale_factor, add_offset float64 [C]; vmin, vmax float32 [C]; nonfinite int64
    [C]; saturated bool [C]: a fixed range is given and vmin < lo or vmax > hi - those points took -+32767; fill_value)."""
    table = np.asarray(table, dtype=np.float64)
    vmin, vmax = table[:, 0], table[:, 1]
    sat = np.zeros(len(table), dtype=bool)
    if fixed is not None:
        with np.errstate(invalid="ignore"):
            sat = (vmin < fixed[:, 0]) | (vmax > fixed[:, 1])      # (NaN rows and NaN vmin / vmax compare false)
    return dict(scale_factor=table[:, 3].copy(), add_offset=table[:, 4].copy(), vmin=vmin.astype(np.float32),
                vmax=vmax.astype(np.float32), nonfinite=table[:, 2].astype(np.int64), saturated=sat, fill_value=FILL)


def pack_frame(x, fixed=None, out=None):
    """Pack any fp32 device frame [C, H, W] (or [1, C, H, W]) on the GPU, on the current stream.  fixed: None or [C, 2]
    (lo, hi) per channel (numpy / nested lists; NaN rows: that channel's own range; resolve_ranges makes one).  out: an
    int16 device tensor [C, H, W] to write the codes to.  Returns dict(q: int16 device tensor [C, H, W], scale_factor,
    add_offset, vmin, vmax, nonfinite, saturated, fill_value) - frame_stats."""
    import torch
    from . import ops
    if isinstance(x, torch.Tensor) and x.dim() == 4 and x.shape[0] == 1:
        x = x[0]
    fixed_dev = None
    if fixed is not None:
        if not isinstance(x, torch.Tensor) or x.dim() != 3:
            raise ValueError("pack_frame takes a fp32 device frame [C, H, W] or [1, C, H, W]")
        fixed = check_fixed(fixed, x.shape[0])
        fixed_dev = torch.from_numpy(fixed).to(x.device)
    table = ops.pack_range(x, fixed_dev)
    q = ops.pack_i16(x, table, out=out)
    res = frame_stats(table.cpu().numpy(), fixed)
    res["q"] = q
    return res


def unpack(q, scale_factor, add_offset):
    """Codes [C, ...] (int16 numpy / tensor) -> float64 numpy: double(q) * scale_factor[c] + add_offset[c], FILL -> NaN."""
    if hasattr(q, "detach"):
        q = q.detach().cpu().numpy()
    q = np.asarray(q)
    shape = (-1,) + (1,) * (q.ndim - 1)
    sf = np.asarray(scale_factor, dtype=np.float64).reshape(shape)
    ao = np.asarray(add_offset, dtype=np.float64).reshape(shape)
    out = q.astype(np.float64) * sf + ao
    out[q == FILL] = np.nan
    return out


def error_bound(scale_factor, lo, hi):
    """The unpack bound of a finite point inside (lo, hi): scale * (0.5 + 2^-30) + 2^-50 * max(|lo|, |hi|)."""
    return np.asarray(scale_factor, dtype=np.float64) * (0.5 + 2.0 ** -30) + 2.0 ** -50 * np.maximum(np.abs(lo), np.abs(hi))


# ---- packed int16 input ("Packed int16 input") -------------------------------------------------------

_NATIVE = np.dtype(np.int16)
_OTHER = _NATIVE.newbyteorder()


class PackedFrame:
    """One frame as int16 codes with their packing - what an encode entry point takes in place of a float32 host array:
    the codes cross the host link (half the bytes) and are unpacked on the GPU (ops.unpack_i16).
      q: one int16 array [C, H, W], or a sequence of C-contiguous int16 blocks [k_i, H, W] whose k_i sum to C (views
        into file mappings: nothing is concatenated).  Native or swapped byte order, the same in every block.
      scale_factor, add_offset: float64 [C], finite.  fill_value: a scalar, [C] (a NaN entry: no fill code for that
        channel) or None (no fill code at all).  multiplier: [C] of values exact in fp32 (tp: 1000), None: all ones.
    x = float32(float64(q) * scale_factor + add_offset) * float32(multiplier), NaN at the fill code (unpack_f32).
    ValueError for wrong shapes and dtypes, mixed byte orders and non-finite scale / offset / multiplier."""

    def __init__(self, q, scale_factor, add_offset, fill_value=FILL, multiplier=None, files=()):
        blocks = [q] if isinstance(q, np.ndarray) else list(q)
        if not blocks or not all(isinstance(b, np.ndarray) for b in blocks):
            raise ValueError("PackedFrame: q must be an int16 numpy array [C, H, W] or a sequence of int16 blocks [k, H, W]")
        for b in blocks:
            if b.dtype not in (_NATIVE, _OTHER) or b.ndim != 3 or b.size == 0:
                raise ValueError(f"PackedFrame: every block must be a non-empty int16 array [k, H, W], got {b.dtype} {b.shape}")
            if b.shape[1:] != blocks[0].shape[1:]:
                raise ValueError(f"PackedFrame: the blocks differ in grid: {b.shape[1:]} and {blocks[0].shape[1:]}")
            if b.dtype.isnative != blocks[0].dtype.isnative:
                raise ValueError("PackedFrame: the blocks mix byte orders")
        if isinstance(q, np.ndarray):
            blocks = [np.ascontiguousarray(q)]
        elif not all(b.flags["C_CONTIGUOUS"] for b in blocks):
            raise ValueError("PackedFrame: every block must be C-contiguous")
        C = sum(b.shape[0] for b in blocks)
        self.blocks = blocks
        self.shape = (C,) + tuple(blocks[0].shape[1:])
        self.swapped = not blocks[0].dtype.isnative
        self.transient = False      # cra5_api sets it on the frames it reads itself: closed once staged
        self._files = list(files)

        def per_channel(name, v, dtype=np.float64):
            try:
                a = np.array(v, dtype=dtype)
            except (TypeError, ValueError):
                raise ValueError(f"PackedFrame: {name} must be numbers, [{C}]") from None
            if a.shape != (C,):
                raise ValueError(f"PackedFrame: {name} must be [{C}], got {a.shape}")
            return a
        self.scale_factor = per_channel("scale_factor", scale_factor)
        self.add_offset = per_channel("add_offset", add_offset)
        if not (np.isfinite(self.scale_factor).all() and np.isfinite(self.add_offset).all()):
            raise ValueError("PackedFrame: scale_factor and add_offset must be finite")
        if fill_value is None:
            fill_value = np.nan
        if np.ndim(fill_value) == 0:
            fill_value = np.full(C, fill_value, dtype=np.float64)
        self.fill = per_channel("fill_value", fill_value)
        given = self.fill[~np.isnan(self.fill)]
        if not ((given == np.rint(given)).all() and (given >= -32768).all() and (given <= QMAX).all()):
            raise ValueError("PackedFrame: a fill_value must be an int16 code (or NaN: none)")
        self.multiplier = per_channel("multiplier", np.ones(C) if multiplier is None else multiplier)
        with np.errstate(over="ignore"):
            exact = self.multiplier.astype(np.float32).astype(np.float64) == self.multiplier
        if not (np.isfinite(self.multiplier).all() and exact.all()):
            raise ValueError("PackedFrame: every multiplier must be finite and exact in float32")

    @classmethod
    def from_decode(cls, d):
        """The dict of decode_from_bin / decode_batch(pack=..., to_host=True) (codes under "x_hat" or "q") -> its frame:
        a packed decode can be re-encoded directly."""
        q = d["q"] if "q" in d else d["x_hat"]
        if hasattr(q, "detach"):
            q = q.detach().cpu().numpy()
        q = np.asarray(q)
        return cls(q.reshape(q.shape[-3:]), d["scale_factor"], d["add_offset"], d.get("fill_value", FILL))

    @property
    def nbytes(self):
        return 2 * self.shape[0] * self.shape[1] * self.shape[2]

    def table(self):
        """float64 [C, 4]: scale, offset, fill (NaN: none), multiplier - ops.UNPACK_FIELDS, the kernel's table."""
        return np.ascontiguousarray(np.stack([self.scale_factor, self.add_offset, self.fill, self.multiplier], axis=1))

    def byteswapped(self):
        """The same frame with its codes in the other byte order (a copy)."""
        other = _OTHER if not self.swapped else _NATIVE
        return PackedFrame([b.astype(other) for b in self.blocks], self.scale_factor, self.add_offset, self.fill,
                           self.multiplier)

    def close(self):
        """Drop the blocks and close the files they map (read_era5_nc_packed); the frame is unusable afterwards."""
        self.blocks = None
        files, self._files = self._files, []
        for f in files:
            f.close()


def unpack_f32(frame):
    """PackedFrame -> float32 numpy [C, H, W]: the definition of "Packed int16 input" on the host, channel by channel -
    float64 multiply, float64 add, one rounding to float32, one float32 multiply; NaN at the fill code."""
    out = np.empty(frame.shape, dtype=np.float32)
    mul = frame.multiplier.astype(np.float32)
    c = 0
    for blk in frame.blocks:
        for k in range(blk.shape[0]):
            q = blk[k].astype(np.int16)                       # (the values, in native order)
            d = q.astype(np.float64) * frame.scale_factor[c]
            d += frame.add_offset[c]
            with np.errstate(over="ignore", invalid="ignore"):
                x = d.astype(np.float32) * mul[c]
            if not np.isnan(frame.fill[c]):
                x[q == np.int16(frame.fill[c])] = np.float32(np.nan)
            out[c] = x
            c += 1
    return out


def read_era5_nc_packed(local_root, time_stamp, vnames, pressure_level, reason=None):
    """The frame of {local_root}/ERA5/{yyyy}/{ts}_pressure.nc / {ts}_single.nc as a PackedFrame whose blocks are views
    of the file mappings, in channel order (pressure variables x `pressure_level`, then the single-level variables; the
    file's level axis may hold more levels, in any order) - or None when the files do not hold plain packed int16:
    a file that is not NetCDF-3, a needed variable that is not i2, lacks scale_factor / add_offset or has a _FillValue
    and a missing_value that differ (the caller then reads the frame through read_data_from_nc).  tp gets the multiplier
    1000 (the model works in tp x 1000).  reason: a list that receives "<file>: <why>" with a None.  The mappings stay
    open until close() of the frame."""
    opened = []
    frame = _read_packed(f"{local_root}/ERA5/{time_stamp[:4]}", time_stamp, vnames, pressure_level, opened, reason)
    if frame is None:
        for f in opened:        # (no view of their mappings is alive any more)
            f.close()
    return frame


def _read_packed(folder, time_stamp, vnames, pressure_level, opened, reason):
    from scipy.io import netcdf_file

    def give_up(path, why):
        if reason is not None:
            reason.append(f"{path}: {why}")

    def open_nc(path):
        with open(path, "rb") as f:
            magic = f.read(4)
        if magic[:3] != b"CDF":
            return None
        opened.append(netcdf_file(path, "r", mmap=True, maskandscale=False))
        return opened[-1]

    blocks, scale, offset, fill, mul = [], [], [], [], []

    def take(path, var, name, rows):
        """`rows` (lists of consecutive indices) of the variable's [n, H, W] codes -> blocks; False: not plain packed i2."""
        att = var._attributes
        if var.data.dtype not in (_NATIVE, _OTHER):
            return give_up(path, f"variable {name!r} is {var.data.dtype.name}, not int16")
        if "scale_factor" not in att or "add_offset" not in att:
            return give_up(path, f"variable {name!r} has no scale_factor / add_offset")
        fv = [np.asarray(att[k]).reshape(-1)[0] for k in ("_FillValue", "missing_value") if k in att]
        if len(fv) == 2 and fv[0] != fv[1]:
            return give_up(path, f"variable {name!r} has _FillValue {fv[0]} and missing_value {fv[1]}")
        n = 0
        for run in rows:
            blk = var.data[0][run[0]:run[-1] + 1] if var.data.ndim == 4 else var.data[0][None]
            if not blk.flags["C_CONTIGUOUS"]:
                return give_up(path, f"variable {name!r} is not stored contiguously")
            blocks.append(blk)
            n += blk.shape[0]
        scale.extend([float(np.asarray(att["scale_factor"]).reshape(-1)[0])] * n)
        offset.extend([float(np.asarray(att["add_offset"]).reshape(-1)[0])] * n)
        fill.extend([float(fv[0]) if fv else np.nan] * n)
        mul.extend([1000.0 if name == "tp" else 1.0] * n)
        return True

    if vnames["pressure"]:
        path = f"{folder}/{time_stamp}_pressure.nc"
        nc = open_nc(path)
        if nc is None:
            return give_up(path, "not a NetCDF-3 file")
        pha = [float(v) for v in nc.variables["level"][:]]
        if not all(v in pha for v in pressure_level):
            return give_up(path, "a level of the model is missing from the level axis")
        level_mapping = [pha.index(v) for v in pressure_level]
        runs = [[level_mapping[0]]]
        for lv in level_mapping[1:]:
            if lv == runs[-1][-1] + 1:
                runs[-1].append(lv)
            else:
                runs.append([lv])
        for name in vnames["pressure"]:
            var = nc.variables[name]
            if var.data.ndim != 4:
                return give_up(path, f"variable {name!r} is not (time, level, latitude, longitude)")
            if not take(path, var, name, runs):
                return None
    if vnames["single"]:
        path = f"{folder}/{time_stamp}_single.nc"
        nc = open_nc(path)
        if nc is None:
            return give_up(path, "not a NetCDF-3 file")
        for name in vnames["single"]:
            var = nc.variables[name]
            if var.data.ndim != 3:
                return give_up(path, f"variable {name!r} is not (time, latitude, longitude)")
            if not take(path, var, name, [[0]]):
                return None
    if any(b.shape[1:] != blocks[0].shape[1:] for b in blocks):
        return give_up(folder, "the variables differ in grid")
    return PackedFrame(blocks, scale, offset, fill, mul, files=opened)


# ---- NetCDF ------------------------------------------------------------------------------------------------------------

_EPOCH = datetime.datetime(1900, 1, 1)


def hours_since_1900(time_stamp):
    """"2024-06-01T06:00:00" -> whole hours since 1900-01-01 00:00:00.0 (the ERA5 time axis)."""
    t = datetime.datetime.strptime(time_stamp[:19], "%Y-%m-%dT%H:%M:%S")
    return int((t - _EPOCH).total_seconds() // 3600)


def split_variables(variables, vnames):
    """Channel names -> (pressure: [(variable, [level strings], [channel rows])] in order of first appearance,
    single: [(variable, channel row)]).  ValueError for a name of neither kind and for a selection that is not
    rectangular (every selected pressure variable must have the same level list, in the same order)."""
    pressure, single, by_name = [], [], {}
    for i, name in enumerate(variables):
        base = next((v for v in vnames["pressure"] if _level_of(name, v) is not None), None)
        if base is not None:
            if base not in by_name:
                by_name[base] = (base, [], [])
                pressure.append(by_name[base])
            by_name[base][1].append(_level_of(name, base))
            by_name[base][2].append(i)
        elif name in vnames["single"]:
            single.append((name, i))
        else:
            raise ValueError(f"write_era5_nc: {name!r} is neither a level of a pressure variable nor a single-level variable")
    for base, levels, _ in pressure[1:]:
        if levels != pressure[0][1]:
            raise ValueError(f"write_era5_nc: the pressure selection is not rectangular - {base!r} has levels {levels}, "
                             f"{pressure[0][0]!r} has {pressure[0][1]} (one level axis per file)")
    return pressure, single


def write_era5_nc(save_root, time_stamp, packed, variables, lat, lon, vnames):
    """Write one packed frame as the NetCDF-3 (64-bit offset) files read_data_from_nc reads:
    {save_root}/ERA5/{yyyy}/{ts}_pressure.nc and {ts}_single.nc.
      packed: the dict of pack_frame / decode_batch(pack=...) - q int16 [C', H, W], scale_factor, add_offset;
      variables: the C' channel names; lat [H] / lon [W]: the decode's coordinates; vnames: dict(pressure, single).
    Dimensions time (1), level, latitude, longitude; coordinates level (f4, hPa), latitude / longitude (f4), time (i4,
    hours since 1900-01-01 00:00:00.0).  A pressure variable is ONE i2 variable (time, level, latitude, longitude) over
    the levels selected for it, in the order selected: its channels must share one scale_factor / add_offset
    (cra5_api.decode_to_nc arranges that) and the selection must be rectangular; a single-level variable is i2 (time,
    latitude, longitude).  Every data variable carries scale_factor, add_offset (float64), _FillValue and missing_value
    (int16 -32768).  tp: the model works in tp x 1000, so its scale_factor and add_offset are divided by 1000 and the
    codes left alone.  A file with no selected variable is not written.  Returns the paths written."""
    from scipy.io import netcdf_file
    variables = list(variables)
    q = packed["q"]
    if hasattr(q, "detach"):
        q = q.detach().cpu().numpy()
    q = np.asarray(q)
    lat, lon = np.asarray(lat, dtype=np.float32), np.asarray(lon, dtype=np.float32)
    if q.dtype != np.int16 or q.shape != (len(variables), len(lat), len(lon)):
        raise ValueError(f"write_era5_nc: q must be int16 [{len(variables)}, {len(lat)}, {len(lon)}], got {q.dtype} {q.shape}")
    sf = np.asarray(packed["scale_factor"], dtype=np.float64)
    ao = np.asarray(packed["add_offset"], dtype=np.float64)
    pressure, single = split_variables(variables, vnames)
    for base, _, rows in pressure:
        if not (np.all(sf[rows] == sf[rows[0]]) and np.all(ao[rows] == ao[rows[0]])):
            raise ValueError(f"write_era5_nc: the levels of {base!r} do not share one scale_factor / add_offset - a NetCDF "
                             "variable has one packing (decode_to_nc packs the levels of a variable with one range)")
    folder = f"{save_root}/ERA5/{time_stamp[:4]}"
    os.makedirs(folder, exist_ok=True)
    hours = hours_since_1900(time_stamp)

    def begin(path, levels=None):
        f = netcdf_file(path, "w", version=2)
        f.createDimension("time", 1)
        if levels is not None:
            f.createDimension("level", len(levels))
        f.createDimension("latitude", len(lat))
        f.createDimension("longitude", len(lon))
        if levels is not None:
            v = f.createVariable("level", "f4", ("level",))
            v[:] = np.array([float(s) for s in levels], dtype=np.float32)
            v.units = "millibars"
        for name, vals, units in (("latitude", lat, "degrees_north"), ("longitude", lon, "degrees_east")):
            v = f.createVariable(name, "f4", (name,))
            v[:] = vals
            v.units = units
        v = f.createVariable("time", "i4", ("time",))
        v[:] = np.array([hours], dtype=np.int32)
        v.units = "hours since 1900-01-01 00:00:00.0"
        return f

    def put(f, name, dims, codes, scale, offset):
        v = f.createVariable(name, "i2", dims)
        v[:] = codes
        if name == "tp":
            scale, offset = scale / 1000.0, offset / 1000.0
        v.scale_factor = np.float64(scale)
        v.add_offset = np.float64(offset)
        setattr(v, "_FillValue", np.int16(FILL))
        v.missing_value = np.int16(FILL)

    paths = []
    if pressure:
        path = f"{folder}/{time_stamp}_pressure.nc"
        f = begin(path, pressure[0][1])
        try:
            for base, _, rows in pressure:
                put(f, base, ("time", "level", "latitude", "longitude"), q[rows][None], sf[rows[0]], ao[rows[0]])
        finally:
            f.close()
        paths.append(path)
    if single:
        path = f"{folder}/{time_stamp}_single.nc"
        f = begin(path)
        try:
            for name, row in single:
                put(f, name, ("time", "latitude", "longitude"), q[row][None], sf[row], ao[row])
        finally:
            f.close()
        paths.append(path)
    return paths
