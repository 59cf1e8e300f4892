"""`cra5_api` - the user API of the reference (cra5/api/cra5_api.py:22-341 in
taohan10200/CRA5) on top of the MI355X-native VAEformer.

Same class / method names, argument meaning, returned dict keys and on-disk layout
(`{local_root}/ERA5/{yyyy}/{ts}_{pressure,single}.nc` in, `{save_root}/{yyyy}/{ts}.bin`
out).  Conscious differences:
  * the CDS downloader (network, credentials in the reference source) is created lazily,
    only when `download_era5_data` is called, and only if `cdsapi` is importable;
  * every method that takes a `time_stamp` also accepts an in-memory array/tensor
    `data=` (268x721x1440, physical units) - the GPU box has neither NetCDF files nor
    xarray;
  * `weights=` lets the caller pass a ready model (synthetic weights offline); the
    default tries the reference checkpoint and raises the reference's error if absent;
  * normalisation is fused into the patch gather and de-normalisation into the
    overlap-add store (one pass over the 1.1 GB frame instead of two);
  * the reference's `return_format='de_normlized'` default typo (returns None) is kept
    as an accepted alias of 'de_normalized' rather than reproduced;
  * a frame with NaN / inf values raises ValueError at the encode edge (the reference would code `int(NaN)`
    garbage silently; masked NetCDF values arrive as NaN);
  * host arrays move through a pinned staging buffer in chunks (csrc/runtime.hip) instead of `.to(device)` /
    `.cpu()`: `decode_from_bin(..., to_host=True | out=array)` returns the reconstruction as a host array;
  * the leg the reference lacks, .bin -> .nc: `decode_to_nc` writes the layout `read_data_from_nc` reads, packed to int16 on
    the GPU (`pack=` of `decode_from_bin` / `decode_batch`; cra5_amd/pack.py).
"""
import contextlib
import json
import os
import threading
import time
from pathlib import Path
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import binfmt, ops, subset
from . import pack as _pk
from . import residual as _res
from .config import RuntimeConfig, runtime_setting
from .zoo import vaeformer_pretrained

_HERE = os.path.dirname(os.path.abspath(__file__))


def _variables_of(config=None):
    """(ERA5 statistics, vnames, total_levels, pressure_level) of the default 268-variable set, or of a reference-style
    python config file that overrides `vnames` / `pressure_level` (cra5_268v_config.py:48-54)."""
    with open(os.path.join(_HERE, "data", "era5_stats.json")) as f:
        stats = json.load(f)
    vnames = dict(pressure=list(stats["pressure"]), single=list(stats["single"]))
    total_levels = list(stats["total_levels"])
    pressure_level = list(total_levels)
    if config is not None:
        ns = {}
        exec(compile(open(config).read(), config, "exec"), ns)  # noqa: S102 (user-supplied config file)
        vnames = ns.get("vnames", vnames)
        pressure_level = ns.get("pressure_level", pressure_level)
    return stats, vnames, total_levels, pressure_level


def _channel_mapping(vnames, pressure_level):
    """cra5_api.py:228-241: pressure variables x levels, then the single-level variables."""
    c2v, v2c = {}, {}
    ch = 0
    for v in vnames['pressure']:
        for level in pressure_level:
            c2v[ch] = v + '_' + str(int(level))
            v2c[v + '_' + str(int(level))] = ch
            ch += 1
    for v in vnames['single']:
        c2v[ch] = v
        v2c[v] = ch
        ch += 1
    return c2v, v2c


def variable_mapping(config=None):
    """(channels_to_vname, vname_to_channels) of the default 268-variable set or of a config file (e.g. a 159-variable
    one) - what cra5_api(config=...).channel_vname_mapping() returns, without a model or a GPU."""
    _, vnames, _, pressure_level = _variables_of(config)
    return _channel_mapping(vnames, pressure_level)


class Selection(NamedTuple):
    """What one decode returns of the frame (cra5_api._select): the model's canonical arguments and the grid they leave."""
    channels: Optional[tuple]       # canonical (VAEformer._selection_args): None = every channel / the globe / no
    box: Optional[tuple]            # thinning / no coarsening
    step: Optional[tuple]
    coarsen: Optional[tuple]
    names: list                     # of the decoded channels, in their order - for the whole grid too
    lat: np.ndarray                 # float64 coordinates of the decoded rows / columns
    lon: np.ndarray
    lat_bnds: Optional[np.ndarray]  # the coarse cells' edges; None without coarsen
    lon_bnds: Optional[np.ndarray]
    shape: tuple                    # (C', Hb, Wb) of one decoded frame
    whole: bool                     # no argument asked for a subset: decode_from_bin's dict carries no extra keys
    regrid: Optional[dict] = None   # the target grid's plan (VAEformer._regrid_arg); lat / lon / the bounds are then its
    points: Optional[dict] = None   # the point list's plan (VAEformer._points_arg); shape is then (C', P), lat / lon [P]

    @property
    def model(self):
        """The keyword arguments of _decompress_frame / _decode_guarded / decode_latent (regrid / points only when asked
        for)."""
        kw = dict(channels=self.channels, box=self.box, step=self.step, coarsen=self.coarsen)
        if self.regrid is not None:
            kw["regrid"] = self.regrid
        if self.points is not None:
            kw["points"] = self.points
        return kw

    @property
    def meta(self):
        """The result dicts' keys: variables, lat, lon - with coarsen also coarsen, lat_bnds, lon_bnds; with regrid also
        regrid (the method), lat_bnds, lon_bnds; with points: lat, lon are the points' (float64 [P]), also points (the
        method) and, for "nearest", node_lat, node_lon - the grid point each one took."""
        meta = dict(variables=self.names, lat=self.lat, lon=self.lon)
        if self.points is not None:
            meta.update(points=self.points["method"])
            if self.points["method"] == "nearest":
                meta.update(node_lat=self.points["node_lat"], node_lon=self.points["node_lon"])
        if self.coarsen is not None:
            meta.update(coarsen=self.coarsen, lat_bnds=self.lat_bnds, lon_bnds=self.lon_bnds)
        if self.regrid is not None:
            meta.update(regrid=self.regrid["method"], lat_bnds=self.lat_bnds, lon_bnds=self.lon_bnds)
        return meta


class cra5_api:
    def __init__(self, config=None, local_root=None, device=None, ceph_cfg=None, weights=None, quality=268, runtime=None):
        self.device = device or ('cuda' if torch.cuda.is_available() else 'cpu')
        print(f'The serving device is {self.device}')
        # (a reference-style python config may override vnames / levels)
        self._stats, self.vnames, self.total_levels, self.pressure_level = _variables_of(config)
        self.level_mapping = [self.total_levels.index(v) for v in self.pressure_level if v in self.total_levels]
        mean, std = self.get_mean_std()
        self.mean = torch.from_numpy(mean[:, np.newaxis, np.newaxis]).to(self.device)
        self.std = torch.from_numpy(std[:, np.newaxis, np.newaxis]).to(self.device)
        self._mean_flat = self.mean.reshape(-1).contiguous()
        self._std_flat = self.std.reshape(-1).contiguous()
        self.channels_to_vname, self.vname_to_channels = self.channel_vname_mapping()
        self.local_root = local_root or f'{os.getcwd()}/data'
        # settings: ONE RuntimeConfig (cra5_amd/config.py); batch_copy_threads / link_serial are properties over it
        self.runtime = runtime if runtime is not None else (getattr(weights, "runtime", None) or RuntimeConfig.from_env())
        self._link_gate = {"h2d": threading.Lock(), "d2h": threading.Lock()}
        self.phase_log = None       # a list: (frame tag, phase, t_start, t_end) per batch-path phase (tools/api_phase_probe.py)
        self._era5 = None
        if weights is not None:
            self.net = weights.eval().to(self.device)
        else:
            self.net = vaeformer_pretrained(quality=quality, pretrained=True, runtime=self.runtime).eval().to(self.device)

    # batch methods: host threads per frame copy between pageable and pinned memory (1 = one numpy copy on the frame thread)
    batch_copy_threads = runtime_setting("batch_copy_threads")
    # batch methods: ONE frame per direction on the host link at a time (round 6).  Twelve frame threads that all issue
    # their 1.11 GB H2D at once share the link - every frame lands after 12 transfer times, the GPU idles until then and
    # the frames then queue for it in a convoy; one at a time, the first frame lands after one transfer time and the GPU
    # starts while the next frame is on the wire.  The link itself runs 57 GB/s in either direction and 97 GB/s both ways
    # at once (profiles/r06_link_probe.txt), so H2D and D2H get a gate each.
    link_serial = runtime_setting("link_serial")

    # ------------------------------------------------------------------ ingest
    def download_era5_data(self, time_stamp=None, save_root=None, data_formate="nc"):
        raise RuntimeError("ERA5 download needs network access + the CDS API (out of scope offline); "
                           "place the NetCDF files under {local_root}/ERA5/{yyyy}/ or pass data=")

    @staticmethod
    def _open_nc(path):
        """-> (get(name) -> ndarray with packing (scale_factor / add_offset / _FillValue) undone, close()).
        xarray + netCDF4 when importable (what the reference uses, cra5_api.py:203-208); otherwise
        scipy.io.netcdf_file, which reads the NetCDF-3 classic / 64-bit-offset files the CDS legacy
        API delivers (NetCDF-4 / HDF5 files need xarray)."""
        try:
            import xarray as xr
        except ImportError:
            xr = None
        if xr is not None:
            ds = xr.open_dataset(path, engine='netcdf4')
            return (lambda name: ds[name].data), ds.close
        from scipy.io import netcdf_file
        with open(path, "rb") as f:
            magic = f.read(4)
        if magic[:3] != b"CDF":
            raise RuntimeError(f"{path}: not a NetCDF-3 file (magic {magic!r}); reading NetCDF-4 needs xarray + "
                               "netCDF4, which this image lacks - pass data= instead")
        nc = netcdf_file(path, "r", mmap=False, maskandscale=True)

        def get(name):
            a = np.ma.filled(nc.variables[name][:], np.nan)
            return np.asarray(a, dtype=np.float32 if a.dtype.kind == "f" else a.dtype)
        return get, nc.close

    def read_data_from_nc(self, time_stamp):
        """cra5_api.py:195-226: (268, 721, 1440) float32, pressure vars x levels then singles,
        tp scaled by 1000."""
        one_step = []
        pressure_file = f'{self.local_root}/ERA5/{time_stamp[:4]}/{time_stamp}_pressure.nc'
        single_file = f'{self.local_root}/ERA5/{time_stamp[:4]}/{time_stamp}_single.nc'
        pget, pclose = self._open_nc(pressure_file)
        sget, sclose = self._open_nc(single_file)
        try:
            pha = [float(v) for v in pget('level')]
            level_mapping = [pha.index(v) for v in self.pressure_level if v in pha]
            for vname in self.vnames['pressure']:
                D = pget(vname)
                for level in level_mapping:
                    one_step.append(D[0][level][None])
            for vname in self.vnames['single']:
                D = sget(vname)
                if vname == 'tp':
                    D = D * 1000
                one_step.append(D)
        finally:
            pclose()
            sclose()
        return np.concatenate(one_step, 0).astype(np.float32, copy=False)

    INGEST = ("host", "packed", "auto")

    def _ingest_arg(self, ingest):
        if ingest not in self.INGEST:
            raise ValueError(f"ingest must be one of {self.INGEST}, got {ingest!r}")
        return ingest

    def _ingest(self, time_stamp, ingest="host"):
        """data=None of the encode entry points -> the frame of the time stamp's NetCDF files.  "host": the float32 array of
        read_data_from_nc; "packed": the files' own int16 codes as a pack.PackedFrame over their mappings, marked
        `transient` (_stage_packed / _frame close it once its codes have left the mappings), ValueError naming the file
        and the reason when they do not hold plain packed int16; "auto": packed where possible, else the host route."""
        if ingest == "host":
            return self.read_data_from_nc(time_stamp)
        reason = []
        frame = _pk.read_era5_nc_packed(self.local_root, time_stamp, self.vnames, self.pressure_level, reason=reason)
        if frame is not None:
            frame.transient = True
            return frame
        if ingest == "packed":
            raise ValueError(f"ingest='packed': {reason[0] if reason else time_stamp}")
        return self.read_data_from_nc(time_stamp)

    def _stage_packed(self, frame, threads=None):
        """pack.PackedFrame -> the fp32 frame in this thread's device frame buffer (api_x_dev), on the current stream: every
        block of codes goes from where it lies (a file mapping) into this thread's pinned int16 buffer and on into this
        thread's int16 device buffer - bytes, half those of the fp32 frame, in ONE turn on the link -, the [C, 4] table
        follows, and csrc/pack.hip's unpack kernel writes the frame.  As _stage_in copies a float32 frame: with a team
        (threads > 1) ops.copy_h2d_staged overlaps the host memcpy with the DMA inside the turn; with one thread the memcpy
        runs on this thread BEFORE its turn (the frame threads copy side by side) and the turn is the DMA alone.
        A `transient` frame (_ingest) is closed once its codes have left the mappings."""
        net = self.net
        threads = threads or self.runtime.copy_threads
        t0 = time.perf_counter()
        try:
            shape = tuple(frame.shape)
            pin = net._pinned("api_q_in", shape, torch.int16)
            qdev = net._buf("api_q_in_dev", shape, torch.int16)
            tpin = net._pinned("api_unpack_table_in", (shape[0], len(ops.UNPACK_FIELDS)), torch.float64)
            table = net._buf("api_unpack_table", (shape[0], len(ops.UNPACK_FIELDS)), torch.float64)
            np.copyto(tpin.numpy(), frame.table())
            swapped = frame.swapped
            if threads > 1:
                with self._link("h2d"):
                    c = 0
                    for blk in frame.blocks:
                        ops.copy_h2d_staged(qdev[c:c + blk.shape[0]], blk, pin, threads=threads)
                        c += blk.shape[0]
                    table.copy_(tpin, non_blocking=True)
            else:
                host = pin.numpy().view(frame.blocks[0].dtype)      # (the blocks' byte order: a plain memcpy)
                c = 0
                for blk in frame.blocks:
                    np.copyto(host[c:c + blk.shape[0]], blk)
                    c += blk.shape[0]
                self._log("stage_in_memcpy", t0)
                with self._link("h2d"):
                    qdev.copy_(pin, non_blocking=True)              # async H2D on this frame's stream
                    table.copy_(tpin, non_blocking=True)
                    if self.link_serial:
                        torch.cuda.current_stream().synchronize()   # the gate is held until the codes have landed
            blk = None      # (no view of a mapping outlives close())
        finally:
            if frame.transient:
                frame.close()
        return ops.unpack_i16(qdev, table, swapped=swapped, out=net._buf("api_x_dev", shape))

    def _frame(self, time_stamp, data):
        """-> the frame as a float32 device tensor.  Host arrays go through this thread's pinned staging buffer
        into this thread's persistent device frame buffer (chunked, host memcpy overlapped with the DMA): the
        returned tensor is that buffer, valid until this thread's next call.  A pack.PackedFrame crosses as int16 codes
        and is unpacked on the device (_stage_packed)."""
        if data is None:
            data = self.read_data_from_nc(time_stamp)
        if isinstance(data, _pk.PackedFrame):
            if self.net.device.type != "cuda":
                try:
                    return torch.from_numpy(_pk.unpack_f32(data)).to(self.device)
                finally:
                    if data.transient:
                        data.close()
            return self._stage_packed(data)
        if isinstance(data, torch.Tensor):
            if data.is_cuda or not self.net.device.type == "cuda":
                return data.to(self.device, dtype=torch.float32)
            data = data.detach().numpy()
        if self.net.device.type != "cuda":
            return torch.from_numpy(np.ascontiguousarray(data, dtype=np.float32)).to(self.device)
        arr = np.ascontiguousarray(data, dtype=np.float32)
        pin = self.net._pinned("api_x_in", tuple(arr.shape), torch.float32)
        xdev = self.net._buf("api_x_dev", tuple(arr.shape))
        return ops.copy_h2d_staged(xdev, arr, pin, threads=self.runtime.copy_threads)

    def _finite_probe(self, frame):
        """One reduction pass over the frame (ops.probe_sums), asynchronous: NaN / inf anywhere make a partial sum
        non-finite."""
        self.net._require_gpu()      # (no CPU fallback: the same error every compute entry point raises)
        return self.net._probe(frame, name="api_in")

    @staticmethod
    def _require_finite(probe):
        if not bool(torch.isfinite(probe).all()):
            raise ValueError("the input frame holds NaN / inf values (masked NetCDF values are read as NaN): fill them "
                             "before encoding - the codec would turn them into arbitrary symbols")

    def _checked(self, frame, run):
        """-> run(), the encode of `frame`, between the launch of the frame's finiteness probe and its verdict."""
        probe = self._finite_probe(frame)
        try:
            res = run()
        except FloatingPointError:
            self._require_finite(probe)     # a non-finite INPUT is the caller's ValueError
            raise
        self._require_finite(probe)
        return res

    def channel_vname_mapping(self):
        """cra5_api.py:228-241."""
        return _channel_mapping(self.vnames, self.pressure_level)

    # ------------------------------------------------------------------ subsets (decode_from_bin / decode_batch)
    # variables=[names] and / or region=(lat_min, lat_max, lon_min, lon_max) in degrees: the decode returns those channels
    # (in the order given) over that box - the same values as the slice of a full decode, bit for bit - and only the
    # subset is written on the GPU, crosses the host link and lands in host memory ("Subset decode").
    # stride=s or (s_lat, s_lon): of that box (default: the globe) only the rows r with r % s_lat == 0 and the columns c
    # with c % s_lon == 0, r / c counted on the GLOBAL grid - stride=6 is the 121 x 240 grid at 1.5 deg, poles included.
    # No interpolation, no averaging: with `full` the full decode of the same file under the same settings,
    # x_hat == full[channels][:, kept_rows][:, :, kept_cols] as bit patterns.  None / 1 / (1, 1): no thinning.
    # coarsen=k or (k_lat, k_lon) (not together with a stride): at the very points stride=k keeps, the AREA-WEIGHTED MEAN
    # of the full decode over the coarse cell round each point - first-order conservative remapping, computed on the GPU
    # in fixed float64 arithmetic ("Coarsening"; (721 - 1) % k_lat == 0 and 1440 % k_lon == 0):
    # coarsen=6 is the conservative 1.5 deg field, 1 / 36 of the bytes.  The dict also carries coarsen, lat_bnds, lon_bnds.
    # regrid=Grid(...) (cra5_amd.regrid; on its own - the target grid is the region and the resolution): the full decode on
    # any rectilinear lat/lon grid, bilinear or first-order conservative, computed on the GPU in fixed float64 arithmetic
    # from the source box the target needs ("Regridding"); only the target grid crosses the host
    # link.  The dict also carries regrid (the method), lat_bnds, lon_bnds.
    grid_box = staticmethod(subset.grid_box)
    resolve_variables = staticmethod(subset.resolve_variables)

    def _names(self, chans=None):
        """The names of the channels `chans`, in that order; None: of every channel of the model."""
        return [self.channels_to_vname.get(c, str(c)) for c in (chans if chans is not None else range(self.net.cfg['out_chans']))]

    def _select(self, variables=None, region=None, stride=None, coarsen=None, regrid=None, points=None):
        """The arguments of the decode methods -> their Selection; without any of them the whole grid's.  regrid (a
        regrid.Grid or its plan): the frame on that target grid - not together with region / stride / coarsen, the
        target grid is the region and the resolution.  points (a points.Points, a [P, 2] array of (lat, lon) or its
        plan): the frame at those positions, [C', P] - with variables only."""
        H, W = self.net.cfg['img_size']
        step, k = subset._stride_or_coarsen(stride, coarsen, H, W)
        whole = variables is None and region is None and step is None and k is None and regrid is None and points is None
        chans = subset.resolve_variables(variables, self.vname_to_channels)
        if points is not None:
            for name, v in (("region", region), ("stride", step), ("coarsen", k), ("regrid", regrid)):
                if v is not None:
                    raise ValueError(f"points and {name}: pass one of the two - a point list names its own positions")
            names = self._names(chans)
            channels = self.net._selection_args(chans)[0]
            plan = self.net._points_arg(points)
            return Selection(channels, None, None, None, names, plan["lat"], plan["lon"], None, None,
                             (len(names), plan["P"]), False, None, plan)
        if regrid is not None:
            for name, v in (("region", region), ("stride", step), ("coarsen", k)):
                if v is not None:
                    raise ValueError(f"regrid and {name} {v!r}: pass one of the two - the target grid is the region and "
                                     f"the resolution")
            names = self._names(chans)
            channels, _, _, _, plan = self.net._selection_args(chans, None, None, None, regrid)
            return Selection(channels, None, None, None, names, plan["lat"], plan["lon"], plan["lat_bnds"], plan["lon_bnds"],
                             (len(names), plan["Ho"], plan["Wo"]), False, plan)
        g = subset.grid_box(region if region is not None else (-90.0, 90.0, 0.0, 360.0), H, W, stride=step, coarsen=k)
        names = self._names(chans)
        channels, box, step, k, _ = self.net._selection_args(chans, g["box"] if region is not None else None, step, k)
        return Selection(channels, box, step, k, names, g["lat"], g["lon"], g.get("lat_bnds"), g.get("lon_bnds"),
                         (len(names), len(g["lat"]), len(g["lon"])), whole)

    def get_mean_std(self):
        """cra5_api.py:243-261."""
        mean_list, std_list = [], []
        for v in self.vnames['pressure']:
            mean_list += [self._stats['mean'][v][i] for i in self.level_mapping]
            std_list += [self._stats['std'][v][i] for i in self.level_mapping]
        for v in self.vnames['single']:
            mean_list.append(self._stats['mean'][v])
            std_list.append(self._stats['std'][v])
        return np.array(mean_list, dtype=np.float32), np.array(std_list, dtype=np.float32)

    def normalization(self, data):
        """cra5_api.py:264-266 (stand-alone form; the hot path fuses it into the patch gather)."""
        return (data - self.mean) / self.std

    def de_normalization(self, data):
        """cra5_api.py:268-271: in place, like the reference."""
        data *= self.std
        data += self.mean
        return data

    # ------------------------------------------------------------------ encode
    def _encode_y(self, frame):
        """normalise + g_a + quant_conv for one physical-units frame (fused normalisation)."""
        with torch.no_grad():
            self.net._require_gpu()
            return self.net._encode_y_guarded(frame, mean=self._mean_flat, std=self._std_flat)

    def _compress_output(self, frame):
        """One physical-units device frame -> the `output` dict of the encode methods: its two strings and z_shape."""
        y_str, z_str = self.net._compress_frame(x=frame, mean=self._mean_flat, std=self._std_flat)
        return {"strings": [[y_str], [z_str]], "z_shape": torch.Size([self.net.Hz, self.net.Wz])}

    @staticmethod
    def _write_bin(save_root, ts, output, write=True):
        """-> {save_root}/{yyyy}/{ts}.bin, the path of the frame's archive file; written unless write is False."""
        path = f'{save_root}/{ts.split("-")[0]}/{ts}.bin'
        if write:
            os.makedirs(os.path.dirname(path), exist_ok=True)
            with Path(path).open("wb") as f:
                binfmt.write_bin(f, output["strings"], output["z_shape"])
        return path

    def encode_to_latent(self, time_stamp=None, save_root=None, latent_type='float', data=None, ingest="host"):
        """cra5_api.py:53-71.  data: a host array / tensor or a pack.PackedFrame; ingest (with data=None): how the NetCDF
        files are read - "host" | "packed" | "auto" (encode_era5_as_bin)."""
        if data is None and self._ingest_arg(ingest) != "host":
            data = self._ingest(time_stamp, ingest)
        frame = self._frame(time_stamp, data)
        with torch.no_grad():
            y = self._checked(frame, lambda: self._encode_y(frame))
            if latent_type == 'float':
                return y.unsqueeze(0)
            if latent_type == 'quantized':
                s = self.net._latent_side_guarded(y)
                return s["y_hat"].reshape(y.shape).unsqueeze(0)

    def latent_to_bin(self, y, save_root=None):
        """cra5_api.py:73-79."""
        with torch.no_grad():
            return self.net.compress_from_latent(y)

    def encode_era5_as_bin(self, time_stamp, save_root=None, return_format='bin', data=None, max_error=None,
                           max_fraction=0.25, ingest="host"):
        """cra5_api.py:81-125.  data: a float32 host array / tensor in physical units, or a pack.PackedFrame - int16 codes
        with their scale_factor / add_offset / fill code: the codes cross the host link, half the bytes, and are unpacked
        on the GPU to the very bits the host unpacking gives ("Packed int16 input"), so the .bin is
        byte-identical; a fill code is a NaN and raises the non-finite-input ValueError.  ingest (with data=None): "host"
        (default) - read_data_from_nc unpacks the NetCDF files on the host; "packed" - the files' int16 codes are staged
        straight from their mappings (pack.read_era5_nc_packed), ValueError naming the file and the reason when they are
        not plain packed int16 NetCDF-3; "auto" - packed where possible, else the host route.
        max_error (a positive number: that bound in normalised units on every channel | a dict
        {variable: bound in physical units}; residual.resolve_tolerance): the frame's own decode is corrected against the
        staged truth on the GPU and the corrections are written beside the unchanged .bin as {save_root}/{yyyy}/{ts}.res -
        decode with residual=True and every point of the corrected channels is within its bound (DESIGN.md section 4,
        "Residual layer").  The dict gains residual = dict(path, bytes, records, escapes, per_channel, tol); more
        corrections than max_fraction of the corrected channels' points raise ResidualBudgetError, no .res is written."""
        save_root = save_root or self.local_root
        tol = self._residual_tol(max_error)
        if return_format in ('latent', 'quantized'):
            if tol is not None:
                raise ValueError(f"encode_era5_as_bin: max_error writes a sidecar beside the .bin; return_format="
                                 f"{return_format!r} writes none")
            return self.encode_to_latent(time_stamp, latent_type='float' if return_format == 'latent' else 'quantized',
                                         data=data, ingest=ingest)
        st1 = time.time()
        if data is None and self._ingest_arg(ingest) != "host":
            data = self._ingest(time_stamp, ingest)
        frame = self._frame(time_stamp, data)
        st2 = time.time()
        with torch.no_grad():
            # g_a and the latent side as ONE GPU phase (what the batch path runs: the same kernels on the same
            # values, the same bytes - no stream sync and host round trip between the two halves)
            output = self._checked(frame, lambda: self._compress_output(frame))
            side = None
            if tol is not None:
                side = self._residual_encode(time_stamp, frame, output, tol, max_fraction)
        st3 = time.time()
        file_url = self._write_bin(save_root, time_stamp, output)
        res = dict(output=output, save_path=file_url)
        if side is not None:
            res["residual"] = self._residual_write(side, file_url)
        st4 = time.time()
        res.update(reading_time=st2 - st1, encoding_time=st3 - st2, saving_time=st4 - st3)
        return res

    # ------------------------------------------------------------------ visualisation (cra5_api.py:273-341)
    @staticmethod
    def _plt():
        import matplotlib
        matplotlib.use("Agg", force=False)
        import matplotlib.pyplot as plt
        return plt

    @staticmethod
    def _host(a):
        return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)

    def show_image(self, reconstruct_data, time_stamp, show_variables=('z_500', 'q_500', 'u_500', 'v_500', 't_500', 'w_500'),
                   save_images=True, save_path=None, data=None):
        """Original / reconstruction / |difference| panels per variable (cra5_api.py:273-315).  `data`: the
        original frame when the NetCDF files are not on disk.  Returns the figure path."""
        plt = self._plt()
        original = self._host(data) if data is not None else self.read_data_from_nc(time_stamp)
        rec = self._host(reconstruct_data)
        rec = rec.reshape(rec.shape[-3:])
        rows = [(original[self.vname_to_channels[v]], rec[self.vname_to_channels[v]]) for v in show_variables]
        fig, axs = plt.subplots(len(rows), 3, figsize=(20, 3 * len(rows)), squeeze=False)
        for i, (ori, new) in enumerate(rows):
            for j, (img, title) in enumerate(((ori, "Original"), (new, "Reconstructed"), (np.abs(ori - new), "Difference"))):
                im = axs[i, j].imshow(img, cmap='jet')
                axs[i, j].set_title(f'{show_variables[i]}_{title}')
                fig.colorbar(im, ax=axs[i, j])
        plt.tight_layout()
        fig_path = (f'{save_path}/{time_stamp}_rconstruction.png' if save_path is not None else
                    f'{self.local_root}/CRA5_vis/{time_stamp[:4]}/{time_stamp}_reconstruction.png')
        os.makedirs(os.path.dirname(fig_path), exist_ok=True)
        if save_images:
            fig.savefig(fig_path)
        plt.close(fig)
        return fig_path

    def show_latent(self, latent, time_stamp, show_channels=(0, 10, 20, 30, 40, 50, 60, 70, 80), save_images=True,
                    save_path=None):
        """One panel per latent channel (cra5_api.py:317-341; the reference's len//4-row grid drops the 9th
        default channel and indexes past its axes - the grid here has enough rows).  Returns the figure path."""
        plt = self._plt()
        lat = self._host(latent)
        lat = lat.reshape(lat.shape[-3:])
        n = len(show_channels)
        fig, axs = plt.subplots((n + 3) // 4, 4, figsize=(24, 3 * ((n + 3) // 4)), squeeze=False)
        axs = axs.flatten()
        for i, ch in enumerate(show_channels):
            im = axs[i].imshow(lat[ch], cmap='jet')
            axs[i].set_title(f'Channel_{ch}')
            fig.colorbar(im, ax=axs[i])
        for ax in axs[n:]:
            ax.axis('off')
        plt.tight_layout()
        fig_path = (f'{save_path}/{time_stamp}_latent.png' if save_path is not None else
                    f'{self.local_root}/CRA5_vis/{time_stamp[:4]}/{time_stamp}_latent.png')
        os.makedirs(os.path.dirname(fig_path), exist_ok=True)
        if save_images:
            fig.savefig(fig_path)
        plt.close(fig)
        return fig_path

    # ------------------------------------------------------------------ many frames at a time
    # The single-frame methods above hand a pageable host array to the device synchronously (one 1.11 GB
    # H2D per frame, 18-80 ms, nothing else running meanwhile) and return x_hat on the device.  A
    # production encode / decode loop streams hourly frames: the batch methods below run them through
    # the frame pipeline (cra5_amd/pipeline.py) with, per in-flight frame, a PINNED host staging buffer
    # and a persistent device frame buffer - the host memcpy into pinned memory and the async H2D / D2H
    # of one frame overlap the GPU and rANS phases of the others (cra5_api.py:81-125,153-192).
    def _pipeline(self, workers):
        from .pipeline import FramePipeline
        p = getattr(self, "_pipe", None)
        if p is None or p.workers != workers:
            if p is not None:
                p.close()
            p = self._pipe = FramePipeline(self.net, workers=workers, device=self.net.device)
        return p

    def _stage_in(self, arr):
        """host array (numpy / CPU tensor, physical units) -> this thread's device frame buffer, through
        this thread's pinned staging buffer, on the current stream.  A pack.PackedFrame: _stage_packed."""
        net = self.net
        if isinstance(arr, _pk.PackedFrame):
            return self._stage_packed(arr, threads=max(1, self.batch_copy_threads))
        if isinstance(arr, torch.Tensor):
            if arr.is_cuda:
                return arr.to(torch.float32)
            arr = arr.numpy()
        pin = net._pinned("api_x_in", tuple(arr.shape), torch.float32)
        if self.batch_copy_threads > 1 and arr.dtype == np.float32 and arr.flags["C_CONTIGUOUS"]:
            # a small team per frame (csrc/runtime.hip): chunk c + 1 is memcpy'd while the DMA engine moves chunk c - the
            # frame is on the device after max(memcpy / team, PCIe) instead of memcpy + PCIe
            with self._link("h2d"):
                return ops.copy_h2d_staged(net._buf("api_x_dev", tuple(arr.shape)), arr, pin, threads=self.batch_copy_threads)
        # host memcpy (+ dtype conversion) by numpy on THIS thread, GIL released: torch's copy_ fans one 1.11 GB copy out
        # over every core of the box (128 threads: 11 GB/s, one thread: 24 GB/s - tools/api_host_probe.sh) and the
        # twelve frame threads then fight over them; twelve single-threaded copies run side by side
        t0 = time.perf_counter()
        np.copyto(pin.numpy(), arr, casting="same_kind")
        self._log("stage_in_memcpy", t0)
        src = pin
        xdev = net._buf("api_x_dev", tuple(src.shape))
        with self._link("h2d"):
            xdev.copy_(pin, non_blocking=True)              # async H2D on this frame's stream
            if self.link_serial:
                torch.cuda.current_stream().synchronize()   # the gate is held until the frame has landed
        return xdev

    def _log(self, phase, t0):
        if self.phase_log is not None:
            self.phase_log.append((threading.get_ident(), phase, t0, time.perf_counter()))

    @contextlib.contextmanager
    def _link(self, direction):
        """Context manager: this thread's turn on the host link in `direction` ("h2d" / "d2h"); logs wait + transfer."""
        t0 = time.perf_counter()
        if self.link_serial:
            self._link_gate[direction].acquire()
        t1 = time.perf_counter()
        try:
            yield
        finally:
            if self.link_serial:
                self._link_gate[direction].release()
            if self.phase_log is not None:
                self.phase_log.append((threading.get_ident(), direction + "_wait", t0, t1))
                self.phase_log.append((threading.get_ident(), direction, t1, time.perf_counter()))

    def _encode_one(self, ts, arr, save_root, write=True, tol=None, max_fraction=None, ingest="host"):
        """One frame of the batch encode on the calling frame thread (its stream, its pinned / device buffers).  tol
        (float32 [C], _residual_tol): the thread then decodes its own strings and writes the residual sidecar."""
        enc, x = self._encode_staged(ts, arr, save_root, write, ingest)
        if tol is not None:
            t0 = time.time()
            with torch.no_grad():
                side = self._residual_encode(ts, x, enc["output"], tol, max_fraction)
            enc["residual"] = self._residual_write(side, enc["save_path"], write)
            enc["encoding_time"] += time.time() - t0
        return enc

    def _encode_staged(self, ts, arr, save_root, write=True, ingest="host"):
        """_encode_one -> (its dict, the frame on the device: this thread's staged copy, which the compress path only
        reads)."""
        t0 = time.time()
        if arr is None:
            arr = self._ingest(ts, ingest)
        t1 = time.time()
        with torch.no_grad():
            x = self._stage_in(arr)

            def run():
                # the frame has landed BEFORE this thread queues for a GPU-phase slot: a slot held while its stream waits
                # 20 ms for the PCIe transfer is a third of the chip's concurrency gone (encode_era5_batch: 38 -> frames/s)
                torch.cuda.current_stream().synchronize()
                return time.perf_counter(), self._compress_output(x)
            t_c, output = self._checked(x, run)
            self._log("compress", t_c)
        t2 = time.time()
        file_url = self._write_bin(save_root, ts, output, write)
        return dict(output=output, reading_time=t1 - t0, encoding_time=t2 - t1, saving_time=time.time() - t2,
                    save_path=file_url), x

    def encode_era5_batch(self, time_stamps, data=None, save_root=None, workers=12, write=True, max_error=None,
                          max_fraction=0.25, ingest="host"):
        """encode_era5_as_bin for many time stamps (`data`: matching list of host arrays or pack.PackedFrame, or None to
        read the NetCDF files - ingest "host" | "packed" | "auto" as in encode_era5_as_bin: with "packed" every frame
        thread stages its files' int16 codes straight from their mappings).  Returns the list of per-frame dicts (same
        keys as encode_era5_as_bin).
        max_error / max_fraction (encode_era5_as_bin): after the compress phase every frame thread decodes its own
        strings, quantises the residual against the staged truth on the GPU and writes {ts}.res beside the (byte-identical)
        {ts}.bin; a frame over the budget ends the call with ResidualBudgetError."""
        save_root = save_root or self.local_root
        self.net._require_gpu()
        tol = self._residual_tol(max_error)
        self._ingest_arg(ingest)
        frames = list(data) if data is not None else [None] * len(time_stamps)
        return self._pipeline(workers).map(lambda it: self._encode_one(it[0], it[1], save_root, write, tol, max_fraction,
                                                                       ingest),
                                           list(zip(time_stamps, frames)))

    def _read_frame(self, path, res_path=None):
        """-> (strings, z shape) of the .bin at `path` and the sidecar of `res_path` on the device (None without one)."""
        strings, shape = self._read_bin(path)
        return strings, shape, self._residual_load(res_path) if res_path is not None else None

    def _decode_device(self, strings, shape, denorm, sel, side=None, what=None, phase="decompress"):
        """One frame's strings -> the selection `sel` of its reconstruction on the device, contiguous [C', Hb, Wb], de-
        normalised in the overlap-add store with `denorm`; logged as `phase` (None: the caller's own phase covers it).
        side (_residual_load): the sidecar's corrections are then added in place (_residual_correct; `what` names the
        frame in its errors), logged as "residual"."""
        t_d = time.perf_counter()
        x_hat = self.net._decompress_frame(strings[0][0], strings[1][0], shape, True,
                                           mean=self._mean_flat if denorm else None,
                                           std=self._std_flat if denorm else None, **sel.model)
        if phase is not None:
            self._log(phase, t_d)
        if side is not None:
            self._residual_correct(x_hat, side, sel, what)
        return x_hat.reshape(x_hat.shape[-len(sel.shape):])

    def _decode_one(self, i, path, denorm, sel, out=None, sink=None, res_path=None, pack=None):
        """One frame of the batch decode on the calling frame thread: .bin -> the Selection `sel` of x_hat -> this thread's
        pinned buffer -> `sink` / `out[i]` / a fresh array.  pack (_pack_arg): the frame is packed to int16 on this
        thread's stream first and the codes cross instead."""
        strings, shape, side = self._read_frame(path, res_path)
        with torch.no_grad():
            return self._frame_out(i, self._decode_device(strings, shape, denorm, sel, side, res_path), pack, out, sink)

    def _frame_out(self, i, x, pk, out, sink):
        """_decode_one's way out: x [C', H, W] on the device -> this thread's pinned buffer in ONE turn on the link ->
        `sink(i, .)` / `out[i]` / a fresh copy.  With pk (pack=) the codes and the table cross instead (half the bytes of
        the fp32 frame) and the item is the dict of pack.pack_frame, q the host array."""
        shape = tuple(x.shape)
        if pk is None:
            pin = self.net._pinned("api_x_out", shape, torch.float32)
            if sink is None and out is not None and self.batch_copy_threads > 1:
                with self._link("d2h"):
                    ops.copy_d2h_staged(out[i], x, pin, threads=self.batch_copy_threads)
                return out[i]
            crossing = [(pin, x)]
        else:
            q, table, fixed = self._pack_device(x, pk, q_out=self.net._buf("api_q_dev", shape, torch.int16),
                                                table_out=self.net._buf("api_pack_table", (shape[0], len(ops.PACK_FIELDS)),
                                                                        torch.float64))
            pin = self.net._pinned("api_q_out", shape, torch.int16)
            tpin = self.net._pinned("api_pack_table_out", tuple(table.shape), torch.float64)
            crossing = [(pin, q), (tpin, table)]
        with self._link("d2h"):
            for host, dev in crossing:
                host.copy_(dev, non_blocking=True)
            torch.cuda.current_stream().synchronize()
        t_s = time.perf_counter()
        try:
            def item(frame):
                return frame if pk is None else dict(_pk.frame_stats(tpin.numpy(), fixed), q=frame)
            if sink is not None:
                return sink(i, item(pin.numpy()))
            if out is not None:
                np.copyto(out[i], pin.numpy())
                return item(out[i])
            return item(pin.numpy().copy())
        finally:
            self._log("consume", t_s)

    def _pack_arg(self, what, pack, return_format, sel, per_variable=False):
        """pack= of the decode methods -> None, or dict(fixed: float64 numpy [C', 2] (pack.resolve_ranges over the decoded
        channels' names), fixed_dev: the same on the device | None when no range is fixed, groups: None - or, with
        per_variable, the channel rows of every pressure variable with more than one decoded level: they share one range)."""
        if pack is None or pack is False:
            return None
        if return_format not in ('de_normalized', 'de_normlized'):
            raise ValueError(f"{what}: pack= packs the de-normalised reconstruction (the ranges are in physical units); "
                             f"return_format={return_format!r} is not supported with it")
        names = sel.names
        fixed = _pk.resolve_ranges(pack, names)
        groups = None
        if per_variable:
            groups = [rows for _, _, rows in _pk.split_variables(names, self.vnames)[0]]
            for rows in groups:
                if not np.array_equal(fixed[rows], np.tile(fixed[rows[0]], (len(rows), 1)), equal_nan=True):
                    raise ValueError(f"{what}: the levels of {names[rows[0]].rsplit('_', 1)[0]!r} go into one NetCDF variable "
                                     "with one packing - key its range by the variable name, not by a level")
            groups = [rows for rows in groups if len(rows) > 1 and np.isnan(fixed[rows[0], 0])]
        dev = None
        if not np.isnan(fixed[:, 0]).all():
            dev = torch.from_numpy(fixed).to(self.net.device)
            torch.cuda.current_stream().synchronize()       # read by every frame thread's stream
        return dict(fixed=fixed, fixed_dev=dev, groups=groups or None)

    def _pack_device(self, x, pk, q_out=None, table_out=None):
        """Pack the device frame x [C', H, W] on the current stream -> (q int16 device, table fp64 device [C', 5], the
        fixed ranges used: float64 numpy [C', 2]).  With pk["groups"] the rows of a group get the group's own (min of
        vmin, max of vmax) as their fixed range: a first range pass, C' x 2 doubles to the host and back, a second one."""
        table = ops.pack_range(x, pk["fixed_dev"], out=table_out)
        fixed = pk["fixed"]
        if pk["groups"]:
            mm = table[:, :2].cpu().numpy()
            fixed = fixed.copy()
            for rows in pk["groups"]:
                fixed[rows] = (np.fmin.reduce(mm[rows, 0]), np.fmax.reduce(mm[rows, 1]))    # (NaN: no finite value at all)
            table = ops.pack_range(x, torch.from_numpy(fixed).to(x.device), out=table)
        return ops.pack_i16(x, table, out=q_out), table, fixed

    @staticmethod
    def _check_out(out, n, frame_shape, dtype=np.float32):
        """`out=` of the batch methods: the C memcpy / DMA behind it writes n x C x H x W values of `dtype` (float32; int16
        with pack=) (`frame_shape` = (C, H, W): the Selection's), so anything else is refused here with a ValueError (not
        an assert that `python -O` drops - ADVICE r5)."""
        if out is None:
            return
        want = (n,) + tuple(frame_shape)          # ([n, C', P] with points=)
        if not isinstance(out, np.ndarray) or out.dtype != dtype or tuple(out.shape) != want \
                or not out.flags["C_CONTIGUOUS"] or not out.flags["WRITEABLE"]:
            raise ValueError(f"`out` must be a writeable C-contiguous {np.dtype(dtype).name} numpy array of shape {list(want)}"
                             f" (got {type(out).__name__} {getattr(out, 'dtype', None)} {getattr(out, 'shape', None)})")

    def roundtrip_batch(self, time_stamps, data=None, save_root=None, workers=12, sink=None, out=None,
                        return_format='de_normalized', ingest="host"):
        """The reference's test.py loop (test.py:14-59: encode_era5_as_bin then decode_from_bin per time stamp) as a
        STREAM: every frame goes host array -> H2D -> g_a -> rANS -> .bin on disk -> .bin read -> rANS -> g_s -> D2H ->
        `sink(i, frame)` / `out[i]`, `workers` frames in flight - the H2D of one frame, the D2H of another and the GPU /
        rANS phases of the rest overlap.  Returns [(encode dict, sink's value | host array), ...].  data items may be
        pack.PackedFrame; ingest (with data=None): as in encode_era5_as_bin."""
        save_root = save_root or self.local_root
        denorm = self._denorm_arg(return_format)
        self._ingest_arg(ingest)
        self.net._require_gpu()
        sel = self._select()
        self._check_out(out, len(time_stamps), sel.shape)
        frames = list(data) if data is not None else [None] * len(time_stamps)

        def one(item):
            i, ts, arr = item
            enc = self._encode_one(ts, arr, save_root, True, ingest=ingest)
            return enc, self._decode_one(i, enc["save_path"], denorm, sel, out, sink)
        return self._pipeline(workers).map(one, [(i, ts, a) for i, (ts, a) in enumerate(zip(time_stamps, frames))])

    def decode_batch(self, time_stamps=None, paths=None, return_format='de_normalized', out=None, workers=12, sink=None,
                     variables=None, region=None, stride=None, coarsen=None, residual=None, pack=None, regrid=None,
                     points=None):
        """decode_from_bin for many frames.  Returns a list of HOST float32 arrays [C, H, W] (views of `out`
        [n, C, H, W] when given, fresh arrays otherwise); the D2H of each reconstruction goes through the
        decoding thread's pinned buffer and overlaps the other frames' work.  `sink(i, frame)`: called on the decoding
        thread with frame i as a [C, H, W] float32 view of that thread's PINNED buffer (valid until the call returns:
        write it to disk, reduce it, copy it) instead of copying it out; the list then holds the sink's return values -
        a long decode loop needs no [n, C, H, W] host array.
        variables / region / stride (decode_from_bin): every frame is the subset [C', Hb, Wb] - `out` must then be
        [n, C', Hb, Wb], `sink` gets [C', Hb, Wb] views; grid_box(region, stride=stride) gives its lat / lon (with a
        stride Hb / Wb count the kept rows / columns: stride=6 over the globe is [C', 121, 240]).
        coarsen (decode_from_bin): the same shapes as stride=coarsen, every point the area-weighted mean of its coarse
        cell - 1 / (k_lat * k_lon) of the bytes cross the host link; grid_box(region, coarsen=coarsen) gives lat / lon
        and the cells' lat_bnds / lon_bnds.
        regrid (decode_from_bin): a regrid.Grid - every frame is [C', Ho, Wo] on that target grid, regridded on the device;
        only the target grid crosses the host link.  `out`, `sink` and `pack` work on the regridded frame.
        points (decode_from_bin): a points.Points or a [P, 2] array of (lat, lon), with variables only - every frame is
        [C', P], the decode at those positions; `out` must be [n, C', P], `sink` gets [C', P] views.  series_batch keeps
        the frames on the device and returns one [T, C', P] array.
        residual (decode_from_bin): True - the .res beside every .bin -, or one sidecar path per frame; every frame is
        corrected on the device before it crosses the host link.
        pack (decode_from_bin; only with return_format 'de_normalized'): "int16" / True / {variable: (lo, hi)} - every frame
        is packed to int16 on its own stream right after decode and residual (cra5_amd.pack, DESIGN.md section 4 "Packed
        int16 output"); the codes and the [C', 5] table cross the link in one turn through an int16 pinned buffer, half the
        bytes of the fp32 copy.  Every list item is then the dict of pack.pack_frame - q (a host int16 array [C', Hb, Wb]),
        scale_factor, add_offset, vmin, vmax, nonfinite, saturated, fill_value; `out` must be a C-contiguous int16 array
        [n, C', Hb, Wb] and q is its view; `sink(i, item)` receives the dict, q a view of the pinned buffer."""
        return self._decode_batch(time_stamps, paths, return_format, out, workers, sink, variables, region, stride, coarsen,
                                  residual, pack, regrid=regrid, points=points)

    @staticmethod
    def _points_alone(what, points, residual=None, pack=None, return_format=None):
        """points= of `what` goes with variables= only: ValueError together with residual, pack or the latent."""
        if points is None:
            return
        for name, v in (("residual", residual), ("pack", pack)):
            if v is not None and v is not False:
                raise ValueError(f"{what}: points= with {name}= is not supported - {name} works on grid frames, a point "
                                 f"list returns [C', P]")
        if return_format == 'latent':
            raise ValueError(f"{what}: return_format='latent' returns the latent; points select positions of the "
                             "reconstruction")

    def _decode_batch(self, time_stamps, paths, return_format, out, workers, sink, variables, region, stride, coarsen,
                      residual, pack, what="decode_batch", per_variable=False, regrid=None, points=None):
        if paths is None:
            paths = [self._bin_path(ts) for ts in time_stamps]
        self._points_alone(what, points, residual, pack, return_format)
        denorm = self._denorm_arg(return_format)
        self.net._require_gpu()
        sel = self._select(variables, region, stride, coarsen, regrid, points)
        sides = self._residual_arg(what, residual, list(paths), return_format, sel.coarsen, sel.regrid)
        pk = self._pack_arg(what, pack, return_format, sel, per_variable)
        self._check_out(out, len(paths), sel.shape, np.int16 if pk is not None else np.float32)

        return self._pipeline(workers).map(lambda it: self._decode_one(it[0], it[1], denorm, sel, out, sink,
                                                                       res_path=sides[it[0]], pack=pk),
                                           list(enumerate(paths)))

    def decode_to_nc(self, time_stamps=None, paths=None, save_root=None, pack="int16", variables=None, region=None,
                     stride=None, coarsen=None, residual=None, workers=12, regrid=None):
        """.bin archives back to the NetCDF files the rest of the tool chain reads: decode_batch(pack=...) with a sink that
        writes every frame, on its decoding thread, as {save_root}/ERA5/{yyyy}/{ts}_pressure.nc / {ts}_single.nc in the
        layout read_data_from_nc reads (pack.write_era5_nc: NetCDF-3 64-bit offset, int16 with scale_factor / add_offset /
        _FillValue per variable, a file without a selected variable is not written).  save_root: default local_root.
        The file names come from time_stamps (needed also with paths=).
        A NetCDF variable has one packing, so the decoded levels of one pressure variable share one range per frame:
        ops.pack_range measures every channel on the device, the variable's (min of vmin, max of vmax) - C' x 2 doubles on
        the host - becomes the fixed range of its levels, and the packing proceeds as for any fixed range.
        pack: "int16" (those per-frame ranges) or {name: (lo, hi)} fixed physical ranges; a name is the NETCDF VARIABLE
        name for a pressure variable ("z": every decoded level of z; a single level such as "z_500" is refused) or the
        channel name of a single-level variable ("t2m"; "tp" in the model's tp x 1000).  The pressure selection must be
        rectangular - every selected pressure variable with the same levels in the same order (ValueError, before any
        decode).  variables / region / stride / coarsen / residual / regrid: as in decode_batch (with regrid= the files'
        latitude / longitude are the target grid's).
        Returns one dict per frame: time_stamp, files (the paths written), bytes (their total size)."""
        if time_stamps is None:
            raise ValueError("decode_to_nc needs time_stamps: they name the NetCDF files")
        time_stamps = list(time_stamps)
        if paths is not None and len(list(paths)) != len(time_stamps):
            raise ValueError("decode_to_nc: time_stamps and paths must have the same length")
        save_root = save_root or self.local_root
        sel = self._select(variables, region, stride, coarsen, regrid)

        def sink(i, item):
            t0 = time.perf_counter()
            files = _pk.write_era5_nc(save_root, time_stamps[i], item, sel.names, sel.lat, sel.lon, self.vnames)
            self._log("write_nc", t0)
            return dict(time_stamp=time_stamps[i], files=files, bytes=sum(os.path.getsize(p) for p in files))
        return self._decode_batch(time_stamps, paths, 'de_normalized', None, workers, sink, variables, region, stride,
                                  coarsen, residual, pack, what="decode_to_nc", per_variable=True, regrid=regrid)

    def _evaluate_one(self, ts, arr, bin_path, save_root, lat_weights, sel, spectrum=False, tol=None, quantiles=None,
                      ingest="host"):
        """One frame of evaluate_batch on the calling frame thread: the truth is staged once into this thread's device
        frame buffer; the reconstruction comes from the in-memory strings (bin_path None) or from `bin_path`, and only
        the per-channel statistics leave the device.  sel.coarsen = (k_lat, k_lon): both frames are coarsened on the device
        by the same kernel (the reconstruction inside its decode, the truth by VAEformer.coarsen_frame) and compared on
        the coarse grid; sel.regrid likewise (VAEformer.regrid_frame), on the target grid.  spectrum: the zonal power
        spectra of the same device pair join the report; quantiles (validated probabilities): its exact quantiles too."""
        from . import metrics
        if bin_path is None:
            enc, x = self._encode_staged(ts, arr, save_root, write=save_root is not None, ingest=ingest)
            strings, shape = enc["output"]["strings"], enc["output"]["z_shape"]
            n_bytes = 12 + sum(4 + len(s[0]) for s in strings)     # the .bin container (binfmt.write_bin)
        else:
            if arr is None:
                arr = self._ingest(ts, ingest)
            with open(bin_path, "rb") as f:
                blob = f.read()
            strings, shape = binfmt.unpack_bin(blob)
            n_bytes = len(blob)
            with torch.no_grad():
                x = self._stage_in(arr)      # (a truth with masked / non-finite values is reported, not refused)
        with torch.no_grad():
            x_hat = self._decode_device(strings, shape, True, sel)
            side = None
            if tol is not None:
                # the reconstruction a decode with the sidecar would see: quantise against the staged truth, correct in place
                t_r = time.perf_counter()
                side = self._residual_build(ts, x, x_hat, tol, None)
                ops.residual_apply(x_hat, side["records"], side["step"], tuple(x_hat.shape))
                if bin_path is None and save_root is not None:
                    self._residual_write(side, enc["save_path"])
                self._log("residual", t_r)
            t_m = time.perf_counter()
            C, H, W = x.shape[-3:]
            x = x.reshape(C, H, W)
            for arg, frame, buf in ((sel.coarsen, self.net.coarsen_frame, "eval_truth_coarse"),
                                    (sel.regrid, self.net.regrid_frame, "eval_truth_regrid")):
                if arg is None:
                    continue
                if (C, H, W) != (self.net.cfg['out_chans'],) + tuple(self.net.cfg['img_size']):
                    raise ValueError(f"{ts}: the truth frame is {(C, H, W)}, the model's grid "
                                     f"{(self.net.cfg['out_chans'],) + tuple(self.net.cfg['img_size'])}")
                # this thread's persistent workspace, like the decode's own buffers: no allocation per frame
                x = frame(x.contiguous(), arg, out=self.net._buf(buf, sel.shape))
            if x_hat.shape != x.shape:
                raise ValueError(f"{ts}: the reconstruction is {tuple(x_hat.shape)}, the truth frame {tuple(x.shape)}")
            err = metrics.reconstruction_error(x_hat, x, lat_weights=lat_weights)
            self._log("metrics", t_m)
            if spectrum:
                t_s = time.perf_counter()
                spec = metrics.zonal_spectrum(x_hat, x, lat_weights=lat_weights)
                self._log("spectrum", t_s)
            if quantiles is not None:
                t_q = time.perf_counter()
                quant = metrics.frame_quantiles(x_hat, x, quantiles, lat_weights=lat_weights)
                self._log("quantiles", t_q)
        std = self._std_flat.detach().cpu().numpy().astype(np.float64)
        rep = dict(time_stamp=ts, variables=list(sel.names))
        rep.update(err)
        rep["rmse_norm"] = err["rmse"] / std
        if spectrum:
            rep.update({k: spec[k] for k in ("wavenumber", "power_truth", "power_recon", "power_error",
                                             "resolved_wavenumber")})
        if quantiles is not None:
            rep.update({k: quant[k] for k in ("quantile", "quantile_truth", "quantile_recon", "quantile_abs_error",
                                              "quantile_shift")})
        rep["bin_bytes"] = n_bytes
        rep["compression_ratio"] = C * H * W * 4 / n_bytes
        if side is not None:
            rep.update(res_bytes=len(side["blob"]), records=side["records_n"], escapes=side["escapes_n"], tol=side["tol"],
                       compression_ratio_total=C * H * W * 4 / (n_bytes + len(side["blob"])))
        return rep

    def evaluate_batch(self, time_stamps, data=None, bins=None, save_root=None, workers=12, lat_weights="era5",
                       coarsen=None, spectrum=False, max_error=None, regrid=None, quantiles=None, ingest="host"):
        """Per-variable reconstruction error of many frames, through the frame pipeline, without copying any
        reconstruction to the host.  Truth frames: `data` (a matching list of host arrays / tensors, physical units) or
        the NetCDF files of `time_stamps`.
          bins=None: codec error - every frame is compressed and decompressed from the in-memory strings; the .bin is
            written to {save_root}/{yyyy}/{ts}.bin (the bytes encode_era5_as_bin writes) only when save_root is given.
          bins=[paths]: dataset check - the existing .bin files (e.g. downloaded CRA5 files) are decoded and compared with
            the matching truth frames (a truth frame with NaN / inf is reported through `nonfinite`, not refused).
        A truth frame may be a pack.PackedFrame (int16 codes, unpacked on the GPU); ingest (with data=None): "host" |
        "packed" | "auto", as in encode_era5_as_bin.
        Returns one dict per frame: time_stamp, variables (channel names), the statistics of
        metrics.reconstruction_error (float64 [C] arrays in physical units; nonfinite int64 [C]), rmse_norm = rmse / std
        (the codec's per-channel normalisation std), bin_bytes (the container size, header included) and
        compression_ratio = C * H * W * 4 / bin_bytes.
        coarsen=k or (k_lat, k_lon): the error at the coarse resolution (coarsen=6: 1.5 deg) - truth and reconstruction are
        both area-averaged on the device (decode_from_bin's coarsen) and compared on the [C, Ho, Wo] grid, "era5" weights
        being latitude_weights(Ho); the reports also carry coarsen, lat and lon of that grid.  compression_ratio stays
        that of the full frame.
        regrid (a regrid.Grid; not with coarsen=): the error on that target grid - truth and reconstruction are both
        regridded on the device by the same kernel (the truth by VAEformer.regrid_frame) and compared there; "era5" weights
        become the grid's area weights (sin north - sin south of every row's cell, mean 1); the reports also carry regrid
        (the method), lat, lon, lat_bnds and lon_bnds.  spectrum=True then needs a target lon that is uniform and closes the
        circle, and a supported width.  Not with max_error.
        spectrum=True: every report also carries the zonal power spectra of metrics.zonal_spectrum on the same device
        pair (with coarsen=, the coarse pair): wavenumber int64 [K], power_truth / power_recon / power_error float64
        [C, K] and resolved_wavenumber int64 [C]; only the spectra leave the device.  The compared width (W, or the coarse
        Wo) must have no prime factor above 5.
        quantiles=(p, ...): 1 to 16 probabilities in [0, 1] - every report also carries the exact quantiles of
        metrics.frame_quantiles on the same device pair (after the max_error correction; with coarsen= / regrid= the coarse
        or target pair, under the lat_weights resolved there, as integer row weights): quantile float64 [Q], quantile_truth /
        quantile_recon / quantile_abs_error / quantile_shift float64 [C, Q]; only the quantiles leave the device.  A bad
        `quantiles` raises before any frame is touched.
        max_error (encode_era5_as_bin; not with coarsen=): the tuning tool of the residual layer - the reconstruction is
        corrected on the device before the metric and the spectrum, as a decode with the sidecar would see it, and every
        report gains res_bytes (the sidecar's size), records, escapes, tol and compression_ratio_total = C * H * W * 4 /
        (bin_bytes + res_bytes); compression_ratio stays that of the .bin.  No budget applies here.  With save_root (and
        bins=None) the .res is written beside the .bin."""
        self.net._require_gpu()
        self._ingest_arg(ingest)
        sel = self._select(coarsen=coarsen, regrid=regrid)
        k = sel.coarsen
        tol = self._residual_tol(max_error)
        if tol is not None and k is not None:
            raise ValueError("evaluate_batch: max_error with coarsen= is not supported - the correction belongs before the "
                             "averaging, on the full grid; evaluate the two separately")
        if tol is not None and sel.regrid is not None:
            raise ValueError("evaluate_batch: max_error with regrid= is not supported - the correction belongs before the "
                             "regridding, on the full grid; evaluate the two separately")
        extra = dict(coarsen=k, lat=sel.lat, lon=sel.lon) if k is not None else {}
        if sel.regrid is not None:
            extra = {key: v for key, v in sel.meta.items() if key != "variables"}
            if isinstance(lat_weights, str) and lat_weights == "era5":
                lat_weights = sel.regrid["area_weights"]
            if spectrum and not sel.regrid["closes_circle"]:
                raise ValueError("evaluate_batch(spectrum=True) with regrid=: the target longitudes must be uniform and close "
                                 "the circle - a zonal spectrum needs whole latitude circles")
        if spectrum:
            Wc = sel.shape[-1]
            if not ops.spectrum_width_ok(Wc):
                raise ValueError(f"evaluate_batch(spectrum=True): the compared width {Wc} is not supported - the row "
                                 f"transform takes 2 <= W <= {ops.SPECTRUM_MAX_W} with no prime factor above 5")
        if quantiles is not None:
            from . import metrics
            Hc, Wc = sel.shape[-2:]
            # validated, computed and uploaded once, here: the frame threads find weights and targets in metrics' cache
            quantiles = tuple(metrics.quantile_plan(quantiles, lat_weights, Hc, Wc, self.mean.device)[2].tolist())
        n = len(time_stamps)
        frames = list(data) if data is not None else [None] * n
        if len(frames) != n or (bins is not None and len(bins) != n):
            raise ValueError("evaluate_batch: time_stamps, data and bins must have the same length")
        paths = list(bins) if bins is not None else [None] * n
        reps = self._pipeline(workers).map(lambda it: self._evaluate_one(it[0], it[1], it[2], save_root, lat_weights, sel,
                                                                         bool(spectrum), tol, quantiles, ingest),
                                           list(zip(time_stamps, frames, paths)))
        for r in reps:
            r.update(extra)
        return reps

    def _aggregate_one(self, path, denorm, sel, acc, seq, res_path=None):
        """One frame of aggregate_batch on the calling frame thread: .bin -> x_hat (or its subset) -> folded into the
        group's device accumulators as turn `seq`, on this frame's stream.  Nothing crosses to the host."""
        strings, shape, side = self._read_frame(path, res_path)
        with torch.no_grad():
            x_hat = self._decode_device(strings, shape, denorm, sel, side, res_path)
            t_a = time.perf_counter()
            if tuple(x_hat.shape) != sel.shape:
                raise ValueError(f"{path}: the reconstruction is {tuple(x_hat.shape)}, the accumulators {sel.shape}")
            acc.add(x_hat, seq=seq)
            self._log("accumulate", t_a)

    def aggregate_batch(self, time_stamps=None, paths=None, stats=("mean", "std", "min", "max"), groups=None, ddof=0,
                        variables=None, region=None, stride=None, return_format='de_normalized', workers=12, to_host=True,
                        coarsen=None, residual=None, regrid=None):
        """Per-grid-point statistics over time of many decoded frames (a daily or monthly mean, the spread, the extremes),
        reduced on the GPU: every .bin is decoded through the frame pipeline exactly as decode_batch decodes it, and
        instead of crossing the host link the reconstruction is folded into device accumulators (cra5_amd.timestats,
        csrc/timestats.hip) on the frame's own stream, in frame order.  Only the finished statistics come back, once.
          stats: any of "mean", "std", "min", "max" (timestats: float64 sums, mean = f32(s / n), std = f32(sqrt(max(0,
            (q - s * s / n) / (n - ddof)))), min / max propagate NaN).  mean, min and max equal a sequential float64 numpy
            loop over decode_batch's frames bit for bit, std to one fp32 ulp; every result is bit-identical from run to
            run and for every `workers`.
          groups: None, or one hashable label per frame (ts[:10] of hourly files: daily statistics) - one result per
            distinct label, the labels in order of first appearance; within a group the frames apply in index order.
          variables / region / stride / coarsen / return_format ('de_normalized' | 'normalized'): as in decode_batch -
            with coarsen=k the statistics are those of the area-averaged frames, in 1 / (k_lat * k_lon) of the accumulator
            memory and of the final host copy; with regrid= (a regrid.Grid) those of the frames on that target grid.
          residual (decode_from_bin): True or one sidecar path per frame - every frame is corrected on the device before
            it is folded in: the statistics are those of the error-bounded frames.
        Returns a dict: variables, lat, lon (also for the full grid; with coarsen also coarsen, lat_bnds, lon_bnds; with regrid
        also regrid, lat_bnds, lon_bnds), n (int; with groups an int64 [G] array), groups
        (the labels, when given) and per statistic a HOST float32 array [C', Hb, Wb] ([G, C', Hb, Wb] with groups), or
        with to_host=False a device tensor of that shape.  A frame that fails (a missing file, a StreamDesyncError) ends
        the call with that frame's error."""
        from .timestats import TimeStats, check_stats
        if paths is None:
            if time_stamps is None:
                raise ValueError("aggregate_batch needs time_stamps or paths")
            paths = [self._bin_path(ts) for ts in time_stamps]
        paths = list(paths)
        if not paths:
            raise ValueError("aggregate_batch: no frame given")
        stats = check_stats(stats, ddof)
        if return_format == 'latent':
            raise ValueError("aggregate_batch: return_format='latent' is the latent, not a reconstruction to reduce; "
                             "use 'de_normalized' or 'normalized'")
        denorm = self._denorm_arg(return_format)
        if groups is None:
            labels, member = [None], [0] * len(paths)
        else:
            groups = list(groups)
            if len(groups) != len(paths):
                raise ValueError(f"aggregate_batch: groups holds {len(groups)} labels for {len(paths)} frames")
            labels = list(dict.fromkeys(groups))
            index = {lab: g for g, lab in enumerate(labels)}
            member = [index[lab] for lab in groups]
        counts = [member.count(g) for g in range(len(labels))]
        if "std" in stats and min(counts) - ddof < 1:
            g = counts.index(min(counts))
            raise ValueError(f"aggregate_batch: std with ddof = {ddof} needs more than {ddof} frame(s) per group; "
                             + (f"group {labels[g]!r} holds {counts[g]}" if groups is not None else f"{counts[g]} given"))
        sel = self._select(variables, region, stride, coarsen, regrid)
        sides = self._residual_arg("aggregate_batch", residual, paths, return_format, sel.coarsen, sel.regrid)
        self.net._require_gpu()

        # every accumulator before the first decode: running out of device memory shows here
        accs = [TimeStats(sel.shape, stats=stats, device=self.net.device, ddof=ddof) for _ in labels]
        seqs, seen = [], [0] * len(labels)
        for g in member:
            seqs.append(seen[g])
            seen[g] += 1

        def one(i):
            try:
                self._aggregate_one(paths[i], denorm, sel, accs[member[i]], seqs[i], sides[i])
            except BaseException as e:
                for a in accs:       # nobody waits for this frame's turn, and the call ends with this frame's error
                    a.abort(e)
                raise
        self._pipeline(workers).map(one, list(range(len(paths))))

        res = sel.meta
        done = [a.result() for a in accs]
        if groups is not None:
            res["groups"] = labels
            res["n"] = np.array([d["n"] for d in done], dtype=np.int64)
        else:
            res["n"] = int(done[0]["n"])
        if not to_host:
            for s in stats:
                res[s] = torch.stack([d[s] for d in done]) if groups is not None else done[0][s]
            return res
        t0 = time.perf_counter()
        pin = self.net._pinned("api_x_out", sel.shape, torch.float32)
        for s in stats:
            host = np.empty(((len(labels),) if groups is not None else ()) + sel.shape, dtype=np.float32)
            for g, d in enumerate(done):
                ops.copy_d2h_staged(host[g] if groups is not None else host, d[s], pin, threads=self.runtime.copy_threads)
            res[s] = host
        self._log("d2h", t0)
        return res

    def series_batch(self, time_stamps=None, paths=None, points=None, variables=None, return_format='de_normalized',
                     workers=12, to_host=True):
        """Time series at stations or along a track: every .bin is decoded through the frame pipeline exactly as
        decode_batch(points=) decodes it, and frame i's un-embed writes its [C', P] values straight into series[i] on the
        device - nothing crosses the host link per frame.  The finished array comes back once.
          points: a cra5_amd.points.Points or a [P, 2] array of (lat, lon) (decode_from_bin); variables: names, or None
          for every channel; return_format: 'de_normalized' | 'normalized'.
        Returns dict(series: float32 [T, C', P] - a HOST array, or with to_host=False a device tensor -, time_stamps (or
        paths, whichever was given), variables, lat, lon (the points', float64 [P]), points (the method) and, for
        "nearest", node_lat / node_lon).  series[i] is decode_from_bin(..., points=, variables=)'s x_hat of frame i bit
        for bit; every frame owns its slot, so the result does not depend on `workers`.  A frame that fails (a missing
        file, a StreamDesyncError) ends the call with that frame's error."""
        if points is None:
            raise ValueError("series_batch needs points= (a cra5_amd.points.Points or a [P, 2] array of (lat, lon))")
        given = "paths" if paths is not None else "time_stamps"
        if paths is None:
            if time_stamps is None:
                raise ValueError("series_batch needs time_stamps or paths")
            time_stamps = list(time_stamps)
            paths = [self._bin_path(ts) for ts in time_stamps]
        paths = list(paths)
        if not paths:
            raise ValueError("series_batch: no frame given")
        self._points_alone("series_batch", points, return_format=return_format)
        denorm = self._denorm_arg(return_format)
        sel = self._select(variables, points=points)
        self.net._require_gpu()
        T = len(paths)
        series = torch.empty((T,) + sel.shape, device=self.net.device, dtype=torch.float32)
        torch.cuda.current_stream().synchronize()

        def one(i):
            strings, shape, _ = self._read_frame(paths[i])
            with torch.no_grad():
                t_d = time.perf_counter()
                self.net._decompress_frame(strings[0][0], strings[1][0], shape, True,
                                           mean=self._mean_flat if denorm else None,
                                           std=self._std_flat if denorm else None, out=series[i], **sel.model)
                self._log("decompress", t_d)
        self._pipeline(workers).map(one, list(range(T)))

        res = dict(series=series, **{given: paths if given == "paths" else time_stamps}, **sel.meta)
        if not to_host:
            return res
        t0 = time.perf_counter()
        host = np.empty(tuple(series.shape), dtype=np.float32)
        per = max(1, min(T, ops.COPY_CHUNK // max(1, 4 * sel.shape[0] * sel.shape[1])))     # frames per staged copy
        pin = self.net._pinned("api_series_out", (per,) + sel.shape, torch.float32)
        for i in range(0, T, per):
            n = min(per, T - i)
            ops.copy_d2h_staged(host[i:i + n], series[i:i + n], pin, threads=self.runtime.copy_threads)
        self._log("d2h", t0)
        res["series"] = host
        return res

    # ------------------------------------------------------------------ residual layer (cra5_amd/residual.py)
    def _residual_tol(self, max_error):
        """max_error -> the per-channel tolerance, float32 numpy [C] in physical units (residual.resolve_tolerance), or
        None."""
        if max_error is None:
            return None
        return _res.resolve_tolerance(max_error, self.vname_to_channels, self._std_flat.detach().cpu().numpy())

    def _residual_build(self, ts, x, x_hat, tol, max_fraction):
        """Quantise the truth x against the plain de-normalised decode x_hat (both whole frames on the device) -> dict(blob:
        the sidecar's bytes, records: the four device arrays, step: device fp32 [C], records_n, escapes_n, per_channel, tol).
        The witnesses are read from x_hat here, before anything corrects it; the arrays reach the host through this
        thread's pinned buffer.  ResidualBudgetError before anything is copied."""
        C, H, W = (int(v) for v in x_hat.shape[-3:])
        if x.numel() != C * H * W or tuple(x.shape[-3:]) != (C, H, W):
            raise ValueError(f"{ts}: the truth frame is {tuple(x.shape)}, the reconstruction {(C, H, W)}")
        x, x_hat = x.reshape(C, H, W), x_hat.reshape(C, H, W)
        dev = x_hat.device
        widx = _res.witness_indices(C, H, W)
        got = ops.residual_gather(x_hat, torch.from_numpy(widx.view(np.int32)).to(dev), (C, H, W))
        idx, q, eidx, ebits, per = ops.residual_quantize(x, x_hat, tol)
        _res.check_budget(per, tol, H * W, max_fraction, self._names())
        parts, off = [], 0
        for t in (got.reshape(-1), idx, q, eidx, ebits):
            parts.append((off, t))
            off = (off + t.numel() * t.element_size() + 15) // 16 * 16
        cap = 1 << max(16, (off - 1).bit_length())        # grows in powers of two: few re-allocations of pinned memory
        pin = self.net._pinned("api_res_out", (cap,), torch.uint8)
        host = []
        with self._link("d2h"):
            for o, t in parts:
                h = pin[o:o + t.numel() * t.element_size()].view(t.dtype)
                h.copy_(t, non_blocking=True)
                host.append(h.numpy())
            torch.cuda.current_stream().synchronize()
        wbits = host[0].reshape(-1, 2)[:, 1].view(np.uint32)
        blob = _res.pack(C, H, W, tol, widx, wbits, host[1].view(np.uint32), host[2], host[3].view(np.uint32),
                         host[4].view(np.uint32))
        return dict(blob=blob, records=(idx, q, eidx, ebits), step=torch.from_numpy(np.float32(2) * tol).to(dev),
                    records_n=int(per[:, 0].sum()), escapes_n=int(per[:, 1].sum()), per_channel=per, tol=tol)

    def _residual_encode(self, ts, x, output, tol, max_fraction):
        """The encoder's side of the residual layer for one frame: decode the frame's own strings (the whole frame,
        de-normalised: the x_hat every decoder of this .bin computes, bit for bit) and quantise the staged truth against
        it."""
        t_r = time.perf_counter()
        x_hat = self._decode_device(output["strings"], output["z_shape"], True, self._select(), phase=None)
        side = self._residual_build(ts, x, x_hat, tol, max_fraction)
        self._log("residual", t_r)
        return side

    @staticmethod
    def _residual_write(side, bin_path, write=True):
        """Write the sidecar beside `bin_path` -> the `residual` entry of the encode dict."""
        path = _res.sidecar_path(bin_path)
        if write:
            os.makedirs(os.path.dirname(path), exist_ok=True)
            with Path(path).open("wb") as f:
                f.write(side["blob"])
        return dict(path=path, bytes=len(side["blob"]), records=side["records_n"], escapes=side["escapes_n"],
                    per_channel=side["per_channel"], tol=side["tol"])

    @staticmethod
    def _residual_arg(what, residual, bin_paths, return_format, coarsen, regrid=None):
        """residual= of the decode methods -> one sidecar path (or None) per frame.  True: the .res beside each .bin."""
        if residual is None or residual is False:
            return [None] * len(bin_paths)
        if return_format not in ('de_normalized', 'de_normlized'):
            raise ValueError(f"{what}: residual= corrects the de-normalised reconstruction (the tolerances are in physical "
                             f"units); return_format={return_format!r} is not supported with it")
        if coarsen is not None:
            raise ValueError(f"{what}: residual= with coarsen= is not supported - the correction belongs before the "
                             "averaging, on points the coarsened decode never materialises")
        if regrid is not None:
            raise ValueError(f"{what}: residual= with regrid= is not supported - the correction belongs before the "
                             "regridding, on points the regridded decode never materialises")
        if residual is True:
            sides = [_res.sidecar_path(p) for p in bin_paths]
        elif isinstance(residual, (str, bytes, os.PathLike)):
            if len(bin_paths) != 1:
                raise ValueError(f"{what}: residual= takes True or one sidecar path per frame, got one path for "
                                 f"{len(bin_paths)} frames")
            sides = [residual]
        else:
            sides = list(residual)
            if len(sides) != len(bin_paths) or not all(isinstance(p, (str, bytes, os.PathLike)) for p in sides):
                raise ValueError(f"{what}: residual= takes True or one sidecar path per frame ({len(bin_paths)} frames)")
        for p in sides:
            if not os.path.exists(p):
                raise FileNotFoundError(f"{what}: residual sidecar {p} not found (written by encode_era5_as_bin / "
                                        "encode_era5_batch with max_error=)")
        return sides

    def _residual_load(self, path):
        """Read and check a sidecar (residual.unpack) -> dict with its records, step, witness indexes on the device."""
        with open(path, "rb") as f:
            side = _res.unpack(f.read())
        grid = (self.net.cfg['out_chans'],) + tuple(self.net.cfg['img_size'])
        if (side["C"], side["H"], side["W"]) != grid:
            raise ValueError(f"{path}: the sidecar belongs to a frame of {(side['C'], side['H'], side['W'])}, the model's "
                             f"grid is {grid}")
        dev = self.net.device

        def up(a):
            return torch.from_numpy(a.view(np.int16 if a.dtype.itemsize == 2 else np.int32)).to(dev, non_blocking=True)
        side["records"] = (up(side["idx"]), up(side["q"]), up(side["eidx"]), up(side["ebits"]))
        side["widx_dev"] = up(side["widx"])
        side["step"] = torch.from_numpy(np.float32(2) * side["tol"]).to(dev, non_blocking=True)
        side["grid"] = grid
        return side

    def _residual_correct(self, x_hat, side, sel, what):
        """Correct the decode's device output IN PLACE (x_hat [.., C', Ho, Wo]: the Selection `sel` of the frame).  The
        sidecar's witnesses inside the subset are compared with the plain decode first:
        ResidualMismatchError before anything is written."""
        out = x_hat.reshape(x_hat.shape[-3:])
        if out.data_ptr() != x_hat.data_ptr():
            raise RuntimeError("residual: the decode's output is not contiguous")
        lut = None
        channels, box, step = sel.channels, sel.box, sel.step
        if channels is not None:
            lut = np.full(side["C"], -1, dtype=np.int32)
            lut[list(channels)] = np.arange(len(channels), dtype=np.int32)
            lut = torch.from_numpy(lut).to(out.device)
        t_r = time.perf_counter()
        got = ops.residual_gather(out, side["widx_dev"], side["grid"], lut, box, step).cpu().numpy()
        _res.check_witnesses(got[:, 0] != 0, got[:, 1].view(np.uint32), side["wbits"], str(what))
        ops.residual_apply(out, side["records"], side["step"], side["grid"], lut, box, step)
        self._log("residual", t_r)

    # ------------------------------------------------------------------ decode
    def _bin_path(self, ts):
        """The default archive path of time stamp `ts`."""
        return f'{self.local_root}/CRA5/{ts[:4]}/{ts}.bin'

    @staticmethod
    def _denorm_arg(return_format):
        """return_format of a reconstruction -> whether it is de-normalised; ValueError for an unknown one."""
        if return_format not in ('de_normalized', 'de_normlized', 'normalized'):
            raise ValueError(f"unknown return_format {return_format!r}")
        return return_format != 'normalized'

    def _read_bin(self, bin_path):
        with Path(bin_path).open("rb") as f:
            return binfmt.unpack_bin(f.read())

    def bin_to_latent(self, bin_path=None, time_stamp=None):
        """cra5_api.py:127-144 (the reference's default path uses an undefined `time_stamp`;
        it is an explicit argument here)."""
        if bin_path is None:
            if time_stamp is None:
                raise ValueError("bin_to_latent needs bin_path or time_stamp")
            bin_path = self._bin_path(time_stamp)
        lstrings, shape = self._read_bin(bin_path)
        with torch.no_grad():
            return self.net.decompress(lstrings, shape, return_format='latent')

    def latent_to_reconstruction(self, y_hat, variables=None, region=None, stride=None, coarsen=None, regrid=None,
                                 points=None):
        """cra5_api.py:146-151 (normalised units).  variables / region / stride / coarsen / regrid / points: that subset,
        that target grid or those positions ([B, C', P]) (decode_from_bin)."""
        with torch.no_grad():
            return self.net.decode_latent(y_hat, **self._select(variables, region, stride, coarsen, regrid, points).model)

    def decode_from_bin(self, time_stamp=None, custom_path=None, return_format='de_normalized', to_host=False, out=None,
                        variables=None, region=None, stride=None, coarsen=None, residual=None, pack=None, regrid=None,
                        points=None):
        """cra5_api.py:153-192.  `to_host=True` (or `out=` a float32 array of the frame's shape): `x_hat` comes back
        as a HOST numpy array through the pinned staging buffer instead of a device tensor.
        variables: names of channel_vname_mapping() (e.g. ["z_500", "t_850", "t2m"]), output channels in that order;
        region: (lat_min, lat_max, lon_min, lon_max) in degrees (grid_box).  Either gives x_hat [C', Hb, Wb] - the slice
        of the full decode, bit for bit - and the dict then also carries `variables`, `lat` and `lon` (float64, lon in
        [0, 360)).
        stride: a positive int or (s_lat, s_lon) - of the box (default: the globe) only the rows r with r % s_lat == 0 and
        the columns c with c % s_lon == 0, r / c counted on the GLOBAL grid (a region's thinned decode is a sub-block of the
        globe's; 1440 % s_lon must be 0): decode_from_bin(ts, stride=6) is the 121 x 240 grid at 1.5 deg.  Again the slice
        of the full decode, bit for bit: x_hat == full[channels][:, kept_rows][:, :, kept_cols]; `lat` / `lon` are those of
        the kept rows / columns, `out` is checked against the thinned shape.  None / 1 / (1, 1): no thinning.
        coarsen: a positive int or (k_lat, k_lon), not together with a stride; 720 % k_lat == 0 and 1440 % k_lon == 0 - at
        the points stride=coarsen keeps, the area-weighted mean of the full decode over the coarse cell round each point
        (latitude band lat -+ k_lat * 0.125 deg clipped at the poles, longitude band lon -+ k_lon * 0.125 deg; first-order
        conservative remapping): decode_from_bin(ts, coarsen=6) is the conservative 1.5 deg field
        [C', 121, 240].  Computed on the GPU in fixed float64 arithmetic: bit-identical from run to run, a region's result
        the sub-block of the globe's; NaN / inf in a window propagate.  The dict also carries `coarsen`, `lat_bnds`
        [Hb, 2] (north, south) and `lon_bnds` [Wb, 2] (west, east).
        regrid: a cra5_amd.regrid.Grid (or its plan) - the full decode on that rectilinear target grid, by bilinear
        interpolation or first-order conservative remapping (the grid's method; DESIGN.md section 4, "Regridding"), on
        the GPU in fixed float64 arithmetic: x_hat is [C', Ho, Wo], rows in the grid's own order, and only the target grid
        crosses the host link.  The un-embed runs on the source box the target needs.  Not together with region / stride
        / coarsen (the target grid is the region), residual or return_format 'latent' (ValueError).  The dict also carries
        `regrid` (the method), `lat`, `lon`, `lat_bnds` [Ho, 2] (north, south) and `lon_bnds` [Wo, 2] (west, east).
        points: a cra5_amd.points.Points(lat, lon, method="bilinear" | "nearest"), or a plain [P, 2] array of (lat, lon)
        rows (bilinear) - stations, a track; any order, duplicates allowed: x_hat is [C', P], the full decode at those
        positions in the order given.  "nearest" is the grid point's value bit for bit (the dict carries node_lat /
        node_lon, the point taken), "bilinear" the bits of regrid=Grid([lat], [lon]) at that point (DESIGN.md section 4,
        "Point sampling").  Only the tokens whose patches hold a node are un-embedded, and only P values per variable
        cross the link.  With variables= only: ValueError together with region / stride / coarsen / regrid / residual /
        pack / return_format 'latent'.  The dict also carries `variables`, `lat`, `lon` (the points', float64 [P], lon in
        [0, 360)) and `points` (the method).
        residual: None | True (the .res beside the .bin: the same path with the extension replaced; a missing file is an
        error) | a sidecar path, written by encode_era5_as_bin(max_error=...).  Its corrections are added on the GPU, in
        place on the decode's output before it goes anywhere else: every point of the corrected channels is then the truth
        bit for bit or within the sidecar's tolerance of it, and a variables / region / stride subset is the slice of the
        corrected full frame, bit for bit.  The sidecar's witness points that fall inside the decoded subset are compared
        with the plain decode first (those outside it are not checked): a difference raises ResidualMismatchError and
        nothing is corrected.  Only with return_format 'de_normalized' and without coarsen= (ValueError otherwise).
        pack: None | "int16" / True (every channel packed over its own range in this frame - of the decoded subset, so a
        region's codes are not the slice of the globe's) | {variable: (lo, hi)} (pack.resolve_ranges: a fixed physical
        range for those channels, keyed by channel name or by pressure variable; under a fixed range a region's codes ARE
        the slice of the globe's, bit for bit).  `x_hat` is then the int16 frame [C', Hb, Wb] packed on the GPU (DESIGN.md
        section 4, "Packed int16 output") - a device tensor, or with to_host=True / out= an int16 array a host array - and
        the dict gains scale_factor, add_offset (float64 [C']), fill_value (-32768, the code of a non-finite value), vmin,
        vmax (float32), nonfinite (int64), saturated (bool: values outside a fixed range took -+32767).  unpack(q) = q *
        scale_factor + add_offset is within scale_factor * (0.5 + 2^-30) + 2^-50 max(|lo|, |hi|) of the decoded value; with
        residual=True the frame is corrected first and then packed, and the distance to the truth is bounded by the
        sidecar's tolerance plus that packing bound.  Only with return_format 'de_normalized' (ValueError otherwise)."""
        self._points_alone("decode_from_bin", points, residual, pack, return_format)
        if return_format == 'latent' and (variables is not None or region is not None or stride is not None
                                          or coarsen is not None or regrid is not None):
            raise ValueError("decode_from_bin: return_format='latent' returns the latent; variables / region / stride / "
                             "coarsen / regrid select a subset of the reconstruction")
        if return_format != 'latent':
            self._denorm_arg(return_format)
        sel = self._select(variables, region, stride, coarsen, regrid, points)
        bin_path = custom_path or self._bin_path(time_stamp)
        res_path = self._residual_arg("decode_from_bin", residual if residual is None or isinstance(residual, bool) else [residual],
                                      [bin_path], return_format, sel.coarsen, sel.regrid)[0]
        pk = self._pack_arg("decode_from_bin", pack, return_format, sel)
        stats = None
        decoding_start = time.time()
        lstrings, shape, side = self._read_frame(bin_path, res_path)
        with torch.no_grad():
            y_hat = self.net.decompress(lstrings, shape, return_format='latent')
            if return_format == 'latent':
                return y_hat
            if return_format == 'normalized':
                x_hat = self.net.decode_latent(y_hat, **sel.model)
            else:
                # fused de-normalisation in the overlap-add store
                x_hat = self.net._decode_guarded(y_hat[0], mean=self._mean_flat, std=self._std_flat, **sel.model)
                if side is not None:
                    self._residual_correct(x_hat, side, sel, res_path)
            if sel.points is not None:
                x_hat = x_hat.reshape(sel.shape)         # [C', P] from either format
            ht, dt = (np.float32, torch.float32) if pk is None else (np.int16, torch.int16)
            if pk is not None:
                x_hat, table, fixed = self._pack_device(x_hat.reshape(x_hat.shape[-3:]), pk)
                stats = _pk.frame_stats(table.cpu().numpy(), fixed)
            if to_host or out is not None:
                src = x_hat.reshape(x_hat.shape[-len(sel.shape):]).contiguous()
                if out is None:
                    out = np.empty(tuple(src.shape), dtype=ht)
                if out.dtype != ht or tuple(out.shape) != tuple(src.shape) or not out.flags["C_CONTIGUOUS"]:
                    raise ValueError("`out` must be a C-contiguous %s array of shape %r" % (np.dtype(ht).name, tuple(src.shape)))
                pin = self.net._pinned("api_x_out" if pk is None else "api_q_out", tuple(src.shape), dt)
                x_hat = ops.copy_d2h_staged(out, src, pin, threads=self.runtime.copy_threads)
        torch.cuda.synchronize()
        res = dict(x_hat=x_hat, decoding_time=time.time() - decoding_start)
        if not sel.whole:
            res.update(sel.meta)
        if stats is not None:
            res.update(stats)
        return res
