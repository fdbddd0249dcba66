"""Native granule ingest: GeoTIFF and netCDF classic
files decoded by libgskyhip.so (ingest.hip) -- the GDALOpenEx / GDALRasterIO step of the
worker (worker/gdalprocess/warp.go:89-118, drill.go:61-69, 142) -- into host
arrays (tests) or straight into HBM tensors (the product path), plus the
metadata GDAL reports for the file (size, type, geotransform, nodata, EPSG,
overviews)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np

from ._lib import (BYTE, FLOAT32, FLOAT64, INT16, INT32, MAX_OVR, UINT16, UINT32, GskyError, RasterInfo, decode_mode,
                   lib, ovr_method)

NP_DTYPE = {BYTE: np.uint8, UINT16: np.uint16, INT16: np.int16, UINT32: np.uint32, INT32: np.int32,
            FLOAT32: np.float32, FLOAT64: np.float64}


@dataclass
class GeoTiffInfo:
    xsize: int
    ysize: int
    n_bands: int
    dtype: int
    signed_byte: bool
    block: Tuple[int, int]
    compression: int
    predictor: int
    planar: int
    epsg: int                 # -1: MODIS sinusoidal sphere, 0: unknown
    geot: Tuple[float, ...]
    nodata: Optional[float]   # None when GDAL_NODATA is absent
    overviews: List[Tuple[int, int]]

    @property
    def srs(self) -> str:
        return "MODIS" if self.epsg == -1 else ("EPSG:%d" % self.epsg if self.epsg > 0 else "")

    def np_dtype(self):
        return np.int8 if self.signed_byte else NP_DTYPE[self.dtype]

    def level_shape(self, level: int) -> Tuple[int, int]:
        return (self.ysize, self.xsize) if level == 0 else self.overviews[level - 1][::-1]


def is_netcdf(path: str) -> bool:
    """warp.go:89-101: "NETCDF:..." and "*.nc" go through the netCDF driver."""
    return path.startswith("NETCDF:") or path.endswith(".nc")


def info(path: str) -> GeoTiffInfo:
    r = RasterInfo()
    fn = lib().gskyhip_netcdf_info if is_netcdf(path) else lib().gskyhip_geotiff_info
    rc = fn(path.encode(), C.byref(r))
    if rc:
        raise GskyError(rc, "raster info (%s)" % path)
    return GeoTiffInfo(r.xsize, r.ysize, r.n_bands, r.dtype, bool(r.signed_byte), (r.block_x, r.block_y),
                       r.compression, r.predictor, r.planar, r.epsg, tuple(r.geot),
                       r.nodata if r.has_nodata else None,
                       [(r.ovr_xsize[k], r.ovr_ysize[k]) for k in range(r.n_ovr)])


def netcdf_srs(path: str, srs_cf: int = 0) -> str:
    """The dataset SRS GSKY_netCDF reports under the srs_cf open option
    (warp.go:95): "EPSG:<n>", a PROJ string, "" (none) or "?" (a CF grid
    mapping outside the supported projections)."""
    buf = C.create_string_buffer(1024)
    rc = lib().gskyhip_netcdf_srs(path.encode(), int(srs_cf), buf, len(buf))
    if rc:
        raise GskyError(rc, "netcdf_srs")
    return buf.value.decode()


def read_host(path: str, band: int = 1, level: int = 0) -> np.ndarray:
    """Band `band` (1-based) of `level` decoded on the host (no device work)."""
    inf = info(path)
    out = np.empty(inf.level_shape(level), inf.np_dtype())
    if is_netcdf(path):
        rc = lib().gskyhip_netcdf_read_host(path.encode(), band, out.ctypes.data, out.nbytes)
    else:
        rc = lib().gskyhip_geotiff_read_host(path.encode(), band, level, out.ctypes.data, out.nbytes)
    if rc:
        raise GskyError(rc, "%s(%s)" % ("gskyhip_netcdf_read_host" if is_netcdf(path) else "gskyhip_geotiff_read_host", path))
    return out


def read(path: str, band: int = 1, level: int = 0, device=None, decode: str = "host", return_stats: bool = False):
    """The same decoded into a new HBM tensor.  decode="host": host-thread
    decompression, one H2D copy of the decoded bytes, GPU block assembly.
    decode="device": one H2D copy of the *compressed* blocks, Deflate decoded,
    un-predicted / un-shuffled and placed by kernels (formats outside that
    path are decoded on the host inside the same call).  return_stats: also
    the tuple (blocks decoded on the device, blocks decoded on the host,
    compressed bytes copied to the device, decoded bytes produced)."""
    import torch
    mode = decode_mode(decode)
    inf = info(path)
    tdt = {np.uint8: torch.uint8, np.int8: torch.int8, np.int16: torch.int16, np.uint16: torch.int16,
           np.int32: torch.int32, np.uint32: torch.int32, np.float32: torch.float32,
           np.float64: torch.float64}[inf.np_dtype()]
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    out = torch.empty(inf.level_shape(level), dtype=tdt, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    nbytes = out.numel() * out.element_size()
    if mode == 0 and not return_stats:
        if is_netcdf(path):
            name = "gskyhip_netcdf_read"
            rc = lib().gskyhip_netcdf_read(path.encode(), band, C.c_void_p(out.data_ptr()), nbytes, C.c_void_p(stream))
        else:
            name = "gskyhip_geotiff_read"
            rc = lib().gskyhip_geotiff_read(path.encode(), band, level, C.c_void_p(out.data_ptr()), nbytes,
                                            C.c_void_p(stream))
        if rc:
            raise GskyError(rc, "%s(%s)" % (name, path))
        return out
    stats = (C.c_int64 * 4)()
    with torch.cuda.device(dev):
        if is_netcdf(path):
            name = "gskyhip_netcdf_read_decode"
            rc = lib().gskyhip_netcdf_read_decode(path.encode(), band, C.c_void_p(out.data_ptr()), nbytes, mode, stats,
                                                  C.c_void_p(stream))
        else:
            name = "gskyhip_geotiff_read_decode"
            rc = lib().gskyhip_geotiff_read_decode(path.encode(), band, level, C.c_void_p(out.data_ptr()), nbytes, mode,
                                                   stats, C.c_void_p(stream))
    if rc:
        raise GskyError(rc, "%s(%s)" % (name, path))
    return (out, tuple(stats)) if return_stats else out


def inflate_blocks(streams, out_sizes, zlib_wrapper: bool = True, where: str = "device", out_need=None, gap: int = 0,
                   fill: int = 0xA5):
    """Decode Deflate streams (bytes objects) in one call, stream k into a
    capacity of out_sizes[k] bytes: gskyhip_inflate_blocks on the current
    device (where="device") or its host twin (where="host").  Returns
    (status list, out_len list, outputs as a list of uint8 arrays of the full
    capacities, the gaps as a list of arrays): the output ranges are laid out
    `gap` bytes apart in a buffer pre-filled with `fill`, and the bytes before,
    between and after them are returned so that a caller can see they were not
    written.  out_need[k] (default: out_sizes[k]) is the least length that
    counts as success."""
    if where not in ("device", "host"):
        raise ValueError('where must be "device" or "host"')
    n = len(streams)
    if len(out_sizes) != n:
        raise ValueError("one output size per stream")
    need = list(out_sizes) if out_need is None else list(out_need)
    in_len = np.array([len(s) for s in streams], np.int64)
    in_off = np.zeros(n, np.int64)
    if n:
        in_off[1:] = np.cumsum(in_len)[:-1]
    src = np.frombuffer(b"".join(streams) + b"\0", np.uint8).copy()   # never empty
    out_cap = np.array(out_sizes, np.int64)
    out_off = np.zeros(n, np.int64)
    at = gap
    for k in range(n):
        out_off[k] = at
        at += int(out_cap[k]) + gap
    total = max(1, at)
    out_need_a = np.array(need, np.int64)
    status = np.full(n, -99, np.int32)
    out_len = np.full(n, -99, np.int64)
    p = lambda a: C.c_void_p(a.ctypes.data)
    if where == "host":
        dst = np.full(total, fill, np.uint8)
        rc = lib().gskyhip_inflate_blocks_host(p(src), p(in_off), p(in_len), n, p(dst), p(out_off), p(out_cap),
                                               p(out_need_a), int(bool(zlib_wrapper)), p(status), p(out_len))
    else:
        import torch
        dev = torch.device("cuda", torch.cuda.current_device())
        dsrc = torch.from_numpy(src).to(dev)
        ddst = torch.full((total,), fill, dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        rc = lib().gskyhip_inflate_blocks(C.c_void_p(dsrc.data_ptr()), p(in_off), p(in_len), n,
                                          C.c_void_p(ddst.data_ptr()), p(out_off), p(out_cap), p(out_need_a),
                                          int(bool(zlib_wrapper)), p(status), p(out_len), C.c_void_p(stream))
        torch.cuda.synchronize(dev)
        dst = ddst.cpu().numpy()
    if rc:
        raise GskyError(rc, "gskyhip_inflate_blocks")
    outs = [dst[int(out_off[k]):int(out_off[k] + out_cap[k])] for k in range(n)]
    gaps, prev = [], 0
    for k in range(n):
        gaps.append(dst[prev:int(out_off[k])])
        prev = int(out_off[k] + out_cap[k])
    gaps.append(dst[prev:])
    return [int(x) for x in status], [int(x) for x in out_len], outs, gaps


def overview_levels(xsize: int, ysize: int, min_size: int = 256) -> List[Tuple[int, int]]:
    """(xsize, ysize) of the pyramid levels gskyhip_build_overviews makes,
    finest first: ceil(n / 2^k) per axis while the level before is larger
    than min_size (<= 0: 256), at most 12."""
    xs = (C.c_int32 * MAX_OVR)()
    ys = (C.c_int32 * MAX_OVR)()
    n = lib().gskyhip_overview_levels(int(xsize), int(ysize), int(min_size), xs, ys)
    if n < 0:
        raise GskyError(n, "overview_levels")
    return [(xs[k], ys[k]) for k in range(n)]


def build_overviews(tensor, nodata: Optional[float] = None, method: str = "nearest", min_size: int = 256,
                    signed_byte: bool = False) -> list:
    """The overview pyramid of a 2-D HBM tensor (uint8, int8, int16, uint16
    or float32), built by the overview kernel on the current stream: a list
    of new tensors, finest first (include/gskyhip.h for the rules)."""
    import torch
    from .tiles import DTYPE_OF_TORCH
    m = ovr_method(method)
    if tensor.dim() != 2 or not tensor.is_cuda:
        raise ValueError("build_overviews takes a 2-D tensor in HBM")
    if tensor.dtype not in DTYPE_OF_TORCH:
        raise GskyError(-2, "build_overviews (%s)" % tensor.dtype)
    t = tensor.contiguous()
    ysize, xsize = t.shape
    sizes = overview_levels(xsize, ysize, min_size)
    out = [torch.empty((h, w), dtype=t.dtype, device=t.device) for w, h in sizes]
    n = len(out)
    ptrs = (C.c_void_p * max(1, n))(*[o.data_ptr() for o in out])
    xs = (C.c_int32 * max(1, n))(*[w for w, _ in sizes])
    ys = (C.c_int32 * max(1, n))(*[h for _, h in sizes])
    with torch.cuda.device(t.device):
        stream = torch.cuda.current_stream(t.device).cuda_stream
        rc = lib().gskyhip_build_overviews(C.c_void_p(t.data_ptr()), DTYPE_OF_TORCH[t.dtype],
                                           int(signed_byte or t.dtype == torch.int8), xsize, ysize,
                                           int(nodata is not None), float(nodata if nodata is not None else -1e10),
                                           m, n, ptrs, xs, ys, C.c_void_p(stream))
    if rc:
        raise GskyError(rc, "build_overviews")
    return out


def register(path: str, band: int = 1, overviews: Optional[str] = None, min_size: int = 256,
             decode: str = "host") -> None:
    """Decode every level of (path, band) into library-owned HBM and register
    it for warp_operation_fast (worker.warp_raster).  overviews = "nearest" /
    "average": a band that comes without overviews gets a pyramid of that
    method down to min_size, built on the GPU (a file's own overviews win).
    decode="device": each level is read with the block decode on the GPU
    (read(..., decode="device"))."""
    mode = decode_mode(decode)
    if mode:
        fn = lib().gskyhip_register_netcdf_decode if is_netcdf(path) else lib().gskyhip_register_geotiff_decode
        rc = fn(path.encode(), band, -1 if overviews is None else ovr_method(overviews), int(min_size), mode)
    elif overviews is None:
        fn = lib().gskyhip_register_netcdf if is_netcdf(path) else lib().gskyhip_register_geotiff
        rc = fn(path.encode(), band)
    else:
        fn = lib().gskyhip_register_netcdf_ovr if is_netcdf(path) else lib().gskyhip_register_geotiff_ovr
        rc = fn(path.encode(), band, ovr_method(overviews), int(min_size))
    if rc:
        raise GskyError(rc, "register (%s)" % path)
