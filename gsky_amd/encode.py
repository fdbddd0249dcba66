"""Output codecs over the C-ABI (include/gskyhip.h): EncodePNG's png.Encode
(utils/ogc_encoders.go:139) for batches of RGBA tiles rendered into HBM, the
opt-in indexed-colour PNG of one-band tiles (encode_png_indexed), and
the WCS GeoTIFF of EncodeGdalOpen / EncodeGdal (ogc_encoders.go:277-450)."""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from ._lib import check, lib


def encode_png(rgba: torch.Tensor, sizes: Optional[Sequence[Tuple[int, int]]] = None,
               n_threads: Optional[int] = None) -> List[bytes]:
    """PNG bytes of every tile of an RGBA batch (n_tiles, max_h, max_w, 4)
    uint8 on the device; sizes (width, height) per tile (default the full
    slot), e.g. TileBatch.tile_sizes."""
    if rgba.dim() != 4 or rgba.shape[-1] != 4 or rgba.dtype != torch.uint8 or not rgba.is_cuda:
        raise ValueError("encode_png: (n, H, W, 4) uint8 device tensor expected")
    rgba = rgba.contiguous()
    n, mh, mw, _ = rgba.shape
    if sizes is None:
        sizes = [(mw, mh)] * n
    wh = np.ascontiguousarray(np.asarray(sizes, np.int32).reshape(n, 2))
    L = lib()
    ws = torch.empty(max(1, int(L.gskyhip_png_workspace_size(n, mw, mh))), dtype=torch.uint8, device=rgba.device)
    cap = int(max(L.gskyhip_png_bound(int(w), int(h)) for w, h in wh)) if n else 0
    out = np.empty(max(1, n * cap), np.uint8)
    lens = np.zeros(max(1, n), np.int64)
    threads = n_threads or max(1, min(16, os.cpu_count() or 1))
    check(L.gskyhip_encode_png(C.c_void_p(rgba.data_ptr()), n, mw, mh, mw * mh * 4, mw * 4,
                               wh.ctypes.data_as(C.c_void_p), C.c_void_p(ws.data_ptr()), ws.numel(),
                               out.ctypes.data_as(C.c_void_p), cap, lens.ctypes.data_as(C.c_void_p), threads,
                               C.c_void_p(torch.cuda.current_stream().cuda_stream)), "encode_png")
    return [out[t * cap:t * cap + int(lens[t])].tobytes() for t in range(n)]


def _ramp_of(palette, who: str) -> Optional[np.ndarray]:
    """The 256 x RGBA ramp of a Palette (GradientRGBAPalette), of a 256 x 4
    array as it is, or None (grey)."""
    if palette is None:
        return None
    if hasattr(palette, "colours"):
        from .raster import gradient_rgba_palette
        return np.ascontiguousarray(gradient_rgba_palette(palette))
    ramp = np.asarray(palette)
    if ramp.shape != (256, 4) or ramp.dtype != np.uint8:
        raise ValueError("%s: palette must be a Palette, a (256, 4) uint8 array or None" % who)
    return np.ascontiguousarray(ramp)


def encode_png_indexed(index: torch.Tensor, palette=None, sizes: Optional[Sequence[Tuple[int, int]]] = None,
                       n_threads: Optional[int] = None) -> List[bytes]:
    """Indexed-colour PNG bytes (colour type 3, gskyhip_encode_png_indexed) of
    every tile of a batch of ByteRasters (n_tiles, max_h, max_w) uint8 on the
    device, 0xFF = nodata, e.g. TileBatch.render_bytes(): what encode_png
    gives for the RGBA of the same rasters decodes to the same pixels, from a
    quarter of the bytes through Deflate.  Opt-in and beyond the reference,
    which always writes truecolour.  palette: a Palette, the 256 x 4 ramp of
    gradient_rgba_palette, or None for a grey layer; sizes (width, height) per
    tile (default the full slot), e.g. TileBatch.tile_sizes."""
    if index.dim() != 3 or index.dtype != torch.uint8 or not index.is_cuda:
        raise ValueError("encode_png_indexed: (n, H, W) uint8 device tensor expected")
    if index.stride(2) != 1 or index.stride(1) < index.shape[2] or index.stride(0) < index.stride(1) * index.shape[1]:
        index = index.contiguous()   # (padded rows and slots are taken as they are)
    n, mh, mw = index.shape
    ramp = _ramp_of(palette, "encode_png_indexed")
    if sizes is None:
        sizes = [(mw, mh)] * n
    wh = np.ascontiguousarray(np.asarray(sizes, np.int32).reshape(n, 2))
    L = lib()
    ws = torch.empty(max(1, int(L.gskyhip_png_indexed_workspace_size(n, mw, mh))), dtype=torch.uint8,
                     device=index.device)
    cap = int(max(L.gskyhip_png_indexed_bound(int(w), int(h)) for w, h in wh)) if n else 0
    out = np.empty(max(1, n * cap), np.uint8)
    lens = np.zeros(max(1, n), np.int64)
    threads = n_threads or max(1, min(16, os.cpu_count() or 1))
    with torch.cuda.device(index.device):
        check(L.gskyhip_encode_png_indexed(C.c_void_p(index.data_ptr()), n, mw, mh, index.stride(0) if n else 0,
                                           index.stride(1), wh.ctypes.data_as(C.c_void_p),
                                           ramp.ctypes.data_as(C.c_void_p) if ramp is not None else None,
                                           C.c_void_p(ws.data_ptr()), ws.numel(), out.ctypes.data_as(C.c_void_p),
                                           cap, lens.ctypes.data_as(C.c_void_p), threads,
                                           C.c_void_p(torch.cuda.current_stream(index.device).cuda_stream)),
              "encode_png_indexed")
    return [out[t * cap:t * cap + int(lens[t])].tobytes() for t in range(n)]


def png_indexed_bound(width: int, height: int) -> int:
    """gskyhip_png_indexed_bound: the most bytes of an indexed PNG of that size (0: bad size)."""
    return int(lib().gskyhip_png_indexed_bound(int(width), int(height)))


def encode_png_indexed_host(index: np.ndarray, palette=None, fixed_only: bool = False) -> bytes:
    """encode_png_indexed of one host tile, an (h, w) uint8 array
    (gskyhip_encode_png_indexed_host; no device, no HIP call): the PNG the
    device path writes for it, byte for byte.  fixed_only: fixed Huffman codes
    only, as GSKYHIP_PNG_FIXED=1."""
    index = np.asarray(index)
    if index.ndim != 2 or index.dtype != np.uint8 or index.size == 0:
        raise ValueError("encode_png_indexed_host: a non-empty (h, w) uint8 array expected")
    index = np.ascontiguousarray(index)
    h, w = index.shape
    ramp = _ramp_of(palette, "encode_png_indexed_host")
    L = lib()
    cap = int(L.gskyhip_png_indexed_bound(w, h))
    out = np.empty(cap, np.uint8)
    size = C.c_int64(0)
    check(L.gskyhip_encode_png_indexed_host(index.ctypes.data_as(C.c_void_p), w, h,
                                            ramp.ctypes.data_as(C.c_void_p) if ramp is not None else None,
                                            int(bool(fixed_only)), out.ctypes.data_as(C.c_void_p), cap,
                                            C.byref(size)), "encode_png_indexed_host")
    return out[:size.value].tobytes()


_TIFF_DTYPES = {torch.uint8: 1, torch.int8: 100, torch.int16: 3, torch.float32: 6}


DEFLATE_HOST, DEFLATE_DEVICE = 0, 1
TIFF_PACKBITS, TIFF_DEFLATE = 32773, 8


def _tiff_options(who, compression, predictor, zlevel, deflate, slab_tiles):
    """The checked (compression code, predictor, zlevel, deflate code, slab_tiles)."""
    if compression not in ("packbits", "deflate"):
        raise ValueError('%s: compression must be "packbits" or "deflate", not %r' % (who, compression))
    if deflate not in ("host", "device"):
        raise ValueError('%s: deflate must be "host" or "device", not %r' % (who, deflate))
    if predictor not in (1, 2, 3) or (compression == "packbits" and predictor != 1):
        raise ValueError("%s: predictor must be 1, 2 or 3 (1 with packbits), not %r" % (who, predictor))
    if not 0 <= int(zlevel) <= 9 or int(slab_tiles) < 0:
        raise ValueError("%s: zlevel must be 0..9 and slab_tiles >= 0" % who)
    return (TIFF_DEFLATE if compression == "deflate" else TIFF_PACKBITS, int(predictor), int(zlevel),
            DEFLATE_DEVICE if deflate == "device" else DEFLATE_HOST, int(slab_tiles))


def encode_geotiff(bands: Sequence[torch.Tensor], geot: Sequence[float], epsg: int,
                   nodata: Optional[Sequence[float]] = None, names: Optional[Sequence[str]] = None,
                   block: Tuple[int, int] = (1024, 256), uint16: bool = False, compression: str = "packbits",
                   predictor: int = 1, zlevel: int = 6, deflate: str = "device", slab_tiles: int = 0,
                   return_stats: bool = False, threads: int = 16):
    """GeoTIFF bytes of a coverage: `bands` (height, width) device tensors of
    one dtype (uint8, int8, int16 -- uint16 when `uint16`, the bits held in
    int16 --, float32), what EncodeGdal writes for format "geotiff" with
    the block size ows.go passes (1024 x 256): COMPRESS=PACKBITS.
    compression="deflate" (beyond the reference, which always writes PackBits)
    makes every tile one zlib stream after TIFF predictor `predictor` (1 none,
    2 horizontal differencing, 3 floating point: float32 only), by this
    library's Deflate encoder at `zlevel` (0 stored, 1-9 the one encoding).
    deflate="device": the tiles are gathered, predicted and deflated in HBM in
    slabs of `slab_tiles` tiles (0: the library's choice) and only compressed
    bytes are copied; deflate="host": the bands are copied to the host and
    `threads` host threads run the same encoder -- the same file.
    return_stats: also the tuple (tiles deflated on the device, raw bytes read
    from HBM, compressed bytes copied to the host, device workspace bytes)."""
    comp, pred, zl, mode, slab = _tiff_options("encode_geotiff", compression, predictor, zlevel, deflate, slab_tiles)
    if not bands:
        raise ValueError("encode_geotiff: no bands")
    dt = bands[0].dtype
    if dt not in _TIFF_DTYPES or any(b.dtype != dt or b.shape != bands[0].shape or not b.is_cuda for b in bands):
        raise ValueError("encode_geotiff: bands must be device tensors of one shape and a GeoTIFF dtype")
    code = 2 if (uint16 and dt == torch.int16) else _TIFF_DTYPES[dt]
    h, w = int(bands[0].shape[0]), int(bands[0].shape[1])
    bands = [b.contiguous() for b in bands]
    n = len(bands)
    L = lib()
    bx, by = int(block[0]), int(block[1])
    ptrs = (C.c_void_p * n)(*[b.data_ptr() for b in bands])   # EmptyTile bands: skipped by the writer
    gt = (C.c_double * 6)(*[float(v) for v in geot])
    nd = np.asarray(nodata, np.float64) if nodata is not None else None
    nm = (C.c_char_p * n)(*[s.encode() for s in names]) if names is not None else None
    size = C.c_int64(0)
    if comp == TIFF_PACKBITS and not return_stats:
        ws = torch.empty(max(1, int(L.gskyhip_geotiff_workspace_size(w, h, n, code, bx, by))), dtype=torch.uint8,
                         device=bands[0].device)
        cap = int(L.gskyhip_geotiff_bound(w, h, n, code, bx, by))
        if cap <= 0:
            raise ValueError("encode_geotiff: bad size / block")
        out = np.empty(cap, np.uint8)
        check(L.gskyhip_encode_geotiff(ptrs, n, code, w, h, gt, int(epsg),
                                       nd.ctypes.data_as(C.c_void_p) if nd is not None else None, nm, bx, by,
                                       C.c_void_p(ws.data_ptr()), ws.numel(), out.ctypes.data_as(C.c_void_p), cap,
                                       C.byref(size), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
              "encode_geotiff")
        return out[:size.value].tobytes()
    cap = int(L.gskyhip_geotiff_bound_opts(w, h, n, code, bx, by, comp))
    if cap <= 0:
        raise ValueError("encode_geotiff: bad size / block")
    out = np.empty(cap, np.uint8)
    stats = (C.c_int64 * 4)()
    with torch.cuda.device(bands[0].device):
        check(L.gskyhip_encode_geotiff_opts(ptrs, n, code, w, h, gt, int(epsg),
                                            nd.ctypes.data_as(C.c_void_p) if nd is not None else None, nm, bx, by,
                                            comp, pred, zl, mode, slab, int(threads),
                                            out.ctypes.data_as(C.c_void_p), cap, C.byref(size), stats,
                                            C.c_void_p(torch.cuda.current_stream(bands[0].device).cuda_stream)),
              "encode_geotiff_opts")
    data = out[:size.value].tobytes()
    return (data, tuple(stats)) if return_stats else data


_HOST_CODES = {np.dtype(np.uint8): 1, np.dtype(np.int8): 100, np.dtype(np.int16): 3, np.dtype(np.float32): 6,
               np.dtype(np.uint16): 2}


def geotiff_bound(width: int, height: int, n_bands: int, dtype, block: Tuple[int, int] = (1024, 256),
                  compression: str = "packbits") -> int:
    """gskyhip_geotiff_bound_opts: the most bytes encode_geotiff[_host] writes (0: bad arguments)."""
    if compression not in ("packbits", "deflate"):
        raise ValueError('geotiff_bound: compression must be "packbits" or "deflate", not %r' % (compression,))
    return int(lib().gskyhip_geotiff_bound_opts(int(width), int(height), int(n_bands), _HOST_CODES[np.dtype(dtype)],
                                                int(block[0]), int(block[1]),
                                                TIFF_DEFLATE if compression == "deflate" else TIFF_PACKBITS))


def encode_geotiff_host(bands: Sequence[np.ndarray], geot: Sequence[float], epsg: int,
                        nodata: Optional[Sequence[float]] = None, names: Optional[Sequence[str]] = None,
                        block: Tuple[int, int] = (1024, 256), compression: str = "packbits", predictor: int = 1,
                        zlevel: int = 6, threads: int = 4) -> bytes:
    """encode_geotiff of host numpy bands (gskyhip_encode_geotiff_host; no
    device, no HIP call): the file encode_geotiff writes for the same samples
    and options, byte for byte.  A band may be None when its name starts with
    "EmptyTile" (it is skipped, as EncodeGdal skips it)."""
    comp, pred, zl, _, _ = _tiff_options("encode_geotiff_host", compression, predictor, zlevel, "host", 0)
    real = [b for b in bands if b is not None] if bands else []
    if not real:
        raise ValueError("encode_geotiff_host: no bands")
    dt = np.dtype(real[0].dtype)
    if dt not in _HOST_CODES or any(b.dtype != dt or b.shape != real[0].shape or b.ndim != 2 for b in real):
        raise ValueError("encode_geotiff_host: bands must be 2-D arrays of one shape and a GeoTIFF dtype")
    code = _HOST_CODES[dt]
    h, w = int(real[0].shape[0]), int(real[0].shape[1])
    bands = [np.ascontiguousarray(b) if b is not None else None for b in bands]
    n = len(bands)
    L = lib()
    bx, by = int(block[0]), int(block[1])
    cap = int(L.gskyhip_geotiff_bound_opts(w, h, n, code, bx, by, comp))
    if cap <= 0:
        raise ValueError("encode_geotiff_host: bad size / block")
    out = np.empty(cap, np.uint8)
    size = C.c_int64(0)
    ptrs = (C.c_void_p * n)(*[b.ctypes.data if b is not None else None for b in bands])
    gt = (C.c_double * 6)(*[float(v) for v in geot])
    nd = np.asarray(nodata, np.float64) if nodata is not None else None
    nm = (C.c_char_p * n)(*[s.encode() for s in names]) if names is not None else None
    check(L.gskyhip_encode_geotiff_host(ptrs, n, code, w, h, gt, int(epsg),
                                        nd.ctypes.data_as(C.c_void_p) if nd is not None else None, nm, bx, by, comp,
                                        pred, zl, int(threads), out.ctypes.data_as(C.c_void_p), cap, C.byref(size)),
          "encode_geotiff_host")
    return out[:size.value].tobytes()



def encode_netcdf(bands: Sequence[torch.Tensor], geot: Sequence[float], epsg: int,
                  nodata: Optional[Sequence[float]] = None, names: Optional[Sequence[str]] = None,
                  zlevel: int = 6, uint16: bool = False, threads: int = 16, deflate: str = "host",
                  slab_rows: int = 0, return_stats: bool = False):
    """netCDF bytes of a coverage: what EncodeGdal writes for format
    "netcdf" with COMPRESS=DEFLATE, ZLEVEL=6 (utils/ogc_encoders.go:263-301):
    `bands` (height, width) device tensors of one dtype (uint8, int8, int16 --
    uint16 when `uint16`, the bits held in int16 --, float32).
    deflate="host": the rows are compressed by `threads` host threads (zlib)
    after a copy of each band to the host.  deflate="device": the chunks are
    shuffled and deflated in HBM, in slabs of `slab_rows` rows (0: the
    library's choice), and only compressed bytes are copied
    (gskyhip_encode_netcdf_deflate); the file differs from the host one in
    the chunk payloads only.  return_stats: also the tuple (chunks deflated
    on the device, raw bytes read from HBM, compressed bytes copied to the
    host, device workspace bytes)."""
    if deflate not in ("host", "device"):
        raise ValueError('deflate must be "host" or "device", not %r' % (deflate,))
    if not bands:
        raise ValueError("encode_netcdf: no bands")
    dt = bands[0].dtype
    if dt not in _TIFF_DTYPES or any(b.dtype != dt or b.shape != bands[0].shape or not b.is_cuda for b in bands):
        raise ValueError("encode_netcdf: bands must be device tensors of one shape and a supported dtype")
    code = 2 if (uint16 and dt == torch.int16) else _TIFF_DTYPES[dt]
    h, w = int(bands[0].shape[0]), int(bands[0].shape[1])
    bands = [b.contiguous() for b in bands]
    n = len(bands)
    L = lib()
    cap = int(L.gskyhip_netcdf_bound(w, h, n, code))
    if cap <= 0:
        raise ValueError("encode_netcdf: bad size / type")
    out = np.empty(cap, np.uint8)
    size = C.c_int64(0)
    ptrs = (C.c_void_p * n)(*[b.data_ptr() for b in bands])
    gt = (C.c_double * 6)(*[float(v) for v in geot])
    nd = np.asarray(nodata, np.float64) if nodata is not None else None
    nm = (C.c_char_p * n)(*[s.encode() for s in names]) if names is not None else None
    if deflate == "host" and not return_stats:
        check(L.gskyhip_encode_netcdf(ptrs, n, code, w, h, gt, int(epsg),
                                      nd.ctypes.data_as(C.c_void_p) if nd is not None else None, nm, int(zlevel),
                                      int(threads), out.ctypes.data_as(C.c_void_p), cap, C.byref(size),
                                      C.c_void_p(torch.cuda.current_stream().cuda_stream)), "encode_netcdf")
        return out[:size.value].tobytes()
    stats = (C.c_int64 * 4)()
    with torch.cuda.device(bands[0].device):
        check(L.gskyhip_encode_netcdf_deflate(ptrs, n, code, w, h, gt, int(epsg),
                                              nd.ctypes.data_as(C.c_void_p) if nd is not None else None, nm,
                                              int(zlevel), int(threads),
                                              DEFLATE_DEVICE if deflate == "device" else DEFLATE_HOST, int(slab_rows),
                                              out.ctypes.data_as(C.c_void_p), cap, C.byref(size), stats,
                                              C.c_void_p(torch.cuda.current_stream(bands[0].device).cuda_stream)),
              "encode_netcdf_deflate")
    data = out[:size.value].tobytes()
    return (data, tuple(stats)) if return_stats else data


def deflate_bound(n: int) -> int:
    """gskyhip_deflate_bound: the most bytes deflate_blocks gives for n input bytes."""
    return int(lib().gskyhip_deflate_bound(int(n)))


def deflate_blocks(blocks, zlib_wrapper: bool = True, level: int = 6, where: str = "device", out_caps=None,
                   return_status: bool = False, fill: int = 0xA5):
    """Compress every block (a bytes-like object) on its own into a zlib
    (zlib_wrapper) or raw Deflate stream: gskyhip_deflate_blocks on the
    current device and stream (where="device") or its host twin
    (where="host"), the counterpart of ingest.inflate_blocks.  Returns the
    list of streams.  out_caps[k] (default: gskyhip_deflate_bound) is block
    k's output capacity; return_status: instead the tuple (status list,
    out_len list, the output ranges as uint8 arrays of the full capacities,
    pre-filled with `fill`), so that a caller can see what was not written."""
    if where not in ("device", "host"):
        raise ValueError('where must be "device" or "host"')
    blocks = [bytes(b) for b in blocks]
    n = len(blocks)
    L = lib()
    in_len = np.array([len(b) for b in blocks], np.int64).reshape(n)
    in_off = np.zeros(n, np.int64)
    if n:
        in_off[1:] = np.cumsum(in_len)[:-1]
    src = np.frombuffer(b"".join(blocks) + b"\0", np.uint8).copy()   # never empty
    out_cap = np.array([L.gskyhip_deflate_bound(int(v)) for v in in_len] if out_caps is None else list(out_caps),
                       np.int64).reshape(n)
    out_off = np.zeros(n, np.int64)
    if n:
        out_off[1:] = np.cumsum(out_cap)[:-1]
    total = max(1, int(out_cap.sum()))
    status = np.full(n, -99, np.int32)
    out_len = np.full(n, -99, np.int64)
    p = lambda a: C.c_void_p(a.ctypes.data)
    if where == "host":
        dst = np.full(total, fill, np.uint8)
        rc = L.gskyhip_deflate_blocks_host(p(src), p(in_off), p(in_len), n, p(dst), p(out_off), p(out_cap),
                                           int(bool(zlib_wrapper)), int(level), p(status), p(out_len))
    else:
        dev = torch.device("cuda", torch.cuda.current_device())
        dsrc = torch.from_numpy(src).to(dev)
        ddst = torch.full((total,), fill, dtype=torch.uint8, device=dev)
        ws_bytes = max(16, int(L.gskyhip_deflate_workspace_size(n, int(in_len.sum()))))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream(dev)
        rc = L.gskyhip_deflate_blocks(C.c_void_p(dsrc.data_ptr()), p(in_off), p(in_len), n,
                                      C.c_void_p(ddst.data_ptr()), p(out_off), p(out_cap), int(bool(zlib_wrapper)),
                                      int(level), C.c_void_p(ws.data_ptr()), ws_bytes, p(status), p(out_len),
                                      C.c_void_p(stream.cuda_stream))
        with torch.cuda.stream(stream):
            dst = ddst.cpu().numpy()
    check(rc, "deflate_blocks")
    if return_status:
        return ([int(x) for x in status], [int(x) for x in out_len],
                [dst[int(out_off[k]):int(out_off[k] + out_cap[k])] for k in range(n)])
    for k in range(n):
        if status[k] != 0:
            raise ValueError("deflate_blocks: block %d has status %d" % (k, int(status[k])))
    return [dst[int(out_off[k]):int(out_off[k] + out_len[k])].tobytes() for k in range(n)]


def encode_netcdf_host(bands: Sequence[np.ndarray], geot: Sequence[float], epsg: int,
                       nodata: Optional[Sequence[float]] = None, names: Optional[Sequence[str]] = None,
                       zlevel: int = 6, uint16: bool = False, threads: int = 4, srs: Optional[str] = None) -> bytes:
    """encode_netcdf of host numpy bands (gskyhip_encode_netcdf_host; no device).
    `srs` (a PROJ string or WKT) replaces `epsg` for an SRS without a code
    (the geostationary family)."""
    codes = {np.dtype(np.uint8): 1, np.dtype(np.int8): 100, np.dtype(np.int16): 3, np.dtype(np.float32): 6,
             np.dtype(np.uint16): 2}
    if not bands:
        raise ValueError("encode_netcdf_host: no bands")
    dt = np.dtype(bands[0].dtype)
    if dt not in codes or any(b.dtype != dt or b.shape != bands[0].shape for b in bands):
        raise ValueError("encode_netcdf_host: bands must be arrays of one shape and a supported dtype")
    code = codes[dt]
    h, w = int(bands[0].shape[0]), int(bands[0].shape[1])
    bands = [np.ascontiguousarray(b) for b in bands]
    n = len(bands)
    L = lib()
    cap = int(L.gskyhip_netcdf_bound(w, h, n, code))
    out = np.empty(cap, np.uint8)
    size = C.c_int64(0)
    ptrs = (C.c_void_p * n)(*[b.ctypes.data for b in bands])
    gt = (C.c_double * 6)(*[float(v) for v in geot])
    nd = np.asarray(nodata, np.float64) if nodata is not None else None
    nm = (C.c_char_p * n)(*[s.encode() for s in names]) if names is not None else None
    if srs:
        check(L.gskyhip_encode_netcdf_srs_host(ptrs, n, code, w, h, gt, srs.encode(),
                                               nd.ctypes.data_as(C.c_void_p) if nd is not None else None, nm,
                                               int(zlevel), int(threads), out.ctypes.data_as(C.c_void_p), cap,
                                               C.byref(size)), "encode_netcdf_host")
        return out[:size.value].tobytes()
    check(L.gskyhip_encode_netcdf_host(ptrs, n, code, w, h, gt, int(epsg),
                                       nd.ctypes.data_as(C.c_void_p) if nd is not None else None, nm, int(zlevel),
                                       int(threads), out.ctypes.data_as(C.c_void_p), cap, C.byref(size)),
          "encode_netcdf_host")
    return out[:size.value].tobytes()
