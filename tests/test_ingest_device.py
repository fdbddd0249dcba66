"""Granule ingest with the block decode on the GPU (ingest.read / register with
decode="device"): the compressed blocks go to HBM, Deflate is decoded there
(inflate.hip), predictors / byte order / HDF5 shuffle are undone and the blocks
placed by kernels.  Every case asserts that the result equals the host decode
(ingest.read_host) bit for bit, and from the call's statistics that the blocks
really were decoded on the device -- a silent fall-back to the host cannot
pass.  Formats outside the device path must take the host path inside the same
call and say so in the statistics."""
import ctypes as C

import numpy as np
import pytest

from gsky_amd import GskyError, ingest
from gsky_amd._lib import lib

from .h5write import Var, write_nc4
from .tiffwrite import geokeys, write_tiff


def _same(got, exp):
    got = got.cpu().numpy()
    assert got.shape == exp.shape and got.dtype.itemsize == exp.dtype.itemsize
    assert np.array_equal(np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(exp).view(np.uint8))


def _device_equals_host(path, band=1, level=0):
    got, st = ingest.read(path, band, level, decode="device", return_stats=True)
    _same(got, ingest.read_host(path, band, level))
    assert st[0] > 0 and st[1] == 0, st      # decoded on the device, nothing on the host
    assert st[2] > 0 and st[3] > 0, st
    return st


def _host_fallback(path, band=1):
    got, st = ingest.read(path, band, decode="device", return_stats=True)
    _same(got, ingest.read_host(path, band))
    assert st[0] == 0 and st[1] > 0, st
    return st


def _data(rng, dt, shape):
    dt = np.dtype(dt)
    if dt.kind == "f":
        return (rng.standard_normal(shape) * 100).astype(dt)
    if dt.itemsize == 1:
        return rng.integers(0, 256, shape).astype(dt)
    # a smooth field plus noise: predictor 2 then gives Deflate something to match
    ramp = np.add.outer(np.arange(shape[0]) * 3, np.arange(shape[1]) * 5)
    return (ramp + rng.integers(-40, 40, shape)).astype(dt)


# ---------------------------------------------------------------- no device needed
def test_decode_argument_checks(tmp_path):
    p = str(tmp_path / "a.tif")
    write_tiff(p, [np.zeros((4, 4), np.uint8)], compression=8)
    with pytest.raises(ValueError):
        ingest.read(p, decode="gpu")
    with pytest.raises(ValueError):
        ingest.register(p, decode=None)
    L = lib()
    stats = (C.c_int64 * 4)(9, 9, 9, 9)
    buf = (C.c_uint8 * 16)()
    # a decode mode that does not exist; a file that does not; a band past the last
    assert L.gskyhip_geotiff_read_decode(p.encode(), 1, 0, buf, 16, 7, stats, None) == -1
    assert L.gskyhip_netcdf_read_decode(p.encode(), 1, buf, 16, -1, stats, None) == -1
    assert L.gskyhip_geotiff_read_decode(str(tmp_path / "none.tif").encode(), 1, 0, buf, 16, 1, stats, None) == 1
    assert list(stats) == [0, 0, 0, 0]
    assert L.gskyhip_geotiff_read_decode(p.encode(), 2, 0, buf, 16, 1, stats, None) == 2
    assert L.gskyhip_geotiff_read_decode(p.encode(), 1, 0, buf, 15, 1, None, None) == -1    # output too small
    assert L.gskyhip_geotiff_read_decode(p.encode(), 1, 0, None, 16, 1, None, None) == -1
    assert L.gskyhip_netcdf_read_decode(str(tmp_path / "none.nc").encode(), 1, buf, 16, 1, stats, None) == 1
    assert L.gskyhip_register_geotiff_decode(p.encode(), 1, 5, 256, 1) == -1                # no such overview method
    assert L.gskyhip_register_netcdf_decode(p.encode(), 1, -1, 256, 3) == -1
    assert L.gskyhip_register_geotiff_decode(None, 1, -1, 256, 1) == -1


# ---------------------------------------------------------------- GeoTIFF
@pytest.mark.gpu
@pytest.mark.parametrize("comp", [1, 8, 32946])
@pytest.mark.parametrize("pred", [1, 2])
def test_gpu_tiles_clipped_on_both_axes(gpu, tmp_path, comp, pred):
    a = _data(np.random.default_rng(comp + pred), np.int16, (33, 40))
    p = str(tmp_path / "t.tif")
    write_tiff(p, [a], tile=(16, 16), compression=comp, predictor=pred)
    st = _device_equals_host(p)
    assert st[0] == 9                         # 3 x 3 tiles
    assert st[3] == 9 * 16 * 16 * 2


@pytest.mark.gpu
@pytest.mark.parametrize("comp", [1, 8])
@pytest.mark.parametrize("dt", [np.uint8, np.int32])
def test_gpu_strips_with_a_short_last_strip(gpu, tmp_path, comp, dt):
    a = _data(np.random.default_rng(comp), dt, (33, 40))
    p = str(tmp_path / "s.tif")
    write_tiff(p, [a], rows_per_strip=5, compression=comp, predictor=2)
    assert _device_equals_host(p)[0] == 7     # 6 strips of 5 rows and one of 3


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(1, 1), (1, 37), (37, 1)])
def test_gpu_smallest_images(gpu, tmp_path, shape):
    a = _data(np.random.default_rng(shape[1]), np.uint16, shape)
    for k, kw in enumerate((dict(), dict(tile=(16, 16)))):
        p = str(tmp_path / ("m%d.tif" % k))
        write_tiff(p, [a], compression=8, predictor=2, **kw)
        _device_equals_host(p)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [np.uint8, np.int16, np.uint16, np.int32, np.float64])
def test_gpu_predictor2_rows_cross_the_scan_pieces(gpu, tmp_path, dt):
    """300 samples a row: five 64-lane pieces with a carry between them."""
    a = _data(np.random.default_rng(np.dtype(dt).itemsize), dt, (21, 300))
    p = str(tmp_path / "w.tif")
    write_tiff(p, [a], rows_per_strip=8, compression=8, predictor=2)
    _device_equals_host(p)
    assert np.array_equal(ingest.read_host(p).view(dt), a)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [np.float32, np.float64])
@pytest.mark.parametrize("be", [False, True])
def test_gpu_predictor3(gpu, tmp_path, dt, be):
    a = _data(np.random.default_rng(3 + be), dt, (21, 300))
    p = str(tmp_path / "f.tif")
    write_tiff(p, [a], tile=(128, 16), compression=8, predictor=3, be=be)
    _device_equals_host(p)
    assert np.array_equal(ingest.read_host(p).view(dt), a)


@pytest.mark.gpu
def test_gpu_block_larger_than_the_window_and_stored_block(gpu, tmp_path):
    rng = np.random.default_rng(8)
    f = rng.standard_normal((128, 128)).astype(np.float32)            # one 64 KiB tile: twice the 32 KiB window
    p = str(tmp_path / "f.tif")
    write_tiff(p, [f], tile=(128, 128), compression=8)
    assert _device_equals_host(p)[3] == 128 * 128 * 4
    b = rng.integers(0, 256, (192, 192)).astype(np.uint8)              # incompressible: Deflate stores it
    p = str(tmp_path / "b.tif")
    write_tiff(p, [b], tile=(192, 192), compression=32946)
    st = _device_equals_host(p)
    assert st[2] > 192 * 192                                           # the stream is larger than the tile


@pytest.mark.gpu
@pytest.mark.parametrize("planar", [1, 2])
@pytest.mark.parametrize("dt,pred", [(np.int16, 2), (np.uint8, 2), (np.float32, 3), (np.uint32, 1)])
def test_gpu_three_samples_chunky_and_planar(gpu, tmp_path, planar, dt, pred):
    rng = np.random.default_rng(planar * 10 + pred)
    bands = [_data(rng, dt, (45, 77)) for _ in range(3)]
    for k, kw in enumerate((dict(rows_per_strip=10), dict(tile=(32, 16)))):
        p = str(tmp_path / ("c%d.tif" % k))
        write_tiff(p, bands, compression=8, predictor=pred, planar=planar, **kw)
        for b in (1, 2, 3):
            _device_equals_host(p, b)
        assert np.array_equal(ingest.read_host(p, 2).view(dt), bands[1])


@pytest.mark.gpu
@pytest.mark.parametrize("big,be", [(True, False), (False, True), (True, True)])
@pytest.mark.parametrize("comp,pred,dt", [(8, 2, np.int16), (1, 1, np.uint32), (8, 2, np.float64), (1, 2, np.uint16)])
def test_gpu_bigtiff_and_big_endian(gpu, tmp_path, big, be, comp, pred, dt):
    rng = np.random.default_rng(comp + pred + 2 * big + be)
    bands = [_data(rng, dt, (50, 70)) for _ in range(2)]
    p = str(tmp_path / "e.tif")
    write_tiff(p, bands, tile=(32, 32), compression=comp, predictor=pred, big=big, be=be, planar=2)
    _device_equals_host(p, 1)
    _device_equals_host(p, 2)
    assert np.array_equal(ingest.read_host(p, 2).view(dt), bands[1])


@pytest.mark.gpu
def test_gpu_internal_overview_level(gpu, tmp_path):
    a = _data(np.random.default_rng(4), np.int16, (60, 80))
    p = str(tmp_path / "o.tif")
    write_tiff(p, [a], tile=(16, 16), compression=8, predictor=2, overviews=([a[::2, ::2].copy()], [a[::4, ::4].copy()]))
    for level in (0, 1, 2):
        _device_equals_host(p, 1, level)
    assert np.array_equal(ingest.read(p, 1, 1, decode="device").cpu().numpy(), a[::2, ::2])


@pytest.mark.gpu
def test_gpu_pillow_files(gpu, tmp_path):
    """libtiff's Deflate files: strips, the predictor tags, chunky RGB; its LZW
    and PackBits files take the host path inside the same call."""
    PIL = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(12)
    f = rng.standard_normal((61, 203)).astype(np.float32)
    for pred in (2, 3):
        p = str(tmp_path / ("f%d.tif" % pred))
        PIL.fromarray(f).save(p, compression="tiff_deflate", tiffinfo={317: pred})
        assert ingest.info(p).predictor == pred
        _device_equals_host(p)
    u = rng.integers(0, 65536, (40, 300)).astype(np.uint16)
    p = str(tmp_path / "u.tif")
    PIL.fromarray(u).save(p, compression="tiff_deflate", tiffinfo={317: 2})
    _device_equals_host(p)
    rgb = rng.integers(0, 256, (50, 61, 3)).astype(np.uint8)
    p = str(tmp_path / "rgb.tif")
    PIL.fromarray(rgb).save(p, compression="tiff_deflate")
    for b in (1, 2, 3):
        _device_equals_host(p, b)
    u[5:9, 10:50] = u[5, 10]
    for comp in ("tiff_lzw", "packbits"):
        p = str(tmp_path / (comp + ".tif"))
        PIL.fromarray(u).save(p, compression=comp)
        _host_fallback(p)


@pytest.mark.gpu
def test_gpu_packbits_written_here_takes_the_host_path(gpu, tmp_path):
    a = _data(np.random.default_rng(2), np.int16, (33, 40))
    p = str(tmp_path / "pb.tif")
    write_tiff(p, [a], tile=(16, 16), compression=32773)
    assert _host_fallback(p)[1] == 9


@pytest.mark.gpu
def test_gpu_damaged_block_is_the_host_paths_error(gpu, tmp_path):
    a = _data(np.random.default_rng(6), np.int16, (33, 40))
    p = str(tmp_path / "cut.tif")
    write_tiff(p, [a], tile=(16, 16), compression=8, predictor=2,
               mangle=lambda i, c: c[:len(c) // 2] if i == 4 else c)
    with pytest.raises(GskyError) as host:
        ingest.read_host(p)
    with pytest.raises(GskyError) as dev:
        ingest.read(p, decode="device")
    assert dev.value.code == host.value.code == -2
    # the device still works afterwards
    q = str(tmp_path / "good.tif")
    write_tiff(q, [a], tile=(16, 16), compression=8, predictor=2)
    _device_equals_host(q)


# ---------------------------------------------------------------- netCDF-4
def _nc4(path, data, increasing=False, time=None, **var_kw):
    ny, nx = data.shape[-2:]
    lat = (-44.0 + 0.2 * np.arange(ny)) if increasing else (-10.0 - 0.2 * np.arange(ny))
    lon = 112.0 + 0.25 * np.arange(nx)
    dims = ([("time", data.shape[0])] if data.ndim == 3 else []) + [("lat", ny), ("lon", nx)]
    variables = [Var("lat", ("lat",), np.asarray(lat, np.float64), filters=()),
                 Var("lon", ("lon",), np.asarray(lon, np.float64), filters=())]
    if data.ndim == 3:
        variables.append(Var("time", ("time",), np.arange(data.shape[0], dtype=np.float64), filters=()))
    kw = var_kw.pop("file_kw", {})
    variables.append(Var("v", tuple(d for d, _ in dims), data, **var_kw))
    write_nc4(path, dims, variables, {"Conventions": "CF-1.6"}, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("filters", [("shuffle", "deflate"), ("deflate",), ("shuffle",), ()],
                         ids=["shuffle-deflate", "deflate", "shuffle", "none"])
@pytest.mark.parametrize("dt", ["<i2", "<f4", "u1", "<f8", ">i4"])
def test_gpu_netcdf4_two_dimensions(gpu, tmp_path, filters, dt):
    rng = np.random.default_rng(len(filters) + np.dtype(dt).itemsize)
    data = _data(rng, np.dtype(dt).newbyteorder("="), (37, 29)).astype(dt)
    for increasing in (False, True):
        p = str(tmp_path / ("d%d.nc" % increasing))
        _nc4(p, data, increasing=increasing, chunks=(8, 8), filters=filters)
        st = _device_equals_host(p)
        assert st[0] == 5 * 4                 # every chunk of the 5 x 4 grid
        exp = data[::-1] if increasing else data
        assert np.array_equal(ingest.read_host(p).view(np.dtype(dt).newbyteorder("=")), exp.astype(exp.dtype.newbyteorder("=")))


@pytest.mark.gpu
@pytest.mark.parametrize("chunks", [(1, 8, 8), (2, 16, 16)], ids=["one-band", "two-bands"])
@pytest.mark.parametrize("increasing", [False, True], ids=["north-up", "south-up"])
def test_gpu_netcdf4_bands_of_a_chunk(gpu, tmp_path, chunks, increasing):
    """(3, 37, 29): a chunk of two leading indices holds bands 1 and 2."""
    data = _data(np.random.default_rng(chunks[0]), np.float32, (3 * 37, 29)).reshape(3, 37, 29)
    p = str(tmp_path / "b.nc")
    _nc4(p, data, increasing=increasing, chunks=chunks, file_kw=dict(superblock=2))
    for b in (1, 2, 3):
        _device_equals_host(p, b)
        exp = data[b - 1][::-1] if increasing else data[b - 1]
        assert np.array_equal(ingest.read(p, b, decode="device").cpu().numpy(), exp)


@pytest.mark.gpu
@pytest.mark.parametrize("fill", [None, -5])
@pytest.mark.parametrize("dt", ["<i2", ">f4"])
def test_gpu_netcdf4_chunks_never_written(gpu, tmp_path, fill, dt):
    data = (np.arange(20 * 30) % 97 + 1).astype(dt).reshape(1, 20, 30)
    p = str(tmp_path / "s.nc")
    atts = {} if fill is None else {"_FillValue": np.dtype(dt).newbyteorder("=").type(fill)}
    for fill_msg in (True, False):
        _nc4(p, data, increasing=True, chunks=(1, 10, 10), skip_chunks=(1, 4), atts=atts, fill_msg=fill_msg)
        st = _device_equals_host(p)
        assert st[0] == 4                     # six chunks, two never written


@pytest.mark.gpu
@pytest.mark.parametrize("skipped", ["deflate", "shuffle", "both"])
def test_gpu_netcdf4_filter_mask_of_one_chunk(gpu, tmp_path, skipped):
    """One chunk stored with a filter mask (the writer skipped a filter for
    it): the file is patched so that chunk (10, 10) is stored anew at the end
    of the file, without the filters its mask names."""
    import struct
    import zlib
    data = (np.arange(20 * 30) % 97 + 1).astype("<i2").reshape(20, 30)
    p = str(tmp_path / "m.nc")
    _nc4(p, data, chunks=(10, 10), filters=("shuffle", "deflate"))
    buf = bytearray(open(p, "rb").read())
    raw = np.ascontiguousarray(data[10:20, 10:20]).tobytes()
    shuffled = np.frombuffer(raw, np.uint8).reshape(-1, 2).T.tobytes()
    old = zlib.compress(shuffled, 4)                       # what the writer stored
    key = struct.pack("<II", len(old), 0) + struct.pack("<QQQ", 10, 10, 0)
    k = buf.find(key)
    assert k >= 0 and buf.find(key, k + 1) < 0
    stored, mask = {"deflate": (shuffled, 2), "shuffle": (zlib.compress(raw, 4), 1), "both": (raw, 3)}[skipped]
    struct.pack_into("<II", buf, k, len(stored), mask)     # the B-tree key: stored size, filter mask
    struct.pack_into("<Q", buf, k + len(key), len(buf))    # the chunk's new address
    buf += stored
    with open(p, "wb") as f:
        f.write(bytes(buf))
    assert np.array_equal(ingest.read_host(p), data)
    assert _device_equals_host(p)[0] == 6


@pytest.mark.gpu
def test_gpu_netcdf4_outside_the_device_path(gpu, tmp_path):
    """fletcher32, contiguous storage and netCDF classic: the host path,
    inside the same call."""
    data = _data(np.random.default_rng(1), np.int16, (2 * 20, 30)).reshape(2, 20, 30)
    p = str(tmp_path / "f.nc")
    _nc4(p, data, chunks=(1, 10, 10), filters=("fletcher32", "shuffle", "deflate"))
    assert _host_fallback(p, 2)[1] == 6
    p = str(tmp_path / "c.nc")
    _nc4(p, data, chunks=None, filters=())
    _host_fallback(p, 2)
    from scipy.io import netcdf_file
    p = str(tmp_path / "classic.nc")
    with netcdf_file(p, "w", version=1) as f:
        f.createDimension("lat", 20)
        f.createDimension("lon", 30)
        v = f.createVariable("v", np.int16, ("lat", "lon"))
        v[:] = data[0]
    _host_fallback(p)


# ---------------------------------------------------------------- register + the drop-in warp
@pytest.mark.gpu
def test_gpu_register_device_decode_then_warp(gpu, tmp_path):
    """register(decode="device", overviews="average") then the drop-in warp of
    one tile: the bytes of the same tile after register(path)."""
    from gsky_amd import synth, worker
    from gsky_amd.tiles import bbox_to_geot
    cfg = synth.config_c2(scale=0.05, tiles_per_side=2, tile_px=128)
    g = cfg.granules[0]
    p = str(tmp_path / "granule.tif")
    geo = [(33550, 12, [g.geot[1], -g.geot[5], 0.0]), (33922, 12, [0, 0, 0, g.geot[0], g.geot[3], 0]),
           geokeys(1, 1, [(3072, 3577)])]
    write_tiff(p, [g.data], tile=(64, 64), compression=8, predictor=2, geo=geo, nodata="%g" % g.nodata)
    bbox, w, h = cfg.tiles[0]
    req = dict(bands=[1], width=w, height=h, dstSRS="EPSG:3857", dstGeot=bbox_to_geot(w, h, bbox))

    def tile(**kw):
        worker.unregister_all()
        ingest.register(p, **kw)
        r = worker.warp_raster(worker.GeoRPCGranule(path=p, **req))
        assert r.error == "OK", r.error
        return worker.raster_array(r.raster).copy()

    plain = tile()
    assert (plain != g.nodata).any()
    assert np.array_equal(tile(decode="device", overviews="average"), plain)
    assert np.array_equal(tile(decode="device"), plain)
    assert np.array_equal(tile(decode="device", overviews="average"), tile(overviews="average"))
    # the file changes on disk: the drop-in reads it again, as it was registered
    worker.unregister_all()
    ingest.register(p, decode="device", overviews="average")
    changed = (g.data // 2).astype(g.data.dtype)
    write_tiff(p, [changed, changed], tile=(64, 64), compression=8, predictor=2, geo=geo, nodata="%g" % g.nodata)
    r = worker.warp_raster(worker.GeoRPCGranule(path=p, **req))
    assert r.error == "OK", r.error
    again = worker.raster_array(r.raster).copy()
    assert not np.array_equal(again, plain)
    assert np.array_equal(again, tile())
    worker.unregister_all()
