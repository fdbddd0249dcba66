"""The opt-in Deflate GeoTIFF of the WCS writer, from host bands
(gskyhip_encode_geotiff_host, encode.encode_geotiff_host): no device needed.

Every tile is one zlib stream of the tile's samples after TIFF predictor 1, 2
or 3.  The file is read back by two independent readers (the project's host
reader, and Pillow's libtiff for single-band files), its tile payloads are the
bytes the Deflate encoder's host twin gives for the predicted tile
(tests/tiffwrite._predict), and its size is held against zlib level 6 on the
same predicted tiles: the factor SIZE_M below is the ratio measured on the two
inputs of test_size (1.0049 for the int16 ramp with predictor 2, 1.0199 for
the float32 field with predictor 3) plus two points -- the
bytes are deterministic, the margin only absorbs another zlib build."""
import ctypes as C
import zlib

import numpy as np
import pytest

from gsky_amd import encode, ingest
from gsky_amd._lib import lib

from .test_geotiff import read_bigtiff
from .tiffwrite import _predict

GT = [1500000.0, 25.0, 0.0, -3900000.0, 0.0, -25.0]
SIZE_M = {"int16": 1.0049 + 0.02, "float32": 1.0199 + 0.02}
E_ARG, E_TYPE = -1, -2


def _band(dtype, h, w, seed=0):
    """A band with structure (a ramp) and noise, so that predictors and matches both have work."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    if dtype == "float32":
        a = (280.0 + 0.05 * x + 0.03 * y + rng.uniform(-0.5, 0.5, (h, w))).astype(np.float32)
        a[h // 3, w // 2] = np.float32("nan")
        a[0, 0] = -0.0
        return a
    info = np.iinfo(dtype)
    a = (3 * x + 2 * y + rng.integers(-4, 5, (h, w))) % (int(info.max) - int(info.min) + 1) + int(info.min)
    return a.astype(dtype)


def _tile_bytes(buf, tags):
    return [buf[o:o + n] for o, n in zip(tags[324], tags[325])]


def _padded_tiles(arr, bx, by, pad):
    """The band's tiles, row-major, edge tiles padded with `pad`: (by, bx, 1) arrays."""
    h, w = arr.shape
    ntx, nty = -(-w // bx), -(-h // by)
    full = np.full((nty * by, ntx * bx), pad, arr.dtype)
    full[:h, :w] = arr
    return [full[ty * by:(ty + 1) * by, tx * bx:(tx + 1) * bx][..., None] for ty in range(nty) for tx in range(ntx)]


def _same_bits(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape
    return a.tobytes() == b.tobytes()


def _read_back(tmp_path, buf, arrs, pillow):
    path = str(tmp_path / "out.tif")
    with open(path, "wb") as f:
        f.write(buf)
    inf = ingest.info(path)
    assert (inf.xsize, inf.ysize, inf.n_bands) == (arrs[0].shape[1], arrs[0].shape[0], len(arrs))
    for k, a in enumerate(arrs):
        assert _same_bits(ingest.read_host(path, k + 1), a), "band %d through the host reader" % (k + 1)
    if pillow and len(arrs) == 1:
        Image = pytest.importorskip("PIL.Image")
        with Image.open(path) as im:
            got = np.asarray(im)
        a = arrs[0]
        assert got.shape == a.shape
        if a.dtype == np.float32:
            assert _same_bits(got.astype(np.float32), a)
        elif a.dtype == np.int8:   # libtiff hands 8-bit samples over as unsigned
            assert np.array_equal(got.astype(np.int64) & 0xFF, a.astype(np.int64) & 0xFF)
        else:
            assert np.array_equal(got.astype(np.int64), a.astype(np.int64))


MATRIX = [(dt, p) for dt in ("uint8", "int8", "int16", "uint16") for p in (1, 2)] + [("float32", p) for p in (1, 2, 3)]


@pytest.mark.parametrize("dtype,predictor", MATRIX)
def test_read_back_two_readers(tmp_path, dtype, predictor):
    a = _band(dtype, 40, 33, seed=predictor)   # 33 x 40 with 16 x 16 tiles: clipped on both axes
    buf = encode.encode_geotiff_host([a], GT, 3577, [5.0], ["b&<1>"], block=(16, 16), compression="deflate",
                                     predictor=predictor)
    tags = read_bigtiff(buf)
    assert tags[259] == [8] and tags[322] == [16] and tags[323] == [16]
    assert (317 in tags) == (predictor != 1) and tags.get(317, [predictor]) == [predictor]
    assert len(tags[324]) == 3 * 3 and float(tags[42113]) == 5.0
    assert 'sample="0">b&amp;&lt;1&gt;<' in tags[42112]
    _read_back(tmp_path, buf, [a], pillow=True)


def test_read_back_two_bands(tmp_path):
    arrs = [_band("int16", 40, 33, seed=s) for s in (11, 12)]
    buf = encode.encode_geotiff_host(arrs, GT, 3577, [-999.0, -999.0], ["a", "b"], block=(16, 16),
                                     compression="deflate", predictor=2)
    tags = read_bigtiff(buf)
    assert tags[277] == [2] and tags[284] == [2] and len(tags[324]) == 2 * 9
    _read_back(tmp_path, buf, arrs, pillow=False)


@pytest.mark.parametrize("dtype,predictor", [("int16", 2), ("float32", 3)])
def test_read_back_tile_larger_than_image(tmp_path, dtype, predictor):
    a = _band(dtype, 40, 300, seed=3)   # 40 rows of 300: one 1024 x 256 tile, larger than the image on both axes
    buf = encode.encode_geotiff_host([a], GT, 4326, None, None, block=(1024, 256), compression="deflate",
                                     predictor=predictor)
    tags = read_bigtiff(buf)
    assert len(tags[324]) == 1 and 42113 not in tags and 42112 not in tags
    _read_back(tmp_path, buf, [a], pillow=True)
    tall = _band(dtype, 300, 40, seed=4)   # and 300 rows of 40: two tiles down, both wider than the image
    buf = encode.encode_geotiff_host([tall], GT, 4326, None, None, block=(1024, 256), compression="deflate",
                                     predictor=predictor)
    assert len(read_bigtiff(buf)[324]) == 2
    _read_back(tmp_path, buf, [tall], pillow=True)


@pytest.mark.parametrize("dtype,predictor,nodata", [("int16", 2, -999.0), ("float32", 3, -1.5)])
def test_tile_payloads_are_the_host_twins(dtype, predictor, nodata):
    a = _band(dtype, 40, 33, seed=7)
    buf = encode.encode_geotiff_host([a], GT, 3577, [nodata], None, block=(16, 16), compression="deflate",
                                     predictor=predictor)
    tags = read_bigtiff(buf)
    assert tags[259] == [8] and tags[317] == [predictor]
    tiles = _tile_bytes(buf, tags)
    want = _padded_tiles(a, 16, 16, np.dtype(dtype).type(nodata))
    assert len(tiles) == len(want) == 9
    streams = encode.deflate_blocks([_predict(t, predictor).tobytes() for t in want], zlib_wrapper=True, level=6,
                                    where="host")
    for k in range(9):
        assert tiles[k] == streams[k], "tile %d" % k
    # band-major, tiles row-major, end to end behind the 16-byte header
    assert tags[324][0] == 16
    assert all(tags[324][k + 1] == tags[324][k] + tags[325][k] for k in range(8))
    # without the predictor tag when it is 1
    plain = read_bigtiff(encode.encode_geotiff_host([a], GT, 3577, [nodata], None, block=(16, 16),
                                                    compression="deflate", predictor=1))
    assert plain[259] == [8] and 317 not in plain


def test_packbits_from_host_bands():
    """compression="packbits": the reference's file, read by the PackBits reader of tests/test_geotiff.py."""
    from .test_geotiff import decode_bands
    arrs = [_band("int16", 40, 33, seed=s) for s in (1, 2)]
    arrs[0][10:30] = 77   # runs
    buf = encode.encode_geotiff_host(arrs, GT, 3577, [3.0, 4.0], ["a", "b"], block=(16, 16))
    tags = read_bigtiff(buf)
    assert tags[259] == [32773] and 317 not in tags
    got = decode_bands(buf, tags)
    assert np.array_equal(got[0], arrs[0]) and np.array_equal(got[1], arrs[1])
    assert len(buf) <= encode.geotiff_bound(33, 40, 2, "int16", (16, 16), "packbits")


def test_constant_band():
    a = np.full((40, 33), 1234, np.int16)
    for predictor in (1, 2):
        buf = encode.encode_geotiff_host([a], GT, 3577, [1234.0], None, block=(16, 16), compression="deflate",
                                         predictor=predictor)
        for t in _tile_bytes(buf, read_bigtiff(buf)):
            # two 256-byte segments of a few tokens each: far below an eighth of the 512 raw bytes
            assert len(t) <= 512 // 8
            assert len(zlib.decompress(t)) == 512


def test_random_band_stays_within_the_bounds():
    a = np.random.default_rng(5).integers(0, 256, (40, 33)).astype(np.uint8)
    buf = encode.encode_geotiff_host([a], GT, 3577, None, None, block=(16, 16), compression="deflate")
    tags = read_bigtiff(buf)
    tiles = _tile_bytes(buf, tags)
    assert all(len(t) <= encode.deflate_bound(256) for t in tiles)
    bound = encode.geotiff_bound(33, 40, 1, "uint8", (16, 16), "deflate")
    assert 0 < len(buf) <= bound
    want = _padded_tiles(a, 16, 16, 0)
    for t, w in zip(tiles, want):
        assert zlib.decompress(t) == w.tobytes()
    # the output buffer may be exactly the bound, and not a byte less
    L = lib()
    ptrs = (C.c_void_p * 1)(a.ctypes.data)
    gt = (C.c_double * 6)(*GT)
    out = np.empty(bound, np.uint8)
    size = C.c_int64(0)
    args = lambda cap: (ptrs, 1, 1, 33, 40, gt, 3577, None, None, 16, 16, 8, 1, 6, 1, out.ctypes.data_as(C.c_void_p),
                        cap, C.byref(size))
    assert L.gskyhip_encode_geotiff_host(*args(bound)) == 0 and out[:size.value].tobytes() == buf
    assert L.gskyhip_encode_geotiff_host(*args(bound - 1)) == E_ARG


def test_zlevel_0_is_stored():
    a = _band("int16", 40, 33, seed=9)
    buf = encode.encode_geotiff_host([a], GT, 3577, None, None, block=(16, 16), compression="deflate", predictor=2,
                                     zlevel=0)
    want = _padded_tiles(a, 16, 16, 0)
    for t, w in zip(_tile_bytes(buf, read_bigtiff(buf)), want):
        raw = _predict(w, 2).tobytes()
        assert len(t) == 2 + 5 + 512 + 4 and (t[2] >> 1) & 3 == 0   # zlib header, one stored block, Adler-32
        assert t[7:7 + 512] == raw and zlib.decompress(t) == raw


def test_empty_tile_band_between_two(tmp_path):
    arrs = [_band("int16", 40, 33, seed=s) for s in (21, 22, 23)]
    names = ["red", "EmptyTile_green", "blue"]
    nodata = [1.0, 2.0, 7.0]
    files = []
    for middle in (arrs[1], None):   # skipped whether or not it has samples
        buf = encode.encode_geotiff_host([arrs[0], middle, arrs[2]], GT, 4326, nodata, names, block=(16, 16),
                                         compression="deflate", predictor=2)
        files.append(buf)
    assert files[0] == files[1]
    tags = read_bigtiff(files[0])
    assert float(tags[42113]) == 7.0   # "blue": the last band that set one
    md = tags[42112]
    assert 'sample="0">red<' in md and 'sample="2">blue<' in md and 'sample="1"' not in md
    tiles = _tile_bytes(files[0], tags)
    assert len(tiles) == 27 and all(t == tiles[9] for t in tiles[9:18])   # one tile, compressed once, repeated
    _read_back(tmp_path, files[0], [arrs[0], np.full((40, 33), 7, np.int16), arrs[2]], pillow=False)


def _size_input(dtype):
    rng = np.random.default_rng(2024)
    y, x = np.mgrid[0:256, 0:256]
    if dtype == "int16":
        return (1000 + 5 * x + 3 * y + rng.integers(-40, 41, (256, 256))).astype(np.int16)
    smooth = 280.0 + 15.0 * np.sin(x / 37.0) * np.cos(y / 53.0) + 0.02 * x
    return (smooth + rng.uniform(-5.0, 5.0, (256, 256))).astype(np.float32)


@pytest.mark.parametrize("dtype,predictor", [("int16", 2), ("float32", 3)])
def test_size(dtype, predictor):
    a = _size_input(dtype)
    deflated = encode.encode_geotiff_host([a], GT, 3577, None, None, block=(64, 64), compression="deflate",
                                          predictor=predictor)
    packbits = encode.encode_geotiff_host([a], GT, 3577, None, None, block=(64, 64), compression="packbits")
    tags = read_bigtiff(deflated)
    ours = sum(tags[325])
    z6 = sum(len(zlib.compress(_predict(t, predictor).tobytes(), 6)) for t in _padded_tiles(a, 64, 64, 0))
    print("%s predictor %d: payloads %d, zlib level 6 %d, ratio %.4f, of raw %.4f; files %d (deflate) %d (packbits)" %
          (dtype, predictor, ours, z6, ours / z6, ours / a.nbytes, len(deflated), len(packbits)))
    assert len(deflated) < len(packbits)
    assert ours <= SIZE_M[dtype] * z6


def _call_host(L, a, **kw):
    p = dict(bands=(C.c_void_p * 1)(a.ctypes.data), n_bands=1, dtype=3, width=33, height=40, geot=(C.c_double * 6)(*GT),
             epsg=3577, nodata=None, names=None, bx=16, by=16, comp=8, pred=2, zlevel=6, threads=2)
    p.update(kw)
    out = np.empty(1 << 20, np.uint8)
    size = C.c_int64(-5)
    rc = L.gskyhip_encode_geotiff_host(p["bands"], p["n_bands"], p["dtype"], p["width"], p["height"], p["geot"],
                                       p["epsg"], p["nodata"], p["names"], p["bx"], p["by"], p["comp"], p["pred"],
                                       p["zlevel"], p["threads"], out.ctypes.data_as(C.c_void_p),
                                       p.get("cap", out.size), C.byref(size) if p.get("size", True) else None)
    return rc, size.value


def _call_opts(L, a, **kw):
    """gskyhip_encode_geotiff_opts with arguments it refuses before any device work."""
    p = dict(bands=(C.c_void_p * 1)(a.ctypes.data), n_bands=1, dtype=3, width=33, height=40, geot=(C.c_double * 6)(*GT),
             bx=16, by=16, comp=8, pred=2, zlevel=6, deflate=1, slab=0)
    p.update(kw)
    out = np.empty(1 << 20, np.uint8)
    size = C.c_int64(-5)
    stats = (C.c_int64 * 4)(9, 9, 9, 9)
    rc = L.gskyhip_encode_geotiff_opts(p["bands"], p["n_bands"], p["dtype"], p["width"], p["height"], p["geot"], 3577,
                                       None, None, p["bx"], p["by"], p["comp"], p["pred"], p["zlevel"], p["deflate"],
                                       p["slab"], 2, out.ctypes.data_as(C.c_void_p), p.get("cap", out.size),
                                       C.byref(size), stats, None)
    return rc, size.value, list(stats)


BAD = [dict(bands=None), dict(geot=None), dict(n_bands=0), dict(n_bands=4097), dict(width=0), dict(height=-1),
       dict(bx=0), dict(by=24), dict(bx=40), dict(comp=5), dict(comp=1), dict(pred=0), dict(pred=4), dict(pred=3),
       dict(comp=32773, pred=2), dict(zlevel=-1), dict(zlevel=10), dict(cap=100)]


def test_argument_checks():
    L = lib()
    a = _band("int16", 40, 33)
    assert _call_host(L, a)[0] == 0
    for bad in BAD:
        assert _call_host(L, a, **bad) == (E_ARG, -5), bad   # nothing reported as written
    assert _call_host(L, a, dtype=9) == (E_TYPE, -5)
    assert _call_host(L, a, size=False)[0] == E_ARG
    f = _band("float32", 40, 33)
    assert _call_host(L, f, dtype=6, pred=3)[0] == 0
    # the device entry point refuses the same, and its own options, before any device work
    for bad in BAD + [dict(deflate=2), dict(deflate=-1), dict(slab=-1)]:
        rc, size, stats = _call_opts(L, a, **bad)
        assert (rc, size, stats) == (E_ARG, -5, [0, 0, 0, 0]), bad
    assert _call_opts(L, a, dtype=9) == (E_TYPE, -5, [0, 0, 0, 0])
    assert L.gskyhip_geotiff_bound_opts(33, 40, 1, 3, 16, 16, 5) == 0
    assert L.gskyhip_geotiff_bound_opts(33, 40, 1, 9, 16, 16, 8) == 0
    assert L.gskyhip_geotiff_bound_opts(0, 40, 1, 3, 16, 16, 8) == 0
    assert L.gskyhip_geotiff_bound_opts(33, 40, 2, 3, 16, 16, 32773) == L.gskyhip_geotiff_bound(33, 40, 2, 3, 16, 16)
    assert L.gskyhip_geotiff_bound_opts(33, 40, 2, 3, 16, 16, 8) >= 18 * encode.deflate_bound(512)
    # bad strings are refused in Python, as encode_netcdf refuses them
    for kw in (dict(compression="lzw"), dict(compression="deflate", predictor=4), dict(predictor=2),
               dict(compression="deflate", zlevel=11)):
        with pytest.raises(ValueError):
            encode.encode_geotiff_host([a], GT, 3577, **kw)
    for kw in (dict(compression="zip"), dict(deflate="gpu"), dict(slab_tiles=-1), dict(predictor=2)):
        with pytest.raises(ValueError):
            encode.encode_geotiff([], GT, 3577, **kw)
