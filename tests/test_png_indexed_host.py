"""Indexed-colour PNG (colour type 3) of one-band tiles, through the host twin
gskyhip_encode_png_indexed_host (no GPU): the format include/gskyhip.h defines
-- chunk order, IHDR, PLTE and tRNS against a numpy restatement of the
formulas, 32 KiB IDAT chunks, the inflated rows, PIL's RGBA decode, the size
bound -- for every shape and content at which the encoder takes another path,
and the argument errors.  tests/test_png_indexed.py holds the device path to
these bytes."""
import ctypes as C
import io
import struct
import zlib

import numpy as np
import pytest

from gsky_amd import synth

SHAPES = [(1, 1), (1, 5), (3, 2), (4, 1), (255, 3), (256, 3), (257, 3), (131, 67), (16, 64), (16, 65)]
E_ARG = -1


def _chunks(png):
    """[(type, data)] of a PNG, every CRC verified."""
    assert png[:8] == b"\x89PNG\r\n\x1a\n"
    p, out = 8, []
    while p < len(png):
        n, = struct.unpack(">I", png[p:p + 4])
        typ = png[p + 4:p + 8]
        data = png[p + 8:p + 8 + n]
        assert len(data) == n
        crc, = struct.unpack(">I", png[p + 8 + n:p + 12 + n])
        assert crc == zlib.crc32(typ + data) & 0xFFFFFFFF, typ
        out.append((typ, data))
        p += 12 + n
    assert p == len(png)
    return out


def expected_table(ramp):
    """The 256 x 4 NRGBA table of the format: entry i < 255 is the
    color.NRGBAModel conversion of ramp[i] (a = 255: the bytes; a = 0: zero;
    else (((c * 0x101) * 0xFFFF) / (a * 0x101) >> 8) & 0xFF per channel) with
    the ramp's alpha, or (i, i, i, 255) for grey; entry 255 is (0, 0, 0, 0)."""
    tab = np.zeros((256, 4), np.uint8)
    for i in range(255):
        if ramp is None:
            tab[i] = (i, i, i, 255)
            continue
        r, g, b, a = (int(v) for v in ramp[i])
        if a == 255:
            tab[i] = (r, g, b, 255)
        elif a == 0:
            tab[i] = (0, 0, 0, 0)
        else:
            tab[i] = [(((c * 0x101) * 0xFFFF) // (a * 0x101) >> 8) & 0xFF for c in (r, g, b)] + [a]
    return tab


def config_ramp():
    """GradientRGBAPalette of docker/gsky_config.json's palette."""
    import gsky_amd
    return gsky_amd.gradient_rgba_palette(gsky_amd.Palette(synth.PALETTE_GSKY, True))


def wrapping_ramp():
    """Alphas in {0, 77, 255} and colour bytes above alpha: the conversion wraps."""
    rng = np.random.default_rng(11)
    ramp = rng.integers(78, 256, (256, 4), dtype=np.uint8)
    ramp[:, 3] = np.array([0, 77, 255], np.uint8)[rng.integers(0, 3, 256)]
    ramp[:3, 3] = (0, 77, 255)
    return ramp


RAMPS = {"config": config_ramp, "wrapping": wrapping_ramp, "grey": lambda: None}


def content(kind, w, h):
    rng = np.random.default_rng(w * 1000 + h)
    if kind == "nodata":
        return np.full((h, w), 0xFF, np.uint8)
    if kind == "constant":
        return np.full((h, w), 37, np.uint8)
    if kind == "noise":
        return rng.integers(0, 256, (h, w), dtype=np.uint8)
    if kind == "blocks":
        small = rng.integers(0, 256, (h // 4 + 1, w // 4 + 1), dtype=np.uint8)
        return np.ascontiguousarray(np.repeat(np.repeat(small, 4, 0), 4, 1)[:h, :w])
    if kind == "gradient":
        return np.ascontiguousarray(np.broadcast_to((np.arange(w) * 255 // max(1, w - 1)).astype(np.uint8), (h, w)))
    raise KeyError(kind)


def check_png(png, index, ramp):
    """Every property of the format for one tile; returns the IDAT chunks."""
    from PIL import Image

    from gsky_amd.encode import png_indexed_bound
    h, w = index.shape
    ch = _chunks(png)
    types = [t for t, _ in ch]
    n_idat = types.count(b"IDAT")
    assert n_idat >= 1 and types == [b"IHDR", b"PLTE", b"tRNS"] + [b"IDAT"] * n_idat + [b"IEND"]
    assert struct.unpack(">IIBBBBB", ch[0][1]) == (w, h, 8, 3, 0, 0, 0)
    table = expected_table(ramp)
    assert ch[1][1] == table[:, :3].tobytes()
    assert ch[2][1] == table[:, 3].tobytes()
    assert ch[-1][1] == b""
    idat = [d for t, d in ch if t == b"IDAT"]
    assert all(len(d) == 32768 for d in idat[:-1]) and 0 < len(idat[-1]) <= 32768
    assert zlib.decompress(b"".join(idat)) == b"".join(b"\0" + index[y].tobytes() for y in range(h))
    im = np.asarray(Image.open(io.BytesIO(png)).convert("RGBA"))
    assert np.array_equal(im, table[index])
    assert len(png) <= png_indexed_bound(w, h)
    return idat


@pytest.mark.parametrize("ramp_name", sorted(RAMPS))
@pytest.mark.parametrize("shape", SHAPES)
def test_shapes(shape, ramp_name):
    """Every shape with noise (literals, few matches) and with 4 x 4 blocks
    (row-above and run matches): 1 x 1 and 4 x 1 have no row above, 255 / 256 /
    257 columns put the 258-byte match limit inside, at and past a row, 64 / 65
    rows straddle the device tokeniser's groups of 64 rows."""
    from gsky_amd.encode import encode_png_indexed_host
    w, h = shape
    ramp = RAMPS[ramp_name]()
    for kind in ("noise", "blocks"):
        index = content(kind, w, h)
        check_png(encode_png_indexed_host(index, ramp), index, ramp)


@pytest.mark.parametrize("ramp_name", sorted(RAMPS))
@pytest.mark.parametrize("kind", ["nodata", "constant", "blocks", "gradient"])
def test_contents(kind, ramp_name):
    """Runs (all nodata: 258-byte matches at distance 1; one constant value),
    upsampled blocks, a left-to-right gradient (every row repeats the one
    above), at 131 x 67 and at 600 x 5 (rows longer than two full matches)."""
    from gsky_amd.encode import encode_png_indexed_host
    ramp = RAMPS[ramp_name]()
    for w, h in ((131, 67), (600, 5)):
        index = content(kind, w, h)
        png = encode_png_indexed_host(index, ramp)
        check_png(png, index, ramp)
        if kind in ("nodata", "constant"):
            assert len(png) < 8 + 25 + 780 + 268 + 12 + 12 + (w * h) // 16   # the runs were found


@pytest.mark.parametrize("ramp_name", sorted(RAMPS))
def test_noise_200(ramp_name):
    """Uniform noise at 200 x 200: 40,200 bytes of rows that do not compress,
    so the stream exceeds 32 KiB and takes two IDAT chunks; with every literal
    about equally frequent the dynamic code is no shorter than 8 bits a byte
    and the choice between it and the fixed code (8 / 9 bits) is exercised;
    fixed_only gives a valid, longer stream."""
    from gsky_amd.encode import encode_png_indexed_host
    ramp = RAMPS[ramp_name]()
    index = content("noise", 200, 200)
    png = encode_png_indexed_host(index, ramp)
    idat = check_png(png, index, ramp)
    assert len(idat) >= 2
    fixed = encode_png_indexed_host(index, ramp, fixed_only=True)
    assert len(check_png(fixed, index, ramp)) >= 2
    assert len(png) <= len(fixed)
    first = b"".join(idat)[2]          # the block header behind the 2-byte zlib header
    assert first & 1 == 1 and (first >> 1) & 3 in (1, 2)     # one final block, fixed or dynamic
    assert (b"".join(check_png(fixed, index, ramp))[2] >> 1) & 3 == 1


def test_fixed_only_blocks():
    """fixed_only on a compressible tile: valid, fixed codes, not shorter."""
    from gsky_amd.encode import encode_png_indexed_host
    ramp = config_ramp()
    index = content("blocks", 131, 67)
    dyn = encode_png_indexed_host(index, ramp)
    fixed = encode_png_indexed_host(index, ramp, fixed_only=True)
    idat = check_png(fixed, index, ramp)
    assert (b"".join(idat)[2] >> 1) & 3 == 1
    assert len(dyn) <= len(fixed)


def test_nodata_index_is_transparent_black():
    """Index 255 decodes to (0, 0, 0, 0) whatever ramp[255] holds, as EncodePNG
    leaves a 0xFF byte (ogc_encoders.go:96, 105)."""
    from PIL import Image

    from gsky_amd.encode import encode_png_indexed_host
    ramp = np.full((256, 4), 200, np.uint8)
    ramp[:, 3] = 255
    index = np.array([[255, 0], [254, 255]], np.uint8)
    for r in (ramp, None):
        im = np.asarray(Image.open(io.BytesIO(encode_png_indexed_host(index, r))).convert("RGBA"))
        assert im[0, 0].tolist() == [0, 0, 0, 0] and im[1, 1].tolist() == [0, 0, 0, 0]
        assert im[0, 1, 3] == 255 and im[1, 0, 3] == 255


def test_palette_argument():
    """A Palette, its ramp and the ramp as an array give the same bytes; a
    wrong array is refused."""
    import gsky_amd
    from gsky_amd.encode import encode_png_indexed_host
    index = content("blocks", 16, 64)
    pal = gsky_amd.Palette(synth.PALETTE_GSKY, True)
    assert encode_png_indexed_host(index, pal) == encode_png_indexed_host(index, config_ramp())
    with pytest.raises(ValueError):
        encode_png_indexed_host(index, np.zeros((255, 4), np.uint8))
    with pytest.raises(ValueError):
        encode_png_indexed_host(np.zeros((0, 4), np.uint8))


def test_errors():
    """w or h <= 0, NULL pointers and a capacity one byte short return
    GSKYHIP_E_ARG and leave the output as it was."""
    import gsky_amd
    L = gsky_amd.lib()
    index = content("blocks", 16, 65)
    h, w = index.shape
    ramp = config_ramp()
    cap = int(L.gskyhip_png_indexed_bound(w, h))
    size = C.c_int64(-7)

    def call(idx, ww, hh, out, cap_, size_ref):
        return L.gskyhip_encode_png_indexed_host(idx, ww, hh, ramp.ctypes.data_as(C.c_void_p), 0, out, cap_, size_ref)

    good = np.full(cap, 0xA5, np.uint8)
    assert call(index.ctypes.data_as(C.c_void_p), w, h, good.ctypes.data_as(C.c_void_p), cap, C.byref(size)) == 0
    n = size.value
    assert 0 < n <= cap and (good[n:] == 0xA5).all()
    check_png(good[:n].tobytes(), index, ramp)
    for args in [(index.ctypes.data_as(C.c_void_p), 0, h, "out", cap, "size"),
                 (index.ctypes.data_as(C.c_void_p), w, 0, "out", cap, "size"),
                 (index.ctypes.data_as(C.c_void_p), -3, h, "out", cap, "size"),
                 (index.ctypes.data_as(C.c_void_p), w, -1, "out", cap, "size"),
                 (None, w, h, "out", cap, "size"),
                 (index.ctypes.data_as(C.c_void_p), w, h, None, cap, "size"),
                 (index.ctypes.data_as(C.c_void_p), w, h, "out", cap, None),
                 (index.ctypes.data_as(C.c_void_p), w, h, "out", n - 1, "size")]:
        out = np.full(cap, 0xA5, np.uint8)
        a = [out.ctypes.data_as(C.c_void_p) if v == "out" else C.byref(size) if v == "size" else v for v in args]
        assert call(*a) == E_ARG, args[1:]
        assert (out == 0xA5).all(), args[1:]
    out = np.full(cap, 0xA5, np.uint8)   # exactly the PNG's length is enough
    assert call(index.ctypes.data_as(C.c_void_p), w, h, out.ctypes.data_as(C.c_void_p), n, C.byref(size)) == 0
    assert size.value == n and np.array_equal(out[:n], good[:n])
    assert L.gskyhip_png_indexed_bound(0, 5) == 0 and L.gskyhip_png_indexed_bound(5, -1) == 0
    assert L.gskyhip_png_indexed_workspace_size(0, 5, 5) == 0
    # the bound and the workspace are sized for 1 + w bytes a row, not 1 + 4 w
    assert L.gskyhip_png_indexed_bound(512, 512) < L.gskyhip_png_bound(512, 512) // 3
    assert L.gskyhip_png_indexed_workspace_size(8, 512, 512) < L.gskyhip_png_workspace_size(8, 512, 512) // 3


def test_truecolour_rows_host_still_refuses_one_byte_pixels():
    """gskyhip_png_deflate_rows_host keeps to bpp 3 and 4."""
    import gsky_amd
    L = gsky_amd.lib()
    rows = np.zeros(10, np.uint8)
    out = np.zeros(64, np.uint8)
    size = C.c_int64(0)
    assert L.gskyhip_png_deflate_rows_host(rows.ctypes.data_as(C.c_void_p), 2, 5, 1, 0,
                                           out.ctypes.data_as(C.c_void_p), 64, C.byref(size)) == E_ARG
