"""Indexed-colour PNG on the device path (gskyhip_encode_png_indexed): the
bytes of the host twin for every tile of tests/test_png_indexed_host.py from a
padded batch, the pixels of the shipped truecolour path (encode_rgba ->
encode_png) for the same rasters, rendered C2 tiles through
TileBatch.render_bytes() against render()'s RGBA, the 4096-row limit of the
device Deflate, GSKYHIP_PNG_ZLIB / GSKYHIP_PNG_FIXED, one size claim and the
argument errors."""
import ctypes as C
import io
import os

import numpy as np
import pytest

from gsky_amd import synth

from .helpers import gpu_batch
from .test_png_indexed_host import SHAPES, check_png, config_ramp, content, wrapping_ramp

pytestmark = pytest.mark.gpu

E_ARG = -1


def _tiles():
    """The host file's tiles: every shape with noise and blocks, every content
    at 131 x 67 and 600 x 5, the two-chunk noise tile."""
    out = [content(kind, w, h) for (w, h) in SHAPES for kind in ("noise", "blocks")]
    out += [content(kind, w, h) for kind in ("nodata", "constant", "gradient") for (w, h) in ((131, 67), (600, 5))]
    out.append(content("noise", 200, 200))
    return out


def _padded(tiles, gpu, pad=5):
    """(a view (n, H, W) whose rows lie W + pad bytes apart, sizes): the tiles
    in the top-left corners, garbage everywhere else."""
    import torch
    H = max(t.shape[0] for t in tiles)
    W = max(t.shape[1] for t in tiles)
    big = np.random.default_rng(3).integers(0, 256, (len(tiles), H + 1, W + pad), dtype=np.uint8)
    for k, t in enumerate(tiles):
        big[k, :t.shape[0], :t.shape[1]] = t
    dev = torch.from_numpy(big).to(gpu)
    return dev[:, :H, :W], [(t.shape[1], t.shape[0]) for t in tiles]


def _decode(png):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(png)).convert("RGBA"))


@pytest.mark.parametrize("ramp_name", ["config", "wrapping", "grey"])
def test_device_equals_host_twin(gpu, ramp_name):
    """Mixed sizes in one padded batch (row_stride > w, garbage in the
    padding): every PNG is the host twin's, byte for byte -- the two-chunk
    noise tile and the 64 / 65-row pair included."""
    from gsky_amd.encode import encode_png_indexed, encode_png_indexed_host
    ramp = {"config": config_ramp, "wrapping": wrapping_ramp, "grey": lambda: None}[ramp_name]()
    tiles = _tiles()
    view, sizes = _padded(tiles, gpu)
    assert view.stride(1) > view.shape[2] and not view.is_contiguous()
    pngs = encode_png_indexed(view, ramp, sizes)
    assert len(pngs) == len(tiles)
    for k, t in enumerate(tiles):
        assert pngs[k] == encode_png_indexed_host(t, ramp), (k, t.shape)
    assert len(check_png(pngs[-1], tiles[-1], ramp)) >= 2
    assert {(16, 64), (16, 65)} <= set(sizes)


def test_same_pixels_as_truecolour(gpu):
    """encode_rgba -> encode_png (the shipped path) and encode_png_indexed of
    the same rasters decode to the same RGBA at every pixel: the config
    palette, a palette with alpha 77 / 0 entries whose colours exceed alpha,
    and grey."""
    import torch

    import gsky_amd
    from gsky_amd.encode import encode_png, encode_png_indexed
    from gsky_amd.raster import encode_rgba
    tiles = [content("noise", 131, 67), content("blocks", 131, 67), content("gradient", 131, 67),
             content("nodata", 16, 64), content("noise", 257, 3), content("noise", 1, 5)]
    tiles[0][::7, ::5] = 0xFF
    view, sizes = _padded(tiles, gpu)
    H, W = view.shape[1:]
    pals = [gsky_amd.Palette(synth.PALETTE_GSKY, True),
            gsky_amd.Palette([(200, 100, 90, 77), (10, 20, 30, 0), (250, 2, 3, 255), (255, 255, 255, 77)], False),
            gsky_amd.Palette([(90, 200, 255, 77), (0, 0, 0, 255)], True), None]
    for pal in pals:
        rgba = torch.zeros((len(tiles), H, W, 4), dtype=torch.uint8, device=gpu)
        for k, t in enumerate(tiles):
            rgba[k, :t.shape[0], :t.shape[1]] = encode_rgba([torch.from_numpy(t).to(gpu)], pal)
        true = encode_png(rgba, sizes)
        indexed = encode_png_indexed(view, pal, sizes)
        for k, t in enumerate(tiles):
            a, b = _decode(true[k]), _decode(indexed[k])
            assert a.shape == (t.shape[0], t.shape[1], 4)
            assert np.array_equal(a, b), (pal, k)
        assert (_decode(indexed[0])[..., 3] == 0).any()


@pytest.mark.parametrize("auto", [False, True])
def test_rendered_tiles(gpu, auto):
    """render_bytes() -> encode_png_indexed decodes to render()'s RGBA tensor,
    for C2 tiles of ragged sizes with transparent pixels; with the layer's
    parameters (one gskyhip_scale call) and with an auto-scale (one per tile)."""
    import gsky_amd
    from gsky_amd.encode import encode_png_indexed
    cfg = synth.config_c2(scale=0.1, tiles_per_side=3, tile_px=200)
    cfg.tiles = [(bb, w - 17 * (i % 3), h - 9 * (i % 2)) for i, (bb, w, h) in enumerate(cfg.tiles)]
    b = gpu_batch(cfg, gpu)
    sp = gsky_amd.ScaleParams(0.0, 0.0, 0.0, cfg.scale[3]) if auto else gsky_amd.ScaleParams(*cfg.scale)
    pal = gsky_amd.Palette(cfg.palette, True)
    rgba = b.render(sp, pal).cpu().numpy().copy()
    assert b.status() == 0
    idx = b.render_bytes(sp)
    assert tuple(idx.shape) == (b.n_tiles, b.max_h, b.max_w) and str(idx.dtype) == "torch.uint8"
    sizes = [(w, h) for (_, w, h) in cfg.tiles]
    pngs = encode_png_indexed(idx, pal, sizes)
    host = idx.cpu().numpy()
    transparent = 0
    for t, (w, h) in enumerate(sizes):
        check_png(pngs[t], np.ascontiguousarray(host[t, :h, :w]), config_ramp())
        assert np.array_equal(_decode(pngs[t]), rgba[t, :h, :w]), t
        assert (host[t, h:] == 0xFF).all() and (host[t, :, w:] == 0xFF).all()
        transparent += int((rgba[t, :h, :w, 3] == 0).any())
    assert transparent >= 1 and (rgba[..., 3] == 255).any()


def test_render_bytes_three_namespaces(gpu):
    """Three namespaces have no index byte: the reference's error text."""
    import gsky_amd
    b = gsky_amd.TileBatch(gsky_amd.GranuleSet(gpu), "EPSG:3857", [], [], namespaces=("r", "g", "b"))
    with pytest.raises(ValueError, match="Cannot encode other than 1 or 3 namespaces into a PNG"):
        b.render_bytes(gsky_amd.ScaleParams(0.0, 1.0, 255.0, 0))


def _with_env(name, fn):
    os.environ[name] = "1"
    try:
        return fn()
    finally:
        del os.environ[name]


def test_row_limit_and_switches(gpu):
    """1 x 4096 is the device Deflate's (the host twin's bytes), 1 x 4097 goes
    to host zlib; GSKYHIP_PNG_ZLIB=1 and GSKYHIP_PNG_FIXED=1 on a small batch."""
    import torch

    from gsky_amd.encode import encode_png_indexed, encode_png_indexed_host
    ramp = config_ramp()
    rng = np.random.default_rng(9)
    for h in (4096, 4097):
        t = (rng.integers(0, 256, (h, 1), dtype=np.uint8) // 64 * 64).astype(np.uint8)
        png, = encode_png_indexed(torch.from_numpy(t).to(gpu)[None], ramp)
        check_png(png, t, ramp)
        assert (png == encode_png_indexed_host(t, ramp)) == (h == 4096)
    tiles = [content("blocks", 131, 67), content("noise", 16, 65), content("nodata", 3, 2)]
    view, sizes = _padded(tiles, gpu)
    dyn = encode_png_indexed(view, ramp, sizes)
    zl = _with_env("GSKYHIP_PNG_ZLIB", lambda: encode_png_indexed(view, ramp, sizes))
    fx = _with_env("GSKYHIP_PNG_FIXED", lambda: encode_png_indexed(view, ramp, sizes))
    for k, t in enumerate(tiles):
        check_png(zl[k], t, ramp)
        check_png(fx[k], t, ramp)
        assert fx[k] == encode_png_indexed_host(t, ramp, fixed_only=True)
        assert dyn[k] == encode_png_indexed_host(t, ramp)
    assert zl[0] != dyn[0]   # zlib's stream, not the GPU deflate's


def test_noise_tile_is_smaller_than_truecolour(gpu):
    """200 x 200 uniform noise under the config palette: a near-uniform byte a
    pixel costs about 8 bits, the same pixel as three or four separately coded
    bytes more, so the indexed PNG is the shorter one.  (No size claim is made
    for other tiles.)"""
    import torch

    import gsky_amd
    from gsky_amd.encode import encode_png, encode_png_indexed
    from gsky_amd.raster import encode_rgba
    t = content("noise", 200, 200)
    pal = gsky_amd.Palette(synth.PALETTE_GSKY, True)
    dev = torch.from_numpy(t).to(gpu)
    true, = encode_png(encode_rgba([dev], pal)[None])
    indexed, = encode_png_indexed(dev[None], pal)
    print("noise 200x200: indexed %d B, truecolour %d B" % (len(indexed), len(true)))
    assert np.array_equal(_decode(true), _decode(indexed))
    assert len(indexed) < len(true)


def test_errors(gpu):
    """A short workspace, a short capacity, a size beyond max_w and a row
    stride below max_w: GSKYHIP_E_ARG, before any HIP call."""
    import torch

    import gsky_amd
    L = gsky_amd.lib()
    n, H, W = 2, 8, 12
    idx = torch.zeros((n, H, W), dtype=torch.uint8, device=gpu)
    ws_bytes = int(L.gskyhip_png_indexed_workspace_size(n, W, H))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=gpu)
    cap = int(L.gskyhip_png_indexed_bound(W, H))
    out = np.full(n * cap, 0xA5, np.uint8)
    lens = np.full(n, -5, np.int64)

    def call(sizes, ws_n=ws_bytes, cap_=cap, row_stride=W, tile_stride=H * W, index=idx.data_ptr(), n_tiles=n):
        wh = np.asarray(sizes, np.int32).reshape(-1, 2)
        return L.gskyhip_encode_png_indexed(C.c_void_p(index), n_tiles, W, H, tile_stride, row_stride,
                                            wh.ctypes.data_as(C.c_void_p), None, C.c_void_p(ws.data_ptr()), ws_n,
                                            out.ctypes.data_as(C.c_void_p), cap_, lens.ctypes.data_as(C.c_void_p), 2,
                                            None)

    full = [(W, H), (W - 1, H)]
    assert call(full, ws_n=ws_bytes - 1) == E_ARG
    assert call(full, cap_=cap - 1) == E_ARG
    assert call([(W + 1, H), (W, H)]) == E_ARG
    assert call([(W, H + 1), (W, H)]) == E_ARG
    assert call([(0, H), (W, H)]) == E_ARG
    assert call(full, row_stride=W - 1) == E_ARG
    assert call(full, tile_stride=H * W - 1) == E_ARG
    assert call(full, index=None) == E_ARG
    assert (out == 0xA5).all() and (lens == -5).all()
    assert call(full, n_tiles=0) == 0 and (lens == -5).all()
    torch.cuda.synchronize()
    assert call(full) == 0
    assert (lens > 0).all()
