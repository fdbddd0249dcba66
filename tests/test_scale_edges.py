"""The scale rule (utils.Scale, raster_scaler.go:30-332) on every device
implementation of it, against the rule in numpy (tests/test_scale_rule.py)
over that module's whole table: every data set under every parameter set.

The implementations (S1..S5), the paths, and the call that reaches each:

  (a) S1 scale_one + scale_minmax / finalize / apply      gsky_amd.scale(), all five types
  (b) S1 through the raw ABI                              lib().gskyhip_scale on n in N_RAW elements, `out` 0..3
      bytes into a larger tensor: scale_apply_kernel packs four bytes into one 32-bit store only when the
      address is aligned and four pixels remain; auto mode with the single minimum and maximum in
      different waves and blocks
  (c) Byte in place                                       after (a) / (b) a Byte input equals the output, every
      other type's input is bit-identical to before
  (d) S5 scale_legacy_kernel                              gsky_amd.scale_legacy() against scale_legacy_rule
  (e) S4 scale_int<T, SAFE> / nn_rgba (render_nn.h)       batch.render(sp, pal) and (sp, None): one value type,
      one namespace, no auto-scale, nearest: launch_render picks lds_mode 0, launch_band_t ends in
      launch_nn_t -> render_nn_kernel.  float32 takes scale_t<float> -> scale_px (S2) there
  (f) S3 scale_t<T> in render_fast_t                      the same with batch.typed = False: value_types 0 gives
      (render_generic.h:447)                              lds_mode -1, dispatch_render_1(general_only = false)
      launches render_fast_kernel, whose tiles are simple and dispatch on tp.vt to render_fast_t<.., T>
  (g) S3 / S2, three namespaces                           n_out = 3: dispatch_render_3 -> render_fast_kernel<3>
      (render_generic.h:451-453); in auto mode canvas_rgba_kernel with n_out = 3 (S2)
  (h) S3 scale_t<T> in render_lds_kernel                  render(sp, pal, resample=1): lds_mode kBilinear,
      (render_lds.h:275)                                  launch_band_t -> launch_lds_t for every integer type
      (float32 RGBA as well; float32 canvases alone go to render_bil_kernel).  On the 1:1 geometry every
      sample is a pixel centre, so bilinear returns the pixel's own value: asserted on the CPU with
      oracle.warp(resample 1) before the GPU is asked
  (h') S2 scale_px in render_band (render_generic.h:284)  a tile that also stacks a float32 granule of an unrendered
      namespace is complex (tile_info), so render_general_kernel renders it: S2 on integer canvases
  (i) S2 after the minmax fold                            triple (0, 0, 0) with RGBA out: render_auto_kernel
      (render_generic.h:247-270), then canvas_rgba_kernel's auto_minmax + make_scale + scale_px; the
      tiles of one batch have different sizes in one slot, so pixel 0 and min / max are per tile
  (j) S1 in fuse.hip                                      gskyhip_fuse_render's outer scale and a scaled layer of
      gskyhip_fuse_layers, one uploaded layer canvas (Int16, Float32): scale_one with the constants of
      host_scale_consts() on fuse_prepare's call path

Bar, every path: identical bytes (np.array_equal on the uint8 band or the
RGBA tile), no tolerance, no pixel left out.  The geometry of (e)-(i) is that
of tests/test_nn_rule.py (same CRS, 1:1, the granule's corner on the tile's),
so a canvas holds its granule's values verbatim; the CPU asserts that with
tile_reference before the GPU is asked.

The table's (0, 1e7, 0) does not reach SAFE == false: its clip of 0 clamps
every value to 0 (asserted in test_scale_rule.py); (0, 1e7, 65535), (0, 3e38,
40000) and the upper `safe` neighbour do.

No departure found: all five implementations give the rule's bytes.

Measured on an MI355X (-s prints the running counts): pixels compared per
path over all types, differences 0 on every one:

  (a) gsky_amd.scale()             64 306 160   (340 cases per integer type, 888 float32)
  (b) raw ABI                         242 820   (840 calls), auto extrema 18 450
  (d) scale_legacy()               48 575 820
  (e) band kernel, palette + grey 121 973 984
  (f) typed generic kernels        64 306 160
  (g) three namespaces             42 827 776
  (h) LDS kernel, bilinear        119 550 584   (h') general kernel 62 921 360
  (i) auto-scale through render     6 638 336
  (j) fuse: outer scale             1 341 952   scaled layer 1 328 128

The module's 41 tests take 4.2 s, start-up of the interpreter and torch
included; the slowest test takes 0.35 s.

Deliberate one-line breaks, each in a scratch build loaded in place of the
library (the whole module ran every time), and the first case that noticed:
  clamp order swapped in scale_int (0 first, then clip) -- (e) int8, domain
    nd0 nodata 0 under (0, 0, 1000) (int8(1000) is -24), 65 280 pixels; (e)
    int16 under (0, 0, 40000), 65 535 pixels; no other path holds scale_int
  the uint8_t wrap cast dropped from scale_t -- (f), (h) and (g) uint8 under
    (1, 1, 1000), 256 pixels per tile; not (e): the nearest-neighbour band
    kernel scales integers with scale_int
  safe = true unconditionally -- (e) int16 under (0, inf, 5), 32 767 pixels;
    (e) uint16 under (0, 3e38, 40000), 65 535 pixels
  go_u8_f32 replaced by (uint8_t)f -- the same two in (e); (f) and (h) of the
    rebuilt types from (1, 1, 1000) on (values above 255 keep their low byte
    in Go and saturate in the cast)
  <= for < in scale_one's value < 0 -- nothing, as it must: 0 becomes 0
  the f == f guard dropped from scale_minmax_kernel -- (a) float32, the
    "specials nodata nan" set under (0, 0, 0) with the log colour scale
  the p0 handling dropped from auto_minmax -- (i): "auto one valid at 0" (1
    pixel) and "auto all equal" of every integer type, "domain v0 nodata 0"
    of uint16 (126 pixels), "auto element 0 NaN" of float32; (g) uint16
  maxVal += 0.1 in double -- nothing, and nothing can: min == max only when
    every valid value is the same, and then value + offset is 0 and the byte 0
    whatever the constant; the 0.1 only keeps the division finite
  scale_apply_kernel's bytewise branch dropped (no tail, no unaligned
    store; the packed store itself left alone, so nothing misaligned is
    stored) -- (a) "auto all nodata" (15 elements) of every type, (b) from
    n = 1 at offset 0 on, 156 of the 168 (triple, n, offset) cases per type
"""
import ctypes as C
import functools

import numpy as np
import pytest

from gsky_amd import synth

from .helpers import gpu_batch
from .test_nn_rule import SRS, T0, bits, nn_gran, nn_tile, tile_reference
from .test_scale_rule import (EXTREMA, INT_TYPES, LEGACY_TYPES, datasets, expected, extrema_array, go_conv, is_auto,
                              params, scale_legacy_rule, scale_rule)

pytestmark = pytest.mark.gpu

PAL = synth.PALETTE_GSKY
TYPES = [np.dtype(t).name for t in INT_TYPES + (np.float32,)]
TNAME = {"uint8": "Byte", "int8": "SignedByte", "int16": "Int16", "uint16": "UInt16", "float32": "Float32"}
N_RAW = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)
GUARD = 0xA5
COUNTS = {}


def _count(path, n):
    COUNTS[path] = COUNTS.get(path, 0) + int(n)


def _show(what):
    print("\n[scale_edges] %s: pixels compared so far, no difference: %s"
          % (what, ", ".join("%s %d" % kv for kv in sorted(COUNTS.items()))))


def _first(bad):
    return "%d cases differ, the first: %r" % (len(bad), bad[:2])


def _dev(a, gpu):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).to(gpu)


def _sp(p):
    import gsky_amd
    return gsky_amd.ScaleParams(*p)


# ---------------------------------------------------------------- (a), (c), (d): the stage calls
@pytest.mark.parametrize("tname", TYPES)
def test_a_scale(gpu, tname):
    """(a) and (c): gsky_amd.scale() over the whole table."""
    import gsky_amd
    bad = []
    for k, (name, data, nd) in enumerate(datasets(np.dtype(tname))):
        for p in params(np.dtype(tname)):
            t = _dev(data, gpu)
            out = gsky_amd.scale([t], [nd], _sp(p))[0].cpu().numpy()
            exp = expected(tname, k, p)
            if not np.array_equal(out, exp):
                bad.append((name, p, int((out != exp).sum())))
            after = t.cpu().numpy()
            if not np.array_equal(bits(after), bits(exp if tname == "uint8" else data)):
                bad.append((name, p, "input after the call"))
            _count("(a) %s" % tname, data.size)
    assert not bad, _first(bad)
    _show("(a) " + tname)


@pytest.mark.parametrize("tname", [np.dtype(t).name for t in LEGACY_TYPES])
def test_d_scale_legacy(gpu, tname):
    """(d): gsky_amd.scale_legacy() over the table of its four types."""
    import gsky_amd
    bad = []
    for name, data, nd in datasets(np.dtype(tname)):
        for p in params(np.dtype(tname)):
            t = _dev(data, gpu)
            out = gsky_amd.scale_legacy(t, nd, _sp(p)).cpu().numpy()
            exp = scale_legacy_rule(data, nd, p[0], p[1], p[2])
            if not np.array_equal(out, exp):
                bad.append((name, p, int((out != exp).sum())))
            if not np.array_equal(bits(t.cpu().numpy()), bits(exp if tname == "uint8" else data)):
                bad.append((name, p, "input after the call"))
            _count("(d) %s" % tname, data.size)
    assert not bad, _first(bad)
    _show("(d) " + tname)


# ---------------------------------------------------------------- (b): the raw ABI
def _raw_scale(gpu, data, tname, nd, p, off):
    """gskyhip_scale with `out` `off` bytes past an aligned address; returns
    (band, guards untouched, the input after the call)."""
    import torch

    from gsky_amd import _lib, lib
    from gsky_amd.raster import TYPE_CODES
    n = data.size
    t = _dev(data, gpu)
    big = torch.full((n + 32,), GUARD, dtype=torch.uint8, device=gpu)
    assert big.data_ptr() % 4 == 0
    sp = _sp(p).c()
    rc = lib().gskyhip_scale(C.c_void_p(t.data_ptr()), TYPE_CODES[TNAME[tname]], n, float(nd), C.byref(sp),
                             C.c_void_p(big.data_ptr() + 8 + off), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(rc, "Scale")
    torch.cuda.synchronize()
    b = big.cpu().numpy()
    lo, hi = 8 + off, 8 + off + n
    return b[lo:hi], bool((b[:lo] == GUARD).all() and (b[hi:] == GUARD).all()), t.cpu().numpy()


def _raw_source(tname):
    """1025 elements of the type: its 'domain v0 nodata -999.0' set (float32:
    the boundaries of (0, 0, 1000)), nodata included."""
    want = "boundaries of (0.0, 0.0, 1000.0)" if tname == "float32" else "domain v0 nodata -999.0"
    name, data, nd = next(d for d in datasets(np.dtype(tname)) if d[0] == want)
    flat = data.reshape(-1)
    src = np.concatenate([flat[:500], flat[760:1285]])
    assert src.size == 1025
    assert (src == go_conv(nd, src.dtype)).any()
    return src, nd


@pytest.mark.parametrize("tname", TYPES)
def test_b_raw_abi_sizes_and_alignment(gpu, tname):
    """(b) and (c): every n of N_RAW at every `out` offset 0..3; the guard
    bytes around `out` stay as they were."""
    src, nd = _raw_source(tname)
    bad = []
    for p in ((0.0, 0.0, 1000.0, 0), (-5.0, 0.5, 300.0, 0), (0.0, 0.0, 0.0, 0)):
        for n in N_RAW:
            data = src[:n]
            exp = scale_rule(data, nd, *p)
            for off in range(4):
                got, guards, after = _raw_scale(gpu, data, tname, nd, p, off)
                if not np.array_equal(got, exp):
                    bad.append((p, n, off, "bytes", int((got != exp).sum())))
                if not guards:
                    bad.append((p, n, off, "guard bytes written"))
                if not np.array_equal(bits(after), bits(exp if tname == "uint8" else data)):
                    bad.append((p, n, off, "input after the call"))
                _count("(b) %s" % tname, n)
    assert not bad, _first(bad)
    _show("(b) " + tname)


@pytest.mark.parametrize("tname", ["int16", "float32"])
def test_b_raw_abi_auto_reduction(gpu, tname):
    """(b): auto mode with one minimum and one maximum, in different waves
    and blocks of scale_minmax_kernel's reduction."""
    bad = []
    for at_min, at_max in EXTREMA:
        d = extrema_array(np.dtype(tname).type, at_min, at_max)
        exp = scale_rule(d, -999.0, 0, 0, 0)
        got, guards, _ = _raw_scale(gpu, d, tname, -999.0, (0.0, 0.0, 0.0, 0), 1)
        if not np.array_equal(got, exp) or not guards:
            bad.append((at_min, at_max, int((got != exp).sum()), guards))
        _count("(b) auto %s" % tname, d.size)
    assert not bad, _first(bad)


# ---------------------------------------------------------------- (e)-(i): through render
def _cfg(name, granules, tiles, pairs, namespaces=("",)):
    return synth.SynthConfig(name, granules, SRS, tiles, pairs, list(namespaces), (0.0, 0.0, 1000.0, 0), PAL,
                             resample=0, mask=None)


def _assert_verbatim(cfg, sets):
    """The canvas of tile t is data set t, bit for bit -- but for pixels equal
    to float32(nodata), which the merge leaves at the canvas nodata (-0.0 under
    a nodata of 0.0) and the rule turns into 0xFF before it looks at them."""
    for t, (_, data, nd) in enumerate(sets):
        refs, merged = tile_reference(cfg, t)
        canvas = merged[0][0]
        assert refs[0].has.all() and canvas.shape == data.shape and canvas.dtype == data.dtype
        same = bits(canvas) == bits(data)
        if data.dtype == np.float32:
            with np.errstate(invalid="ignore"):
                hole = data == np.float32(nd)
            assert (same | hole).all() and (canvas[hole] == np.float32(nd)).all()
        else:
            assert same.all()


@functools.lru_cache(None)
def render_case(tname, complex_=False):
    """One batch per type: tile k is data set k of the table, under its own
    granule; complex_: every tile also stacks a 4 x 4 float32 granule of a
    namespace that is not rendered."""
    sets = datasets(np.dtype(tname))
    gs = [nn_gran(d, 1.0, 0.0, 0.0, nd, T0, "P%d" % k) for k, (_, d, nd) in enumerate(sets)]
    tiles = [nn_tile(d.shape[1], d.shape[0]) for _, d, _ in sets]
    pairs = [[k] for k in range(len(sets))]
    if complex_:
        assert tname != "float32"
        gs.append(nn_gran(np.ones((4, 4), np.float32), 1.0, 0.0, 0.0, -1.0, T0, "other", ns="other"))
        pairs = [[k, len(sets)] for k in range(len(sets))]
    cfg = _cfg("scale %s" % tname, gs, tiles, pairs)
    _assert_verbatim(cfg, sets)
    assert len({t[1:] for t in tiles}) > 3          # tiles of different sizes in one slot
    return cfg


@functools.lru_cache(None)
def _ramp(pal):
    from oracle import oracle as O
    return O.gradient_palette(PAL, True) if pal else None


@functools.lru_cache(None)
def expected_rgba(tname, k, p, pal):
    from oracle import oracle as O
    band = expected(tname, k, p)
    h, w = band.shape
    return O.encode_rgba([band], w, h, _ramp(pal))


def _compare(path, tname, got, p, pal, bad):
    for k, (name, data, _) in enumerate(datasets(np.dtype(tname))):
        exp = expected_rgba(tname, k, p, pal)
        h, w = data.shape
        if not np.array_equal(got[k, :h, :w], exp):
            bad.append((path, name, p, "palette" if pal else "grey", int((got[k, :h, :w] != exp).any(-1).sum())))
        _count(path, h * w)


def _batch(cfg, gpu):
    if not hasattr(cfg, "_scale_batch"):
        cfg._scale_batch = gpu_batch(cfg)
    return cfg._scale_batch


def _simple(b, tname):
    from gsky_amd import _lib
    from gsky_amd.raster import TYPE_CODES
    info = b.tile_info()
    return (info[:, 0] == 0).all() and (info[:, 1] == 0).all() and b.value_types == _lib.VT_BIT[TYPE_CODES[TNAME[tname]]]


@pytest.mark.parametrize("tname", TYPES)
def test_e_band_kernel_and_i_auto(gpu, oracle, tname):
    """(e): the nearest-neighbour band kernel, palette and grey, every
    non-auto parameter set; (i): the auto sets through the minmax fold and
    canvas_rgba_kernel."""
    import gsky_amd
    b = _batch(render_case(tname), gpu)
    assert b.typed
    pal = gsky_amd.Palette(PAL, True)
    bad = []
    for p in params(np.dtype(tname)):
        path = "(i) %s" % tname if is_auto(*p[:3]) else "(e) %s" % tname
        for use_pal in (True, False):
            got = b.render(_sp(p), pal if use_pal else None).cpu().numpy()
            assert b.status() == 0
            _compare(path, tname, got, p, use_pal, bad)
    assert _simple(b, tname)
    assert not bad, _first(bad)
    _show("(e) (i) " + tname)


@pytest.mark.parametrize("tname", TYPES)
def test_f_generic_typed_kernels(gpu, oracle, tname):
    """(f): batch.typed = False -- render_fast_t's scale_t<T>; the auto sets
    again take (i)'s kernels, from the generic dispatch."""
    import gsky_amd
    b = _batch(render_case(tname), gpu)
    pal = gsky_amd.Palette(PAL, True)
    bad = []
    b.typed = False
    try:
        for p in params(np.dtype(tname)):
            got = b.render(_sp(p), pal).cpu().numpy()
            assert b.status() == 0
            _compare("(f) %s" % tname, tname, got, p, True, bad)
        assert _simple(b, tname)
    finally:
        b.typed = True
    assert not bad, _first(bad)
    _show("(f) " + tname)


@pytest.mark.parametrize("tname", TYPES[:4])
def test_h_lds_kernel_bilinear(gpu, oracle, tname):
    """(h): resample = 1 on the 1:1 geometry -- render_lds_kernel's scale_t<T>
    for every integer type; the oracle's bilinear warp returns the granule
    itself, so the nearest-neighbour expectation holds."""
    import gsky_amd
    from gsky_amd.tiles import bbox_to_geot
    cfg = render_case(tname)
    O = oracle
    for g, (bb, w, h) in zip(cfg.granules, cfg.tiles):
        arr, bbox, _, _ = O.warp(O.make_granule(g.data, g.geot, g.nodata), O.crs(SRS), O.crs(SRS),
                                 bbox_to_geot(w, h, bb), w, h, 1)
        assert list(bbox) == [0, 0, w, h] and np.array_equal(bits(arr), bits(g.data))
    b = _batch(cfg, gpu)
    pal = gsky_amd.Palette(PAL, True)
    bad = []
    for p in params(np.dtype(tname)):
        if is_auto(*p[:3]):
            continue
        for use_pal in (True, False):
            got = b.render(_sp(p), pal if use_pal else None, resample=1).cpu().numpy()
            assert b.status() == 0
            _compare("(h) %s" % tname, tname, got, p, use_pal, bad)
    assert _simple(b, tname)
    assert not bad, _first(bad)
    _show("(h) " + tname)


@pytest.mark.parametrize("tname", TYPES[:4])
def test_h_general_kernel_scale_px(gpu, oracle, tname):
    """(h'): complex tiles -- render_general_kernel's render_band applies
    scale_px (S2) to integer canvases."""
    import gsky_amd
    b = _batch(render_case(tname, True), gpu)
    pal = gsky_amd.Palette(PAL, True)
    bad = []
    for p in params(np.dtype(tname)):
        got = b.render(_sp(p), pal).cpu().numpy()
        assert b.status() == 0
        _compare("(h') %s" % tname, tname, got, p, True, bad)
    info = b.tile_info()
    assert (info[:, 0] == 0).all() and (info[:, 1] == 1).all()
    assert not bad, _first(bad)
    _show("(h') " + tname)


@functools.lru_cache(None)
def rgb_case(tname):
    """Three namespaces: tile t stacks data sets 3t, 3t + 1, 3t + 2 of one
    shape as r, g, b -- different slices of the domain, different nodata."""
    sets = datasets(np.dtype(tname))
    big = [k for k, (_, d, _) in enumerate(sets) if d.shape == sets[0][1].shape]
    groups = [big[i:i + 3] for i in range(0, len(big) - 2, 3)]
    gs, tiles, pairs = [], [], []
    for grp in groups:
        pairs.append([])
        for k, ns in zip(grp, "rgb"):
            _, d, nd = sets[k]
            pairs[-1].append(len(gs))
            gs.append(nn_gran(d, 1.0, 0.0, 0.0, nd, T0, "P%d" % k, ns=ns))
        tiles.append(nn_tile(d.shape[1], d.shape[0]))
    assert len(groups) >= 4
    return _cfg("scale rgb %s" % tname, gs, tiles, pairs, namespaces=("r", "g", "b")), groups


@pytest.mark.parametrize("tname", TYPES)
def test_g_three_namespaces(gpu, oracle, tname):
    """(g): RGB -- render_fast_kernel<3>'s three scale_t<T>; the auto sets
    through canvas_rgba_kernel with three canvases."""
    cfg, groups = rgb_case(tname)
    b = _batch(cfg, gpu)
    bad = []
    for typed in (True, False):
        b.typed = typed
        for p in params(np.dtype(tname)):
            got = b.render(_sp(p), None).cpu().numpy()
            assert b.status() == 0
            for t, grp in enumerate(groups):
                bands = [expected(tname, k, p) for k in grp]
                h, w = bands[0].shape
                exp = oracle.encode_rgba(bands, w, h, None)
                if not np.array_equal(got[t, :h, :w], exp):
                    bad.append((typed, p, grp, int((got[t, :h, :w] != exp).any(-1).sum())))
                _count("(g) %s" % tname, h * w)
    b.typed = True
    info = b.tile_info()
    assert (info[:, 0] == 0).all() and (info[:, 1] == 0).all()
    assert not bad, _first(bad)
    _show("(g) " + tname)


# ---------------------------------------------------------------- (j): fuse.hip
FUSE_SETS = {"int16": ("domain v0 nodata -999.0",), "float32": ("boundaries of (0.0, 0.0, 1000.0)", "log set nodata -9999.0")}


@pytest.mark.parametrize("tname", sorted(FUSE_SETS))
def test_j_fuse_outer_scale_and_scaled_layer(gpu, oracle, tname):
    """(j): one uploaded layer canvas; every non-auto parameter set as
    gskyhip_fuse_render's outer scale (the layer unscaled) and, without a
    colour scale (the inner ScaleParams carry none), as the layer's own scale
    under gskyhip_fuse_layers, whose fused Byte canvas is then the band."""
    import torch

    import gsky_amd
    from gsky_amd import fusion
    pal = gsky_amd.Palette(PAL, True)
    bad = []
    for want in FUSE_SETS[tname]:
        k, (name, data, nd) = next((k, d) for k, d in enumerate(datasets(np.dtype(tname))) if d[0] == want)
        h, w = data.shape
        buf = np.zeros((1, 1, w * h * 4), np.uint8)
        buf[0, 0, : data.nbytes] = data.reshape(-1).view(np.uint8)
        cv = torch.from_numpy(buf).to(gpu)
        tiles = fusion.tile_table([(w, h)], gpu)
        for p in params(np.dtype(tname)):
            if is_auto(*p[:3]):
                continue
            plain = [fusion.LayerCanvases(cv, TNAME[tname], nd, gsky_amd.ScaleParams(0.0, 0.0, 0.0, 0))]
            rgba = fusion.render_fused_canvases(plain, tiles, 1, w, h, _sp(p), pal).cpu().numpy()
            if not np.array_equal(rgba[0], expected_rgba(tname, k, p, True)):
                bad.append(("outer", name, p, int((rgba[0] != expected_rgba(tname, k, p, True)).any(-1).sum())))
            _count("(j) outer %s" % tname, data.size)
            if p[3] == 0:
                scaled = [fusion.LayerCanvases(cv, TNAME[tname], nd, _sp(p))]
                out, post, _ = fusion.fuse_canvases(scaled, tiles, 1, w, h)
                got = out.cpu().numpy()[0, 0, : w * h].reshape(h, w)
                if post != "Byte" or not np.array_equal(got, expected(tname, k, p)):
                    bad.append(("layer", name, p, post, int((got != expected(tname, k, p)).sum())))
                _count("(j) layer %s" % tname, data.size)
        assert np.array_equal(cv.cpu().numpy(), buf)      # the layer canvas is never written
    assert not bad, _first(bad)
    _show("(j) " + tname)
