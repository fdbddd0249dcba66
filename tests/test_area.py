"""Area resampling (GSKYHIP_RESAMPLE_AVERAGE = 3, GSKYHIP_RESAMPLE_MODE = 4)
on every code path that takes it, against the rule in numpy fp64
(tests/test_area_rule.py).

The paths, and the call that reaches each:

  (i)   average_value / mode_value (render_generic.h, warp_window_kernel)  batch.warp_windows(3), (4)
  (ii)  render_avg_kernel (render_area.h)   batch.render(sp, resample=3, rgba=False) and
        render_coverage(..., resample=3) on float32 granules without a mask layer
  (iii) the generic kernels (area_fetch, render_common.h; warped_value on complex tiles):
        batch.typed = False, MODE, and every integer type, RGBA, RGB, mask-layer and
        canvas=True call

Part A is the same-CRS geometry of test_bilinear_edges.py part A with the
destination pixel a dyadic multiple of the 16 m source pixel: every source
coordinate, every u and v and every footprint bound is exact in fp64
(`area_grid` asserts the coordinates).  Source pixels per destination pixel:
1/2, 1 (aligned, and shifted by half a pixel), 2 aligned, 3.5 and 20 (the tap
cap: stride 3, 7 taps of weight 1 per axis).

Bars: identical nodata mask with no pixel left out; (i) and (iii) float32
within 1 ulp_f32 of float32(rule) and integers exact; (ii) (fp32 weights and
sums) within 1e-4 * M, M the largest |valid value| of the tile's granules
(CUBIC_RTOL of tests/test_cubic.py).  The mask-layer raster warps by nearest
neighbour.  The merge of several entries is `_merge` of tests/test_cubic.py.

Part B reprojects EPSG:4326 -> EPSG:3857 and EPSG:3577 (Albers, rotated
against the destination grid) -> EPSG:3857 at about 3 source pixels per
destination pixel; its bounds are derived in the tests' docstrings.

Worst errors measured on an MI355X (every test prints its own; -s shows them):

  (i)   warp_windows       AVERAGE and MODE: 0 ulp on every case (bit-equal to float32(rule));
                           integers: no difference
  (ii)  render_avg_kernel  A1 noise 9.44e-8 * M at 1:2, 0 at 1:1 aligned (one tap of weight 1),
                           8.14e-8 at 1:1 shifted, 6.10e-8 at 2:1, 6.77e-8 at 3.5:1, 6.92e-9 at 20:1
                           (the fp64 rule, rounded once); A2 NaN nodata 6.20e-8, no nodata 6.11e-8;
                           A3 two entries 6.10e-8; A4 window shapes 8.14e-8
  (iii) generic kernels    as (i), typed or not, canvases, RGBA, RGB, MODE, and with the mask layer
  B1    plane              of the bound: EPSG:4326 0.079 on all three paths; Albers 0.468 ((ii) 0.464)
  B2    quadratic          EPSG:4326 (rows exactly linear, the transformer uses none of its 0.125 px):
                           1.16e-4 absolute on (i) / (iii), 7.39e-4 on (ii), on values of 2e4 -- a
                           footprint off by one pixel would show as 0.7; Albers 10.2 absolute, 0.063
                           of the bound, on all three paths
"""
import numpy as np
import pytest

from gsky_amd import synth

from .helpers import gpu_batch
from .test_bilinear_edges import ND, PX, SRS, X0, Y0, _noise
from .test_cubic import INT_SCALES, T0, TYPE_NAME, _canvas, _check, _gran, _isnd, _merge, _poly_pair, _Worst
from .test_area_rule import AVERAGE, MODE, area_grid, area_points, half_extents
from .test_cubic_rule import _coords, to_type

pytestmark = pytest.mark.gpu


class _W(_Worst):
    def show(self):
        print("\n[area] %s: %s" % (self.case, ", ".join("%s %.3g" % kv for kv in sorted(self.v.items()))))


# ---------------------------------------------------------------- the reference
def _tile(w, h, spd=1.0, ox=0.0, oy=0.0):
    """A w x h tile whose pixels are `spd` source pixels (of PX metres) wide,
    its top-left at source pixel (ox, oy) of the part-A grid."""
    px = PX * spd
    x0, y1 = X0 + ox * PX, Y0 - oy * PX
    return ((x0, y1 - h * px, x0 + w * px, y1), w, h)


def _src(data, left, top, nodata=ND, ts=T0, poly="P", ns=""):
    """A granule of PX-metre pixels with its top-left corner at source pixel (left, top)."""
    return _gran(data, 1.0, left, top, nodata, ts, poly, ns)


class _Ref:
    """The rule for one granule on one tile: `val` the window value in the
    granule's type (window fill where no sample is taken), `sample` the
    unrounded fp64 sample, `win` the window, `hx` / `hy` the half extents."""

    def __init__(self, g, tile, mode=False):
        dt = g.data.dtype.type
        taps = g.data.view(np.uint8) if dt == np.int8 else g.data   # a signed byte is a byte to the sample
        self.sample, self.has, self.win, self.hx, self.hy = area_grid(taps, g.nodata, g.geot, tile, mode)
        nd = g.nodata if g.nodata is not None else -1e10
        self.nd = dt(nd) if dt == np.float32 else dt(np.clip(nd, np.iinfo(dt).min, np.iinfo(dt).max))
        with np.errstate(invalid="ignore"):
            self.val = np.where(self.has, to_type(self.sample, dt), self.nd)
        v = g.data[~_isnd(g.data, self.nd)].astype(np.float64)
        v = v[~np.isnan(v)]
        self.big = float(np.abs(v).max()) if v.size else 1.0
        x, y, w, h = self.win
        self.inwin = np.zeros(self.val.shape, bool)
        self.inwin[y:y + h, x:x + w] = True


def _batch(case, granules, tiles, pairs, namespaces=("",), mask=None, scale=(0.0, 1.0, 0.0, 0), palette=None,
           resample=AVERAGE):
    cfg = synth.SynthConfig(case, granules, SRS, tiles, pairs, list(namespaces), scale, palette, resample=resample,
                            mask=mask)
    return cfg, gpu_batch(cfg)


def _check_windows(b, granules, tiles, pairs, refs, worst, case, res=AVERAGE):
    """Path (i): every pair's warped window."""
    wins = b.warp_windows(res)
    assert len(wins) == sum(len(p) for p in pairs)
    p = n = 0
    for t in range(len(tiles)):
        for k, gi in enumerate(pairs[t]):
            arr, bbox, tname, nd = wins[p]
            p += 1
            r, g = refs[t][k], granules[gi]
            assert tname == TYPE_NAME[g.data.dtype.type] and bbox == r.win, (case, t, gi, bbox, r.win)
            assert nd == r.nd or (np.isnan(nd) and np.isnan(r.nd)), (case, t, gi, nd)
            x, y, w, h = r.win
            sl = (slice(y, y + h), slice(x, x + w))
            n += _check("(i) res %d" % res, arr.cpu().numpy(), r.val[sl], r.sample[sl], r.nd, r.big, worst,
                        (case, t, gi))
    return n


def _run(case, granules, tiles, pairs, worst, res=AVERAGE):
    """One single-namespace batch without a mask layer through (i), the typed
    canvases-only call ((ii) for float32 at AVERAGE) and the same call with
    typed = False ((iii)).  Returns (batch, refs per tile and entry, merged
    canvases per tile, the typed and the generic canvases)."""
    import gsky_amd
    cfg, b = _batch(case, granules, tiles, pairs, resample=res)
    sp = gsky_amd.ScaleParams(*cfg.scale)
    dt = granules[0].data.dtype.type
    refs = [[_Ref(granules[gi], tiles[t], res == MODE) for gi in pairs[t]] for t in range(len(tiles))]
    merged = [_merge([granules[gi] for gi in pairs[t]], refs[t]) for t in range(len(tiles))]
    _check_windows(b, granules, tiles, pairs, refs, worst, case, res)
    band = dt == np.float32 and res == AVERAGE
    out = []
    for path, typed in (("(ii)" if band else "(iii) typed", True), ("(iii)", False)):
        b.typed = typed
        cv = _canvas(b.render(sp, resample=res, rgba=False), b, dt)
        assert b.status() == 0
        for t, (_, w, h) in enumerate(tiles):
            val, sample, nd, big, _ = merged[t]
            _check(path, cv[t, :h, :w], val, sample, nd, big, worst, (case, t), fp32=path == "(ii)")
        out.append(cv)
    b.typed = True
    return b, refs, merged, out[0], out[1]


# ---------------------------------------------------------------- part A
# source pixels per destination pixel, and the granule's corner in source pixels
RATIOS = [(0.5, 5.0, 3.0), (1.0, 5.0, 3.0), (1.0, 5.5, 3.5), (2.0, 6.0, 4.0), (3.5, 10.5, 7.0), (20.0, 60.0, 40.0)]
RATIO_IDS = ["up2", "1to1", "1to1_half", "down2", "down3.5", "down20"]


def _noise_case(spd, left, top, seed=41, w=48, h=40):
    """A w x h tile at `spd` source pixels per pixel and a noise granule with
    15 % nodata that starts (left, top) source pixels inside it and ends
    inside it too."""
    rng = np.random.default_rng(seed)
    nx, ny = int(round((w - 12) * spd)), int(round((h - 10) * spd))
    return _src(_noise(rng, ny, nx, 0.15), left, top), _tile(w, h, spd)


@pytest.mark.parametrize("spd,left,top", RATIOS, ids=RATIO_IDS)
def test_noise(gpu, spd, left, top):
    """A1: noise in [-1000, 1000] with 15 % nodata at every ratio; the
    granule lies inside the tile, so the footprints of its edge pixels are
    clipped by the band on all four sides.  The typed call is served by the
    band kernel (its fp32 sums differ from the generic kernels' somewhere),
    render_coverage writes the same values, and beyond 2:1 more than half of
    the pixels differ from the bilinear result of the same batch."""
    import torch

    import gsky_amd
    w, h = (24, 20) if spd == 20.0 else (48, 40)
    g, tile = _noise_case(spd, left, top, w=w, h=h)
    worst = _W("A1 %g:1" % spd)
    b, refs, merged, band, generic = _run("A1 %g" % spd, [g], [tile], [[0]], worst)
    r = refs[0][0]
    exp_h = max(0.5, 0.5 * spd)
    assert (r.hx[r.inwin] == exp_h).all() and (r.hy[r.inwin] == exp_h).all()
    assert r.has.sum() > 0.6 * r.inwin.sum() and (~r.has & r.inwin).any()    # 15 % nodata leaves holes at the low ratios
    sp = gsky_amd.ScaleParams(0.0, 1.0, 0.0, 0)
    cov = torch.full((h, w), -1.0, dtype=torch.float32, device=b.device)
    b.render_coverage(sp, cov, [0], resample=AVERAGE)
    assert b.status() == 0
    assert np.array_equal(cov.cpu().numpy(), band[0, :h, :w], equal_nan=True)
    if spd > 2.0:   # (at an aligned 2:1 the bilinear sample is the 2 x 2 mean too)
        bil = _canvas(b.render(sp, resample=1, rgba=False), b, np.float32)
        assert ((band[0, :h, :w] != bil[0, :h, :w]) & r.has).sum() > 0.5 * r.has.sum()
    if 1.0 < spd <= 8.0:   # fractional or several taps in fp32: not the generic kernels' values everywhere
        assert (band[0, :h, :w] != generic[0, :h, :w]).any()
    # MODE on the same float data: windows and both canvases (generic kernels)
    _run("A1 mode %g" % spd, [g], [tile], [[0]], worst, MODE)
    worst.show()


@pytest.mark.parametrize("nodata,hole", [(float("nan"), float("nan")), (None, None)], ids=["nan", "none"])
def test_nodata_variants(gpu, nodata, hole):
    """A2: NaN nodata (NaN taps are dropped) and no nodata at all, at 2:1
    and 3.5:1."""
    rng = np.random.default_rng(42)
    granules, tiles = [], []
    for spd, left, top in RATIOS[3:5]:
        nx, ny = int(36 * spd), int(30 * spd)
        v = _noise(rng, ny, nx, 0.0)
        if hole is not None:
            v[rng.random((ny, nx)) < 0.15] = hole
        granules.append(_src(v, left, top, nodata))
        tiles.append(_tile(48, 40, spd))
    worst = _W("A2 nodata %r" % nodata)
    _, refs, merged, _, _ = _run("A2", granules, tiles, [[0], [1]], worst)
    for t in range(2):
        r = refs[t][0]
        assert r.has.sum() > 1000 and not np.isnan(merged[t][0][r.has]).any()
    worst.show()


@pytest.mark.parametrize("newer_first", [True, False], ids=["fill", "overwrite"])
def test_merge_two_granules(gpu, newer_first):
    """A3: two overlapping float32 granules a day apart with 15 % nodata at
    2:1, merged in both time orders and both orders of the request's list."""
    rng = np.random.default_rng(43)
    hi, lo = _poly_pair()
    new = _src(_noise(rng, 60, 80, 0.15), 8.0, 6.0, ts=T0 + 86400.0, poly=hi if newer_first else lo)
    old = _src(_noise(rng, 80, 60, 0.15), 40.0, 14.0, ts=T0, poly=lo if newer_first else hi)
    tile = _tile(64, 48, 2.0)
    worst = _W("A3 %s" % ("fill" if newer_first else "overwrite"))
    _, refs, merged, _, _ = _run("A3", [new, old], [tile, tile], [[0, 1], [1, 0]], worst)
    for t in range(2):
        modes = merged[t][4]
        assert [m[0] for m in modes] == ([False, True] if newer_first else [False, False])
        assert all(m[1] > 300 for m in modes)
        assert np.array_equal(merged[t][0], merged[0][0])
    both = ~_isnd(refs[0][0].val, ND) & ~_isnd(refs[0][1].val, ND)
    assert both.sum() > 300 and np.array_equal(merged[0][0][both], refs[0][0].val[both])   # the newer value wins
    worst.show()


def test_window_shapes(gpu):
    """A4: windows narrower than the tile; a window one pixel wide and one
    one pixel high (4:1, a granule a quarter of a destination pixel across:
    u, respectively v, falls back to zero and that half extent to 0.5); a 513
    x 5 tile, which crosses the band kernel's 512-column block and leaves
    ragged lanes in a band of fewer rows than a block; and a tile over the
    band's bottom-right corner, where footprints are clipped."""
    rng = np.random.default_rng(44)
    granules = [_src(_noise(rng, 30, 24, 0.15), 30.0, 12.0),          # 12 x 15 pixels of a 48 x 40 tile at 2:1
                _src(_noise(rng, 40, 1, 0.0), 20.75, 8.0),            # 4:1, one pixel wide, reaching the pixel centres' boxes
                _src(_noise(rng, 1, 60, 0.0), 8.0, 20.75),            # 4:1, one pixel high
                _src(_noise(rng, 14, 1040, 0.15), -6.0, -3.0),        # 2:1 under a 513 x 5 tile, overhanging it
                _src(_noise(rng, 50, 70, 0.15), -30.0, -21.0)]        # its corner at (40, 29) source pixels of tile 4
    tiles = [_tile(48, 40, 2.0), _tile(24, 20, 4.0), _tile(24, 20, 4.0), _tile(513, 5, 2.0), _tile(32, 24, 2.0)]
    worst = _W("A4")
    _, refs, _, _, _ = _run("A4", granules, tiles, [[k] for k in range(5)], worst)
    # (a window is the footprint plus the half-pixel round of warp.go:200-217: one more column and row)
    assert refs[0][0].win == [15, 6, 13, 16]
    assert refs[1][0].win == [5, 2, 1, 11] and refs[2][0].win == [2, 5, 16, 1]
    r1, r2 = refs[1][0], refs[2][0]
    assert (r1.hx[r1.inwin] == 0.5).all() and (r1.hy[r1.inwin] == 2.0).all() and r1.has.sum() == 10
    assert (r2.hx[r2.inwin] == 2.0).all() and (r2.hy[r2.inwin] == 0.5).all() and r2.has.sum() == 15
    assert refs[3][0].win == [0, 0, 513, 5] and refs[3][0].has[:, 512].any()
    assert refs[4][0].win == [0, 0, 21, 16] and refs[4][0].has[14, :20].any() and refs[4][0].has[:15, 19].any()
    worst.show()


def _classes(dt, rng, ny, nx):
    """A class map: 4 classes in patches of 3 x 3 source pixels with 10 % of
    single-pixel speckle and a few nodata (5) pixels."""
    vals = np.array({np.uint8: [10, 20, 30, 200], np.int16: [-300, 7, 1000, 32000]}[dt], dt)
    coarse = rng.integers(0, 4, (-(-ny // 3), -(-nx // 3)))
    v = np.repeat(np.repeat(coarse, 3, 0), 3, 1)[:ny, :nx]
    sp = rng.random((ny, nx)) < 0.1
    v = np.where(sp, rng.integers(0, 4, (ny, nx)), v)
    out = vals[v]
    out[rng.random((ny, nx)) < 0.03] = 5
    return out


@pytest.mark.parametrize("dt", [np.uint8, np.int16], ids=["byte", "int16"])
def test_mode_class_map(gpu, dt):
    """A5: MODE on class maps at 2:1 and 3.5:1: windows, typed and generic
    canvases, all exact; the result holds only the map's classes, and differs
    from the nearest-neighbour result somewhere (the speckle is voted out)."""
    import gsky_amd
    rng = np.random.default_rng(45)
    granules, tiles = [], []
    for spd, left, top in RATIOS[3:5]:
        granules.append(_src(_classes(dt, rng, int(30 * spd), int(36 * spd)), left, top, 5.0))
        tiles.append(_tile(48, 40, spd))
    worst = _W("A5 mode %s" % np.dtype(dt).name)
    b, refs, merged, typed, _ = _run("A5", granules, tiles, [[0], [1]], worst, MODE)
    nn = _canvas(b.render(gsky_amd.ScaleParams(0.0, 1.0, 0.0, 0), resample=0, rgba=False), b, dt)
    for t in range(2):
        r = refs[t][0]
        assert set(np.unique(r.val[r.has]).tolist()) <= set(np.unique(granules[t].data).tolist()) - {5}
        assert r.has.sum() > 1000 and ((typed[t, :40, :48] != nn[t, :40, :48]) & r.has).sum() > 20
    worst.show()


def _ramp(dt, rng, ny, nx):
    """Values over the whole range of the type (a signed byte as its byte), a
    few nodata (5) pixels."""
    if dt == np.int8:
        return _ramp(np.uint8, rng, ny, nx).view(np.int8)
    info = np.iinfo(dt)
    v = rng.integers(info.min, info.max + 1, (ny, nx)).astype(np.int64)
    v[:, : nx // 4] = info.max          # saturated plateaus: the mean of equal extremes is the extreme
    v[: ny // 4, :] = info.min
    v[v == 5] = 6
    v[rng.random((ny, nx)) < 0.1] = 5
    return v.astype(dt)


@pytest.mark.parametrize("dt", [np.uint8, np.int8, np.int16, np.uint16])
def test_integer_types(gpu, dt):
    """A6: integer granules (generic kernels) at AVERAGE, 2:1 and 3.5:1:
    floor(r + 0.5) saturated, signed-byte taps as 0..255; windows, typed
    canvases, canvas=True and RGBA through the palette, all exact.  The RGBA
    equals utils.Scale + EncodePNG of the averaged canvas."""
    import gsky_amd
    from gsky_amd.raster import encode_rgba, scale
    rng = np.random.default_rng(46)
    granules, tiles = [], []
    for spd, left, top in RATIOS[3:5]:
        granules.append(_src(_ramp(dt, rng, int(30 * spd), int(36 * spd)), left, top, 5.0))
        tiles.append(_tile(48, 40, spd))
    worst = _W("A6 %s" % np.dtype(dt).name)
    b, refs, merged, _, _ = _run("A6 %s" % np.dtype(dt).name, granules, tiles, [[0], [1]], worst)
    for t in range(2):   # rounding ties occur: a 2 x 2 mean ends in .5 for a quarter of the blocks
        r = refs[t][0]
        frac = r.sample[r.has] - np.floor(r.sample[r.has])
        assert (frac == 0.5).any() or t == 1
    sp, pal = gsky_amd.ScaleParams(*INT_SCALES[dt]), gsky_amd.Palette(synth.PALETTE_GSKY, True)
    for typed in (True, False):
        b.typed = typed
        rgba_only = b.render(sp, pal, resample=AVERAGE).cpu().numpy().copy()
        rgba, cv = b.render(sp, pal, resample=AVERAGE, canvas=True)
        assert b.status() == 0
        rgba = rgba.cpu().numpy()
        c = _canvas(cv, b, dt)
        for t, (_, w, h) in enumerate(tiles):
            val, sample, nd, big, _ = merged[t]
            _check("(iii) canvas", c[t, :h, :w], val, sample, nd, big, worst, (dt, typed, t))
            canvas = b.canvas_view(cv, t, 0, TYPE_NAME[dt])[:h, :w].clone().contiguous()
            u8 = scale([canvas], [5.0], sp, [TYPE_NAME[dt]])
            exp = encode_rgba(u8, pal).cpu().numpy()
            assert (exp[..., 3] > 0).any() and np.array_equal(rgba[t, :h, :w], exp), (dt, typed, t)
            assert np.array_equal(rgba_only[t, :h, :w], exp), (dt, typed, t)
    worst.show()


def test_rgb_three_namespaces(gpu):
    """A7: one RGB render of three namespaces (dispatch_render_3) at 2:1:
    each canvas matches the rule, the RGBA equals Scale + EncodePNG of the
    canvases; float32 RGBA with a palette of one namespace alongside."""
    import gsky_amd
    from gsky_amd.raster import encode_rgba, scale
    rng = np.random.default_rng(47)
    granules = [_src(_noise(rng, 60, 72, 0.15), 4.0 + 2 * k, 2.0 + k, poly="P%d" % k, ns=ns)
                for k, ns in enumerate("rgb")]
    tile = _tile(48, 40, 2.0)
    cfg, b = _batch("A7 rgb", granules, [tile], [[0, 1, 2]], namespaces=("r", "g", "b"),
                    scale=(1000.0, 0.0, 2000.0, 0))
    sp = gsky_amd.ScaleParams(*cfg.scale)
    worst = _W("A7 rgb")
    refs = [[_Ref(g, tile) for g in granules]]
    _check_windows(b, granules, [tile], [[0, 1, 2]], refs, worst, "A7 rgb")
    for typed in (True, False):
        b.typed = typed
        rgba, cv = b.render(sp, None, resample=AVERAGE, canvas=True)
        assert b.status() == 0
        bands = []
        for k in range(3):
            r = refs[0][k]
            _check("(iii)", _canvas(cv, b, np.float32, k)[0], r.val, r.sample, r.nd, r.big, worst, (typed, k))
            bands.append(b.canvas_view(cv, 0, k, "Float32").clone().contiguous())
        exp = encode_rgba(scale(bands, [ND] * 3, sp, ["Float32"] * 3)).cpu().numpy()
        assert (exp[..., 3] > 0).any() and np.array_equal(rgba[0].cpu().numpy(), exp), typed
    worst.show()


def _nearest(g, tile):
    """The nearest-neighbour warp of a granule on a same-CRS tile (warp.go:271-300)."""
    sx, sy = _coords(g, tile)
    ny, nx = g.data.shape
    ix, iy = np.floor(sx + 1e-10).astype(np.int64), np.floor(sy + 1e-10).astype(np.int64)
    okx, oky = (sx >= 0) & (ix < nx), (sy >= 0) & (iy < ny)
    v = g.data[np.clip(iy, 0, ny - 1)[:, None], np.clip(ix, 0, nx - 1)[None, :]]
    return v, oky[:, None] & okx[None, :]


@pytest.mark.parametrize("res", [AVERAGE, MODE], ids=["average", "mode"])
def test_mask_layer(gpu, res):
    """A8: a uint8 mask raster (value "00000001": bit 0) of single-pixel
    noise under float32 data at 2:1: the masked set is the nearest-warped
    mask's, bit for bit -- an averaged or voted bit field would differ at
    about half of the pixels -- and the data is the rule's.  Generic kernels
    (a mask layer has no band kernel)."""
    import gsky_amd
    rng = np.random.default_rng(48)
    ny, nx = 60, 72
    qa = rng.integers(0, 4, (ny, nx)).astype(np.uint8)
    data = _noise(rng, ny, nx, 0.15)
    granules = [_src(data, 4.0, 2.0), _src(qa, 4.0, 2.0, None, ns="qa")]
    tile = _tile(48, 40, 2.0)
    mask = dict(id="qa", value="00000001", inclusive=False)
    cfg, b = _batch("A8", granules, [tile], [[0, 1]], mask=mask, resample=res)
    sp = gsky_amd.ScaleParams(*cfg.scale)
    rd = _Ref(granules[0], tile, res == MODE)
    qv, qok = _nearest(granules[1], tile)
    masked = qok & ((qv & 1) > 0)
    rq = _Ref(granules[1], tile, res == MODE)       # what the mask would be under the data's rule
    assert rd.win == rq.win and ((((rq.val & 1) > 0) != masked) & rd.has).sum() > 200
    assert (masked & rd.has).sum() > 300 and (~masked & rd.has).sum() > 300
    val, sample, nd, big, _ = _merge([granules[0]], [rd], [masked])
    worst = _W("A8 mask res %d" % res)
    for typed in (True, False):
        b.typed = typed
        cv = _canvas(b.render(sp, resample=res, rgba=False), b, np.float32)
        assert b.status() == 0
        _check("(iii) mask", cv[0, :40, :48], val, sample, nd, big, worst, typed)
    worst.show()


# ---------------------------------------------------------------- part B
B_W = B_H = 32        # the tile
B_N = 400             # the granule, B_N x B_N pixels
FP32_ULPS = 64        # (ii): at most 5 x 5 taps, each weight, product and sum rounded once in fp32


def _reprojected(kind):
    """One granule and one EPSG:3857 tile of B_W x B_H pixels at about 3
    source pixels per pixel, centred on the granule; the exact fp64 source
    coordinates (pixel units, centres at +0.5) of every tile pixel from the
    published formulas of tests/test_warp_exact.py.  Returns (geot, srs, tile,
    SX, SY)."""
    from .test_warp_exact import albers, merc_inv
    if kind == "longlat":      # EPSG:4326 at 0.01 degree over lon 130..134, lat -22..-26
        res, lon_c, lat_c = 0.01, 132.0, -24.0
        geot, srs = [lon_c - 0.5 * B_N * res, res, 0.0, lat_c + 0.5 * B_N * res, 0.0, -res], "EPSG:4326"
        px = 3.0 * np.radians(res) * 6378137.0
        fwd = lambda lon, lat: (np.degrees(lon), np.degrees(lat))
    else:                      # EPSG:3577 at 1 km, 17 degrees east of the central meridian: rotated rows
        res, lon_c, lat_c = 1000.0, 149.0, -35.5
        xc, yc = albers(np.radians(lon_c), np.radians(lat_c))
        geot = [round(float(xc), -3) - 0.5 * B_N * res, res, 0.0, round(float(yc), -3) + 0.5 * B_N * res, 0.0, -res]
        srs = "EPSG:3577"
        px = 3.0 * res / np.cos(np.radians(lat_c))
        fwd = albers
    cx, cy = synth.merc_fwd(lon_c, lat_c)
    bb = (float(cx - 0.5 * B_W * px), float(cy - 0.5 * B_H * px), float(cx + 0.5 * B_W * px),
          float(cy + 0.5 * B_H * px))
    X = bb[0] + (np.arange(B_W) + 0.5) * ((bb[2] - bb[0]) / B_W)
    Y = bb[3] - (np.arange(B_H) + 0.5) * ((bb[3] - bb[1]) / B_H)
    lon, lat = merc_inv(*np.meshgrid(X, Y))
    ax, ay = fwd(lon, lat)
    return geot, srs, (bb, B_W, B_H), (ax - geot[0]) / geot[1], (ay - geot[3]) / geot[5]


def _render_b(kind, data, worst, check):
    """The granule `data` through warp_windows(3), the band kernel and the
    generic kernels; check(path, got (B_H x B_W float64), n_ulp) judges each."""
    import gsky_amd
    geot, srs, tile, SX, SY = _reprojected(kind)
    g = synth.SynthGranule(np.ascontiguousarray(data, np.float32), geot, srs, None, T0, "P")
    cfg = synth.SynthConfig("B " + kind, [g], "EPSG:3857", [tile], [[0]], [""], (0.0, 1.0, 0.0, 0), None,
                            resample=AVERAGE)
    b = gpu_batch(cfg)
    (arr, bbox, tname, _), = b.warp_windows(AVERAGE)
    assert tname == "Float32" and bbox == [0, 0, B_W, B_H]     # the window is the tile: no pixel is left out
    check("(i)", arr.cpu().numpy().astype(np.float64), 2)
    for path, typed, n_ulp in (("(ii)", True, FP32_ULPS), ("(iii)", False, 2)):
        b.typed = typed
        cv = _canvas(b.render(gsky_amd.ScaleParams(0.0, 1.0, 0.0, 0), resample=AVERAGE, rgba=False), b, np.float32)
        assert b.status() == 0
        got = cv[0, :B_H, :B_W].astype(np.float64)
        assert not (got == np.float32(-1e10)).any()
        check(path, got, n_ulp)


def _geometry_b(kind):
    """SX, SY, HX, HY of the exact transform, with the part's assertions: the
    ratio is about 3, the Albers rows are rotated, and every footprint -- at
    the exact half extents plus the transformer's share of 0.25 + 0.125 -- lies
    more than a pixel inside the granule."""
    _, _, _, SX, SY = _reprojected(kind)
    HX, HY = half_extents(SX, SY)
    assert 1.2 < HX.min() and HX.max() < 2.0 and 1.2 < HY.min() and HY.max() < 2.0, (HX.min(), HX.max(), HY.min(), HY.max())
    if kind == "albers":
        assert np.abs(np.diff(SY, axis=1)).min() > 0.1 and np.abs(np.diff(SX, axis=0)).min() > 0.1
    m = 1.0 + 0.375
    assert (SX - HX - m > 0).all() and (SX + HX + m < B_N).all() and (SY - HY - m > 0).all() and (SY + HY + m < B_N).all()
    return SX, SY, HX, HY


@pytest.mark.parametrize("kind", ["longlat", "albers"])
def test_reprojected_plane(gpu, kind):
    """B1: a plane f = a + b x + c y over the source pixel grid, no nodata.
    Along one axis the rule is the mean over [x0, x1] = [sx - hx, sx + hx] of
    the piecewise-constant function that holds f's pixel-centre value on each
    pixel.  Whole pixels contribute their true centroid; a partial pixel of
    covered length w contributes its centre, which lies (1 - w) / 2 off the
    centroid of its covered part, towards the outside.  So the sample is the
    plane at the box's centre plus b (wr (1 - wr) - wl (1 - wl)) / (4 hx) with
    wl, wr the covered lengths at the two ends: at most |b| / (16 hx) -- zero
    for a symmetric cut (wl = wr), which is the sense in which the symmetric
    box returns the centre's value.  The centre itself is the approximate
    transformer's, within 0.125 source pixels (|dx| + |dy|, warp.go:219) of
    the exact transform, worth 0.125 max(|b|, |c|) <= 0.125 (|b| + |c|); and
    each half extent moves by at most 0.25 (half of: two neighbours and twice
    the centre, 0.125 each), which enters only through the 1 / (16 h) term,
    taken at h - 0.25.  Bound: 0.125 (|b| + |c|) + |b| / (16 (hx - 0.25)) +
    |c| / (16 (hy - 0.25)) + n ulp_f32(M): n = 2 on (i) and (iii) (float32
    taps and one rounding of the result), FP32_ULPS on (ii)."""
    SX, SY, HX, HY = _geometry_b(kind)
    a0, bx, cy = 10.0, 3.0, -2.0
    yy, xx = np.mgrid[0:B_N, 0:B_N].astype(np.float64)
    data = (a0 + bx * (xx + 0.5) + cy * (yy + 0.5)).astype(np.float32)
    exact = a0 + bx * SX + cy * SY
    big = float(np.abs(data).max())
    ulp = float(np.spacing(np.float32(big)))
    bound = 0.125 * (abs(bx) + abs(cy)) + abs(bx) / (16.0 * (HX - 0.25)) + abs(cy) / (16.0 * (HY - 0.25))
    worst = _W("B1 plane %s" % kind)

    def check(path, got, n_ulp):
        err = np.abs(got - exact)
        worst.add(path + " / bound", err / (bound + n_ulp * ulp))
        assert (err <= bound + n_ulp * ulp).all(), (path, float((err / (bound + n_ulp * ulp)).max()))

    _render_b(kind, data, worst, check)
    worst.show()


@pytest.mark.parametrize("kind", ["longlat", "albers"])
def test_reprojected_quadratic(gpu, kind):
    """B2: f = (x - xc)^2 + (y - yc)^2 over the source pixel grid ((xc, yc)
    the granule's centre), no nodata, against the numpy rule at the exact
    fp64 transforms and their half extents (for a smooth f the rule gives f(s)
    + (hx^2 + hy^2) / 3).  f is separable, so the sample is the sum of two 1-D
    means, each the mean m over [x0, x1] of the piecewise-constant g holding
    f's pixel-centre values.  Two points a, b of the band have |g(a) - g(b)|
    <= G (|a - b| + 1), G the largest |f'| between them (their pixel centres
    are at most |a - b| + 1 apart).  Moving the ends to x0', x1' changes the
    mean by (int_x1^x1' (g - m) - int_x0^x0' (g - m)) / (x1' - x0'), at most
    (d0 + d1) G (L + d0 + d1 + 1) / L' with L = x1 - x0 = 2 hx, d0, d1 the
    moves and L' >= L - d0 - d1 the new length.  The GPU's centre is within
    0.125 of the exact one along an axis and its half extent within 0.25
    (test_reprojected_plane), so d0, d1 <= 0.375: per axis 0.75 G (2 h +
    1.75) / (2 h - 0.75), G = 2 (|s - c| + h + 1.375).  Plus n ulp_f32(M) as
    in B1.  The bound follows the transformer's tolerance, which at these
    gradients outweighs the footprint's own term (h^2 / 3): the measured
    error, printed as a share of the bound, is what shows the footprint."""
    SX, SY, HX, HY = _geometry_b(kind)
    c = 0.5 * B_N
    yy, xx = np.mgrid[0:B_N, 0:B_N].astype(np.float64)
    data = ((xx + 0.5 - c) ** 2 + (yy + 0.5 - c) ** 2).astype(np.float32)
    ref, has = area_points(data, None, SX, SY, HX, HY)
    assert has.all()
    smooth = (SX - c) ** 2 + (SY - c) ** 2 + (HX ** 2 + HY ** 2) / 3.0
    # the rule on the exact transform against the smooth value: the partial end pixels' |f'| / (16 h) of B1 per
    # axis, and 1 / 12 per axis for a whole pixel's centre value against its mean
    grad = lambda s, h: 2.0 * (np.abs(s - c) + h + 1.0)
    assert (np.abs(ref - smooth) <= grad(SX, HX) / (16.0 * HX) + grad(SY, HY) / (16.0 * HY) + 2.0 / 12.0).all()
    axis = lambda s, h: 0.75 * 2.0 * (np.abs(s - c) + h + 1.375) * (2.0 * h + 1.75) / (2.0 * h - 0.75)
    bound = axis(SX, HX) + axis(SY, HY)
    big = float(np.abs(data[int(SY.min()) - 3:int(SY.max()) + 4, int(SX.min()) - 3:int(SX.max()) + 4]).max())
    ulp = float(np.spacing(np.float32(big)))
    worst = _W("B2 quadratic %s" % kind)

    def check(path, got, n_ulp):
        err = np.abs(got - ref)
        worst.add(path + " / bound", err / (bound + n_ulp * ulp))
        worst.add(path + " abs", err)
        assert (err <= bound + n_ulp * ulp).all(), (path, float((err / (bound + n_ulp * ulp)).max()))

    _render_b(kind, data, worst, check)
    worst.show()
