"""Cubic convolution resampling (GSKYHIP_RESAMPLE_CUBIC) on every code path
that takes it, against the rule in numpy fp64 (tests/test_cubic_rule.py).

The paths, and the call that reaches each:

  (i)   cubic_value (render_generic.h, warp_window_kernel)  batch.warp_windows(2)
  (ii)  render_cub_kernel (render_cub.h)   batch.render(sp, resample=2, rgba=False) and
        render_coverage(..., resample=2) on float32 granules without a mask layer
  (iii) the generic kernels (cub_fetch, render_common.h): batch.typed = False, and
        every integer type, RGBA, RGB, mask-layer and canvas=True call

cubic_value and cub_fetch are wrappers: the fp64 rule itself is cubic_rule()
(resample.h), with bilinear_rule() beside it for the fall-back; path (ii)
takes both for its border pixels and bil4_renorm() for its nodata fall-back.

Part A is the same-CRS geometry of test_bilinear_edges.py part A (EPSG:3857
on both sides, power-of-two geotransforms, every source coordinate exact in
fp64; `_rule` asserts it).  Part B reprojects EPSG:4326 -> EPSG:3857.

Bars: identical nodata mask with no pixel left out; (i) and (iii) float32
within 1 ulp_f32 of float32(rule); integers exact; (ii) (fp32 weights and
sums) within 1e-4 * M, M the largest |valid value| of the tile's granules.
The merge of several entries is tile_merger.go's (stack by geoStamp
descending; an entry older than the canvas fills holes only), in `_merge`.

Worst errors measured on an MI355X (every test prints its own; -s shows them):

  (i)   warp_windows       0 ulp on every case (bit-equal to float32(rule)); integers: no difference;
                           A8 (Int32 / UInt32 / Float64 sources, bilinear and cubic) 0 ulp
  (ii)  render_cub_kernel  A1 (quadratic) 0; A2 noise 1.17e-7 * M (1:2; 1.15e-7 at 1:1, 1.14e-7 at 2:1);
                           A3 1.09e-7; A5 two entries 1.47e-7; A6 NaN nodata 1.85e-7, no nodata
                           1.04e-7, NaN data 1.23e-7
  (iii) generic kernels    as (i), typed or not, canvases, RGBA, RGB and with the mask layer
  B                        (ii) 5.3e-4 of the bound, (iii) 1.6e-4 (EPSG:4326 -> 3857 rows are
                           exactly linear, so the transformer uses none of its 0.125 px)
"""
import numpy as np
import pytest

from gsky_amd import synth

from .helpers import gpu_batch
from .test_bilinear_edges import ND, PX, SRS, X0, Y0, _noise, _rule, _tile
from .test_cubic_rule import _coords, cubic_rule, quadratic, to_type

pytestmark = pytest.mark.gpu

CUBIC = 2
CUBIC_RTOL = 1e-4        # the project's resampling bar (BASELINE north_star)
TYPE_NAME = {np.float32: "Float32", np.uint8: "Byte", np.int8: "SignedByte", np.int16: "Int16", np.uint16: "UInt16"}
T0 = 1577836800.0


# ---------------------------------------------------------------- the reference
def _gran(data, ratio, left, top, nodata=ND, ts=T0, poly="P", ns=""):
    """A same-CRS granule whose pixels are `ratio` destination pixels wide,
    its top-left corner at destination pixel (left, top) of the part-A grid."""
    geot = [X0 + left * PX, ratio * PX, 0.0, Y0 - top * PX, 0.0, -ratio * PX]
    return synth.SynthGranule(np.ascontiguousarray(data), geot, SRS, nodata, ts, poly, ns)


def _fnv32a(s):
    h = 0x811C9DC5
    for c in s.encode():
        h = ((h ^ c) * 0x01000193) & 0xFFFFFFFF
    return h


def _isnd(a, nd):
    return np.isnan(a) if (a.dtype.kind == "f" and np.isnan(nd)) else a == nd


class _Ref:
    """The rule for one granule on one tile: `val` the window value in the
    granule's type (window fill where no sample is taken), `sample` the
    unrounded fp64 sample, `cub` the 16-tap pixels, `win` the window."""

    def __init__(self, g, tile):
        dt = g.data.dtype.type
        taps = g.data.view(np.uint8) if dt == np.int8 else g.data   # a signed byte is a byte to the sample
        self.sample, self.has, self.cub, self.win = cubic_rule(taps, g.nodata, g.geot, tile)
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


def _merge(granules, refs, masked=None):
    """RasterMerger.Run of one tile's entries (tile_merger.go:286-297, 47): the
    stack sorted by geoStamp descending (stable), each entry writing its
    samples that differ from the nodata -- all of them, or only into holes
    when it is older than the canvas."""
    order = sorted(range(len(granules)), key=lambda k: -(granules[k].timestamp + _fnv32a(granules[k].polygon)))
    nd = refs[0].nd
    val = np.full(refs[0].val.shape, nd)
    sample = np.zeros(val.shape)
    cts, modes = 0.0, []
    for k in order:
        fill = granules[k].timestamp < cts
        if not fill:
            cts = granules[k].timestamp
        take = ~_isnd(refs[k].val, nd)
        if masked is not None:
            take &= ~masked[k]
        if fill:
            take &= _isnd(val, nd)
        val[take] = refs[k].val[take]
        sample[take] = refs[k].sample[take]
        modes.append((fill, int(take.sum())))
    return val, sample, nd, max(r.big for r in refs), modes


class _Worst:
    def __init__(self, case):
        self.case, self.v = case, {}

    def add(self, path, err):
        if err.size:
            self.v[path] = max(self.v.get(path, 0.0), float(err.max()))

    def show(self):
        print("\n[cubic] %s: %s" % (self.case, ", ".join("%s %.3g" % kv for kv in sorted(self.v.items()))))


def _check(path, got, val, sample, nd, big, worst, where, fp32=False):
    """One raster against the rule: identical nodata mask and NaN set; then
    integers exact, float32 within 1 ulp of float32(rule) -- or, on the fp32
    path, within 1e-4 * big of the fp64 sample."""
    assert got.dtype == val.dtype and got.shape == val.shape, (path, where, got.dtype, got.shape)
    assert np.array_equal(_isnd(got, nd), _isnd(val, nd)), (path, where)
    v = ~_isnd(val, nd)
    if val.dtype.kind != "f":
        d = np.abs(got[v].astype(np.int64) - val[v].astype(np.int64))
        worst.add(path + " diff", d)
        assert not d.any(), (path, where, int(d.max()))
        return int(v.sum())
    assert np.array_equal(np.isnan(got) & v, np.isnan(val) & v), (path, where)
    v &= ~np.isnan(val)
    if fp32:
        err = np.abs(got[v].astype(np.float64) - sample[v]) / big
        worst.add(path + " /M", err)
        assert err.size == 0 or err.max() <= CUBIC_RTOL, (path, where, err.max())
    else:
        err = np.abs(got[v].astype(np.float64) - val[v].astype(np.float64)) / np.spacing(np.abs(val[v])).astype(np.float64)
        worst.add(path + " ulp", err)
        assert err.size == 0 or err.max() <= 1.0, (path, where, err.max())
    return int(v.sum())


def _canvas(cv, b, dt, k=0):
    """(n_tiles, max_h, max_w) typed view of namespace k's canvases."""
    n = b.max_h * b.max_w * np.dtype(dt).itemsize
    return cv.cpu().numpy()[:, k, :n].copy().view(dt).reshape(-1, b.max_h, b.max_w)


def _batch(case, granules, tiles, pairs, namespaces=("",), mask=None, scale=(0.0, 1.0, 0.0, 0), palette=None):
    cfg = synth.SynthConfig(case, granules, SRS, tiles, pairs, list(namespaces), scale, palette, resample=CUBIC,
                            mask=mask)
    return cfg, gpu_batch(cfg)


def _check_windows(b, granules, tiles, pairs, refs, worst, case):
    """Path (i): every pair's warped window."""
    wins = b.warp_windows(CUBIC)
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
            n += _check("(i)", arr.cpu().numpy(), r.val[sl], r.sample[sl], r.nd, r.big, worst, (case, t, gi))
    return n


def _run(case, granules, tiles, pairs, worst):
    """One single-namespace batch without a mask layer through (i), the typed
    canvases-only call ((ii) for float32) and the same call with typed = False
    ((iii)).  Returns (batch, refs per tile and entry, merged canvases per
    tile, the typed and the generic canvases)."""
    import gsky_amd
    cfg, b = _batch(case, granules, tiles, pairs)
    sp = gsky_amd.ScaleParams(*cfg.scale)
    dt = granules[0].data.dtype.type
    refs = [[_Ref(granules[gi], tiles[t]) for gi in pairs[t]] for t in range(len(tiles))]
    merged = [_merge([granules[gi] for gi in pairs[t]], refs[t]) for t in range(len(tiles))]
    _check_windows(b, granules, tiles, pairs, refs, worst, case)
    out = []
    for path, typed in (("(ii)" if dt == np.float32 else "(iii) typed", True), ("(iii)", False)):
        b.typed = typed
        cv = _canvas(b.render(sp, resample=CUBIC, rgba=False), b, dt)
        assert b.status() == 0
        for t, (_, w, h) in enumerate(tiles):
            val, sample, nd, big, _ = merged[t]
            _check(path, cv[t, :h, :w], val, sample, nd, big, worst, (case, t), fp32=path == "(ii)")
        out.append(cv)
    b.typed = True
    return b, refs, merged, out[0], out[1]


# ---------------------------------------------------------------- part A
# ratio (destination pixels per source pixel) and the sub-pixel shift of the
# granule's corner: source phases 1/2; 1/4 and 3/4; 1/4
PHASES = [(1.0, 0.5), (2.0, 0.0), (0.5, 0.125)]


@pytest.mark.parametrize("ratio,shift", PHASES, ids=["1to1", "up2", "down2"])
def test_quadratic(gpu, ratio, shift):
    """A1: a float32 quadratic, no nodata, a 24 x 20 granule inside a 64 x 48
    tile that does not start at the grid's origin."""
    data, _ = quadratic(20, 24)
    g = _gran(data, ratio, 7 + shift, 4 + shift, None)
    tile = _tile(64, 48, 2, 1)
    worst = _Worst("A1 ratio %g" % ratio)
    _, refs, _, _, _ = _run("A1 r%g" % ratio, [g], [tile], [[0]], worst)
    r = refs[0][0]
    assert r.win[0] == 5 and r.win[1] == 3 and r.cub.sum() >= 80
    worst.show()


def _noise_case(ratio, shift, seed=31):
    rng = np.random.default_rng(seed)
    nx, ny = int(round(56 / ratio)), int(round(40 / ratio))
    return _gran(_noise(rng, ny, nx, 0.02), ratio, 5 + shift, 3 + shift), _tile(64, 48, 2, 1)


@pytest.mark.parametrize("ratio,shift", PHASES, ids=["1to1", "up2", "down2"])
def test_noise(gpu, ratio, shift):
    """A2: noise in [-1000, 1000] with 2 % nodata: a wrong tap or weight moves
    a pixel by ~1e-1 * M.  At least half of the in-window pixels take the
    16-tap sample (the rule's own count), and more than half differ from the
    bilinear result of the same batch."""
    import gsky_amd
    g, tile = _noise_case(ratio, shift)
    worst = _Worst("A2 ratio %g" % ratio)
    b, refs, _, band, generic = _run("A2 r%g" % ratio, [g], [tile], [[0]], worst)
    r = refs[0][0]
    assert r.cub.sum() >= 0.5 * r.inwin.sum(), (int(r.cub.sum()), int(r.inwin.sum()))
    bil = _canvas(b.render(gsky_amd.ScaleParams(0.0, 1.0, 0.0, 0), resample=1, rgba=False), b, np.float32)
    _, w, h = tile
    assert ((band[0, :h, :w] != bil[0, :h, :w]) & r.inwin).sum() > 0.5 * r.inwin.sum()
    # fp32 weights against fp64: the band kernel served the typed call, not the generic kernels
    assert (band[0, :h, :w] != generic[0, :h, :w]).any()
    worst.show()


def test_kernel_shape_edges(gpu):
    """A3: a 520 x 9 tile (one 512-column block and 8 columns of the next, a
    row count below the 16-row band), granules of 3 x 3 and 4 x 4 pixels (no
    pixel, and one source cell, with all 16 taps), a granule overhanging all
    four tile edges, and a 17-row tile 65 columns wide."""
    rng = np.random.default_rng(32)
    granules = [_gran(_noise(rng, 14, 530, 0.02), 1.0, -3.5, -2.5),
                _gran(_noise(rng, 3, 3, 0.0), 4.0, 5.25, 3.5),
                _gran(_noise(rng, 4, 4, 0.0), 4.0, 5.25, 3.5),
                _gran(_noise(rng, 50, 60, 0.02), 1.0, -10.5, -8.5),
                _gran(_noise(rng, 30, 80, 0.02), 1.0, 1.25, 1.75)]
    tiles = [_tile(520, 9), _tile(40, 30), _tile(40, 30), _tile(40, 30), _tile(65, 17)]
    worst = _Worst("A3")
    _, refs, _, _, _ = _run("A3", granules, tiles, [[k] for k in range(5)], worst)
    assert refs[0][0].cub[:, 512:].any() and refs[0][0].cub[:, :512].any()
    assert refs[1][0].cub.sum() == 0 and refs[2][0].cub.sum() == 16 and refs[3][0].cub.sum() > 600
    worst.show()


def _steps(dt, rng):
    """Step edges between the type's extremes (the overshoot saturates), a
    few mid values and nodata pixels."""
    if dt == np.int8:         # as bytes: 0 / 255 are the signed bytes 0 / -1
        return _steps(np.uint8, rng).view(np.int8)
    lo, hi = (np.iinfo(dt).min, np.iinfo(dt).max)
    v = np.full((20, 24), lo, np.int64)
    v[:, 6:11] = hi
    v[8:13, :] = np.where(v[8:13, :] == hi, lo, hi)
    v[15:, 14:] = rng.integers(lo, hi + 1, (5, 10))
    v[v == 5] = 6
    v[3, 18] = v[17, 3] = 5
    return v.astype(dt)


INT_SCALES = {np.uint8: (0.0, 0.0, 250.0, 0), np.int8: (100.0, 0.0, 200.0, 0), np.int16: (20000.0, 0.0, 50000.0, 0),
              np.uint16: (0.0, 0.0, 60000.0, 0)}


@pytest.mark.parametrize("dt", [np.uint8, np.int8, np.int16, np.uint16])
def test_integer_types(gpu, dt):
    """A4: integer granules (generic kernels): floor(r + 0.5), the overshoot
    at a step between the type's extremes saturated, signed-byte taps as
    0..255; windows, typed canvases and RGBA through the palette, all exact.
    The RGBA equals utils.Scale + EncodePNG of the cubic canvas."""
    import gsky_amd
    from gsky_amd.raster import encode_rgba, scale
    rng = np.random.default_rng(33)
    data = _steps(dt, rng)
    granules = [_gran(data, 2.0, 7.0, 4.0, 5.0), _gran(data, 1.0, 7.5, 4.5, 5.0)]
    tiles = [_tile(64, 48, 2, 1), _tile(40, 30, 2, 1)]
    pairs = [[0], [1]]
    worst = _Worst("A4 %s" % np.dtype(dt).name)
    b, refs, merged, _, _ = _run("A4 %s" % np.dtype(dt).name, granules, tiles, pairs, worst)
    info = np.iinfo(np.uint8 if dt == np.int8 else dt)
    for t in range(2):   # the rule itself overshoots on these inputs
        r = refs[t][0]
        assert (r.sample[r.cub] < info.min - 0.5).any() and (r.sample[r.cub] > info.max + 0.5).any()
    sp, pal = gsky_amd.ScaleParams(*INT_SCALES[dt]), gsky_amd.Palette(synth.PALETTE_GSKY, True)
    for typed in (True, False):
        b.typed = typed
        rgba_only = b.render(sp, pal, resample=CUBIC).cpu().numpy().copy()
        rgba, cv = b.render(sp, pal, resample=CUBIC, canvas=True)
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


def _poly_pair():
    """Two polygon names, the first with the larger FNV-1a hash by more than a day of seconds."""
    names = sorted(("P%d" % k for k in range(8)), key=_fnv32a)
    assert _fnv32a(names[-1]) - _fnv32a(names[0]) > 10 * 86400
    return names[-1], names[0]


@pytest.mark.parametrize("newer_first", [True, False], ids=["fill", "overwrite"])
def test_merge_two_granules(gpu, newer_first):
    """A5: two overlapping float32 granules a day apart with 10 % nodata.  The
    stack is ordered by geoStamp (timestamp + polygon hash): with the newer
    granule first the older one fills its holes (fill mode), with the older
    first the newer overwrites it; both orders of the request's list."""
    rng = np.random.default_rng(34)
    hi, lo = _poly_pair()
    new = _gran(_noise(rng, 30, 40, 0.1), 1.0, 4.5, 3.5, ts=T0 + 86400.0, poly=hi if newer_first else lo)
    old = _gran(_noise(rng, 40, 30, 0.1), 1.0, 20.25, 6.75, ts=T0, poly=lo if newer_first else hi)
    tile = _tile(64, 48, 1, 2)
    worst = _Worst("A5 %s" % ("fill" if newer_first else "overwrite"))
    _, refs, merged, _, _ = _run("A5", [new, old], [tile, tile], [[0, 1], [1, 0]], worst)
    for t in range(2):
        modes = merged[t][4]
        assert [m[0] for m in modes] == ([False, True] if newer_first else [False, False])
        assert all(m[1] > 300 for m in modes)
        assert np.array_equal(merged[t][0], merged[0][0])
    both = ~_isnd(refs[0][0].val, ND) & ~_isnd(refs[0][1].val, ND)
    assert both.sum() > 300 and np.array_equal(merged[0][0][both], refs[0][0].val[both])   # the newer value wins
    worst.show()


def test_rgb_three_namespaces(gpu):
    """A5: one RGB render of three namespaces (dispatch_render_3): each
    canvas matches the rule, the RGBA equals Scale + EncodePNG of the canvases."""
    import gsky_amd
    from gsky_amd.raster import encode_rgba, scale
    rng = np.random.default_rng(35)
    granules = [_gran(_noise(rng, 24, 30, 0.02), 2.0, 2.0 + k, 1.0 + 0.5 * k, poly="P%d" % k, ns=ns)
                for k, ns in enumerate("rgb")]
    tile = _tile(64, 48, 1, 1)
    cfg, b = _batch("A5 rgb", granules, [tile], [[0, 1, 2]], namespaces=("r", "g", "b"),
                    scale=(1000.0, 0.0, 2000.0, 0))
    sp = gsky_amd.ScaleParams(*cfg.scale)
    worst = _Worst("A5 rgb")
    refs = [[_Ref(g, tile) for g in granules]]
    _check_windows(b, granules, [tile], [[0, 1, 2]], refs, worst, "A5 rgb")
    for typed in (True, False):
        b.typed = typed
        rgba, cv = b.render(sp, None, resample=CUBIC, canvas=True)
        assert b.status() == 0
        bands = []
        for k in range(3):
            r = refs[0][k]
            _check("(iii)", _canvas(cv, b, np.float32, k)[0], r.val, r.sample, r.nd, r.big, worst, (typed, k))
            bands.append(b.canvas_view(cv, 0, k, "Float32").clone().contiguous())
        exp = encode_rgba(scale(bands, [ND] * 3, sp, ["Float32"] * 3)).cpu().numpy()
        assert (exp[..., 3] > 0).any() and np.array_equal(rgba[0].cpu().numpy(), exp), typed
    worst.show()


@pytest.mark.parametrize("nodata,hole,p_nan", [(float("nan"), float("nan"), 0.0), (None, None, 0.0),
                                               (ND, ND, 0.01)], ids=["nan", "none", "nan_data"])
def test_nodata_variants(gpu, nodata, hole, p_nan):
    """A6: NaN nodata (a NaN tap hands the pixel to the bilinear rule); no
    nodata at all (only the edge fallback); NaN among the data under a finite
    nodata (it propagates through the 16 taps)."""
    rng = np.random.default_rng(36)
    granules, tiles = [], []
    for ratio, shift in PHASES[:2]:
        nx, ny = int(round(56 / ratio)), int(round(40 / ratio))
        v = _noise(rng, ny, nx, 0.0)
        if hole is not None:
            v[rng.random((ny, nx)) < 0.02] = hole
        if p_nan:
            v[rng.random((ny, nx)) < p_nan] = np.nan
        granules.append(_gran(v, ratio, 5 + shift, 3 + shift, nodata))
        tiles.append(_tile(64, 48, 2, 1))
    worst = _Worst("A6 nodata %r nan-data %g" % (nodata, p_nan))
    _, refs, merged, _, _ = _run("A6", granules, tiles, [[0], [1]], worst)
    for t in range(2):
        r = refs[t][0]
        assert r.cub.sum() >= 0.5 * r.inwin.sum()
        if nodata is None:
            assert r.cub.sum() > 0.7 * r.inwin.sum() and not _isnd(r.val[r.inwin & r.has], r.nd).any()
        if p_nan:
            assert np.isnan(merged[t][0]).sum() > 100
    worst.show()


def test_mask_layer(gpu):
    """A7: a piecewise-constant uint8 mask raster (value "00000001": bit 0)
    warped by the same cubic rule as the data: CC of a constant is that
    constant, so inside a piece the masked set is the piece's bit; across a
    step the rule's rounded sample decides.  Generic kernels (a mask layer
    has no band kernel)."""
    import gsky_amd
    rng = np.random.default_rng(37)
    ny, nx = 22, 30
    qa = np.zeros((ny, nx), np.uint8)
    qa[:, 10:20] = 1
    qa[8:15, :] += 2
    qa[16:, 22:] = 1
    data = _noise(rng, ny, nx, 0.02)
    granules = [_gran(data, 2.0, 2.0, 1.0), _gran(qa, 2.0, 2.0, 1.0, None, ns="qa")]
    tile = _tile(64, 48, 1, 1)
    mask = dict(id="qa", value="00000001", inclusive=False)
    cfg, b = _batch("A7", granules, [tile], [[0, 1]], mask=mask)
    sp = gsky_amd.ScaleParams(*cfg.scale)
    rd, rm = _Ref(granules[0], tile), _Ref(granules[1], tile)
    assert rd.win == rm.win
    masked = (rm.val & 1) > 0
    inside = np.zeros_like(masked)
    inside[3:13, 26:38] = True      # iX in 12..16, iY in 1..5: all 16 taps hold the value 1
    assert masked[inside & rd.inwin].all() and (masked & ~_isnd(rd.val, ND)).sum() > 300
    assert (~masked & ~_isnd(rd.val, ND)).sum() > 300
    val, sample, nd, big, _ = _merge([granules[0]], [rd], [masked])
    worst = _Worst("A7 mask")
    for typed in (True, False):
        b.typed = typed
        cv = _canvas(b.render(sp, resample=CUBIC, rgba=False), b, np.float32)
        assert b.status() == 0
        _check("(iii) mask", cv[0, :48, :64], val, sample, nd, big, worst, typed)
    worst.show()


@pytest.mark.parametrize("resample", [1, CUBIC], ids=["bilinear", "cubic"])
def test_promoted_source_types(gpu, monkeypatch, resample):
    """A8: Int32, UInt32 and Float64 bands, which the warp promotes to a
    float32 window (warp.go:339-343): the only samples whose taps are not of
    the window's type, read through load_dbl() by bilinear_value() and
    cubic_value() (path (i), warp_windows(1) and (2)).  One 8 x 8 granule per
    type with one nodata pixel off-centre on a 16 x 16 tile at 1:2: the rule
    itself yields pixels of all four kinds -- 16 taps, the nodata fall-back,
    the bilinear border, the -1 edge -- asserted before the GPU is asked.
    Values span each type's range (float32 holds none of them exactly).
    TileBatch has no name for a UInt32 tensor, so the test registers the
    library's type code for its duration.  Bar: path (i)'s."""
    import torch

    from gsky_amd import _lib, tiles as tiles_mod
    monkeypatch.setitem(tiles_mod.DTYPE_OF_TORCH, torch.uint32, _lib.UINT32)
    rng = np.random.default_rng(38)
    nd = 5.0
    datas = [rng.integers(-2 ** 31, 2 ** 31 - 1, (8, 8)).astype(np.int32),
             rng.integers(0, 2 ** 32 - 1, (8, 8)).astype(np.uint32), rng.uniform(-1000.0, 1000.0, (8, 8))]
    for d in datas:
        d[2, 5] = nd
    granules = [_gran(d, 2.0, 0.0, 0.0, nd, poly="P%d" % k) for k, d in enumerate(datas)]
    tile = _tile(16, 16)
    worst = _Worst("A8 promoted types, resample %d" % resample)
    refs = []
    for g in granules:
        sample, has, cub, win = cubic_rule(g.data, nd, g.geot, tile)
        sx, sy = _coords(g, tile)
        fx, fy = np.floor(sx - 0.5), np.floor(sy - 0.5)
        inside = ((fy >= 1) & (fy + 2 < 8))[:, None] & ((fx >= 1) & (fx + 2 < 8))[None, :]
        edge = (fy == -1)[:, None] | (fx == -1)[None, :]
        assert win == [0, 0, 16, 16] and has.all()
        assert cub.any() and (inside & ~cub).any() and (~inside & ~edge).any() and edge.any()
        if resample == 1:
            sample, has, _, win = _rule(g.data, nd, g.geot, tile)
        refs.append((np.where(has, sample.astype(np.float32), np.float32(nd)), sample))
        assert (refs[-1][0].astype(np.float64) != sample).any()   # the promotion rounds
    cfg = synth.SynthConfig("A8", granules, SRS, [tile] * 3, [[0], [1], [2]], [""], (0.0, 1.0, 0.0, 0), None,
                            resample=resample)
    wins = gpu_batch(cfg).warp_windows(resample)
    assert len(wins) == 3
    for k, (arr, bbox, tname, wnd) in enumerate(wins):
        val, sample = refs[k]
        assert tname == "Float32" and wnd == nd and bbox == [0, 0, 16, 16], (k, tname, wnd, bbox)
        big = float(np.abs(datas[k].astype(np.float64)).max())
        n = _check("(i)", arr.cpu().numpy(), val, sample, np.float32(nd), big, worst, (resample, datas[k].dtype))
        assert n == 256
    worst.show()


# ---------------------------------------------------------------- part B
def test_reprojected_plane(gpu):
    """B: EPSG:4326 -> EPSG:3857, config_c3 at 64-px granules (2 x 2 of
    them), a 128 x 128 coverage in 64 x 64 chunks through render_coverage.
    Every granule holds one global plane a + b * lon + c * lat and no nodata.
    Cubic convolution (and the bilinear rule with all four taps) reproduces a
    plane, so a pixel's value is the plane at its source coordinate, which
    the approximate transformer places within 0.125 source pixels (|dx| +
    |dy|, warp.go:219) of the exact inverse Mercator: the bound is 0.125 *
    (|b_px| + |c_px|), b_px / c_px the plane's slopes per source pixel, plus
    the float32 rounding of the taps and the sum: (ii) 16 ulp_f32(M) (20 fp32
    operations of at most 0.5 ulp on partial sums below 1.5625 M, the
    largest sum of |weights|), (iii) 2 ulp_f32(M) (taps and result rounded
    once).  Checked: every pixel at least 0.625 source pixels from an edge of
    the granule that holds it -- within 0.5 px of an edge (the outer one, or
    a seam: either neighbour samples up to 0.5 px past its edge) the
    bilinear rule drops the taps outside and returns the edge pixels'
    values, not the plane; 0.125 px is the transformer's share."""
    import torch

    import gsky_amd
    from gsky_amd import coverage
    n, out = 64, 128
    cfg = synth.config_c3(scale=n / 2048.0, chunk_px=64, grid=2, out_px=out)
    assert cfg.granules[0].data.shape == (n, n) and len(cfg.tiles) == 4 and len(cfg.granules) == 4
    a0, bl, cl = 10.0, 3.0, -2.0
    for g in cfg.granules:
        gt = g.geot
        lon = gt[0] + gt[1] * (np.arange(n) + 0.5)
        lat = gt[3] + gt[5] * (np.arange(n) + 0.5)
        g.data = (a0 + bl * lon[None, :] + cl * lat[:, None]).astype(np.float32)
        g.nodata = None
    gt0 = cfg.granules[0].geot
    b_px, c_px = abs(bl * gt0[1]), abs(cl * gt0[5])
    # the exact source position of every output pixel, and its distance to its granule's edges
    x0, y0, x1, y1 = cfg.bbox
    mx = x0 + (np.arange(out) + 0.5) * (x1 - x0) / out
    my = y1 - (np.arange(out) + 0.5) * (y1 - y0) / out
    lon, _ = synth.merc_inv(mx, 0.0 * mx)
    _, lat = synth.merc_inv(0.0 * my, my)
    plane = a0 + bl * lon[None, :] + cl * lat[:, None]
    px = (lon - 112.0) / gt0[1]
    py = (-10.0 - lat) / -gt0[5]
    dist = lambda p: np.minimum(p % n, n - p % n)
    ok = (dist(py) >= 0.625)[:, None] & (dist(px) >= 0.625)[None, :]
    assert ok.mean() > 0.9
    big = float(max(np.abs(g.data).max() for g in cfg.granules))
    ulp = float(np.spacing(np.float32(big)))
    chunks = coverage.chunk_requests(cfg.bbox, out, out, 64, 64)
    bt = gpu_batch(cfg)
    offs = coverage.band_offsets(chunks, 0, out)
    worst = _Worst("B plane")
    for path, typed, n_ulp in (("(ii)", True, 16), ("(iii)", False, 2)):
        bt.typed = typed
        band = torch.full((out, out), -1.0, dtype=torch.float32, device=bt.device)
        bt.render_coverage(gsky_amd.ScaleParams(*cfg.scale), band, offs, resample=CUBIC)
        assert bt.status() == 0
        got = band.cpu().numpy().astype(np.float64)
        assert not (got[ok] == np.float32(-1e10)).any()
        err = np.abs(got - plane)[ok]
        worst.add(path + " / bound", err / (0.125 * (b_px + c_px) + n_ulp * ulp))
        assert err.max() <= 0.125 * (b_px + c_px) + n_ulp * ulp, (path, err.max())
    worst.show()
