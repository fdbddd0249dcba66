"""Cubic B-spline and Lanczos resampling (GSKYHIP_RESAMPLE_CUBICSPLINE = 5,
GSKYHIP_RESAMPLE_LANCZOS = 6) on every code path that takes them, against the
rule in numpy fp64 (tests/test_kernel_rule.py), after tests/test_cubic.py.

The paths, and the call that reaches each:

  (i)   kernel_value (render_generic.h, warp_window_kernel)  batch.warp_windows(code)
  (ii)  render_kern_kernel (render_kern.h)   batch.render(sp, resample=code, rgba=False) and
        render_coverage(..., resample=code) on float32 granules without a mask layer
  (iii) the generic kernels (kern_fetch, render_common.h): batch.typed = False, and
        every integer type, RGBA, RGB, mask-layer and canvas=True call

Part A is the same-CRS geometry of test_bilinear_edges.py part A (every source
coordinate exact in fp64).  Part B reprojects EPSG:4326 and EPSG:3577 (Albers)
to EPSG:3857.

Bars: identical nodata mask with no pixel left out.  (i) and (iii): float32
within 1 ulp_f32 of float32(rule) (the spline is a polynomial in the written
order, so bit-equal is expected; the device's fp64 sin and numpy's may differ
in the last place, which moves a Lanczos sample by about 1e-15 * M); integers
exact, but that under Lanczos a pixel of the kernel sum whose numpy sample
lies within 1e-9 * max(1, M) of k + 0.5 is left out, at most 0.1 % of a case's
compared pixels (the hand-over is bilinear_rule() itself, exact on a tie too).
(ii) (fp32 weights and sums): |got - sample| <= 1e-4 * M * S / accW, S = sum
|w| and accW = sum w of the surviving taps from the numpy rule -- the
project's 1e-4 resampling bar scaled by the sum's condition number (at most
2.75: test_kernel_rule.test_centre_condition_bounds; about 45 fp32 operations
of 2^-24 give about 2.7e-6 * M * S / accW); 1e-4 * M on the bilinear hand-over.
M is the largest |valid value| of the tile's granules.

Every test prints its worst errors (-s shows them); DESIGN.md 2 records them.
"""
import numpy as np
import pytest

from gsky_amd import synth

from .helpers import gpu_batch
from .test_bilinear_edges import ND, SRS, _noise, _tile
from .test_cubic import INT_SCALES, PHASES, T0, TYPE_NAME, _canvas, _fnv32a, _gran, _isnd, _poly_pair
from .test_cubic_rule import _coords, to_type
from .test_kernel_rule import LANCZOS, RADIUS, SPLINE, kernel_grid, plane_error
from .test_warp_exact import albers, merc_inv

pytestmark = pytest.mark.gpu

RTOL = 1e-4              # the project's resampling bar (BASELINE north_star)
TIE = 1e-9               # Lanczos integers: distance of the numpy sample to k + 0.5 that leaves a pixel out
CODES = [pytest.param(SPLINE, id="spline"), pytest.param(LANCZOS, id="lanczos")]
NAME = {SPLINE: "spline", LANCZOS: "lanczos"}


# ---------------------------------------------------------------- the reference
class _Ref:
    """The rule for one granule on one tile: `val` the window value in the
    granule's type (window fill where no sample is taken), `sample` the
    unrounded fp64 sample, `kern` the pixels of the kernel sum, `tol` the
    path-(ii) bound per unit of M, `win` the window."""

    def __init__(self, g, tile, code):
        dt = g.data.dtype.type
        taps = g.data.view(np.uint8) if dt == np.int8 else g.data   # a signed byte is a byte to the sample
        self.sample, self.has, self.kern, self.win, acc_w, s_abs = kernel_grid(taps, g.nodata, g.geot, tile, code)
        self.tol = np.where(self.kern, RTOL * s_abs / acc_w, RTOL)
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
    when it is older than the canvas.  Returns (val, sample, (tol, kern), nd, M,
    modes)."""
    order = sorted(range(len(granules)), key=lambda k: -(granules[k].timestamp + _fnv32a(granules[k].polygon)))
    nd = refs[0].nd
    val = np.full(refs[0].val.shape, nd)
    sample, tol = np.zeros(val.shape), np.full(val.shape, RTOL)
    kern = np.zeros(val.shape, bool)
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
        tol[take] = refs[k].tol[take]
        kern[take] = refs[k].kern[take]
        modes.append((fill, int(take.sum())))
    return val, sample, (tol, kern), nd, max(r.big for r in refs), modes


class _Worst:
    def __init__(self, case):
        self.case, self.v = case, {}

    def add(self, path, err):
        if np.size(err):
            self.v[path] = max(self.v.get(path, 0.0), float(np.max(err)))

    def show(self):
        print("\n[kernel] %s: %s" % (self.case, ", ".join("%s %.3g" % kv for kv in sorted(self.v.items()))))


def _check(path, code, got, val, sample, aux, nd, big, worst, where, fp32=False):
    """One raster against the rule (the module's bars); aux = (tol, kern)."""
    tol, kern = aux
    assert got.dtype == val.dtype and got.shape == val.shape, (path, where, got.dtype, got.shape)
    assert np.array_equal(_isnd(got, nd), _isnd(val, nd)), (path, where)
    v = ~_isnd(val, nd)
    if val.dtype.kind != "f":
        if code == LANCZOS:   # a kernel sum on a rounding tie may round either way (the hand-over is exact)
            tie = kern & (np.abs(sample - (np.floor(sample) + 0.5)) <= TIE * max(1.0, big))
            n_tie, n_all = int((tie & v).sum()), int(v.sum())
            worst.add(path + " ties", np.array([n_tie]))
            assert n_tie <= 0.001 * n_all, (path, where, n_tie, n_all)
            v &= ~tie
        d = np.abs(got[v].astype(np.int64) - val[v].astype(np.int64))
        worst.add(path + " diff", d)
        assert not d.any(), (path, where, int(d.max()))
        return int(v.sum())
    assert np.array_equal(np.isnan(got) & v, np.isnan(val) & v), (path, where)
    v &= ~np.isnan(val)
    if fp32:
        err = np.abs(got[v].astype(np.float64) - sample[v]) / big
        worst.add(path + " /M", err)
        worst.add(path + " /bound", err / tol[v])
        assert err.size == 0 or (err <= tol[v]).all(), (path, where, float((err / tol[v]).max()))
    else:
        err = np.abs(got[v].astype(np.float64) - val[v].astype(np.float64)) / np.spacing(np.abs(val[v])).astype(np.float64)
        worst.add(path + " ulp", err)
        assert err.size == 0 or err.max() <= 1.0, (path, where, err.max())
    return int(v.sum())


def _batch(case, code, granules, tiles, pairs, namespaces=("",), mask=None, scale=(0.0, 1.0, 0.0, 0), palette=None):
    cfg = synth.SynthConfig(case, granules, SRS, tiles, pairs, list(namespaces), scale, palette, resample=code,
                            mask=mask)
    return cfg, gpu_batch(cfg)


def _check_windows(b, code, granules, tiles, pairs, refs, worst, case):
    """Path (i): every pair's warped window."""
    wins = b.warp_windows(code)
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
            n += _check("(i)", code, arr.cpu().numpy(), r.val[sl], r.sample[sl], (r.tol[sl], r.kern[sl]), r.nd,
                        r.big, worst, (case, t, gi))
    return n


def _run(case, code, granules, tiles, pairs, worst):
    """One single-namespace batch without a mask layer through (i), the typed
    canvases-only call ((ii) for float32) and the same call with typed = False
    ((iii)).  Returns (batch, refs per tile and entry, merged canvases per
    tile, the typed and the generic canvases)."""
    import gsky_amd
    cfg, b = _batch(case, code, granules, tiles, pairs)
    sp = gsky_amd.ScaleParams(*cfg.scale)
    dt = granules[0].data.dtype.type
    refs = [[_Ref(granules[gi], tiles[t], code) for gi in pairs[t]] for t in range(len(tiles))]
    merged = [_merge([granules[gi] for gi in pairs[t]], refs[t]) for t in range(len(tiles))]
    _check_windows(b, code, granules, tiles, pairs, refs, worst, case)
    out = []
    for path, typed in (("(ii)" if dt == np.float32 else "(iii) typed", True), ("(iii)", False)):
        b.typed = typed
        cv = _canvas(b.render(sp, resample=code, rgba=False), b, dt)
        assert b.status() == 0
        for t, (_, w, h) in enumerate(tiles):
            val, sample, tol, nd, big, _ = merged[t]
            _check(path, code, cv[t, :h, :w], val, sample, tol, nd, big, worst, (case, t), fp32=path == "(ii)")
        out.append(cv)
    b.typed = True
    return b, refs, merged, out[0], out[1]


# ---------------------------------------------------------------- part A
def _noise_case(ratio, shift, seed, p_nd=0.15):
    """A granule 50 x 30 destination pixels large at (3, 2) + shift of a 48 x
    40 tile that starts at (2, 1): it overhangs the tile's right edge."""
    rng = np.random.default_rng(seed)
    nx, ny = int(round(50 / ratio)), int(round(30 / ratio))
    return _gran(_noise(rng, ny, nx, p_nd), ratio, 5 + shift, 3 + shift), _tile(48, 40, 2, 1)


@pytest.mark.parametrize("ratio,shift", PHASES, ids=["1to1", "up2", "down2"])
@pytest.mark.parametrize("code", CODES)
def test_noise(gpu, code, ratio, shift):
    """A2: noise in [-1000, 1000] with 15 % nodata.  A third of the in-window
    pixels or more take the kernel sum, others the hand-over; the band kernel
    served the typed call, and the kernel differs from bilinear."""
    import gsky_amd
    g, tile = _noise_case(ratio, shift, 61)
    worst = _Worst("A2 %s ratio %g" % (NAME[code], ratio))
    b, refs, _, band, generic = _run("A2 r%g" % ratio, code, [g], [tile], [[0]], worst)
    r = refs[0][0]
    assert r.kern.sum() >= 0.3 * r.inwin.sum(), (int(r.kern.sum()), int(r.inwin.sum()))
    assert (r.has & ~r.kern).sum() >= 20
    bil = _canvas(b.render(gsky_amd.ScaleParams(0.0, 1.0, 0.0, 0), resample=1, rgba=False), b, np.float32)
    _, w, h = tile
    assert ((band[0, :h, :w] != bil[0, :h, :w]) & r.kern).sum() > 0.5 * r.kern.sum()
    # fp32 weights against fp64: the band kernel served the typed call, not the generic kernels
    assert (band[0, :h, :w] != generic[0, :h, :w]).any()
    worst.show()


@pytest.mark.parametrize("nodata,hole", [(float("nan"), float("nan")), (None, None)], ids=["nan", "none"])
@pytest.mark.parametrize("code", CODES)
def test_nodata_variants(gpu, code, nodata, hole):
    """A6: NaN nodata (a NaN centre tap hands the pixel over, a NaN outer tap
    is dropped); no nodata at all (only the band's edge drops taps)."""
    rng = np.random.default_rng(62)
    granules, tiles = [], []
    for ratio, shift in PHASES[:2]:
        nx, ny = int(round(50 / ratio)), int(round(30 / ratio))
        v = _noise(rng, ny, nx, 0.0)
        if hole is not None:
            v[rng.random((ny, nx)) < 0.15] = hole
        granules.append(_gran(v, ratio, 5 + shift, 3 + shift, nodata))
        tiles.append(_tile(48, 40, 2, 1))
    worst = _Worst("A6 %s nodata %r" % (NAME[code], nodata))
    _, refs, _, _, _ = _run("A6", code, granules, tiles, [[0], [1]], worst)
    for t in range(2):
        r = refs[t][0]
        assert r.kern.sum() >= 0.3 * r.inwin.sum()
        if nodata is None:
            assert r.kern.sum() > 0.8 * r.inwin.sum() and not _isnd(r.val[r.inwin & r.has], r.nd).any()
    worst.show()


@pytest.mark.parametrize("newer_first", [True, False], ids=["fill", "overwrite"])
@pytest.mark.parametrize("code", CODES)
def test_merge_two_granules(gpu, code, newer_first):
    """A5: two overlapping float32 granules a day apart with 15 % nodata, in
    both time orders and both orders of the request's list."""
    rng = np.random.default_rng(63)
    hi, lo = _poly_pair()
    new = _gran(_noise(rng, 26, 30, 0.15), 1.0, 2.5, 1.5, ts=T0 + 86400.0, poly=hi if newer_first else lo)
    old = _gran(_noise(rng, 30, 24, 0.15), 1.0, 16.25, 4.75, ts=T0, poly=lo if newer_first else hi)
    tile = _tile(48, 40, 1, 2)
    worst = _Worst("A5 %s %s" % (NAME[code], "fill" if newer_first else "overwrite"))
    _, refs, merged, _, _ = _run("A5", code, [new, old], [tile, tile], [[0, 1], [1, 0]], worst)
    for t in range(2):
        modes = merged[t][5]
        assert [m[0] for m in modes] == ([False, True] if newer_first else [False, False])
        assert all(m[1] > 100 for m in modes)
        assert np.array_equal(merged[t][0], merged[0][0])
    both = ~_isnd(refs[0][0].val, ND) & ~_isnd(refs[0][1].val, ND)
    assert both.sum() > 100 and np.array_equal(merged[0][0][both], refs[0][0].val[both])   # the newer value wins
    worst.show()


@pytest.mark.parametrize("code", CODES)
def test_kernel_shape_edges(gpu, code):
    """A3: a window one pixel wide and one one pixel high (a granule reaching a
    quarter pixel into the tile), a 513 x 5 tile (one 512-column block and one
    column of the next, fewer rows than a band), and granules of 2 x 2 and 3 x
    3 pixels (one source cell, and four, with a centre 2 x 2)."""
    rng = np.random.default_rng(64)
    granules = [_gran(_noise(rng, 30, 30, 0.15), 1.0, -29.75, 2.5),
                _gran(_noise(rng, 30, 30, 0.15), 1.0, 3.5, -29.75),
                _gran(_noise(rng, 12, 520, 0.15), 1.0, -3.5, -2.5),
                _gran(_noise(rng, 2, 2, 0.0), 4.0, 5.25, 3.5),
                _gran(_noise(rng, 3, 3, 0.0), 4.0, 5.25, 3.5)]
    tiles = [_tile(48, 40), _tile(48, 40), _tile(513, 5), _tile(40, 30), _tile(40, 30)]
    worst = _Worst("A3 %s" % NAME[code])
    _, refs, _, _, _ = _run("A3", code, granules, tiles, [[k] for k in range(5)], worst)
    assert refs[0][0].win[2] == 1 and refs[1][0].win[3] == 1
    assert refs[2][0].kern[:, 512:].any() and refs[2][0].kern[:, :512].any()
    assert refs[3][0].kern.sum() == 16 and refs[4][0].kern.sum() == 64
    worst.show()


def _int_noise(dt, rng, ny, nx, nd=5):
    """Integer noise over the type's whole range with 15 % nodata (a signed
    byte as the byte the sample sees, wrapped)."""
    if dt == np.int8:
        return _int_noise(np.uint8, rng, ny, nx, nd).view(np.int8)
    info = np.iinfo(dt)
    v = rng.integers(info.min, info.max + 1, (ny, nx))
    v[v == nd] = nd + 1
    v[rng.random((ny, nx)) < 0.15] = nd
    return v.astype(dt)


@pytest.mark.parametrize("dt", [np.uint8, np.int8, np.int16, np.uint16])
@pytest.mark.parametrize("code", CODES)
def test_integer_types(gpu, code, dt):
    """A4: integer granules (generic kernels) of noise over the type's whole
    range: floor(r + 0.5), saturation (Lanczos overshoots the range; the
    spline, a convex combination, never does), signed-byte taps as 0..255;
    windows, typed canvases and RGBA through the palette.  The RGBA equals
    utils.Scale + EncodePNG of the canvas."""
    import gsky_amd
    from gsky_amd.raster import encode_rgba, scale
    rng = np.random.default_rng(65)
    granules = [_gran(_int_noise(dt, rng, 20, 24), 2.0, 7.0, 4.0, 5.0),
                _gran(_int_noise(dt, rng, 20, 24), 1.0, 7.5, 4.5, 5.0)]
    tiles = [_tile(48, 40, 2, 1), _tile(40, 30, 2, 1)]
    pairs = [[0], [1]]
    worst = _Worst("A4 %s %s" % (NAME[code], np.dtype(dt).name))
    b, refs, merged, _, _ = _run("A4 %s" % np.dtype(dt).name, code, granules, tiles, pairs, worst)
    info = np.iinfo(np.uint8 if dt == np.int8 else dt)
    for t in range(2):
        r = refs[t][0]
        over = (r.sample[r.kern] < info.min - 0.5).any() or (r.sample[r.kern] > info.max + 0.5).any()
        assert over == (code == LANCZOS), (t, over)
    sp, pal = gsky_amd.ScaleParams(*INT_SCALES[dt]), gsky_amd.Palette(synth.PALETTE_GSKY, True)
    for typed in (True, False):
        b.typed = typed
        rgba_only = b.render(sp, pal, resample=code).cpu().numpy().copy()
        rgba, cv = b.render(sp, pal, resample=code, canvas=True)
        assert b.status() == 0
        rgba = rgba.cpu().numpy()
        c = _canvas(cv, b, dt)
        for t, (_, w, h) in enumerate(tiles):
            val, sample, tol, nd, big, _ = merged[t]
            _check("(iii) canvas", code, c[t, :h, :w], val, sample, tol, nd, big, worst, (dt, typed, t))
            canvas = b.canvas_view(cv, t, 0, TYPE_NAME[dt])[:h, :w].clone().contiguous()
            u8 = scale([canvas], [5.0], sp, [TYPE_NAME[dt]])
            exp = encode_rgba(u8, pal).cpu().numpy()
            assert (exp[..., 3] > 0).any() and np.array_equal(rgba[t, :h, :w], exp), (dt, typed, t)
            assert np.array_equal(rgba_only[t, :h, :w], exp), (dt, typed, t)
    worst.show()


@pytest.mark.parametrize("code", CODES)
def test_rgb_three_namespaces(gpu, code):
    """One RGB render of three namespaces (dispatch_render_3): each canvas
    matches the rule, the RGBA equals Scale + EncodePNG of the canvases."""
    import gsky_amd
    from gsky_amd.raster import encode_rgba, scale
    rng = np.random.default_rng(66)
    granules = [_gran(_noise(rng, 18, 22, 0.15), 2.0, 2.0 + k, 1.0 + 0.5 * k, poly="P%d" % k, ns=ns)
                for k, ns in enumerate("rgb")]
    tile = _tile(48, 40, 1, 1)
    cfg, b = _batch("A5 rgb", code, granules, [tile], [[0, 1, 2]], namespaces=("r", "g", "b"),
                    scale=(1000.0, 0.0, 2000.0, 0))
    sp = gsky_amd.ScaleParams(*cfg.scale)
    worst = _Worst("A5 %s rgb" % NAME[code])
    refs = [[_Ref(g, tile, code) for g in granules]]
    _check_windows(b, code, granules, [tile], [[0, 1, 2]], refs, worst, "A5 rgb")
    for typed in (True, False):
        b.typed = typed
        rgba, cv = b.render(sp, None, resample=code, canvas=True)
        assert b.status() == 0
        bands = []
        for k in range(3):
            r = refs[0][k]
            _check("(iii)", code, _canvas(cv, b, np.float32, k)[0], r.val, r.sample, (r.tol, r.kern), r.nd, r.big, worst,
                   (typed, k))
            bands.append(b.canvas_view(cv, 0, k, "Float32").clone().contiguous())
        exp = encode_rgba(scale(bands, [ND] * 3, sp, ["Float32"] * 3)).cpu().numpy()
        assert (exp[..., 3] > 0).any() and np.array_equal(rgba[0].cpu().numpy(), exp), typed
    worst.show()


@pytest.mark.parametrize("code", CODES)
def test_mask_layer(gpu, code):
    """A7: a uint8 mask raster of single-pixel noise (value "00000001": bit 0).
    Under both rules the mask warps by nearest neighbour (mask_res(),
    resample.h), so the masked set is the nearest-warped mask's, bit for bit:
    a convolved mask would differ at almost every pixel.  Generic kernels (a
    mask layer has no band kernel)."""
    import gsky_amd
    rng = np.random.default_rng(67)
    ny, nx = 18, 22
    qa = rng.integers(0, 4, (ny, nx)).astype(np.uint8)
    data = _noise(rng, ny, nx, 0.15)
    granules = [_gran(data, 2.0, 2.0, 1.0), _gran(qa, 2.0, 2.0, 1.0, None, ns="qa")]
    tile = _tile(48, 40, 1, 1)
    mask = dict(id="qa", value="00000001", inclusive=False)
    cfg, b = _batch("A7", code, granules, [tile], [[0, 1]], mask=mask)
    sp = gsky_amd.ScaleParams(*cfg.scale)
    rd = _Ref(granules[0], tile, code)
    # the nearest-neighbour rule (warp.go:271-300) on the part-A geometry
    sx, sy = _coords(granules[1], tile)
    okx, oky = (sx >= 0) & (sx + 1e-10 < nx), (sy >= 0) & (sy + 1e-10 < ny)
    ix, iy = np.where(okx, sx + 1e-10, 0).astype(np.int64), np.where(oky, sy + 1e-10, 0).astype(np.int64)
    near = np.where(oky[:, None] & okx[None, :] & rd.inwin, qa[iy[:, None], ix[None, :]], 0)
    masked = (near & 1) > 0
    valid = ~_isnd(rd.val, ND)
    assert (masked & valid).sum() > 200 and (~masked & valid).sum() > 200
    val, sample, tol, nd, big, _ = _merge([granules[0]], [rd], [masked])
    worst = _Worst("A7 %s mask" % NAME[code])
    for typed in (True, False):
        b.typed = typed
        cv = _canvas(b.render(sp, resample=code, rgba=False), b, np.float32)
        assert b.status() == 0
        _check("(iii) mask", code, cv[0, :40, :48], val, sample, tol, nd, big, worst, typed)
    worst.show()


@pytest.mark.parametrize("code", CODES)
def test_promoted_source_types(gpu, monkeypatch, code):
    """A8: Int32, UInt32 and Float64 bands, which the warp promotes to a
    float32 window (warp.go:339-343): taps read through load_dbl() by
    kernel_value() (path (i)).  One 8 x 8 granule per type with one nodata
    pixel on a 16 x 16 tile at 1:2."""
    import torch

    from gsky_amd import _lib, tiles as tiles_mod
    monkeypatch.setitem(tiles_mod.DTYPE_OF_TORCH, torch.uint32, _lib.UINT32)
    rng = np.random.default_rng(68)
    nd = 5.0
    datas = [rng.integers(-2 ** 31, 2 ** 31 - 1, (8, 8)).astype(np.int32),
             rng.integers(0, 2 ** 32 - 1, (8, 8)).astype(np.uint32), rng.uniform(-1000.0, 1000.0, (8, 8))]
    for d in datas:
        d[2, 5] = nd
    granules = [_gran(d, 2.0, 0.0, 0.0, nd, poly="P%d" % k) for k, d in enumerate(datas)]
    tile = _tile(16, 16)
    worst = _Worst("A8 %s promoted types" % NAME[code])
    refs = []
    for g in granules:
        sample, has, kern, win, acc_w, s_abs = kernel_grid(g.data, nd, g.geot, tile, code)
        assert win == [0, 0, 16, 16] and has.all() and kern.any() and (~kern).any()
        refs.append((np.where(has, sample.astype(np.float32), np.float32(nd)), sample,
                     (np.where(kern, RTOL * s_abs / acc_w, RTOL), kern)))
        assert (refs[-1][0].astype(np.float64) != sample).any()   # the promotion rounds
    cfg = synth.SynthConfig("A8", granules, SRS, [tile] * 3, [[0], [1], [2]], [""], (0.0, 1.0, 0.0, 0), None,
                            resample=code)
    wins = gpu_batch(cfg).warp_windows(code)
    assert len(wins) == 3
    for k, (arr, bbox, tname, wnd) in enumerate(wins):
        val, sample, tol = refs[k]
        assert tname == "Float32" and wnd == nd and bbox == [0, 0, 16, 16], (k, tname, wnd, bbox)
        big = float(np.abs(datas[k].astype(np.float64)).max())
        n = _check("(i)", code, arr.cpu().numpy(), val, sample, tol, np.float32(nd), big, worst, datas[k].dtype)
        assert n == 256
    worst.show()


def test_bad_codes_are_argument_errors(gpu):
    """Codes 7 and -1 return GSKYHIP_E_ARG from gskyhip_render_tiles and
    gskyhip_warp_windows."""
    import gsky_amd
    from gsky_amd._lib import GskyError
    g, tile = _noise_case(1.0, 0.5, 69)
    cfg, b = _batch("E", SPLINE, [g], [tile], [[0]])
    sp = gsky_amd.ScaleParams(*cfg.scale)
    for bad in (7, -1):
        for call in (lambda: b.render(sp, resample=bad, rgba=False), lambda: b.warp_windows(bad)):
            with pytest.raises(GskyError) as ei:
                call()
            assert ei.value.code == -1


# ---------------------------------------------------------------- part B
def _plane_bound(code, b_px, c_px, n_ulp, big):
    """(0.125 + e_K) (|b| + |c|) + n_ulp ulp_f32(M): 0.125 px is the approximate
    transformer's tolerance (warp.go:219), e_K the rule's own error on a plane
    of unit slope (the numpy rule on a grid of phases: about 2e-16 for the
    spline, about 0.020 px for Lanczos), the last term the float32 rounding of
    taps and sums."""
    return (0.125 + plane_error(code)) * (b_px + c_px) + n_ulp * float(np.spacing(np.float32(big)))


@pytest.mark.parametrize("code", CODES)
def test_reprojected_plane_longlat(gpu, code):
    """B: EPSG:4326 -> EPSG:3857, config_c3 at 64-px granules (2 x 2 of them),
    a 128 x 128 coverage in 64 x 64 chunks through render_coverage.  Every
    granule holds one global plane a + b * lon + c * lat and no nodata; checked
    are the pixels whose taps all lie inside the granule that holds them (R +
    0.625 source pixels from its edges), against the plane at the exact fp64
    inverse Mercator of the pixel centre."""
    import torch

    import gsky_amd
    from gsky_amd import coverage
    n, out, R = 64, 128, RADIUS[code]
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
    x0, y0, x1, y1 = cfg.bbox
    mx = x0 + (np.arange(out) + 0.5) * (x1 - x0) / out
    my = y1 - (np.arange(out) + 0.5) * (y1 - y0) / out
    lon, _ = synth.merc_inv(mx, 0.0 * mx)
    _, lat = synth.merc_inv(0.0 * my, my)
    plane = a0 + bl * lon[None, :] + cl * lat[:, None]
    px = (lon - 112.0) / gt0[1]
    py = (-10.0 - lat) / -gt0[5]
    dist = lambda p: np.minimum(p % n, n - p % n)
    ok = (dist(py) >= R + 0.625)[:, None] & (dist(px) >= R + 0.625)[None, :]
    assert ok.mean() > 0.7
    big = float(max(np.abs(g.data).max() for g in cfg.granules))
    chunks = coverage.chunk_requests(cfg.bbox, out, out, 64, 64)
    bt = gpu_batch(cfg)
    offs = coverage.band_offsets(chunks, 0, out)
    worst = _Worst("B %s longlat plane" % NAME[code])
    for path, typed, n_ulp in (("(ii)", True, 16), ("(iii)", False, 2)):
        bt.typed = typed
        band = torch.full((out, out), -1.0, dtype=torch.float32, device=bt.device)
        bt.render_coverage(gsky_amd.ScaleParams(*cfg.scale), band, offs, resample=code)
        assert bt.status() == 0
        got = band.cpu().numpy().astype(np.float64)
        assert not (got[ok] == np.float32(-1e10)).any()
        err = np.abs(got - plane)[ok]
        bound = _plane_bound(code, b_px, c_px, n_ulp, big)
        worst.add(path + " / bound", err / bound)
        assert err.max() <= bound, (path, err.max(), bound)
    worst.show()


@pytest.mark.parametrize("code", CODES)
def test_reprojected_plane_albers(gpu, code):
    """B: EPSG:3577 (Albers) -> EPSG:3857, config_c2 at 80-px granules (2 x 2,
    overlapping by 4 px), 2 x 2 tiles of 128 px.  Every granule holds one
    global plane a + b * X + c * Y of the Albers coordinates and no nodata;
    checked are the pixels that lie R + 0.625 source pixels inside one granule
    or more, and as far from the edges of every other, against the plane at
    the exact fp64 transform (tests/test_warp_exact.py)."""
    import gsky_amd
    R = RADIUS[code]
    cfg = synth.config_c2(scale=0.02, tiles_per_side=2, tile_px=128, grid=2)
    a0, bm, cm = 100.0, 1e-3, -2e-3
    for g in cfg.granules:
        ny, nx = g.data.shape
        assert (ny, nx) == (80, 80)
        X = g.geot[0] + g.geot[1] * (np.arange(nx) + 0.5)
        Y = g.geot[3] + g.geot[5] * (np.arange(ny) + 0.5)
        g.data = (a0 + bm * X[None, :] + cm * Y[:, None]).astype(np.float32)
        g.nodata = None
        g.overviews = []
    psz = cfg.granules[0].geot[1]
    b_px, c_px = abs(bm * psz), abs(cm * psz)
    big = float(max(np.abs(g.data).max() for g in cfg.granules))
    cfg.namespaces, cfg.scale, cfg.palette, cfg.resample = [""], (0.0, 1.0, 0.0, 0), None, code
    b = gpu_batch(cfg)
    sp = gsky_amd.ScaleParams(*cfg.scale)
    worst = _Worst("B %s albers plane" % NAME[code])
    m = R + 0.625
    n_ok = 0
    for path, typed, n_ulp in (("(ii)", True, 16), ("(iii)", False, 2)):
        b.typed = typed
        cv = _canvas(b.render(sp, resample=code, rgba=False), b, np.float32)
        assert b.status() == 0
        for t, (bb, w, h) in enumerate(cfg.tiles):
            jj, ii = np.mgrid[0:h, 0:w]
            X = bb[0] + (ii + 0.5) * (bb[2] - bb[0]) / w
            Y = bb[3] - (jj + 0.5) * (bb[3] - bb[1]) / h
            ax, ay = albers(*merc_inv(X, Y))
            plane = a0 + bm * ax + cm * ay
            clear, inside = np.ones((h, w), bool), np.zeros((h, w), bool)
            for g in cfg.granules:
                sx, sy = (ax - g.geot[0]) / g.geot[1], (ay - g.geot[3]) / g.geot[5]
                inn = (sx >= m) & (sx <= 80 - m) & (sy >= m) & (sy <= 80 - m)
                far = (sx <= -m) | (sx >= 80 + m) | (sy <= -m) | (sy >= 80 + m)
                clear &= inn | far
                inside |= inn
            ok = clear & inside
            n_ok += int(ok.sum())
            got = cv[t, :h, :w].astype(np.float64)
            assert not (got[ok] == np.float32(-1e10)).any()
            err = np.abs(got - plane)[ok]
            bound = _plane_bound(code, b_px, c_px, n_ulp, big)
            worst.add(path + " / bound", err / bound)
            assert err.size == 0 or err.max() <= bound, (path, t, err.max(), bound)
    assert n_ok > 2 * 0.4 * 4 * 128 * 128, n_ok
    worst.show()
