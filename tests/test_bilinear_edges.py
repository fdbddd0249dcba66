"""Edge rules of bilinear resampling (GWKBilinearResample4Sample) on every
bilinear code path of the product, on small inputs.

The paths, and the call that reaches each:

  (i)   bilinear_value (render_generic.h, warp_window_kernel)   batch.warp_windows(1)
  (ii)  render_bil_kernel (render_bil.h)  batch.render(sp, resample=1, rgba=False) on float32 granules
        -- the canvases-only call of WCS GetCoverage.  render(..., canvas=True)
        with RGBA beside the canvases takes the generic dispatch (launch_render
        picks the band kernels for RGBA only or canvases only), so it is path
        (iii), not this one.
  (iii) the generic kernels (bil_fetch, render_common.h)        batch.typed = False, same call
  (iv)  render_lds_kernel (render_lds.h)  integer granules: render(sp, pal, resample=1) for RGBA,
                                          render(..., rgba=False) for typed canvases

The fp64 rule of (i), (iii), (iv) and of (ii)'s fp64 branch is one function,
bilinear_rule() (resample.h); bilinear_value and bil_fetch wrap it with their
own tap loads.  (ii)'s fp32 renormalisation is bil4_renorm() (resample.h).

Part A needs no oracle: source and destination are both EPSG:3857, so neither
side reprojects and the warp is the affine map of the two geotransforms.  They
are built from powers of two, every source coordinate is exact in fp64, and
the expected value of each pixel is written here in numpy fp64 straight from
the rule: taps at floor(s - 0.5), the -1 edge rule, taps outside the band or
equal to the nodata dropped, accDiv == 1 -> accR, accDiv < 1e-5 -> no sample,
else accR / accDiv; outside the warped window (warp.go:200-217: the granule's
footprint in destination pixels) the window fill.  Bars: identical nodata
mask with no pixel left out; (i) and (iii) within 1 ulp_f32 of the reference
and bit-exact where one tap carries the sample; (ii) (fp32 weights) within
1e-4 * M, M the granule's largest |valid value|.

Part B compares the reprojected paths with the CPU oracle at the edges the
full-size tests alone reached: separable rows with tap reuse at 1:1, float
canvases past one 512-column block, NaN / non-float32 / absent nodata, NaN
data, 0-4 dropped taps, sign-mixed data, several entries per pixel, and the
integer types of render_lds_kernel, where a result may differ from the oracle
by 1 only on a rounding tie (helpers.bilinear_tie_masks).

Nothing in part A departed from the rule.  Part B found two departures, both
fixed with this module: signed-byte taps read as int8 (every negative value
came out 0; render_common.h bil_tap), and render_bil_kernel's fp32 weights
missing the merge nodata by an ulp where all taps hold float32(nodata) of a
nodata no float32 equals (render_bil.h, the fp64 branch).

Worst errors measured on an MI355X (every test prints its own; -s shows them):

  (i)   warp_windows      A: 0 ulp on every case (bit-equal to float32(rule))
                          B: equal to the oracle but for 8.1e-8 relative (1 ulp_f32)
                             on the multi-entry tiles; integers: no difference
  (ii)  render_bil_kernel A: 1.1e-7 * M (A1 at 1:2; A4 at 1:1 1.07e-7; A2 exact)
                          B: 1.5e-7 relative at 1:1 (B1), 1.9e-6 with no nodata (B2,
                             float32(0.1) beside 200), 6.6e-7 multi-entry (B4), 6.2e-7 on POOL rows;
                             sign-mixed (B3) 1.2e-7 * M, which is 1.3e-3 relative to
                             |ref| at the worst zero crossing
  (iii) generic kernels   as (i)
  (iv)  render_lds_kernel uint8, int8, int16, uint16, RGBA and canvases: no
                          difference from the oracle, on or off a rounding tie
"""
import numpy as np
import pytest

from gsky_amd import synth
from gsky_amd.tiles import bbox_to_geot

from .helpers import bilinear_tie_masks, cast_cfg, gpu_batch, oracle_inputs, oracle_render

pytestmark = pytest.mark.gpu

BILINEAR_RTOL = 1e-4     # the project's bilinear bar (BASELINE north_star)
SRS = "EPSG:3857"
PX = 16.0                # destination pixel size, metres
X0, Y0 = 2.0 ** 23, -(2.0 ** 22)   # top-left corner of every part-A tile
ND = -9999.0

# ---------------------------------------------------------------- part A: the rule in numpy
def _round_coord(c, n):   # warp.go:69-80
    return 0 if c < 0 else min(int(c + 1e-10), n - 1)


def _rule(data, nodata, sgt, tile):
    """GWKBilinearResample4Sample of one granule (`data`, geotransform `sgt`)
    on one same-CRS tile, fp64.  Returns (sample, has: a sample is taken,
    ntap: valid taps of non-zero weight, window [xoff, yoff, w, h])."""
    bb, w, h = tile
    gt = bbox_to_geot(w, h, bb)
    ny, nx = data.shape
    d = data.astype(np.float64)
    sx = ((gt[0] + (np.arange(w) + 0.5) * gt[1]) - sgt[0]) / sgt[1]
    sy = ((gt[3] + (np.arange(h) + 0.5) * gt[5]) - sgt[3]) / sgt[5]
    for s in (sx, sy):   # dyadic grid: the coordinates carry no rounding
        assert np.array_equal(s * 2.0 ** 24, np.round(s * 2.0 ** 24))

    def axis(s):
        i = np.floor(s - 0.5).astype(np.int64)
        r = 1.5 - (s - i)
        edge = i == -1
        return np.where(edge, 0, i), np.where(edge, 1.0, r)

    ix, rx = axis(sx)
    iy, ry = axis(sy)
    acc_r = np.zeros((h, w))
    acc_d = np.zeros((h, w))
    ntap = np.zeros((h, w), np.int32)
    nan_nd = nodata is not None and np.isnan(nodata)
    for k in range(4):
        xx, yy = ix + (k & 1), iy + (k >> 1)
        wk = np.outer((1.0 - ry) if k >> 1 else ry, (1.0 - rx) if k & 1 else rx)
        use = ((yy >= 0) & (yy < ny))[:, None] & ((xx >= 0) & (xx < nx))[None, :]
        v = d[np.clip(yy, 0, ny - 1)[:, None], np.clip(xx, 0, nx - 1)[None, :]]
        if nodata is not None:
            use &= ~((v == nodata) | (np.isnan(v) if nan_nd else False))
        acc_d += np.where(use, wk, 0.0)
        acc_r += np.where(use, v * wk, 0.0)
        ntap += use & (wk > 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        sample = np.where(acc_d == 1.0, acc_r, acc_r / acc_d)
    has = ~(acc_d < 0.00001)
    # the warped window: the granule's footprint in destination pixels
    left, right = (sgt[0] - gt[0]) / gt[1], (sgt[0] + nx * sgt[1] - gt[0]) / gt[1]
    top, bottom = (sgt[3] - gt[3]) / gt[5], (sgt[3] + ny * sgt[5] - gt[3]) / gt[5]
    wx0, wy0 = _round_coord(left, w), _round_coord(top, h)
    wx1, wy1 = _round_coord(right + 0.5, w), _round_coord(bottom + 0.5, h)
    inwin = np.zeros((h, w), bool)
    inwin[wy0:wy1 + 1, wx0:wx1 + 1] = True
    return sample, has & inwin, ntap, [wx0, wy0, wx1 - wx0 + 1, wy1 - wy0 + 1]


def _granule(data, ratio, left, top, nodata=ND):
    """A same-CRS granule whose pixels are `ratio` destination pixels wide,
    its top-left corner at destination pixel (left, top) of a part-A tile."""
    geot = [X0 + left * PX, ratio * PX, 0.0, Y0 - top * PX, 0.0, -ratio * PX]
    return synth.SynthGranule(np.ascontiguousarray(data, np.float32), geot, SRS, nodata, 1577836800.0, "P")


def _tile(w, h, ox=0, oy=0):
    """A w x h part-A tile with its top-left at destination pixel (ox, oy)."""
    x0, y1 = X0 + ox * PX, Y0 - oy * PX
    return ((x0, y1 - h * PX, x0 + w * PX, y1), w, h)


def _noise(rng, ny, nx, p_nd=0.15):
    v = rng.uniform(-1000.0, 1000.0, (ny, nx)).astype(np.float32)
    v[rng.random((ny, nx)) < p_nd] = ND
    return v


def _canvases(cv, b, dtype=np.float32):
    """(n_tiles, max_h, max_w) typed view of the first namespace's canvases."""
    n = b.max_h * b.max_w * np.dtype(dtype).itemsize
    return cv.cpu().numpy()[:, 0, :n].copy().view(dtype).reshape(-1, b.max_h, b.max_w)


class _Worst:
    """Largest error seen per path, printed at the end of a test."""

    def __init__(self, case):
        self.case, self.v = case, {}

    def add(self, path, err):
        if err.size:
            self.v[path] = max(self.v.get(path, 0.0), float(err.max()))

    def show(self):
        print("\n[bilinear_edges] %s: %s" % (self.case, ", ".join("%s %.3g" % kv for kv in sorted(self.v.items()))))


def _assert_fp64_path(path, got, sample, has, ntap, nd32, worst, where):
    """Paths (i) and (iii): the mask, 1 ulp_f32, single-tap pixels bit-exact."""
    ref32 = sample.astype(np.float32)
    exp = np.where(has, ref32, nd32)
    assert np.array_equal(got == nd32, exp == nd32), (path, where)
    v = exp != nd32
    err = np.abs(got[v].astype(np.float64) - ref32[v].astype(np.float64)) / np.spacing(np.abs(ref32[v]))
    worst.add(path + " ulp", err)
    assert err.size == 0 or err.max() <= 1.0, (path, where, err.max())
    one = v & (ntap == 1)
    assert np.array_equal(got[one], ref32[one]), (path, where)
    return int(v.sum()), int(one.sum())


def _assert_fp32_path(path, got, sample, has, nd32, big, worst, where):
    """Path (ii), fp32 weights: the mask, 1e-4 of the data's scale."""
    exp = np.where(has, sample.astype(np.float32), nd32)
    assert np.array_equal(got == nd32, exp == nd32), (path, where)
    v = exp != nd32
    err = np.abs(got[v].astype(np.float64) - sample[v]) / big
    worst.add(path + " /M", err)
    assert err.size == 0 or err.max() <= BILINEAR_RTOL, (path, where, err.max())


def _run_same_crs(granules, tiles, pairs, worst, case):
    """One batch through paths (i), (ii), (iii) against _rule.  One granule
    per tile.  Returns (valid pixels, single-tap pixels) checked on path (i)."""
    import gsky_amd
    cfg = synth.SynthConfig(case, granules, SRS, tiles, pairs, [""], (0.0, 1.0, 0.0, 0), None, resample=1)
    sp = gsky_amd.ScaleParams(*cfg.scale)
    b = gpu_batch(cfg)
    refs = []
    for t, tile in enumerate(tiles):
        (gi,) = pairs[t]
        g = granules[gi]
        refs.append(_rule(g.data, g.nodata, g.geot, tile))
    nd32 = np.float32(ND)
    n_valid = n_one = 0
    wins = b.warp_windows(1)
    assert len(wins) == len(tiles)
    for t, (arr, bbox, tname, nd) in enumerate(wins):
        sample, has, ntap, win = refs[t]
        assert tname == "Float32" and nd == ND and bbox == win, (case, t, bbox, win)
        sl = (slice(win[1], win[1] + win[3]), slice(win[0], win[0] + win[2]))
        nv, no = _assert_fp64_path("(i)", arr.cpu().numpy(), sample[sl], has[sl], ntap[sl], nd32, worst, (case, t))
        n_valid, n_one = n_valid + nv, n_one + no
    for path, typed in (("(ii)", True), ("(iii)", False)):
        b.typed = typed
        cv = _canvases(b.render(sp, resample=1, rgba=False), b)
        assert b.status() == 0
        for t, (_, w, h) in enumerate(tiles):
            sample, has, ntap, _ = refs[t]
            got = cv[t, :h, :w]
            if typed:
                g = granules[pairs[t][0]].data
                big = float(np.abs(g[g != ND]).max())
                _assert_fp32_path(path, got, sample, has, nd32, big, worst, (case, t))
            else:
                _assert_fp64_path(path, got, sample, has, ntap, nd32, worst, (case, t))
    return n_valid, n_one


OFFSETS = (0.0, 0.25, 0.5 - 2.0 ** -10)


@pytest.mark.parametrize("ratio", [1.0, 0.5, 2.0], ids=["1to1", "down2", "up2"])
def test_same_crs_scale_and_phase(gpu, ratio):
    """A1: 1:1, 2:1 down- and 1:2 upsampling at sub-pixel phases 0, 1/4 and
    1/2 - 2^-10 (x and y phases paired differently), the tile overhanging all
    four band edges: the -1 rule on both axes, the partial taps past the right
    and bottom edge, the window fill around them."""
    rng = np.random.default_rng(11)
    worst = _Worst("A1 ratio %g" % ratio)
    nx, ny = int(round(70 / ratio)), int(round(36 / ratio))
    for k, ox in enumerate(OFFSETS):
        oy = OFFSETS[(k + 1) % 3]
        # source phase `o` of the pixel centres: the granule's corner moves by -o source pixels
        g = _granule(_noise(rng, ny, nx), ratio, 3 - ox * ratio, 4 - oy * ratio)
        tiles = [_tile(77, 45), _tile(40, 30, 1, 2), _tile(50, 20, 30, 25)]
        nv, no = _run_same_crs([g], tiles, [[0]] * 3, worst, "A1 r%g ox%g oy%g" % (ratio, ox, oy))
        assert nv > 2000
    worst.show()


@pytest.mark.parametrize("shift,sampled", [(-20, False), (-16, True)])
def test_same_crs_accdiv_threshold(gpu, shift, sampled):
    """A2: 1:1 with x phase 2^shift, y phase 0: the far column's weight is
    2^shift and nodata fills every other source column, so half of the pixels
    have that column alone.  2^-20 < 1e-5: no sample, the canvas nodata;
    2^-16 > 1e-5: that tap's value, bit-exact on the fp64 paths."""
    rng = np.random.default_rng(12)
    data = _noise(rng, 20, 64, 0.0)
    data[:, 0::2] = ND
    off = 2.0 ** shift
    g = _granule(data, 1.0, 2 - off, 2)
    tile = _tile(60, 18, 4, 3)    # inside the band: sx = c + 2.5 + off
    sample, has, ntap, _ = _rule(g.data, ND, g.geot, tile)
    lone = np.zeros((18, 60), bool)
    lone[:, 0::2] = True          # iSrcX = c + 2 even: the near column is nodata
    assert np.array_equal(has, ~lone if not sampled else np.ones_like(lone))
    if sampled:   # the lone far tap at (c + 3, r + 1), weight 2^-16
        assert np.array_equal(sample[lone].astype(np.float32), data[1:19, 3:63][lone])
    worst = _Worst("A2 2^%d" % shift)
    nv, no = _run_same_crs([g], [tile], [[0]], worst, "A2 2^%d" % shift)
    assert no == nv == (18 * 60 if sampled else 18 * 30)
    worst.show()


@pytest.mark.parametrize("ratio", [1.0, 4.0], ids=["1to1", "up4"])
def test_same_crs_tiny_bands(gpu, ratio):
    """A3: bands of 1x1, 1x7, 7x1 and 2x2 pixels inside a 70x20 tile (band
    size - 1 == 0: no pixel has all four taps inside)."""
    rng = np.random.default_rng(13)
    worst = _Worst("A3 ratio %g" % ratio)
    shapes = [(1, 1), (1, 7), (7, 1), (2, 2)]
    granules = [_granule(_noise(rng, ny, nx, 0.0), ratio, 5.25, 3.5) for (ny, nx) in shapes]
    granules[1].data[0, 3] = ND
    granules[3].data[1, 0] = ND
    nv, _ = _run_same_crs(granules, [_tile(70, 20)] * 4, [[k] for k in range(4)], worst, "A3 r%g" % ratio)
    assert nv >= 1 + 6 + 7 + 3
    worst.show()


WIDTHS = (1, 63, 64, 65, 511, 512, 513, 577)
HEIGHTS = (1, 15, 16, 17)


@pytest.mark.parametrize("ratio", [1.0, 2.0], ids=["1to1_reuse", "up2"])
def test_same_crs_tile_shapes(gpu, ratio):
    """A4: every tile width around the 64-column lane slots and the
    512-column block, every height around the 16-row band, as mixed sizes in
    one batch over one granule that covers them all.  At 1:1 every row below
    the first of a wave steps the source row by +1 (the separable path with
    tap reuse); at 1:2 the LINEAR all-taps-inside path."""
    rng = np.random.default_rng(14)
    worst = _Worst("A4 ratio %g" % ratio)
    nx, ny = int(600 / ratio), int(32 / ratio)
    g = _granule(_noise(rng, ny, nx, 0.1), ratio, -0.25 * ratio, -0.25 * ratio)
    tiles = [_tile(w, h, 1 + (3 * i + j) % 7, 1 + (i + 2 * j) % 5)
             for i, w in enumerate(WIDTHS) for j, h in enumerate(HEIGHTS)]
    _run_same_crs([g], tiles, [[0]] * len(tiles), worst, "A4 r%g" % ratio)
    worst.show()


# ---------------------------------------------------------------- part B: oracle parity
def _same(a, b):
    """Equal, NaN equal to NaN."""
    return (a == b) | (np.isnan(a) & np.isnan(b))


def _is_nd(a, nd):
    return np.isnan(a) if np.isnan(nd) else a == nd


def _assert_close(got, exp, nd, worst, path, where, big=None):
    """_check_windows's rule, NaN-aware: identical nodata, NaN where the
    oracle has NaN, every other value within 1e-4 relative -- or, with `big`,
    within 1e-4 * big absolute (sign-mixed data)."""
    g64, e64 = got.astype(np.float64), exp.astype(np.float64)
    assert np.array_equal(_is_nd(g64, nd), _is_nd(e64, nd)), (path, where)
    v = ~_is_nd(e64, nd)
    assert np.array_equal(np.isnan(g64[v]), np.isnan(e64[v])), (path, where)
    v &= ~np.isnan(e64)
    diff = np.abs(g64[v] - e64[v])
    rel = diff / np.maximum(np.abs(e64[v]), 1e-30)
    worst.add(path + " rel", rel)
    if big is None:
        assert rel.size == 0 or rel.max() <= BILINEAR_RTOL, (path, where, rel.max())
    else:
        worst.add(path + " /M", diff / big)
        assert diff.size == 0 or diff.max() <= BILINEAR_RTOL * big, (path, where, diff.max() / big)
    return int(v.sum())


def _float_parity(O, cfg, worst, big=None):
    """Paths (i), (ii), (iii) of a float32 config against the oracle."""
    import gsky_amd
    gr, crs, ts, ph, ns, geots, slots, mask_ns = oracle_inputs(O, cfg)
    b = gpu_batch(cfg)
    wins = b.warp_windows(1)
    p = n = 0
    for t, (bb, w, h) in enumerate(cfg.tiles):
        for gi in cfg.pairs[t]:
            arr, bbox, nd, dt = O.warp(gr[gi], crs[gi], O.crs(cfg.dst_srs), geots[t], w, h, 1)
            g_arr, g_bbox, g_type, g_nd = wins[p]
            p += 1
            assert list(bbox) == g_bbox and g_type == "Float32" and _same(np.float64(nd), np.float64(g_nd)), (t, gi)
            n += _assert_close(g_arr.cpu().numpy(), arr, nd, worst, "(i)", (t, gi), big)
    sp = gsky_amd.ScaleParams(*cfg.scale)
    _, ecv, created = oracle_render(O, cfg, canvas=True)
    assert created[:, 0].all()
    e = ecv[:, 0, : b.max_h * b.max_w * 4].view(np.float32).reshape(-1, b.max_h, b.max_w)
    nodata = cfg.granules[0].nodata
    cnd = np.float32(nodata if nodata is not None else -1e10)
    for path, typed in (("(ii)", True), ("(iii)", False)):
        b.typed = typed
        g = _canvases(b.render(sp, resample=1, rgba=False), b)
        assert b.status() == 0
        for t, (_, w, h) in enumerate(cfg.tiles):
            _assert_close(g[t, :h, :w], e[t, :h, :w], cnd, worst, path, t, big)
    return n, e, b


def _c3_one_to_one(n, extra_pairs):
    """config_c3 at 1:1: 3 x 3 granules of n px, one chunk of 3n x 3n (all
    nine granules on it), and the same chunk again once per granule list of
    `extra_pairs`."""
    cfg = synth.config_c3(scale=n / 2048.0, chunk_px=3 * n, grid=3, out_px=3 * n)
    assert cfg.granules[0].data.shape == (n, n) and len(cfg.tiles) == 1 and len(cfg.pairs[0]) == 9
    cfg.tiles = cfg.tiles * (1 + len(extra_pairs))
    cfg.pairs = cfg.pairs + [list(p) for p in extra_pairs]
    return cfg


# single-entry tiles (the reuse fires), then seams of two entries side by side
# and one above the other (it must not)
EXTRA_PAIRS = ([0], [4], [8], [3, 4], [1, 4], [5, 8, 7])


def test_separable_reuse_at_one_to_one(gpu, oracle):
    """B1: EPSG:4326 -> 3857 at 1:1 (200-px granules, a 600 x 600 chunk, past
    the 512-column block).  Rows are separable (dY == 0) and consecutive
    output rows step the source row by exactly +1 on most rows, which is the
    condition of render_bil_kernel's tap reuse; single-entry tiles take it,
    seam tiles with two or three entries must not."""
    n = 200
    cfg = _c3_one_to_one(n, EXTRA_PAIRS)
    # the input's own property, from the closed-form inverse: iy = floor(sy - 0.5) per output row
    (x0, y0, x1, y1), w, h = cfg.tiles[0]
    _, lat = synth.merc_inv(0.0, y1 - (np.arange(h) + 0.5) * (y1 - y0) / h)
    steps = inside = 0
    for gj in range(3):
        gt = cfg.granules[3 * gj].geot
        sy = (lat - gt[3]) / gt[5]
        rows = (sy >= 1.0) & (sy < n - 1.0)        # all taps inside this granule row
        iy = np.floor(sy - 0.5)
        pair = rows[1:] & rows[:-1]
        inside += int(pair.sum())
        steps += int((pair & (np.diff(iy) == 1.0)).sum())
    assert inside > 500 and steps >= inside / 2, (steps, inside)
    worst = _Worst("B1 1:1 reuse")
    nchecked, _, _ = _float_parity(oracle, cfg, worst)
    assert nchecked > 600 * 600
    worst.show()


def _holes(rng, n):
    """30 % nodata plus solid 5 x 5 blocks."""
    m = rng.random((n, n)) < 0.3
    for _ in range(max(4, n * n // 400)):
        y, x = rng.integers(0, n - 5, 2)
        m[y:y + 5, x:x + 5] = True
    return m


NODATA_CASES = [(-9999.0, -9999.0, 0.0), (float("nan"), float("nan"), 0.0), (0.1, np.float32(0.1), 0.0),
                (None, np.float32(0.1), 0.0), (-9999.0, -9999.0, 0.01)]


@pytest.mark.parametrize("nodata,hole,p_nan", NODATA_CASES,
                         ids=["m9999", "nan", "not_f32", "none", "m9999_nan_data"])
def test_nodata_variety_float32(gpu, oracle, nodata, hole, p_nan):
    """B2: the 1:1 shape (100-px granules) with holes at 30 % plus 5 x 5
    blocks, so 0, 1, 2, 3 and 4 taps are dropped: nodata -9999; NaN; 0.1,
    which no float32 equals -- the holes then hold float32(0.1) and must be
    sampled like any value; no nodata at all; and -9999 with NaN among the
    data, which must come out NaN on both sides."""
    n = 100
    cfg = _c3_one_to_one(n, ([4], [3, 4], [1, 4]))
    rng = np.random.default_rng(22)
    counts = set()
    for g in cfg.granules:
        m = _holes(rng, n)
        quad = m[:-1, :-1].astype(int) + m[:-1, 1:] + m[1:, :-1] + m[1:, 1:]
        counts |= set(np.unique(quad).tolist())
        g.data = g.data.copy()
        g.data[g.data == -9999.0] = 150.0         # config_c3's own 1 % nodata: plain data here
        g.data[m] = hole
        if p_nan:
            g.data[~m & (rng.random((n, n)) < p_nan)] = np.nan
        g.nodata = nodata
    assert counts == {0, 1, 2, 3, 4}
    worst = _Worst("B2 nodata %r nan-data %g" % (nodata, p_nan))
    _, e, _ = _float_parity(oracle, cfg, worst)
    if p_nan:
        assert np.isnan(e[0]).mean() > 0.01
    worst.show()


def test_sign_mixed_high_contrast(gpu, oracle):
    """B3: white noise in [-1000, 1000] (a wrong tap or weight shows at full
    scale), 1e-4 * M absolute; the error relative to |ref| is printed only --
    near a zero crossing the sample is a difference of large terms."""
    n = 100
    cfg = _c3_one_to_one(n, ([4], [3, 4]))
    rng = np.random.default_rng(23)
    for g in cfg.granules:
        nod = g.data == -9999.0
        g.data = rng.uniform(-1000.0, 1000.0, (n, n)).astype(np.float32)
        g.data[nod] = -9999.0
    worst = _Worst("B3 sign-mixed")
    _float_parity(oracle, cfg, worst, big=1000.0)
    worst.show()


def test_pool_rows_float32(gpu, oracle):
    """Albers (EPSG:3577) float32 granules: rows the approximate transformer
    splits (POOL rows: linear leaves) on render_bil_kernel's one-pixel-at-a-
    time path, tiles 513 and 77 px wide, seams of up to four entries."""
    cfg = cast_cfg(synth.config_c2(scale=0.05, tiles_per_side=2, tile_px=64), np.float32)
    sizes = [(513, 48), (77, 50), (77, 33), (513, 17)]
    cfg.tiles = [(bb, *sizes[i]) for i, (bb, _, _) in enumerate(cfg.tiles)]
    cfg.resample = 1
    cfg.scale = (0.0, 1.0, 0.0, 0)
    worst = _Worst("B POOL rows")
    n, _, b = _float_parity(oracle, cfg, worst)
    b.tile_info()
    assert b.plan_counters["pool_leaves"] > 0 and n > 20000
    worst.show()


def _multi_entry_cfg(dt):
    """Five overlapping EPSG:4326 granules of 120 px at 0.01 degrees with
    holes (25 % + blocks): three timestamps apart, two the same; three
    EPSG:3857 tiles near 1:1 listing them in different orders."""
    rng = np.random.default_rng(24)
    n, res = 120, 0.01
    corners = [(130.0, -20.0), (130.5, -20.3), (130.3, -20.6), (130.8, -20.1), (130.2, -20.25)]
    days = [3, 1, 2, 5, 5]
    nod = -9999.0 if dt == np.float32 else -999.0
    gs = []
    for k, ((lon, lat), day) in enumerate(zip(corners, days)):
        v = (300.0 * k + rng.uniform(0.0, 250.0, (n, n))).astype(dt)
        v[_holes(rng, n) & (rng.random((n, n)) < 0.85)] = nod
        gs.append(synth.SynthGranule(v, [lon, res, 0.0, lat, 0.0, -res], "EPSG:4326", nod,
                                     1577836800.0 + 86400.0 * day, "P%d" % k))
    tiles = []
    for (lo0, la0, lo1, la1, w, h) in [(130.1, -21.3, 131.9, -20.0, 180, 140), (130.4, -20.9, 131.3, -20.2, 90, 77),
                                       (129.9, -20.5, 130.7, -19.9, 80, 64)]:
        (x0, x1), (y0, y1) = synth.merc_fwd(np.array([lo0, lo1]), np.array([la0, la1]))
        tiles.append(((float(x0), float(y0), float(x1), float(y1)), w, h))
    pairs = [[0, 1, 2, 3, 4], [4, 2, 0, 3, 1], [3, 4, 0]]
    return synth.SynthConfig("multi", gs, SRS, tiles, pairs, [""], (0.0, 0.0, 1500.0, 0), synth.PALETTE_GSKY,
                             resample=1)


def test_multi_entry_float_canvas(gpu, oracle):
    """B4: several entries per pixel, float32 canvases: an older entry after
    a newer one fills only the holes (fill_mode), equal timestamps keep their
    order, and every hole edge is a dropped-tap sample of two or three stacks."""
    cfg = _multi_entry_cfg(np.float32)
    cfg.scale = (0.0, 1.0, 0.0, 0)
    worst = _Worst("B4 multi-entry float")
    _, e, _ = _float_parity(oracle, cfg, worst)
    levels = set(np.unique(np.floor(e[0][e[0] != -9999.0] / 300.0)).tolist())
    assert levels >= {0.0, 1.0, 2.0, 3.0, 4.0}      # every granule decides pixels of the first tile
    worst.show()


def _assert_integer_parity(O, cfg, dt, worst):
    """The warped windows, render_lds_kernel and the generic kernels against
    the oracle, RGBA and typed canvas: identical nodata mask; a value may
    differ, by 1, only where a stack entry's unrounded sample sits on a
    rounding tie."""
    import gsky_amd
    sp, pal = gsky_amd.ScaleParams(*cfg.scale), gsky_amd.Palette(cfg.palette, True)
    ties, tie_wins = bilinear_tie_masks(O, cfg, windows=True)
    exp, ecv, created = oracle_render(O, cfg, canvas=True)
    assert created[:, 0].all()
    b = gpu_batch(cfg)
    assert bin(b.value_types).count("1") == 1
    # path (i): every warped window
    gr, crs, ts, ph, ns, geots, slots, mask_ns = oracle_inputs(O, cfg)
    wins = b.warp_windows(1)
    p = 0
    for t, (bb, w, h) in enumerate(cfg.tiles):
        for gi in cfg.pairs[t]:
            arr, bbox, wnd, wdt = O.warp(gr[gi], crs[gi], O.crs(cfg.dst_srs), geots[t], w, h, 1)
            g_arr, g_bbox, g_type, g_nd = wins[p]
            assert list(bbox) == g_bbox and g_nd == wnd and g_arr.cpu().numpy().dtype == arr.dtype, (t, gi)
            d = np.abs(g_arr.cpu().numpy().astype(np.int32) - arr.astype(np.int32))
            worst.add("(i) off-tie diff", d[~tie_wins[p]])
            assert not d[~tie_wins[p]].any() and d.max(initial=0) <= 1, (t, gi)
            p += 1
    nb = np.dtype(dt).itemsize
    e = ecv[:, 0, : b.max_h * b.max_w * nb].view(dt).reshape(-1, b.max_h, b.max_w)
    nd = dt(cfg.granules[0].nodata)
    n_tie = n_valid = 0
    for path, typed in (("(iv)", True), ("(iii)", False)):
        b.typed = typed
        rgba = b.render(sp, pal, resample=1).cpu().numpy().copy()
        assert b.status() == 0
        g = _canvases(b.render(sp, pal, resample=1, rgba=False), b, dt)
        for t, (_, w, h) in enumerate(cfg.tiles):
            gt, et, tie = g[t, :h, :w], e[t, :h, :w], ties[t]
            assert np.array_equal(gt == nd, et == nd), (path, t)
            d = np.abs(gt.astype(np.int32) - et.astype(np.int32))
            worst.add(path + " off-tie diff", d[~tie])
            worst.add(path + " on-tie diff", d[tie])
            assert not d[~tie].any(), (path, t, int(d[~tie].max()))
            assert d.max() <= 1, (path, t)
            n_tie += int(tie.sum())
            n_valid += int((et != nd).sum())
            assert np.array_equal(rgba[t, :h, :w, 3] > 0, exp[t, :h, :w, 3] > 0), (path, t)
            ne = (rgba[t, :h, :w] != exp[t, :h, :w]).any(-1)
            assert not (ne & ~tie).any(), (path, t)
    assert n_valid > 0.3 * 2 * cfg.out_pixels      # real data under the comparison
    return n_tie, e


@pytest.mark.parametrize("dt", [np.uint8, np.int8, np.int16, np.uint16])
def test_integer_bilinear_lds_path(gpu, oracle, dt):
    """B5: integer bilinear (render_lds_kernel; the generic kernels beside
    it), RGBA and typed canvas, tiles 77 and 513 px wide."""
    cfg = cast_cfg(synth.config_c2(scale=0.05, tiles_per_side=2, tile_px=64), dt)
    sizes = [(513, 48), (77, 50), (77, 33), (513, 17)]
    cfg.tiles = [(bb, *sizes[i]) for i, (bb, _, _) in enumerate(cfg.tiles)]
    cfg.resample = 1
    cfg.scale = {np.uint8: (0.0, 0.0, 250.0, 0), np.int8: (100.0, 0.0, 200.0, 0)}.get(dt, cfg.scale)
    worst = _Worst("B5 %s" % np.dtype(dt).name)
    _assert_integer_parity(oracle, cfg, dt, worst)
    worst.show()


def test_multi_entry_int16_rgba(gpu, oracle):
    """B4, int16 through the palette: the same overlapping stacks on
    render_lds_kernel (RGBA and typed canvas) under the tie rule."""
    cfg = _multi_entry_cfg(np.int16)
    worst = _Worst("B4 multi-entry int16")
    n_tie, e = _assert_integer_parity(oracle, cfg, np.int16, worst)
    assert set(np.unique(e[0][e[0] != -999] // 300).tolist()) >= {0, 1, 2, 3, 4}
    worst.show()
