"""The area rules (GSKYHIP_RESAMPLE_AVERAGE / _MODE, include/gskyhip.h) in
numpy fp64, and checks of the rules themselves.  tests/test_area.py holds
every GPU path to `area_grid` and `area_points`; this module needs no GPU.

The rule is modelled on GDAL's GWKAverageOrMode and is not pinned against it.
A pixel's footprint in the source is the box [sx - hx, sx + hx] x [sy - hy,
sy + hy], hx = max(0.5, 0.5 (|u.x| + |v.x|)), hy alike, u and v the
differences of the pixel's source coordinate to its neighbours' inside the
pair's window; the taps along an axis are `area_taps`, at most 8 of them; a
pixel's taps are the outer product, rows outer; AVERAGE is the weighted mean
of the taps that do not hold the nodata, MODE the value of the heaviest class
of equal taps, ties to the class met first.  Every sum runs in scan order in
fp64 (Python floats: one rounding per operation, no contraction).
"""
import math

import numpy as np

from gsky_amd.tiles import bbox_to_geot

from .test_bilinear_edges import ND, _granule, _rule, _tile
from .test_cubic_rule import _coords, to_type
from .test_overviews import ref_level

AVERAGE, MODE = 3, 4


# ---------------------------------------------------------------- the rule
def area_taps(s, h, n):
    """The taps of [s - h, s + h] along an axis of n source pixels and their
    weights: ([xx, ...], [w, ...], stride)."""
    x0, x1 = s - h, s + h
    if not (math.isfinite(x0) and math.isfinite(x1)):
        return [], [], 0
    lo, hi = max(math.floor(x0), 0.0), min(math.ceil(x1), float(n))
    if hi <= lo:
        return [], [], 0
    lo, hi = int(lo), int(hi)
    stride = (hi - lo + 7) // 8
    taps = list(range(lo, hi, stride))
    if stride == 1:
        return taps, [min(xx + 1.0, x1) - max(float(xx), x0) for xx in taps], 1
    return taps, [1.0] * len(taps), stride


def _is_nd(d, nodata):
    return nodata is not None and (d == nodata or (nodata != nodata and d != d))


def _scan(d, nodata, sx, sy, hx, hy):
    """The surviving taps of one pixel in scan order: [(value, w), ...]."""
    ny, nx = d.shape
    xs, wxs, _ = area_taps(sx, hx, nx)
    ys, wys, _ = area_taps(sy, hy, ny)
    out = []
    for yy, wy in zip(ys, wys):
        for xx, wx in zip(xs, wxs):
            w = wx * wy
            v = float(d[yy, xx])
            if _is_nd(v, nodata) or not w > 0.0:
                continue
            out.append((v, w))
    return out


def average_rule(d, nodata, sx, sy, hx, hy):
    """(sample, has) of one pixel; d: the taps as the sample sees them, fp64."""
    acc_w = acc_r = 0.0
    for v, w in _scan(d, nodata, sx, sy, hx, hy):
        acc_w += w
        acc_r += v * w
    if acc_w < 0.00001:
        return 0.0, False
    return acc_r / acc_w, True


def mode_rule(d, nodata, sx, sy, hx, hy):
    classes = []   # [value, weight] in order of first appearance
    for v, w in _scan(d, nodata, sx, sy, hx, hy):
        for c in classes:
            if c[0] == v:          # a NaN tap equals nothing: a class of its own
                c[1] += w
                break
        else:
            classes.append([v, w])
    best = None
    for c in classes:
        if best is None or c[1] > best[1]:
            best = c
    return (best[0], True) if best else (0.0, False)


def half_extents(sx, sy, ok=None):
    """hx, hy of every pixel of a window from the (h, w) arrays of its source
    coordinates: u from the next pixel of the row, else the previous one, else
    zero; v alike along rows; a neighbour whose transform failed (ok False)
    counts as absent."""
    h, w = sx.shape
    ok = np.ones((h, w), bool) if ok is None else ok

    def diff(a, axis):
        n = a.shape[axis]
        out = np.zeros(a.shape)
        idx = np.arange(n)
        a_, ok_ = np.moveaxis(a, axis, 0), np.moveaxis(ok, axis, 0)
        o_ = np.moveaxis(out, axis, 0)
        for i in idx:
            nxt = (ok_[i + 1] if i + 1 < n else np.zeros(ok_[0].shape, bool))
            prv = (ok_[i - 1] if i > 0 else np.zeros(ok_[0].shape, bool))
            fwd = a_[min(i + 1, n - 1)] - a_[i]
            bwd = a_[i] - a_[max(i - 1, 0)]
            o_[i] = np.where(nxt, fwd, np.where(prv, bwd, 0.0))
        return out

    ux, uy, vx, vy = diff(sx, 1), diff(sy, 1), diff(sx, 0), diff(sy, 0)
    return np.maximum(0.5, 0.5 * (np.abs(ux) + np.abs(vx))), np.maximum(0.5, 0.5 * (np.abs(uy) + np.abs(vy)))


def area_points(data, nodata, sx, sy, hx, hy, mode=False):
    """The rule at arrays of coordinates and half extents: (sample, has)."""
    d = data.astype(np.float64)
    rule = mode_rule if mode else average_rule
    sample, has = np.zeros(sx.shape), np.zeros(sx.shape, bool)
    for k in np.ndindex(sx.shape):
        sample[k], has[k] = rule(d, nodata, float(sx[k]), float(sy[k]), float(hx[k]), float(hy[k]))
    return sample, has


def area_grid(data, nodata, sgt, tile, mode=False):
    """The rule of one granule (`data`: the taps as the sample sees them,
    geotransform `sgt`) on one same-CRS tile.  Returns (sample, has: a sample
    is taken, window [xoff, yoff, w, h], hx, hy over the tile); outside the
    window has is False.  The footprint's neighbours are the window's."""
    _, _, _, win = _rule(data, nodata, sgt, tile)     # the window, and the assertion that coordinates are exact
    bb, w, h = tile
    gt = bbox_to_geot(w, h, bb)
    sx = ((gt[0] + (np.arange(w) + 0.5) * gt[1]) - sgt[0]) / sgt[1]
    sy = ((gt[3] + (np.arange(h) + 0.5) * gt[5]) - sgt[3]) / sgt[5]
    x, y, ww, wh = win
    gx, gy = np.meshgrid(sx[x:x + ww], sy[y:y + wh])
    hxw, hyw = half_extents(gx, gy)
    s, hs = area_points(data, nodata, gx, gy, hxw, hyw, mode)
    sample, has = np.zeros((h, w)), np.zeros((h, w), bool)
    hx, hy = np.full((h, w), 0.5), np.full((h, w), 0.5)
    sl = (slice(y, y + wh), slice(x, x + ww))
    sample[sl], has[sl], hx[sl], hy[sl] = s, hs, hxw, hyw
    return sample, has, win, hx, hy


# ---------------------------------------------------------------- checks
def test_constant():
    from gsky_amd import _lib
    assert _lib.RESAMPLE_AVERAGE == AVERAGE == 3 and _lib.RESAMPLE_MODE == MODE == 4
    assert _lib.RESAMPLE_CUBIC == 2


def test_constant_field_gives_the_constant():
    data = np.full((12, 15), 7.25, np.float32)
    rng = np.random.default_rng(1)
    for _ in range(200):
        sx, sy = rng.uniform(-1.0, 16.0), rng.uniform(-1.0, 13.0)
        hx, hy = rng.choice([0.5, 1.0, 1.75, 3.0, 20.5]), rng.choice([0.5, 1.0, 1.75, 3.0, 20.5])
        for rule in (average_rule, mode_rule):
            r, has = rule(data.astype(np.float64), ND, sx, sy, hx, hy)
            inside = sx + hx > 0 and sx - hx < 15 and sy + hy > 0 and sy - hy < 12
            assert has == inside
            if has:
                assert abs(r - 7.25) <= 1e-15 * 7.25 * 64, (rule.__name__, r)   # the mean of equal values, 64 taps
                if rule is mode_rule:
                    assert r == 7.25


def test_half_pixel_footprint_is_the_bilinear_rule():
    """hx = hy = 0.5: the taps and weights of GWKBilinearResample4Sample, its
    -1 edge rule included; 64 random dyadic phases of a 15 x 12 band with 15 %
    nodata on a 24 x 20 tile that overhangs every edge of the band."""
    rng = np.random.default_rng(2)
    data = rng.uniform(-1000.0, 1000.0, (12, 15)).astype(np.float32)
    data[rng.random((12, 15)) < 0.15] = ND
    worst, n = 0.0, 0
    for _ in range(64):
        left, top = 4 + rng.integers(0, 256) / 256.0, 3 + rng.integers(0, 256) / 256.0
        g = _granule(data, 1.0, left, top)
        tile = _tile(24, 20)
        bs, bh, _, win = _rule(g.data, ND, g.geot, tile)
        sx, sy = _coords(g, tile)
        gx, gy = np.meshgrid(sx, sy)
        s, has = area_points(g.data, ND, gx, gy, np.full(gx.shape, 0.5), np.full(gx.shape, 0.5))
        inwin = np.zeros(has.shape, bool)
        inwin[win[1]:win[1] + win[3], win[0]:win[0] + win[2]] = True
        assert np.array_equal(has & inwin, bh)
        assert not (has & ~inwin).any()        # the window holds every pixel that has a tap
        worst = max(worst, float(np.abs(s - bs)[bh].max()) / 1000.0)
        n += int(bh.sum())
    print("\n[area rule] half-pixel footprint against the bilinear rule: %d samples, worst %.3g of the scale" % (n, worst))
    assert n > 5000 and worst <= 1e-12


def test_aligned_two_to_one_is_the_block_mean():
    rng = np.random.default_rng(3)
    data = rng.integers(-1000, 1001, (12, 16)).astype(np.float32)   # integers: float32 sums of four are exact
    holes = data.copy()
    holes[rng.random(data.shape) < 0.15] = ND
    tile = _tile(8, 6)
    for d, nodata in ((data, None), (holes, ND)):
        g = _granule(d, 0.5, 0.0, 0.0, nodata)
        sample, has, win, hx, hy = area_grid(g.data, nodata, g.geot, tile)
        assert win == [0, 0, 8, 6] and (hx == 1.0).all() and (hy == 1.0).all()
        blocks = d.astype(np.float64).reshape(6, 2, 8, 2).transpose(0, 2, 1, 3).reshape(6, 8, 4)
        valid = np.ones(blocks.shape, bool) if nodata is None else blocks != nodata
        cnt = valid.sum(-1)
        assert np.array_equal(has, cnt > 0)
        mean = np.where(valid, blocks, 0.0).sum(-1) / np.maximum(cnt, 1)
        assert np.abs(sample - mean)[has].max() <= 1e-13 * 1000.0
        if nodata is None:
            assert np.array_equal(sample, mean)      # exact: weights of 1, sums of integers
            lvl1 = ref_level(d, None, "average")     # the ingest pyramid's level 1 (tests/test_overviews.py)
            assert lvl1.dtype == np.float32 and np.array_equal(sample.astype(np.float32), lvl1)


def test_fractional_coverage():
    """3.5 : 1 along x, 1 : 1 along y, centre at 5.25: [3.5, 7.0] covers half
    of pixel 3 and pixels 4, 5, 6."""
    d = np.arange(40, dtype=np.float64).reshape(4, 10) ** 2
    taps, w, stride = area_taps(5.25, 1.75, 10)
    assert taps == [3, 4, 5, 6] and w == [0.5, 1.0, 1.0, 1.0] and stride == 1
    r, has = average_rule(d, None, 5.25, 1.5, 1.75, 0.5)
    assert has and r == (0.5 * d[1, 3] + d[1, 4] + d[1, 5] + d[1, 6]) / 3.5
    # clipped at the band's edge: [-0.75, 2.75] keeps pixels 0, 1 and three quarters of 2
    taps, w, _ = area_taps(1.0, 1.75, 10)
    assert taps == [0, 1, 2] and w == [1.0, 1.0, 0.75]
    r, _ = average_rule(d, None, 1.0, 1.5, 1.75, 0.5)
    assert r == (d[1, 0] + d[1, 1] + 0.75 * d[1, 2]) / 2.75
    # both axes: weights multiply
    r, _ = average_rule(d, None, 5.25, 1.25, 1.75, 0.5)
    row = lambda y: 0.5 * d[y, 3] + d[y, 4] + d[y, 5] + d[y, 6]
    assert abs(r - (0.25 * row(0) + 0.75 * row(1)) / 3.5) <= 1e-13 * d.max()
    # outside the band, and non-finite coordinates: no taps
    assert area_taps(-3.0, 1.75, 10)[0] == [] and area_taps(12.0, 1.75, 10)[0] == []
    assert area_taps(float("nan"), 0.5, 10)[0] == [] and area_taps(float("inf"), 0.5, 10)[0] == []
    assert area_taps(1e300, 0.5, 10)[0] == []


def test_tap_cap():
    """A footprint of 41 source pixels: stride 6, 7 taps, weights of 1."""
    taps, w, stride = area_taps(30.0, 20.5, 100)     # [9.5, 50.5]: pixels 9 .. 50
    assert stride == 6 and taps == [9, 15, 21, 27, 33, 39, 45] and w == [1.0] * 7
    d = np.arange(100 * 3, dtype=np.float64).reshape(3, 100)
    r, has = average_rule(d, None, 30.0, 1.5, 20.5, 0.5)
    assert has and r == sum(d[1, t] for t in taps) / 7.0
    # 8 and 9 pixels: the last unstrided footprint and the first strided one
    assert area_taps(10.0, 4.0, 100)[2] == 1 and len(area_taps(10.0, 4.0, 100)[0]) == 8
    taps, w, stride = area_taps(10.0, 4.25, 100)     # [5.75, 14.25]: pixels 5 .. 14
    assert stride == 2 and taps == [5, 7, 9, 11, 13] and w == [1.0] * 5
    for h in (4.25, 12.0, 31.5, 500.0):
        assert len(area_taps(50.3, h, 100)[0]) <= 8


def test_mode():
    d = np.array([[1, 1, 2, 3],
                  [2, 1, 2, 3],
                  [5, 5, 5, 5]], np.float64)
    assert mode_rule(d, None, 1.5, 1.0, 1.5, 1.0) == (1.0, True)          # 3 x 2 taps: 1 three times, 2 twice
    # weights decide: row 0, columns 1..3 at 0.5, 1, 0.5 -- classes 1 (0.5), 2 (1.0), 3 (0.5)
    assert area_taps(2.5, 1.0, 4)[:2] == ([1, 2, 3], [0.5, 1.0, 0.5])
    assert mode_rule(d, None, 2.5, 0.5, 1.0, 0.5) == (2.0, True)
    # a weighted tie: columns 2, 3 of row 0 at weights 1, 1 -- the class met first wins, either way round
    assert mode_rule(d, None, 3.0, 0.5, 1.0, 0.5) == (2.0, True)
    assert mode_rule(d[:, ::-1].copy(), None, 1.0, 0.5, 1.0, 0.5) == (3.0, True)
    # ... and a later, heavier class beats it: [0.25, 3.75] weighs 1 at 0.75 + 0.75 and 2 at 1 + 1
    assert mode_rule(np.array([[1.0, 2.0, 2.0, 1.0]]), None, 2.0, 0.5, 1.75, 0.5) == (2.0, True)
    assert mode_rule(np.array([[1.0, 2.0, 3.0, 1.0]]), None, 2.0, 0.5, 1.75, 0.5) == (1.0, True)
    # nodata dropped: with 1 the nodata the majority of the first case is 2
    assert mode_rule(d, 1.0, 1.5, 1.0, 1.5, 1.0) == (2.0, True)
    assert mode_rule(d, 5.0, 2.0, 2.5, 2.0, 0.5) == (0.0, False)          # all nodata: no sample
    assert average_rule(d, 5.0, 2.0, 2.5, 2.0, 0.5) == (0.0, False)
    # NaN taps that are not nodata: a class each, so two NaNs lose to two equal values
    n = np.array([[np.nan, np.nan, 4.0, 4.0]])
    assert mode_rule(n, None, 2.0, 0.5, 2.0, 0.5) == (4.0, True)
    r, has = mode_rule(n, None, 1.0, 0.5, 1.0, 0.5)                       # NaN, NaN: the first class
    assert has and r != r
    assert mode_rule(n, float("nan"), 2.0, 0.5, 2.0, 0.5) == (4.0, True)  # NaN nodata drops them
    assert mode_rule(n, float("nan"), 1.0, 0.5, 1.0, 0.5) == (0.0, False)


def test_integer_exit():
    assert to_type(np.array([2.5, 3.49, -0.5, -0.51, 300.0, -7.0]), np.uint8).tolist() == [3, 3, 0, 0, 255, 0]
    assert to_type(np.array([-32768.6, 40000.0, 1.5, -1.5]), np.int16).tolist() == [-32768, 32767, 2, -1]
    assert to_type(np.array([65535.4, 65535.5, -3.0]), np.uint16).tolist() == [65535, 65535, 0]
    assert to_type(np.array([127.5, 200.0, 260.0]), np.int8).tolist() == [-128, -56, -1]
