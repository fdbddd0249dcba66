"""The cubic convolution rule (GSKYHIP_RESAMPLE_CUBIC, include/gskyhip.h) in
numpy fp64, and checks of the rule itself.  tests/test_cubic.py holds every
GPU path to `cubic_rule`; this module needs no GPU.

The rule is GDAL 3.0.1 GWKCubicResample4Sample on the geometry of
test_bilinear_edges.py part A (both sides EPSG:3857, power-of-two
geotransforms, every source coordinate exact in fp64): 4 x 4 taps around
floor(s - 0.5), rows first, CC() evaluated in the order it is written in; a
pixel with a tap outside the band, or equal to the band's nodata, has the
bilinear rule's value (`_rule` of test_bilinear_edges.py).
"""
import numpy as np

from gsky_amd.tiles import bbox_to_geot

from .test_bilinear_edges import ND, _granule, _rule, _tile


def cc(t, f0, f1, f2, f3):
    """GWKCubicResample4Sample's 1-D convolution, every operation in this order."""
    t2 = t * t
    t3 = t2 * t
    return f1 + 0.5 * (t * (f2 - f0) + t2 * (2.0 * f0 - 5.0 * f1 + 4.0 * f2 - f3) + t3 * (3.0 * (f1 - f2) + f3 - f0))


def cubic_rule(data, nodata, sgt, tile):
    """The rule of one granule (`data`: the taps as the sample sees them,
    geotransform `sgt`) on one same-CRS tile, fp64.  Returns (sample, has: a
    sample is taken, cub: the pixel takes the 16-tap sample, window [xoff,
    yoff, w, h]); where cub is False, sample / has are the bilinear rule's."""
    bsample, bhas, _, win = _rule(data, nodata, sgt, tile)
    bb, w, h = tile
    gt = bbox_to_geot(w, h, bb)
    ny, nx = data.shape
    cub = np.zeros((h, w), bool)
    if nx < 4 or ny < 4:
        return bsample, bhas, cub, win
    d = data.astype(np.float64)
    sx = ((gt[0] + (np.arange(w) + 0.5) * gt[1]) - sgt[0]) / sgt[1]
    sy = ((gt[3] + (np.arange(h) + 0.5) * gt[5]) - sgt[3]) / sgt[5]
    fx, fy = np.floor(sx - 0.5), np.floor(sy - 0.5)
    tx, ty = (sx - 0.5 - fx)[None, :], (sy - 0.5 - fy)[:, None]
    inside = ((fy - 1 >= 0) & (fy + 2 < ny))[:, None] & ((fx - 1 >= 0) & (fx + 2 < nx))[None, :]
    ix = np.clip(fx, 1, nx - 3).astype(np.int64)
    iy = np.clip(fy, 1, ny - 3).astype(np.int64)
    anynd = np.zeros((h, w), bool)
    rows = []
    for j in range(-1, 3):
        f = [d[(iy + j)[:, None], (ix + i)[None, :]] for i in range(-1, 3)]
        if nodata is not None:
            for v in f:
                anynd |= (v == nodata) | (np.isnan(v) if np.isnan(nodata) else False)
        rows.append(cc(tx, *f))
    with np.errstate(invalid="ignore"):
        r = cc(ty, *rows)
    inwin = np.zeros((h, w), bool)
    inwin[win[1]:win[1] + win[3], win[0]:win[0] + win[2]] = True
    cub = inside & ~anynd
    return np.where(cub, r, bsample), np.where(cub, inwin, bhas), cub, win


def to_type(r, dt):
    """Output conversion of a sample: float32 cast; integers floor(r + 0.5),
    saturated (a signed byte is a byte 0..255 to the sample, wrapped back)."""
    if dt == np.float32:
        return r.astype(np.float32)
    v = np.floor(r + 0.5)
    if dt == np.int8:
        return np.clip(v, 0, 255).astype(np.uint8).view(np.int8)
    info = np.iinfo(dt)
    return np.clip(v, info.min, info.max).astype(dt)


def quadratic(ny, nx, c=(3, -2, 5, 1, -1, 2)):
    """A float32 quadratic surface with small integer coefficients, and its
    value at fractional pixel-centre coordinates (x, y) = (sx - 0.5, sy - 0.5)."""
    fn = lambda x, y: c[0] + c[1] * x + c[2] * y + c[3] * x * x + c[4] * x * y + c[5] * y * y
    y, x = np.mgrid[0:ny, 0:nx].astype(np.float64)
    return fn(x, y).astype(np.float32), fn


def _coords(g, tile):
    bb, w, h = tile
    gt = bbox_to_geot(w, h, bb)
    sx = ((gt[0] + (np.arange(w) + 0.5) * gt[1]) - g.geot[0]) / g.geot[1]
    sy = ((gt[3] + (np.arange(h) + 0.5) * gt[5]) - g.geot[3]) / g.geot[5]
    return sx, sy


def test_constant():
    from gsky_amd import _lib
    assert _lib.RESAMPLE_CUBIC == 2 and _lib.RESAMPLE_BILINEAR == 1 and _lib.RESAMPLE_NEAREST == 0


def test_rule_reproduces_a_quadratic_exactly():
    data, fn = quadratic(20, 24)
    for ratio, shift in ((1.0, 0.5), (0.5, 0.25), (2.0, 0.0)):
        g = _granule(data, ratio, 3 - shift * ratio, 2 - shift * ratio, None)
        tile = _tile(64, 48)
        sample, has, cub, win = cubic_rule(g.data, None, g.geot, tile)
        sx, sy = _coords(g, tile)
        exact = fn((sx - 0.5)[None, :], (sy - 0.5)[:, None])
        assert cub.sum() >= 80 and has[cub].all()
        assert np.abs(sample[cub] - exact[cub]).max() == 0.0   # error 0: every term is exact in fp64
        assert (np.abs(sample - exact)[has & ~cub] > 0).any()   # the bilinear fallback is not


def test_rule_does_not_reproduce_a_cubic():
    x = np.arange(24, dtype=np.float64)
    data = np.repeat((x ** 3)[None, :], 20, 0).astype(np.float32)
    g = _granule(data, 1.0, 3 - 0.25, 2, None)   # tx = 1/4 (at tx = 1/2 the symmetric taps do reproduce x^3)
    tile = _tile(64, 48)
    sample, has, cub, _ = cubic_rule(g.data, None, g.geot, tile)
    sx, _ = _coords(g, tile)
    exact = np.repeat(((sx - 0.5) ** 3)[None, :], 48, 0)
    assert cub.sum() > 200 and np.abs(sample[cub] - exact[cub]).min() > 0.05   # 3/32 at every pixel


def test_rule_at_zero_phase_returns_the_centre_tap():
    rng = np.random.default_rng(5)
    data = rng.uniform(-1000.0, 1000.0, (20, 24)).astype(np.float32)
    g = _granule(data, 1.0, 3, 2, None)     # pixel centres coincide: tx = ty = 0
    sample, has, cub, win = cubic_rule(g.data, None, g.geot, _tile(64, 48))
    assert win == [3, 2, 25, 21]            # warp.go:200-217: the footprint plus the half-pixel round
    exp = np.zeros((48, 64))
    exp[2:22, 3:27] = data
    assert cub[3:20, 4:25].all() and np.array_equal(sample[cub], exp[cub])


def test_rule_small_bands():
    rng = np.random.default_rng(6)
    for n, ncub in ((3, 0), (4, 1)):
        data = rng.uniform(-1000.0, 1000.0, (n, n)).astype(np.float32)
        g = _granule(data, 4.0, 5.25, 3.5, None)
        tile = _tile(40, 30)
        sample, has, cub, _ = cubic_rule(g.data, None, g.geot, tile)
        bs, bh, _, _ = _rule(g.data, None, g.geot, tile)
        sx, sy = _coords(g, tile)
        cell = (np.floor(sy - 0.5) == 1)[:, None] & (np.floor(sx - 0.5) == 1)[None, :]
        assert np.array_equal(cub, cell if ncub else np.zeros_like(cell)) and cub.sum() == 16 * ncub
        assert np.array_equal(sample[~cub], bs[~cub], equal_nan=True) and np.array_equal(has[~cub], bh[~cub])
        if ncub:
            assert (sample[cub] != bs[cub]).any()


def test_rule_nodata_tap_falls_back():
    rng = np.random.default_rng(7)
    data = rng.uniform(-1000.0, 1000.0, (12, 12)).astype(np.float32)
    data[5, 6] = ND
    g = _granule(data, 1.0, 2.5, 2.5)
    tile = _tile(20, 20)
    sample, has, cub, _ = cubic_rule(g.data, ND, g.geot, tile)
    bs, bh, _, _ = _rule(g.data, ND, g.geot, tile)
    sx, sy = _coords(g, tile)
    near = (np.abs(np.floor(sy - 0.5) + 0.5 - 5) <= 2)[:, None] & (np.abs(np.floor(sx - 0.5) + 0.5 - 6) <= 2)[None, :]
    assert not cub[near].any() and near.sum() == 16 and cub.sum() == 9 * 9 - 16
    assert np.array_equal(sample[~cub & bh], bs[~cub & bh])
    assert to_type(np.array([-3.2, 260.4, 127.5]), np.uint8).tolist() == [0, 255, 128]
    assert to_type(np.array([-3.2, 260.4, 200.0]), np.int8).tolist() == [0, -1, -56]
    assert to_type(np.array([-40000.0, 40000.0, -0.5]), np.int16).tolist() == [-32768, 32767, 0]
