"""The two point kernels, cubic B-spline and Lanczos (GSKYHIP_RESAMPLE_CUBICSPLINE
= 5, GSKYHIP_RESAMPLE_LANCZOS = 6, include/gskyhip.h), in numpy fp64, and checks
of the rule itself.  tests/test_kernel.py holds every GPU path to
`kernel_grid`; this module needs no GPU.

The rule (R = 2: 4 x 4 taps, R = 3: 6 x 6): fx = floor(sx - 0.5), tx = sx - 0.5
- fx; the centre 2 x 2 (fx + {0, 1}, fy + {0, 1}) must lie inside the band and
hold no nodata, else the pixel has the bilinear rule's value (`_rule` of
test_bilinear_edges.py; `bilinear_points` here is the same rule at arbitrary
points).  Weights w[i] = K(i - t), i = 1 - R .. R; rows outer, columns inner:
a tap outside the band or equal to the nodata is dropped, else w = wx[i] *
wy[j], accW += w, accR += d * w; r = accR / accW.  Every operation is an fp64
numpy operation in the order kernel_rule() (resample.h) writes it.
"""
import itertools
import math

import numpy as np

from .test_bilinear_edges import ND, _granule, _noise, _rule, _tile
from .test_cubic_rule import _coords

SPLINE, LANCZOS = 5, 6
RADIUS = {SPLINE: 2, LANCZOS: 3}


def k_spline(x):
    a = np.abs(np.asarray(x, np.float64))
    a2 = a * a
    inner = ((4.0 - 6.0 * a2) + 3.0 * (a2 * a)) / 6.0
    u = 2.0 - a
    outer = (u * u * u) / 6.0
    return np.where(a < 1.0, inner, np.where(a < 2.0, outer, 0.0))


def k_lanczos(x):
    x = np.asarray(x, np.float64)
    p = math.pi * x
    q = p / 3.0
    with np.errstate(divide="ignore", invalid="ignore"):
        v = np.sin(p) * np.sin(q) / (p * q)
    return np.where(x == 0.0, 1.0, np.where(np.abs(x) >= 3.0, 0.0, v))


KERNEL = {SPLINE: k_spline, LANCZOS: k_lanczos}


def weights(code, t):
    """w[i] = K((double)i - t) for i = 1 - R .. R; t any array, the taps on a new last axis."""
    R = RADIUS[code]
    t = np.asarray(t, np.float64)
    return np.stack([KERNEL[code](float(i) - t) for i in range(1 - R, R + 1)], -1)


def _isnd(v, nodata):
    if nodata is None:
        return np.zeros(np.shape(v), bool)
    return (v == nodata) | (np.isnan(v) if np.isnan(nodata) else False)


def bilinear_points(d, nodata, sx, sy):
    """GWKBilinearResample4Sample (bilinear_rule(), resample.h) at the points
    (sx, sy) of an fp64 band d.  Returns (sample, has).  A coordinate that is
    not finite, or beyond the int range, has no tap inside the band."""
    ny, nx = d.shape
    sx, sy = np.broadcast_arrays(np.asarray(sx, np.float64), np.asarray(sy, np.float64))

    def axis(s, n):
        with np.errstate(invalid="ignore"):
            f = np.floor(s - 0.5)
            near = np.isfinite(f) & (f >= -1.0) & (f < n)
        i = np.where(near, f, -5.0).astype(np.int64)   # -5: both taps outside
        with np.errstate(invalid="ignore"):
            r = 1.5 - (s - i)
        edge = i == -1
        return np.where(edge, 0, i), np.where(edge, 1.0, r)

    ix, rx = axis(sx, nx)
    iy, ry = axis(sy, ny)
    acc_r, acc_d = np.zeros(sx.shape), np.zeros(sx.shape)
    for k in range(4):
        xx, yy = ix + (k & 1), iy + (k >> 1)
        with np.errstate(invalid="ignore", over="ignore"):
            wk = ((1.0 - rx) if k & 1 else rx) * ((1.0 - ry) if k >> 1 else ry)
        use = (yy >= 0) & (yy < ny) & (xx >= 0) & (xx < nx)
        v = d[np.clip(yy, 0, ny - 1), np.clip(xx, 0, nx - 1)]
        use &= ~_isnd(v, nodata)
        acc_d = np.where(use, acc_d + wk, acc_d)
        with np.errstate(invalid="ignore"):
            acc_r = np.where(use, acc_r + v * wk, acc_r)
    with np.errstate(divide="ignore", invalid="ignore"):
        sample = np.where(acc_d == 1.0, acc_r, acc_r / acc_d)
    return sample, ~(acc_d < 0.00001)


def kernel_points(data, nodata, sx, sy, code, drop=None):
    """The rule at the points (sx, sy) (arrays of one shape) of a band `data`
    (the taps as the sample sees them).  drop: optional (2 R, 2 R) bool, taps
    [j][i] to drop besides those the band drops (the property tests).  Returns
    (sample, has, kern: the pixel takes the kernel sum, accW, S = sum |w| of
    the surviving taps; accW and S are 1 where kern is False)."""
    R = RADIUS[code]
    d = np.asarray(data).astype(np.float64)
    ny, nx = d.shape
    sx, sy = np.broadcast_arrays(np.asarray(sx, np.float64), np.asarray(sy, np.float64))
    with np.errstate(invalid="ignore"):
        fx, fy = np.floor(sx - 0.5), np.floor(sy - 0.5)
        inside = (fx >= 0.0) & (fx + 1.0 < nx) & (fy >= 0.0) & (fy + 1.0 < ny)
    ix = np.where(inside, fx, 0.0).astype(np.int64)
    iy = np.where(inside, fy, 0.0).astype(np.int64)
    cnd = np.zeros(sx.shape, bool)
    for k in range(4):
        cnd |= _isnd(d[np.clip(iy + (k >> 1), 0, ny - 1), np.clip(ix + (k & 1), 0, nx - 1)], nodata)
    kern = inside & ~cnd
    with np.errstate(invalid="ignore"):
        tx = np.where(inside, sx - 0.5 - fx, 0.0)
        ty = np.where(inside, sy - 0.5 - fy, 0.0)
    wx, wy = weights(code, tx), weights(code, ty)
    acc_r, acc_w, s_abs = np.zeros(sx.shape), np.zeros(sx.shape), np.zeros(sx.shape)
    for j in range(2 * R):
        yy = iy + 1 - R + j
        for i in range(2 * R):
            xx = ix + 1 - R + i
            use = (yy >= 0) & (yy < ny) & (xx >= 0) & (xx < nx)
            v = d[np.clip(yy, 0, ny - 1), np.clip(xx, 0, nx - 1)]
            use &= ~_isnd(v, nodata)
            if drop is not None and drop[j][i]:
                continue
            w = wx[..., i] * wy[..., j]
            acc_w = np.where(use, acc_w + w, acc_w)
            with np.errstate(invalid="ignore", over="ignore"):
                acc_r = np.where(use, acc_r + v * w, acc_r)
            s_abs = np.where(use, s_abs + np.abs(w), s_abs)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = acc_r / acc_w
    bs, bh = bilinear_points(d, nodata, sx, sy)
    return (np.where(kern, r, bs), np.where(kern, True, bh), kern, np.where(kern, acc_w, 1.0),
            np.where(kern, s_abs, 1.0))


def kernel_grid(data, nodata, sgt, tile, code):
    """The rule of one granule (`data`, geotransform `sgt`) on one same-CRS
    tile.  Returns (sample, has, kern, window [xoff, yoff, w, h], accW, S);
    outside the warped window no sample is taken."""
    _, _, _, win = _rule(data, nodata, sgt, tile)
    bb, w, h = tile
    from gsky_amd.tiles import bbox_to_geot
    gt = bbox_to_geot(w, h, bb)
    sx = ((gt[0] + (np.arange(w) + 0.5) * gt[1]) - sgt[0]) / sgt[1]
    sy = ((gt[3] + (np.arange(h) + 0.5) * gt[5]) - sgt[3]) / sgt[5]
    sample, has, kern, acc_w, s_abs = kernel_points(data, nodata, sx[None, :], sy[:, None], code)
    inwin = np.zeros((h, w), bool)
    inwin[win[1]:win[1] + win[3], win[0]:win[0] + win[2]] = True
    return sample, has & inwin, kern & inwin, win, acc_w, s_abs


def plane_error(code, n=64):
    """e_K: the rule's own error on the plane f = x (per source pixel of slope)
    over an n-point grid of phases, no tap dropped: |sum w[i] (i - t) / sum w[i]|."""
    R = RADIUS[code]
    t = np.arange(n) / n
    w = weights(code, t)
    i = np.arange(1 - R, R + 1, dtype=np.float64)
    return float(np.abs((w * (i[None, :] - t[:, None])).sum(-1) / w.sum(-1)).max())


# ---------------------------------------------------------------- the tests
CODES = [SPLINE, LANCZOS]
T = np.arange(4096) / 4096.0


def test_constant():
    from gsky_amd import _lib
    assert _lib.RESAMPLE_CUBICSPLINE == 5 and _lib.RESAMPLE_LANCZOS == 6
    assert _lib.RESAMPLE_CUBIC == 2 and _lib.RESAMPLE_MODE == 4


def test_weights():
    ws = weights(SPLINE, T)
    assert (ws >= 0.0).all() and np.abs(ws.sum(-1) - 1.0).max() <= 4e-16
    wl = weights(LANCZOS, T).sum(-1)
    assert wl.min() >= 0.994 and wl.max() <= 1.0, (wl.min(), wl.max())
    x = np.linspace(0.0, 4.0, 4097)
    for code in CODES:
        K, R = KERNEL[code], RADIUS[code]
        assert np.array_equal(K(x), K(-x))
        assert not K(x[x >= R]).any() and K(0.0) == (1.0 if code == LANCZOS else 4.0 / 6.0)
        assert K(float(R) - 0.25) != 0.0


def _drop_patterns(R, rng, n=40):
    """Drop patterns over the outer taps (the centre 2 x 2 always survives):
    none, all, every positive outer tap is added by the caller, and random ones."""
    pats = [np.zeros((2 * R, 2 * R), bool), np.ones((2 * R, 2 * R), bool)]
    pats += [rng.random((2 * R, 2 * R)) < p for p in (0.15, 0.5, 0.85) for _ in range(n // 3)]
    for p in pats:
        p[R - 1:R + 1, R - 1:R + 1] = False
    return pats


def _phase_points(n, R, nx=12, ny=12):
    """An n x n grid of phases at the centre cell of an nx x ny band."""
    t = np.arange(n) / n
    return (nx // 2 + 0.5 + t)[None, :], (ny // 2 + 0.5 + t)[:, None]


def test_constant_field():
    """A constant field gives the constant under any drop pattern: the spline
    within 64 * 2^-53 relative, Lanczos within 1e-14 * S / accW."""
    rng = np.random.default_rng(50)
    for code in CODES:
        R = RADIUS[code]
        sx, sy = _phase_points(32, R)
        for c in (1.0, -1234.5678, 1e-3):
            data = np.full((12, 12), c)
            for drop in _drop_patterns(R, rng):
                r, has, kern, acc_w, s_abs = kernel_points(data, None, sx, sy, code, drop)
                assert kern.all() and has.all()
                rel = np.abs(r - c) / abs(c)
                bound = 64 * 2.0 ** -53 if code == SPLINE else 1e-14 * s_abs / acc_w
                assert (rel <= bound).all(), (code, c, float(rel.max()))


def test_plane_and_integer_phase():
    """The spline reproduces a plane to 1e-12 of its range; at integer phase
    Lanczos returns the tap itself within 1e-13 M."""
    y, x = np.mgrid[0:12, 0:12].astype(np.float64)
    plane = 7.0 + 3.0 * x - 2.0 * y
    sx, sy = _phase_points(32, 2)
    r, _, kern, _, _ = kernel_points(plane, None, sx, sy, SPLINE)
    exact = 7.0 + 3.0 * (sx - 0.5) - 2.0 * (sy - 0.5)
    assert kern.all() and np.abs(r - exact).max() <= 1e-12 * (plane.max() - plane.min())
    assert plane_error(SPLINE) <= 1e-15 and 0.015 <= plane_error(LANCZOS) <= 0.025
    rng = np.random.default_rng(51)
    data = rng.uniform(-1000.0, 1000.0, (12, 12))
    ix, iy = np.arange(3, 8), np.arange(3, 8)
    r, _, kern, _, _ = kernel_points(data, None, (ix + 0.5)[None, :], (iy + 0.5)[:, None], LANCZOS)
    assert kern.all() and np.abs(r - data[3:8, 3:8]).max() <= 1e-13 * np.abs(data).max()
    r, _, _, _, _ = kernel_points(data, None, (ix + 0.5)[None, :], (iy + 0.5)[:, None], SPLINE)
    assert np.abs(r - data[3:8, 3:8]).max() > 1.0   # the spline smooths: it does not interpolate


def test_centre_condition_bounds():
    """With the centre 2 x 2 kept, the worst drop pattern (every positive outer
    tap dropped) on a 64 x 64 grid of phases: Lanczos accW >= 0.79 and S / accW
    <= 2.75; spline accW >= 0.69.  Without the condition Lanczos' accW reaches 0."""
    t = np.arange(64) / 64.0
    for code in CODES:
        R = RADIUS[code]
        w = weights(code, t)
        w2 = w[:, None, :, None] * w[None, :, None, :]          # [ty, tx, j, i]
        centre = np.zeros((2 * R, 2 * R), bool)
        centre[R - 1:R + 1, R - 1:R + 1] = True
        keep = centre[None, None] | (w2 < 0.0)
        acc_w = np.where(keep, w2, 0.0).sum((-1, -2))
        s_abs = np.where(keep, np.abs(w2), 0.0).sum((-1, -2))
        if code == LANCZOS:
            assert acc_w.min() >= 0.79 and (s_abs / acc_w).max() <= 2.75, (acc_w.min(), (s_abs / acc_w).max())
            assert np.unravel_index(acc_w.argmin(), acc_w.shape) == (32, 32)
            # GDAL's unconditional renormalisation: dropping the centre instead leaves almost nothing
            assert np.abs(np.where(~centre[None, None], w2, 0.0).sum((-1, -2))).min() < 1e-3
        else:
            assert acc_w.min() >= 0.69 and abs(acc_w.min() - (2.0 / 3.0 + 1.0 / 6.0) ** 2) < 1e-15
            assert (w2 >= 0.0).all()
    # the same bound through kernel_points, with a random pattern on top
    rng = np.random.default_rng(52)
    data = rng.uniform(-1000.0, 1000.0, (12, 12))
    sx, sy = _phase_points(16, 3)
    for drop in _drop_patterns(3, rng, 12):
        _, _, kern, acc_w, s_abs = kernel_points(data, None, sx, sy, LANCZOS, drop)
        assert kern.all() and acc_w.min() >= 0.79 and (s_abs / acc_w).max() <= 2.75


def test_hand_over():
    """A nodata or out-of-band centre tap gives exactly `_rule`'s bilinear
    value: a 15 x 12 band with 15 % nodata under a 24 x 20 tile overhanging
    every edge, at 64 dyadic phases."""
    rng = np.random.default_rng(53)
    data = _noise(rng, 12, 15, 0.15)
    n_hand = n_kern = 0
    for code in CODES:
        for py, px in itertools.product(range(8), range(8)):
            g = _granule(data, 1.0, 4 + px / 8.0, 3 + py / 8.0)
            tile = _tile(24, 20)
            sample, has, kern, win, _, _ = kernel_grid(g.data, ND, g.geot, tile, code)
            bs, bh, _, bwin = _rule(g.data, ND, g.geot, tile)
            assert win == bwin
            assert np.array_equal(has[~kern], bh[~kern])
            sel = ~kern & bh
            assert np.array_equal(sample[sel], bs[sel])
            sx, sy = _coords(g, tile)
            fx, fy = np.floor(sx - 0.5)[None, :], np.floor(sy - 0.5)[:, None]
            inside = (fx >= 0) & (fx + 1 < 15) & (fy >= 0) & (fy + 1 < 12)
            assert not kern[~np.broadcast_to(inside, kern.shape)].any()
            assert (sample[kern] != bs[kern]).any() and has[kern].all()
            n_hand += int(sel.sum())
            n_kern += int(kern.sum())
    assert n_hand > 5000 and n_kern > 5000, (n_hand, n_kern)


def test_far_coordinates_take_no_sample():
    rng = np.random.default_rng(54)
    data = rng.uniform(-1000.0, 1000.0, (12, 12))
    bad = np.array([np.nan, np.inf, -np.inf, 1e300, -1e300, 3e9, -3e9])
    for code in CODES:
        for sx, sy in ((bad, np.full(bad.shape, 5.25)), (np.full(bad.shape, 5.25), bad), (bad, bad)):
            _, has, kern, _, _ = kernel_points(data, None, sx, sy, code)
            assert not has.any() and not kern.any()
        _, has, kern, _, _ = kernel_points(data, None, np.array([5.25]), np.array([6.75]), code)
        assert has.all() and kern.all()
