"""Geostationary (Himawari-like) granules through the warp, checked without
the oracle (it does not know this family), in the manner of
tests/test_warp_exact.py: granules hold their own pixel index as float32, so
each window value names the picked source pixel, and the exact source
coordinate of every tile pixel comes from the CGMS 4.4.3.2 formulation of
tests/test_geos.py (not the product's code).

This is the first family whose transform fails over large parts of ordinary
requests: scan angles off the disc have no longitude / latitude, ground
beyond the limb has no scan angle.  The limb tests drive whole tiles through
the planner's failed-point paths (SuggestedWarpOutput2's full-grid fallback,
exact rows whose end points fail, failed leaves).

Rim clipping: after failures the reference's SuggestedWarpOutput2 samples a
21 x 21 grid of the source; the window is the extent of the samples that
transform, so visible pixels beyond the outermost samples (about 0.91 of the
disc radius along the axes; beyond 64 degrees of latitude for the full disc)
may fall outside the window.  That is GDAL's
known behaviour on geostationary sources and is reproduced, not repaired: the
tests require every visible pixel within 0.8 of the disc radius, and allow
the rim to be missing."""
import math

import numpy as np
import pytest

from gsky_amd import synth
from gsky_amd.tiles import bbox_to_geot

from .helpers import gpu_batch
from .test_geos import H8, HIMAWARI, cgms

pytestmark = pytest.mark.gpu

R_MERC = 6378137.0
R_DISC = H8["h"] * math.asin(H8["r_eq"] / (H8["h"] + H8["r_eq"]))   # scan angle of the equatorial limb x h: ~5434 km
REGION = (-2700000.0, 100000.0)    # top-left of the regional granule: 4400 km over Australia, SW of the sub-satellite point


def merc_inv(x, y):
    return np.degrees(x / R_MERC), np.degrees(np.arctan(np.sinh(y / R_MERC)))


def merc_fwd(lon, lat):
    return R_MERC * math.radians(lon), R_MERC * math.asinh(math.tan(math.radians(lat)))


def _index_granules(cfg):
    for g in cfg.granules:   # each granule holds its pixel index
        ny, nx = g.data.shape
        assert nx * ny < 1 << 24
        g.data = np.arange(nx * ny, dtype=np.float32).reshape(ny, nx)
        g.nodata = -1.0
        g.overviews = []


def _exact(cfg, t, k):
    """Exact source pixel coordinates, visibility and visibility margin of
    every pixel centre of tile t against granule k."""
    bb, w, h = cfg.tiles[t]
    gt = bbox_to_geot(w, h, bb)
    g = cfg.granules[k]
    jj, ii = np.mgrid[0:h, 0:w]
    lon, lat = merc_inv(gt[0] + (ii + 0.5) * gt[1], gt[3] + (jj + 0.5) * gt[5])
    ax, ay, vis, margin = cgms(lon, lat, **H8)
    return (ax - g.geot[0]) / g.geot[1], (ay - g.geot[3]) / g.geot[5], vis, margin


def _picked(win, w, h):
    """The window as a whole-tile array of picked pixel indices (-1: none)."""
    arr, (xoff, yoff, ww, hh), tname, nd = win
    assert tname == "Float32"
    v = np.full((h, w), -1, np.int64)
    if ww > 0 and hh > 0:
        v[yoff:yoff + hh, xoff:xoff + ww] = arr.cpu().numpy().astype(np.int64)
    return v


def _check_pair(cfg, t, k, win, required, stats):
    """The pick rules of test_warp_exact._check_picks for one (tile, granule)
    pair, plus: nothing picked where the formulation says "not visible"
    (margins below 1e-12 excused, counted), every `required(sx, sy, vis)`
    pixel picked."""
    bb, w, h = cfg.tiles[t]
    ny, nx = cfg.granules[k].data.shape
    sx, sy, vis, margin = _exact(cfg, t, k)
    v = _picked(win, w, h)
    ok = v >= 0
    rounding = np.abs(margin) < 1e-12
    stats["excused"] += int((ok & ~vis & rounding).sum())
    assert not (ok & ~vis & ~rounding).any(), (t, k, "picked beyond the limb")
    okv = ok & vis
    px, py = v % nx, v // nx
    dx = np.maximum(np.maximum(px - sx, sx - (px + 1)), 0.0)
    dy = np.maximum(np.maximum(py - sy, sy - (py + 1)), 0.0)
    if okv.any():
        stats["worst"] = max(stats["worst"], float(np.maximum(dx, dy)[okv].max()))
    with np.errstate(invalid="ignore"):
        tx, ty = np.floor(sx + 1e-10), np.floor(sy + 1e-10)
        diff = okv & ((px != tx) | (py != ty))
        near = np.minimum(np.abs(sx - np.round(sx)), np.abs(sy - np.round(sy))) <= 0.125
    assert not (diff & ~near).any(), (t, k)
    need = required(sx, sy, vis & ~rounding)
    stats["missing"] += int((need & ~ok).sum())
    stats["required"] += int(need.sum())
    stats["n_px"] += int(okv.sum())
    stats["n_diff"] += int(diff.sum())
    # visible pixels of the granule that are not picked (reported, allowed): the rim clipping, and the
    # ring about 0.2 degrees wide where CGMS's visibility expression still holds but the point is past
    # the tangent limb, which is PROJ's rule and the product's
    inside = vis & (sx > 1) & (sy > 1) & (sx < nx - 1) & (sy < ny - 1)
    stats["clipped"] += int((inside & ~ok).sum())
    return v, sx, sy, vis


def _stats():
    return dict(n_px=0, n_diff=0, worst=0.0, excused=0, missing=0, required=0, clipped=0)


def _report(name, s):
    print("%s: %d px picked, %d (%.3f %%) another cell, worst %.4f px; %d required, %d missing; %d excused at the "
          "limb; %d visible granule pixels outside the windows" % (
              name, s["n_px"], s["n_diff"], 100.0 * s["n_diff"] / max(1, s["n_px"]), s["worst"], s["required"],
              s["missing"], s["excused"], s["clipped"]))


# ---------------------------------------------------------------- 1. regional
def _regional_cfg(n=2200, res=2000.0, tiles_per_side=6, origins=(REGION,)):
    return synth.config_geos(n=n, res=res, origins=list(origins), tiles_per_side=tiles_per_side, tile_px=256)


def _outline_sagitta_px(g):
    """SuggestedWarpOutput2 samples each source edge at twentieths: the worst
    distance, in source pixels, between the true outline in EPSG:3857 and the
    chord of two neighbouring samples (what its hull falls short by)."""
    from gsky_amd.tiles import crs_transform   # only to go from the granule's edge to longitude / latitude ...
    ny, nx = g.data.shape
    worst = 0.0
    for edge in range(4):
        for s in range(20):
            u = (s + np.linspace(0.0, 1.0, 17)) / 20.0
            px = {0: u * nx, 1: u * nx, 2: np.zeros(17), 3: np.full(17, float(nx))}[edge]
            py = {0: np.zeros(17), 1: np.full(17, float(ny)), 2: u * ny, 3: u * ny}[edge]
            lon, lat, ok = crs_transform(g.srs, "EPSG:4326", g.geot[0] + px * g.geot[1], g.geot[3] + py * g.geot[5])
            assert ok.all()
            # ... checked against the formulation before use
            fx, fy, vis, _ = cgms(lon, lat, **H8)
            assert vis.all() and np.abs(fx - (g.geot[0] + px * g.geot[1])).max() < 1e-3
            m = np.array([merc_fwd(a, b) for a, b in zip(lon, lat)])
            a, b = m[0], m[-1]
            tt = np.clip(((m - a) @ (b - a)) / ((b - a) @ (b - a)), 0.0, 1.0)
            foot = a + tt[:, None] * (b - a)                 # nearest chord point of every outline point
            flon, flat = merc_inv(foot[:, 0], foot[:, 1])
            cx, cy, _, _ = cgms(flon, flat, **H8)            # ... back in source pixels
            d = np.hypot((cx - g.geot[0]) / g.geot[1] - px, (cy - g.geot[3]) / g.geot[5] - py)
            worst = max(worst, float(d.max()))
    return worst


def test_regional_granule_picks_and_completeness(gpu):
    """2200^2 at 2 km over Australia (well inside the disc: its farthest
    corner at 0.94 of the disc radius), 6 x 6 EPSG:3857 tiles of 256^2."""
    cfg = _regional_cfg()
    g = cfg.granules[0]
    n = g.data.shape[0]
    far = max(math.hypot(x, y) for x in (REGION[0], REGION[0] + n * 2000.0) for y in (REGION[1], REGION[1] - n * 2000.0))
    assert far / R_DISC < 0.95
    sag = _outline_sagitta_px(g)
    print("outline sagitta over a twentieth of an edge: %.2f px of %d (%.3f %% of the side)" % (sag, n, 100.0 * sag / n))
    assert sag < 0.005 * n          # far below the 5 % margin of the completeness rule
    assert len(cfg.tiles) == 36 and all(ks == [0] for ks in cfg.pairs)
    _index_granules(cfg)
    wins = gpu_batch(cfg, gpu).warp_windows()
    s = _stats()
    m = 0.05 * n
    for t in range(len(cfg.tiles)):
        _check_pair(cfg, t, 0, wins[t], lambda sx, sy, vis: vis & (sx > m) & (sx < n - m) & (sy > m) & (sy < n - m), s)
    _report("regional", s)
    assert s["n_px"] > 300_000, s
    assert s["worst"] <= 0.125 + 1e-6, s
    assert s["n_diff"] / s["n_px"] < 0.15
    assert s["excused"] == 0
    assert s["required"] > 250_000 and s["missing"] == 0, s


# ---------------------------------------------------------------- 2. limb
Z2_FAR = (2, 1, 1)   # 90 W .. 0, 0 .. 66.5 N: wholly on the far side of the Earth from 140.7 E


def _limb_cfg(tiles):
    cfg = synth.config_geos(n=1100, res=10000.0, tiles=tiles)
    cfg.pairs = [[0] for _ in tiles]   # the indexer's footprint is the whole world (the disc crosses 180): every tile
    return cfg


def _limb_required(sx, sy, vis):
    with np.errstate(invalid="ignore"):
        return vis & (np.hypot(sx - 550.0, sy - 550.0) * 10000.0 <= 0.8 * R_DISC)


def test_limb_sample_geometry():
    """(CPU) The 21 x 21 fallback grid of a 1100-pixel granule at 10 km has
    its samples 550 km apart: along the axes the outermost visible ones sit at
    0.91 of the disc radius and the next ring at 0.81, so a required radius of
    0.8 is inside the sampled extent even without the outer ring."""
    from gsky_amd.tiles import crs_transform
    step = 1100 / 20 * 10000.0
    assert 5.43e6 < R_DISC < 5.44e6 and 5500000.0 > R_DISC
    x = np.arange(-10, 11) * step
    _, _, ok = crs_transform(HIMAWARI, "EPSG:4326", x, np.zeros(21))
    assert ok.tolist() == [abs(k) <= 9 for k in range(-10, 11)]
    _, _, ok = crs_transform(HIMAWARI, "EPSG:4326", np.zeros(21), x)
    assert ok.tolist() == [abs(k) <= 9 for k in range(-10, 11)]
    assert 0.90 < 9 * step / R_DISC < 0.92 and 0.80 < 8 * step / R_DISC < 0.82


LIMB_TILES = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 0, 1), (1, 1, 1), Z2_FAR]


def test_limb_tiles_have_no_pixel_on_the_limb():
    """(CPU) At most 16 pixels of the limb tests may be excused as rounding
    (|visibility margin| < 1e-12): the chosen tiles have none."""
    cfg = _limb_cfg([(synth._webmerc_tile_bbox(*z), 256, 256) for z in LIMB_TILES])
    n = 0
    for t in range(len(cfg.tiles)):
        n += int((np.abs(_exact(cfg, t, 0)[3]) < 1e-12).sum())
    assert n <= 16
    assert n == 0


@pytest.mark.parametrize("z,x,y", LIMB_TILES[:5])
def test_limb_full_disc_world_tiles(gpu, z, x, y):
    """One full-disc granule of 1100^2 at 10 km (+-5500 km: corners and rims
    are space) under the z0 world tile and each of the four z1 tiles.

    The disc crosses the antimeridian: PROJ wraps the fallback grid's
    easternmost samples to -179.26 degrees, and the plain minimum of the
    samples' destination x would start the window of the two western z1 tiles
    at pixel 1.06, leaving column 0 (longitude -179.65, half a disc radius
    from the centre: 39 of their 269 required pixels each) outside it.  The
    planner closes the x extent to the destination's periodic edges in that
    case (plan.hip geos_seam), so these tiles hold the rule too.  MI355X:
    z0 3890 required, east tiles 7499, west tiles 269, none missing."""
    cfg = _limb_cfg([(synth._webmerc_tile_bbox(z, x, y), 256, 256)])
    _index_granules(cfg)
    b = gpu_batch(cfg, gpu)
    wins = b.warp_windows()
    assert b.status() == 0
    s = _stats()
    v, sx, sy, vis = _check_pair(cfg, 0, 0, wins[0], _limb_required, s)
    _report("limb z%d (%d, %d), window %s" % (z, x, y, wins[0][1]), s)
    assert (v >= 0).sum() > 1000          # every one of these tiles sees part of the disc
    assert s["worst"] <= 0.125 + 1e-6, s
    assert s["excused"] <= 16
    assert s["required"] > 200 and s["missing"] == 0, s


def test_limb_far_side_tile_is_nodata(gpu):
    """A tile on the far side of the Earth returns only nodata, status 0.
    (With the sub-satellite point at 140.7 E every z1 tile reaches the
    antimeridian, which is on the disc; the far side starts at z2.)"""
    cfg = _limb_cfg([(synth._webmerc_tile_bbox(*Z2_FAR), 256, 256)])
    assert not _exact(cfg, 0, 0)[2].any()
    _index_granules(cfg)
    b = gpu_batch(cfg, gpu)
    wins = b.warp_windows()
    assert b.status() == 0
    arr, bbox, tname, nd = wins[0]
    assert nd == -1.0 and (arr.cpu().numpy() == -1.0).all()
    # ... and through the fused path: every canvas pixel nodata -> transparent
    import gsky_amd
    rgba = b.render(gsky_amd.ScaleParams(0.0, 0.0, 1000.0, 0), gsky_amd.Palette(cfg.palette, True)).cpu().numpy()
    assert b.status() == 0
    assert (rgba[..., 3] == 0).all()


# ---------------------------------------------------------------- 3. narrow windows
def test_limb_narrow_window_exact_path(gpu):
    """A window of 5 columns across the limb, which the planner transforms
    exactly (n <= 5).  (The disc crosses the antimeridian, so the x extent of
    the transformed samples is the whole world and a window is as wide as its
    tile: the tile itself is 5 pixels of one degree, 84 to 79 degrees west of
    the sub-satellite point, 20 S to 20 N; the limb is at 81.3 on the equator.)"""
    x0, y0 = merc_fwd(H8["lon0"] - 84.0, -20.0)
    x1, y1 = merc_fwd(H8["lon0"] - 79.0, 20.0)
    cfg = _limb_cfg([((x0, y0, x1, y1), 5, 256)])
    _index_granules(cfg)
    b = gpu_batch(cfg, gpu)
    wins = b.warp_windows()
    assert b.status() == 0
    xoff, yoff, ww, hh = wins[0][1]
    print("narrow window: x %d, y %d, %d x %d" % (xoff, yoff, ww, hh))
    assert (xoff, ww) == (0, 5) and hh > 200
    s = _stats()
    v, sx, sy, vis = _check_pair(cfg, 0, 0, wins[0], _limb_required, s)
    _report("narrow", s)
    assert s["worst"] <= 0.125 + 1e-6 and s["missing"] == 0 and s["excused"] <= 16
    # columns 0-1 are beyond the limb in every row, columns 3-4 on the disc and inside the granule
    assert not vis[:, :2].any() and vis[:, 3:].all()
    assert (v[yoff:yoff + hh, :2] == -1).all()
    assert (v[yoff:yoff + hh, 3:] >= 0).all()


def test_limb_rows_that_begin_off_the_disc(gpu):
    """A tile from 80 to 40 degrees west of the sub-satellite point at 56-64 N,
    where the limb lies 72-75 degrees away: every window row begins beyond the
    limb and ends on the disc, so its first end point fails."""
    x0, y0 = merc_fwd(H8["lon0"] - 80.0, 56.0)
    x1, y1 = merc_fwd(H8["lon0"] - 40.0, 64.0)
    cfg = _limb_cfg([((x0, y0, x1, y1), 256, 128)])
    _index_granules(cfg)
    b = gpu_batch(cfg, gpu)
    wins = b.warp_windows()
    assert b.status() == 0
    xoff, yoff, ww, hh = wins[0][1]
    s = _stats()
    v, sx, sy, vis = _check_pair(cfg, 0, 0, wins[0], _limb_required, s)
    _report("rows off-disc", s)
    wvis = vis[yoff:yoff + hh, xoff:xoff + ww]
    rows = ~wvis[:, 0] & wvis[:, -1]
    print("window %d x %d at (%d, %d): %d rows begin off the disc and end on it" % (ww, hh, xoff, yoff, int(rows.sum())))
    assert rows.sum() >= 100
    assert s["worst"] <= 0.125 + 1e-6 and s["missing"] == 0
    assert s["n_px"] > 2000 and s["excused"] <= 16
    # in those rows pixels are picked on the disc, none beyond the limb (asserted in _check_pair)
    assert ((v[yoff:yoff + hh, xoff:xoff + ww] >= 0) & wvis)[rows].any(axis=1).all()


# ---------------------------------------------------------------- 4. bilinear
def test_regional_bilinear_of_a_linear_field(gpu):
    """Bilinear interpolation of a linear field is the field: at pixels at
    least 2 px inside the granule the value is a (sx - 0.5) + b (sy - 0.5) to
    the approximate transformer's 0.125 px on each axis, plus float32 rounding."""
    a, bq = 1.0, 0.5
    cfg = _regional_cfg(tiles_per_side=3)
    g = cfg.granules[0]
    ny, nx = g.data.shape
    g.data = (a * np.arange(nx, dtype=np.float32)[None, :] + bq * np.arange(ny, dtype=np.float32)[:, None])
    assert g.data.dtype == np.float32 and g.data.max() < 1 << 22     # multiples of 0.5: exact
    g.nodata = -1.0
    g.overviews = []
    wins = gpu_batch(cfg, gpu).warp_windows(resample=1)
    tol = 0.125 * (abs(a) + abs(bq)) + 4 * float(g.data.max()) * 2.0 ** -23
    n = 0
    worst = 0.0
    for t, (bb, w, h) in enumerate(cfg.tiles):
        arr, (xoff, yoff, ww, hh), tname, nd = wins[t]
        assert tname == "Float32"
        sx, sy, vis, _ = _exact(cfg, t, 0)
        val = np.full((h, w), np.nan)
        val[yoff:yoff + hh, xoff:xoff + ww] = arr.cpu().numpy().astype(np.float64)
        inside = vis & (sx >= 2) & (sx <= nx - 2) & (sy >= 2) & (sy <= ny - 2) & np.isfinite(val)
        assert not (val[inside] == nd).any(), t
        err = np.abs(val - (a * (sx - 0.5) + bq * (sy - 0.5)))[inside]
        if err.size:
            worst = max(worst, float(err.max()))
        n += int(inside.sum())
    print("bilinear of a linear field: %d px, worst |error| %.4f (bound %.4f)" % (n, worst, tol))
    assert n > 100_000
    assert worst <= tol


# ---------------------------------------------------------------- 5. fused path
def test_fused_render_equals_the_standalone_chain(gpu):
    """TileBatch.render (merge + scale + palette fused over the row records)
    over two overlapping regional granules equals warp_windows ->
    raster_merger_run -> scale -> palette of this library, bit for bit."""
    import gsky_amd
    x0, y0 = merc_fwd(112.0, -38.0)
    x1, y1 = merc_fwd(150.0, -12.0)
    span = max(x1 - x0, y1 - y0) / 2
    tiles = [((x0 + i * span, y1 - (j + 1) * span, x0 + (i + 1) * span, y1 - j * span), 256, 256)
             for j in range(2) for i in range(2)]
    cfg = synth.config_geos(n=1100, res=4000.0, origins=[REGION, (REGION[0] + 400000.0, REGION[1] - 200000.0)], tiles=tiles)
    assert all(ks == [0, 1] for ks in cfg.pairs)
    params, pal = gsky_amd.ScaleParams(*cfg.scale), gsky_amd.Palette(cfg.palette, True)
    b = gpu_batch(cfg, gpu)
    got = b.render(params, pal).cpu().numpy()
    assert b.status() == 0
    wins = b.warp_windows()
    p = 0
    for t, ((bb, w, h), ks) in enumerate(zip(cfg.tiles, cfg.pairs)):
        rasters = []
        for k in ks:
            arr, (xoff, yoff, ww, hh), tname, nd = wins[p]
            p += 1
            assert ww > 0 and hh > 0
            g = cfg.granules[k]
            rasters.append(gsky_amd.FlexRaster(arr, w, h, xoff, yoff, tname, nd, g.namespace, g.timestamp, g.polygon))
        canvas, nod = gsky_amd.raster_merger_run(rasters, [""])[""]
        u8 = gsky_amd.scale([canvas], [nod], params)[0]
        exp = gsky_amd.encode_rgba([u8], pal).cpu().numpy()
        assert np.array_equal(got[t], exp), t
        assert (exp[..., 3] > 0).mean() > 0.2, t     # the tile shows data
    # the west tiles reach beyond the granules: part of them stays transparent
    assert (got[0][..., 3] == 0).any()


# ---------------------------------------------------------------- 6. drop-in
@pytest.mark.parametrize("case", ["regional", "limb"])
def test_worker_warp_raster_equals_warp_windows(gpu, case):
    import torch

    from gsky_amd import worker
    if case == "regional":
        cfg = _regional_cfg(n=1100, res=4000.0, tiles_per_side=3)
        t = 4
    else:
        cfg = _limb_cfg([(synth._webmerc_tile_bbox(1, 1, 1), 256, 256)])
        t = 0
    _index_granules(cfg)
    g = cfg.granules[0]
    b = gpu_batch(synth.subset(cfg, [t]), gpu)
    arr, bbox, tname, nd = b.warp_windows()[0]
    assert b.status() == 0
    bb, w, h = cfg.tiles[t]
    path = "/g/data/himawari8/%s.nc" % case
    worker.register_granule(path, 1, torch.from_numpy(g.data).to(gpu), g.geot, g.srs, g.nodata)
    try:
        res = worker.warp_raster(worker.GeoRPCGranule(path=path, bands=[1], width=w, height=h, dstSRS="EPSG:3857",
                                                      dstGeot=bbox_to_geot(w, h, bb)))
        assert res.error == "OK", res.error
        assert res.raster.bbox == list(bbox)
        assert res.raster.rasterType == tname and res.raster.noData == nd
        got = worker.raster_array(res.raster)
        exp = arr.cpu().numpy()
        assert got.tobytes() == exp.tobytes()
        assert (exp >= 0).sum() > 1000
    finally:
        worker.unregister_all()
