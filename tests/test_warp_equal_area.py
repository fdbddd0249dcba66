"""Lambert azimuthal equal area, cylindrical equal area and ellipsoidal
Mercator granules (and destinations) through the warp, checked without the
oracle (it does not know these families), in the manner of
tests/test_warp_exact.py: granules hold values that name their element
(synth.index_granule), so each window value names the picked source pixel,
and the exact source coordinate of every tile pixel comes from the Snyder
formulations of tests/test_equal_area.py / tests/test_merc.py (not the
product's code).

Rules, per (tile, granule) pair:
  * a picked pixel lies within the approximate transformer's 0.125 px of the
    exact source position, and where it is not the exact cell, the exact
    position is within 0.125 px of a cell boundary;
  * nothing is picked where the exact transform fails;
  * every pixel whose exact source position is more than 1 px inside the
    granule is picked.
The share of neighbouring-cell picks and the worst distance are printed."""
import math

import numpy as np
import pytest

from gsky_amd import synth
from gsky_amd.tiles import bbox_to_geot, crs_transform

from .helpers import gpu_batch
from .test_equal_area import EASE_R, GRS80, WGS84, _es, snyder_cea, snyder_laea, write_cf_nc
from .test_merc import snyder_merc

pytestmark = pytest.mark.gpu

R_MERC = 6378137.0
ES84 = _es(WGS84[1])

# exact forward (lon, lat in degrees -> projected metres) of every source CRS used below
FORWARD = {
    "EPSG:3035": lambda lon, lat: snyder_laea(lon, lat, 52.0, 10.0, GRS80[0], _es(GRS80[1]), 4321000.0, 3210000.0),
    "EPSG:6931": lambda lon, lat: snyder_laea(lon, lat, 90.0, 0.0, WGS84[0], ES84),
    "EASE2N_45W": lambda lon, lat: snyder_laea(lon, lat, 90.0, -45.0, WGS84[0], ES84),
    "EPSG:6933": lambda lon, lat: snyder_cea(lon, lat, 30.0, 0.0, WGS84[0], ES84),
    "EPSG:3832": lambda lon, lat: snyder_merc(lon, lat, 150.0, WGS84[0], ES84),
    "EPSG:3395": lambda lon, lat: snyder_merc(lon, lat, 0.0, WGS84[0], ES84),
}
EASE2N_45W = "+proj=laea +lat_0=90 +lon_0=-45 +x_0=0 +y_0=0 +datum=WGS84 +units=m +no_defs"


def merc_inv(x, y):
    return np.degrees(x / R_MERC), np.degrees(np.arctan(np.sinh(y / R_MERC)))


def _pixel_centres(tile):
    bb, w, h = tile
    gt = bbox_to_geot(w, h, bb)
    jj, ii = np.mgrid[0:h, 0:w]
    return gt[0] + (ii + 0.5) * gt[1], gt[3] + (jj + 0.5) * gt[5]


def _exact_from_merc(cfg, t, fwd):
    """Exact source pixel coordinates of every pixel centre of EPSG:3857 tile t."""
    X, Y = _pixel_centres(cfg.tiles[t])
    lon, lat = merc_inv(X, Y)
    ax, ay = fwd(lon, lat)
    g = cfg.granules[0]
    return (ax - g.geot[0]) / g.geot[1], (ay - g.geot[3]) / g.geot[5], np.isfinite(ax) & np.isfinite(ay)


def _picked(win, w, h):
    """The window as a whole-tile array of picked values (-1: none)."""
    arr, (xoff, yoff, ww, hh), tname, nd = win
    assert tname == "Int16" and nd == -1.0
    v = np.full((h, w), -1, np.int64)
    if ww > 0 and hh > 0:
        v[yoff:yoff + hh, xoff:xoff + ww] = arr.cpu().numpy().astype(np.int64)
    return v


def _check_pair(cfg, t, win, sx, sy, valid, stats):
    bb, w, h = cfg.tiles[t]
    ny, nx = cfg.granules[0].data.shape
    v = _picked(win, w, h)
    ok = v >= 0
    assert not (ok & ~valid).any(), (t, "picked where the exact transform fails")
    with np.errstate(invalid="ignore"):
        sxz, syz = np.where(valid, sx, 0.0), np.where(valid, sy, 0.0)
        px, py = synth.index_decode(np.where(ok, v, 0), np.clip(sxz, -1e6, 1e6), np.clip(syz, -1e6, 1e6))
        dx = np.maximum(np.maximum(px - sxz, sxz - (px + 1)), 0.0)
        dy = np.maximum(np.maximum(py - syz, syz - (py + 1)), 0.0)
        assert not (ok & ((px < 0) | (py < 0) | (px >= nx) | (py >= ny))).any(), t
        if ok.any():
            stats["worst"] = max(stats["worst"], float(np.maximum(dx, dy)[ok].max()))
        tx, ty = np.floor(sxz + 1e-10), np.floor(syz + 1e-10)
        diff = ok & ((px != tx) | (py != ty))
        near = np.minimum(np.abs(sxz - np.round(sxz)), np.abs(syz - np.round(syz))) <= 0.125
    assert not (diff & ~near).any(), t
    need = valid & (sx > 1) & (sx < nx - 1) & (sy > 1) & (sy < ny - 1)
    stats["missing"] += int((need & ~ok).sum())
    stats["required"] += int(need.sum())
    stats["n_px"] += int(ok.sum())
    stats["n_diff"] += int(diff.sum())
    return v


def _stats():
    return dict(n_px=0, n_diff=0, worst=0.0, missing=0, required=0)


def _report(name, s):
    print("%s: %d px picked, %d (%.3f %%) another cell, worst %.4f px; %d required, %d missing" % (
        name, s["n_px"], s["n_diff"], 100.0 * s["n_diff"] / max(1, s["n_px"]), s["worst"], s["required"], s["missing"]))


def _run_source_case(name, cfg, fwd, gpu):
    b = gpu_batch(cfg, gpu)
    wins = b.warp_windows()
    assert b.status() == 0
    s = _stats()
    per_tile = []
    for t in range(len(cfg.tiles)):
        sx, sy, valid = _exact_from_merc(cfg, t, fwd)
        v = _check_pair(cfg, t, wins[t], sx, sy, valid, s)
        per_tile.append(int((v >= 0).sum()))
    _report(name, s)
    assert s["worst"] <= 0.125 + 1e-6, s
    assert s["missing"] == 0, s
    return s, per_tile


# ---------------------------------------------------------------- 1. oblique LAEA source
def test_oblique_laea_source(gpu):
    """One 1000^2 granule in EPSG:3035 at 1 km centred on 50 N 10 E under 3 x 3 EPSG:3857 tiles of 256^2."""
    cfg = synth.config_laea_europe()
    assert len(cfg.tiles) == 9 and cfg.granules[0].data.shape == (1000, 1000)
    s, per_tile = _run_source_case("oblique laea", cfg, FORWARD["EPSG:3035"], gpu)
    assert s["required"] > 200_000 and per_tile[4] == 256 * 256


# ---------------------------------------------------------------- 2. polar LAEA source
@pytest.mark.parametrize("srs,key", [("EPSG:6931", "EPSG:6931"), (EASE2N_45W, "EASE2N_45W")])
def test_polar_laea_source(gpu, srs, key):
    """The 25-km EASE-Grid 2.0 North grid under the four z1 world tiles.  In
    the two southern tiles the forward succeeds and lands outside the granule,
    but for the four corners of the square grid, which reach 12728 km from the
    pole (the south pole itself lies at 12742 km): there the exact transform
    decides, as everywhere."""
    cfg = synth.config_ease2_north(srs)
    assert cfg.granules[0].data.shape == (720, 720) and len(cfg.tiles) == 4
    s, per_tile = _run_source_case("polar laea " + key, cfg, FORWARD[key], gpu)
    assert min(per_tile[:2]) > 50_000
    for t in (2, 3):   # south: nothing but the corners of the grid
        sx, sy, valid = _exact_from_merc(cfg, t, FORWARD[key])
        inside = (sx > -0.125) & (sx < 720.125) & (sy > -0.125) & (sy < 720.125)
        print("south tile %d: %d px picked, %d px of the grid's corners" % (t, per_tile[t], int(inside.sum())))
        assert per_tile[t] <= int(inside.sum()) < 0.25 * 256 * 256


# ---------------------------------------------------------------- 3. CEA source
def test_cea_source(gpu):
    """The 36-km EASE-Grid 2.0 Global grid under the four z1 world tiles,
    whose top / bottom rows lie beyond 85.0445664 degrees."""
    cfg = synth.config_ease2_global()
    assert cfg.granules[0].data.shape == (406, 964)
    s, per_tile = _run_source_case("cea", cfg, FORWARD["EPSG:6933"], gpu)
    sx, sy, valid = _exact_from_merc(cfg, 0, FORWARD["EPSG:6933"])
    # the tile's top edge (85.0511) is above the grid's (85.0445664): the exact transform decides, row by row
    print("cea: source row of the first tile's top pixel centres %.4f (< 0: above the grid)" % float(sy[0].max()))
    assert min(per_tile) > 60_000 and s["required"] > 200_000


# ---------------------------------------------------------------- 4. Mercator across the antimeridian
def test_pdc_mercator_source_across_the_antimeridian(gpu):
    cfg = synth.config_pdc_mercator()
    assert cfg.granules[0].data.shape == (1024, 1024)
    assert abs(cfg.tiles[0][0][2] - 20037508.34) < 0.01 and abs(cfg.tiles[1][0][0] + 20037508.34) < 0.01
    s, per_tile = _run_source_case("pdc mercator", cfg, FORWARD["EPSG:3832"], gpu)
    assert min(per_tile) > 20_000, per_tile   # both tiles filled from the one granule


# ---------------------------------------------------------------- 5. new kinds as destination
def _dest_cfg(dst_srs):
    nx, ny, res = 2000, 1000, 0.05
    g = synth.SynthGranule(synth.index_granule(nx, ny), [-25.0, res, 0.0, 72.0, 0.0, -res], "EPSG:4326", -1.0, 1577836800.0)
    x, y, ok = crs_transform("EPSG:4326", dst_srs, [-5.0, 45.0, 20.0, 20.0], [50.0, 50.0, 35.0, 62.0])
    assert ok.all()
    cx, cy, half = 0.5 * (x[0] + x[1]), 0.5 * (y[2] + y[3]), 0.5 * (x[1] - x[0])
    tiles = synth._grid_tiles((cx - half, cy - half, cx + half, cy + half), 2, 2, 256)
    return synth.SynthConfig("DST", [g], dst_srs, tiles, [[0]] * 4, [""], (0.0, 0.0, 32761.0, 0), synth.PALETTE_GSKY)


@pytest.mark.parametrize("dst_srs", ["EPSG:3035", "EPSG:6933", "EPSG:3395"])
def test_new_kinds_as_destination(gpu, dst_srs):
    """A 2000 x 1000 longitude / latitude granule at 0.05 degree over Europe
    under tiles in the new CRS: the device inverse.  The longitude / latitude
    of a pixel centre is taken from the host inverse and checked against the
    formulation's forward before use (to the inverse's contract of 1e-3 m,
    1e-6 of the smallest source pixel here)."""
    cfg = _dest_cfg(dst_srs)
    g = cfg.granules[0]
    b = gpu_batch(cfg, gpu)
    wins = b.warp_windows()
    assert b.status() == 0
    s = _stats()
    for t in range(4):
        X, Y = _pixel_centres(cfg.tiles[t])
        lon, lat, ok = crs_transform(dst_srs, "EPSG:4326", X.ravel(), Y.ravel())
        if dst_srs != "EPSG:6933":   # (its upper tiles reach beyond the pole line: no inverse there)
            assert ok.all()
        assert ok.mean() > 0.8
        fx, fy = FORWARD[dst_srs](lon[ok], lat[ok])
        assert float(np.maximum(np.abs(fx - X.ravel()[ok]), np.abs(fy - Y.ravel()[ok])).max()) <= 1e-3
        sx = np.where(ok, (lon - g.geot[0]) / g.geot[1], np.nan).reshape(X.shape)
        sy = np.where(ok, (lat - g.geot[3]) / g.geot[5], np.nan).reshape(X.shape)
        _check_pair(cfg, t, wins[t], sx, sy, ok.reshape(X.shape), s)
    _report("destination " + dst_srs, s)
    assert s["worst"] <= 0.125 + 1e-6 and s["missing"] == 0, s
    assert s["required"] > 100_000


# ---------------------------------------------------------------- 6. bilinear
def test_bilinear_of_a_linear_field(gpu):
    """Bilinear interpolation of a linear field over case 1 is the field: at
    pixels at least 2 px inside the granule the value is a (sx - 0.5) + b (sy -
    0.5) to the approximate transformer's 0.125 px on each axis, plus float32
    rounding."""
    a, bq = 1.0, 0.5
    cfg = synth.config_laea_europe()
    g = cfg.granules[0]
    ny, nx = g.data.shape
    g.data = (a * np.arange(nx, dtype=np.float32)[None, :] + bq * np.arange(ny, dtype=np.float32)[:, None])
    assert g.data.max() < 1 << 22     # multiples of 0.5: exact
    wins = gpu_batch(cfg, gpu).warp_windows(resample=1)
    tol = 0.125 * (abs(a) + abs(bq)) + 4 * float(g.data.max()) * 2.0 ** -23
    n, worst = 0, 0.0
    for t, (bb, w, h) in enumerate(cfg.tiles):
        arr, (xoff, yoff, ww, hh), tname, nd = wins[t]
        assert tname == "Float32"
        sx, sy, valid = _exact_from_merc(cfg, t, FORWARD["EPSG:3035"])
        val = np.full((h, w), np.nan)
        val[yoff:yoff + hh, xoff:xoff + ww] = arr.cpu().numpy().astype(np.float64)
        inside = valid & (sx >= 2) & (sx <= nx - 2) & (sy >= 2) & (sy <= ny - 2)
        assert np.isfinite(val[inside]).all() and not (val[inside] == nd).any(), t
        err = np.abs(val - (a * (sx - 0.5) + bq * (sy - 0.5)))[inside]
        if err.size:
            worst = max(worst, float(err.max()))
        n += int(inside.sum())
    print("bilinear of a linear field: %d px, worst |error| %.4f (bound %.4f)" % (n, worst, tol))
    assert n > 100_000
    assert worst <= tol


# ---------------------------------------------------------------- 7. fused path, drop-in
@pytest.mark.parametrize("case", ["laea_europe", "ease2_global"])
def test_fused_render_equals_the_standalone_chain(gpu, case):
    """TileBatch.render (merge + scale + palette fused over the row records)
    equals warp_windows -> raster_merger_run -> scale -> palette of this
    library, bit for bit."""
    import gsky_amd
    cfg = synth.config_laea_europe() if case == "laea_europe" else synth.config_ease2_global()
    params, pal = gsky_amd.ScaleParams(*cfg.scale), gsky_amd.Palette(cfg.palette, True)
    b = gpu_batch(cfg, gpu)
    got = b.render(params, pal).cpu().numpy()
    assert b.status() == 0
    wins = b.warp_windows()
    g = cfg.granules[0]
    for t, (bb, w, h) in enumerate(cfg.tiles):
        arr, (xoff, yoff, ww, hh), tname, nd = wins[t]
        assert ww > 0 and hh > 0
        rasters = [gsky_amd.FlexRaster(arr, w, h, xoff, yoff, tname, nd, g.namespace, g.timestamp, g.polygon)]
        canvas, nod = gsky_amd.raster_merger_run(rasters, [""])[""]
        u8 = gsky_amd.scale([canvas], [nod], params)[0]
        exp = gsky_amd.encode_rgba([u8], pal).cpu().numpy()
        assert np.array_equal(got[t], exp), t
        assert (exp[..., 3] > 0).mean() > 0.2, t     # the tile shows data


def _drop_in_equals(gpu, cfg, t, path, srs=None, nodata=None, registered=True, srs_cf=0):
    import torch

    from gsky_amd import worker
    g = cfg.granules[0]
    b = gpu_batch(synth.subset(cfg, [t]), gpu)
    arr, bbox, tname, nd = b.warp_windows()[0]
    assert b.status() == 0
    bb, w, h = cfg.tiles[t]
    if registered:
        worker.register_granule(path, 1, torch.from_numpy(g.data).to(gpu), g.geot, srs or g.srs, g.nodata)
    try:
        res = worker.warp_raster(worker.GeoRPCGranule(path=path, bands=[1], width=w, height=h, dstSRS="EPSG:3857",
                                                      dstGeot=bbox_to_geot(w, h, bb), sRSCf=srs_cf))
        assert res.error == "OK", res.error
        assert res.raster.bbox == list(bbox)
        assert res.raster.rasterType == tname and res.raster.noData == nd
        exp = arr.cpu().numpy()
        assert worker.raster_array(res.raster).tobytes() == exp.tobytes()
        assert (exp >= 0).sum() > 1000
    finally:
        worker.unregister_all()


@pytest.mark.parametrize("srs", ["EPSG:6931", EASE2N_45W])
def test_worker_warp_raster_equals_warp_windows(gpu, srs):
    _drop_in_equals(gpu, synth.config_ease2_north(srs), 1, "/g/data/ease2/north.nc")


# ---------------------------------------------------------------- 8. ingest
def test_cf_netcdf_renders_as_the_registered_array(gpu, tmp_path):
    """A CF lambert_azimuthal_equal_area netCDF holding case 1's granule,
    opened by the drop-in's own ingest, renders identically to the same array
    under "EPSG:3035" (warp_windows, which the registered array equals too)."""
    cfg = synth.config_laea_europe()
    g = cfg.granules[0]
    g.nodata = -999.0   # write_cf_nc's _FillValue; the values are all >= 0
    ny, nx = g.data.shape
    p = str(tmp_path / "laea.nc")
    write_cf_nc(p, g.data, g.geot[0] + g.geot[1] * (np.arange(nx) + 0.5), g.geot[3] + g.geot[5] * (np.arange(ny) + 0.5),
                {"grid_mapping_name": "lambert_azimuthal_equal_area", "latitude_of_projection_origin": 52.0,
                 "longitude_of_projection_origin": 10.0, "false_easting": 4321000.0, "false_northing": 3210000.0,
                 "semi_major_axis": GRS80[0], "inverse_flattening": GRS80[1]})
    for t in (0, 4):
        _drop_in_equals(gpu, cfg, t, p, registered=False, srs_cf=1)
        _drop_in_equals(gpu, cfg, t, "/g/data/laea/registered.nc", srs="EPSG:3035")
