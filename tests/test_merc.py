"""Mercator on an ellipsoid (1SP / 2SP), and on a sphere with lat_ts != 0 or
k_0 != 1: host-side checks, no GPU and no oracle (the oracle knows only the
web-mercator sphere).

The product restates PROJ 6.1.1's merc.cpp.  It is pinned here by the worked
examples of EPSG Guidance Note 7-2 (variants A and B) and of Snyder (PP 1395,
Clarke 1866), and by the closed form written below from Snyder 7-7 / 7-8 --
not taken from the product's code.  Not compared with PROJ itself."""
import math

import numpy as np
import pytest

from gsky_amd import GskyError
from gsky_amd.tiles import crs_transform, parse_crs

from .test_equal_area import CLARKE, E_CRS, WGS84, _es, cf_srs, check_against, same_transform, wkt, wrap

VARIANT_A = "+proj=merc +a=6377397.155 +rf=299.1528128 +lon_0=110 +k_0=0.997 +x_0=3900000 +y_0=900000"
VARIANT_B = "+proj=merc +a=6378245 +rf=298.3 +lat_ts=42 +lon_0=51"


def snyder_merc(lon, lat, lon0, a, es, k0=1.0, lat_ts=None, x0=0.0, y0=0.0):
    """Snyder 7-6 / 7-7: y = a k0 (atanh(sin phi) - e atanh(e sin phi))."""
    lam = wrap(np.radians(np.asarray(lon, np.float64)) - math.radians(lon0))
    s = np.sin(np.radians(np.asarray(lat, np.float64)))
    e = math.sqrt(es)
    if lat_ts is not None:
        ps = math.radians(lat_ts)
        k0 = math.cos(ps) / math.sqrt(1.0 - es * math.sin(ps) ** 2)
    return x0 + a * k0 * lam, y0 + a * k0 * (np.arctanh(s) - e * np.arctanh(e * s))


EXAMPLES = [
    ("epsg_gn72_variant_a", VARIANT_A, 120.0, -3.0, 5009726.58, 569150.82, 0.01, 1e-7),
    ("epsg_gn72_variant_b", VARIANT_B, 53.0, 53.0, 165704.29, 5171848.07, 0.01, 1e-7),
    # the book's northing carries rounded intermediates: fp64 gives 4139145.655
    ("snyder_merc_ellipsoid", "+proj=merc %s +lon_0=180 +k_0=1" % CLARKE, -75.0, 35.0, 11688673.7, 4139145.6, 0.1, 1e-6),
]


@pytest.mark.parametrize("name,srs,lon,lat,ex,ey,bar,bar_deg", EXAMPLES, ids=[e[0] for e in EXAMPLES])
def test_published_worked_example(name, srs, lon, lat, ex, ey, bar, bar_deg):
    assert parse_crs(srs).kind == 10
    x, y, ok = crs_transform("EPSG:4326", srs, [lon], [lat])
    assert ok[0]
    print("%s forward: x %.4f y %.4f (published %r %r)" % (name, x[0], y[0], ex, ey))
    assert abs(x[0] - ex) <= bar and abs(y[0] - ey) <= bar
    lo, la, ok = crs_transform(srs, "EPSG:4326", [ex], [ey])
    assert ok[0]
    print("%s inverse: lon %.9f lat %.9f" % (name, lo[0], la[0]))
    assert abs(lo[0] - lon) <= bar_deg and abs(la[0] - lat) <= bar_deg


def test_variant_b_scale_factor():
    assert abs(parse_crs(VARIANT_B).k0 - 0.744260894) <= 5e-10   # the published k0, to its last digit


@pytest.mark.parametrize("name,srs,kw", [
    ("1sp_wgs84", "EPSG:3395", dict(lon0=0.0, a=WGS84[0], es=_es(WGS84[1]))),
    ("1sp_pdc", "EPSG:3832", dict(lon0=150.0, a=WGS84[0], es=_es(WGS84[1]))),
    ("1sp_k0", VARIANT_A, dict(lon0=110.0, a=6377397.155, es=_es(299.1528128), k0=0.997, x0=3900000.0, y0=900000.0)),
    ("2sp", VARIANT_B, dict(lon0=51.0, a=6378245.0, es=_es(298.3), lat_ts=42.0)),
    ("2sp_sphere", "+proj=merc +R=6371228 +lat_ts=30 +lon_0=-60", dict(lon0=-60.0, a=6371228.0, es=0.0, lat_ts=30.0)),
])
def test_merc_against_snyder(name, srs, kw):
    assert parse_crs(srs).kind == 10
    rng = np.random.default_rng(7)
    lon, lat = rng.uniform(-180, 180, 2000), rng.uniform(-85, 85, 2000)
    fx, fy = snyder_merc(lon, lat, **kw)
    check_against("merc " + name, srs, lon, lat, fx, fy)


# ---------------------------------------------------------------- failure rule, wrap
@pytest.mark.parametrize("srs", ["EPSG:3395", VARIANT_B, "+proj=merc +R=6371228 +lat_ts=30"])
def test_forward_fails_at_the_poles(srs):
    d = 1e-9
    x, y, ok = crs_transform("EPSG:4326", srs, [10.0] * 4, [90.0, -90.0, 90.0 - d, -90.0 + d])
    assert ok.tolist() == [False, False, True, True]
    assert np.isfinite(y[2:]).all() and y[2] > 0 > y[3]


def test_pdc_mercator_wraps_the_longitude_difference():
    """Central meridian 150 E: the antimeridian is inside the map."""
    x, y, ok = crs_transform("EPSG:4326", "EPSG:3832", [179.9, -179.9, 150.0, -30.0 + 1e-9], [0.0] * 4)
    assert ok.all()
    assert abs((x[1] - x[0]) - math.radians(0.2) * WGS84[0]) < 1e-6
    assert abs(x[2]) < 1e-9 and x[0] > 0 and x[1] > x[0]
    assert x[3] < 0   # just east of the map's own edge at 30 W
    lo, la, ok = crs_transform("EPSG:3832", "EPSG:4326", x[:2], y[:2])
    assert abs(lo[0] - 179.9) < 1e-9 and abs(lo[1] + 179.9) < 1e-9


# ---------------------------------------------------------------- parser
WEB_SPELLINGS = ["+proj=merc +a=6378137 +b=6378137 +lat_ts=0.0 +lon_0=0.0 +x_0=0.0 +y_0=0 +k=1.0 +units=m +nadgrids=@null "
                 "+wktext +no_defs", "+proj=merc +lon_0=0 +k=1 +x_0=0 +y_0=0 +R=6378137 +units=m +nadgrids=@null +no_defs"]


@pytest.mark.parametrize("srs", WEB_SPELLINGS + ["EPSG:3857", "+proj=webmerc +datum=WGS84"])
def test_web_mercator_spellings_keep_their_kind(srs):
    c, ref = parse_crs(srs), parse_crs("EPSG:3857")
    assert c.kind == 1 and c.es == 0.0 and c.a == 6378137.0 and c.k0 == 1.0 and c.lam0 == 0.0
    x, y, _ = crs_transform("EPSG:4326", srs, [151.2, -70.0], [-33.8, 60.0])
    xr, yr, _ = crs_transform("EPSG:4326", "EPSG:3857", [151.2, -70.0], [-33.8, 60.0])
    assert np.array_equal(x, xr) and np.array_equal(y, yr)
    assert bytes(c) == bytes(ref)


def test_cf_web_mercator_is_served_by_its_code_as_before(tmp_path):
    """The CF mercator mapping exactly as the netCDF writer records EPSG:3857
    (a sphere true to scale at the equator) is the web-mercator kind: from the
    CF attributes alone it stays unsupported, as before -- the file's EPSG
    code serves it (tests/test_netcdf_out.py) -- and never turns into kind 10."""
    from gsky_amd import ingest

    from .test_equal_area import DATA, grid_axes, write_cf_nc
    p = str(tmp_path / "w.nc")
    xs, ys, gt = grid_axes(4000000.0, 3000000.0)
    write_cf_nc(p, DATA, xs, ys, {"grid_mapping_name": "mercator", "standard_parallel": 0.0,
                                  "longitude_of_projection_origin": 0.0, "false_easting": 0.0, "false_northing": 0.0,
                                  "earth_radius": 6378137.0})
    assert ingest.netcdf_srs(p, 1) == "?"
    # the same sphere true to scale at 30 degrees is an ordinary Mercator
    write_cf_nc(p, DATA, xs, ys, {"grid_mapping_name": "mercator", "standard_parallel": 30.0,
                                  "longitude_of_projection_origin": 0.0, "false_easting": 0.0, "false_northing": 0.0,
                                  "earth_radius": 6378137.0})
    assert parse_crs(ingest.netcdf_srs(p, 1)).kind == 10


def test_parser_forms_agree(tmp_path):
    rng = np.random.default_rng(4)
    lon, lat = rng.uniform(-180, 180, 200), rng.uniform(-80, 80, 200)
    ell = {"semi_major_axis": WGS84[0], "inverse_flattening": WGS84[1], "false_easting": 0.0, "false_northing": 0.0}
    # 1SP: EPSG:3832
    cf = cf_srs(tmp_path, dict(ell, grid_mapping_name="mercator", longitude_of_projection_origin=150.0,
                               scale_factor_at_projection_origin=1.0), "a.nc")
    params = [("central_meridian", 150.0), ("scale_factor", 1.0), ("false_easting", 0.0), ("false_northing", 0.0)]
    for other in ("+proj=merc +lon_0=150 +k=1 +x_0=0 +y_0=0 +datum=WGS84 +units=m +no_defs",
                  "+proj=merc +lon_0=150 +k_0=1 +a=6378137 +rf=298.257223563", wkt("Mercator_1SP", params, *WGS84),
                  wkt("Mercator_1SP", [], 1.0, 0.0, authority=3832), cf):
        assert parse_crs(other).kind == 10
        same_transform("EPSG:3832", other, lon, lat)
    same_transform("EPSG:3395", "+proj=merc +lon_0=0 +k=1 +x_0=0 +y_0=0 +datum=WGS84 +units=m +no_defs", lon, lat)
    # a Mercator_1SP node that carries the web-mercator code stays web mercator
    assert parse_crs(wkt("Mercator_1SP", params, *WGS84, authority=3857)).kind == 1
    # 2SP: variant B
    cf = cf_srs(tmp_path, {"grid_mapping_name": "mercator", "longitude_of_projection_origin": 51.0, "standard_parallel": 42.0,
                           "false_easting": 0.0, "false_northing": 0.0, "semi_major_axis": 6378245.0,
                           "inverse_flattening": 298.3}, "b.nc")
    params = [("standard_parallel_1", 42.0), ("central_meridian", 51.0), ("false_easting", 0.0), ("false_northing", 0.0)]
    for other in (wkt("Mercator_2SP", params, 6378245.0, 298.3), cf, VARIANT_B.replace("+lat_ts=42", "+lat_ts=-42")):
        assert parse_crs(other).kind == 10
        same_transform(VARIANT_B, other, lon, lat)
    names = ("kind", "a", "es", "lam0", "phi0", "phi1", "phi2", "x0", "y0", "k0")
    key = lambda s: tuple(getattr(parse_crs(s), n) for n in names)
    assert len({key(s) for s in ("EPSG:3395", "EPSG:3832", VARIANT_A, VARIANT_B, "EPSG:3857")}) == 5


@pytest.mark.parametrize("srs", ["+proj=merc +lat_ts=90 +datum=WGS84", "+proj=merc +lat_ts=-90 +R=6371228",
                                 "+proj=merc +lat_ts=120 +datum=WGS84", "+proj=merc +k_0=0 +datum=WGS84",
                                 "+proj=merc +k_0=-0.5 +datum=WGS84"])
def test_parser_rejects(srs):
    with pytest.raises(GskyError) as e:
        parse_crs(srs)
    assert e.value.code == E_CRS
