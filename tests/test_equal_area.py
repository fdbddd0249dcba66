"""Lambert azimuthal equal area (+proj=laea) and cylindrical equal area
(+proj=cea) on an ellipsoid or a sphere: host-side checks, no GPU and no
oracle (the oracle does not know these families).  Mercator: tests/test_merc.py.

The product restates PROJ 6.1.1's laea.cpp / cea.cpp.  It is pinned here by
  * published worked examples: EPSG Guidance Note 7-2 (EPSG:3035), Snyder's
    Map Projections -- A Working Manual (PP 1395; LAEA ellipsoid and sphere,
    CEA ellipsoid), and the EASE-Grid 2.0 definition (Brodzik et al. 2012:
    the global grid's half extents), and
  * an independent formulation written below from Snyder's equations -- q
    (3-12), the authalic latitude beta (3-11), Rq (3-13), D and B (24-19,
    24-20) -- not taken from the product's code.
Not compared with PROJ itself.  The inverse is more exact than PROJ 6.1.1's
three-term authalic series by design (round trip within a millimetre)."""
import json
import math

import numpy as np
import pytest

from gsky_amd import GskyError, ingest
from gsky_amd.tiles import crs_transform, parse_crs

E_CRS = -4
GRS80 = (6378137.0, 298.257222101)
WGS84 = (6378137.0, 298.257223563)
EASE_R = 6371228.0
CLARKE = "+a=6378206.4 +es=0.00676866"


def _es(rf):
    return 0.0 if rf == 0 else (2.0 - 1.0 / rf) / rf


def wrap(dlam):
    """Longitude difference in radians to (-pi, pi]."""
    return -((-dlam + np.pi) % (2 * np.pi) - np.pi)


def q_of(phi, es):
    """Snyder 3-12, with the logarithm written as an inverse hyperbolic tangent."""
    s = np.sin(phi)
    if es == 0:
        return 2.0 * s
    e = math.sqrt(es)
    return (1.0 - es) * (s / (1.0 - es * s * s) + np.arctanh(e * s) / e)


def snyder_laea(lon, lat, lat0, lon0, a, es, x0=0.0, y0=0.0):
    """Snyder section 24: sphere 24-2 .. 24-4 (k'), ellipsoid 24-17 .. 24-25."""
    lam = wrap(np.radians(np.asarray(lon, np.float64)) - math.radians(lon0))
    phi = np.radians(np.asarray(lat, np.float64))
    p1 = math.radians(lat0)
    if es == 0:
        kp = np.sqrt(2.0 / (1.0 + math.sin(p1) * np.sin(phi) + math.cos(p1) * np.cos(phi) * np.cos(lam)))
        return (x0 + a * kp * np.cos(phi) * np.sin(lam),
                y0 + a * kp * (math.cos(p1) * np.sin(phi) - math.sin(p1) * np.cos(phi) * np.cos(lam)))
    qp = float(q_of(np.float64(math.pi / 2), es))
    q = q_of(phi, es)
    if abs(lat0) == 90.0:   # 24-23 / 24-25
        rho = a * np.sqrt(qp - q if lat0 > 0 else qp + q)
        return x0 + rho * np.sin(lam), y0 + (-rho if lat0 > 0 else rho) * np.cos(lam)
    beta = np.arcsin(q / qp)
    b1 = math.asin(float(q_of(np.float64(p1), es)) / qp)
    Rq = a * math.sqrt(qp / 2.0)
    m1 = math.cos(p1) / math.sqrt(1.0 - es * math.sin(p1) ** 2)
    D = a * m1 / (Rq * math.cos(b1))
    B = Rq * np.sqrt(2.0 / (1.0 + math.sin(b1) * np.sin(beta) + math.cos(b1) * np.cos(beta) * np.cos(lam)))
    return (x0 + B * D * np.cos(beta) * np.sin(lam),
            y0 + (B / D) * (math.cos(b1) * np.sin(beta) - math.sin(b1) * np.cos(beta) * np.cos(lam)))


def snyder_cea(lon, lat, lat_ts, lon0, a, es, x0=0.0, y0=0.0):
    """Snyder section 10: 10-1 / 10-2 (sphere), 10-13 .. 10-15 (ellipsoid)."""
    lam = wrap(np.radians(np.asarray(lon, np.float64)) - math.radians(lon0))
    phi = np.radians(np.asarray(lat, np.float64))
    ps = math.radians(lat_ts)
    k0 = math.cos(ps) / math.sqrt(1.0 - es * math.sin(ps) ** 2)
    return x0 + a * k0 * lam, y0 + a * q_of(phi, es) / (2.0 * k0)


# ---------------------------------------------------------------- published worked examples
EXAMPLES = [
    # name, srs, lon, lat, x, y, bar on x / y, bar on lon / lat in degrees
    ("epsg_gn72_laea", "EPSG:3035", 5.0, 50.0, 3962799.45, 2999718.85, 0.01, 1e-7),
    ("snyder_laea_ellipsoid", "+proj=laea %s +lat_0=40 +lon_0=-100" % CLARKE, -110.0, 30.0, -965932.1, -1056814.9,
     0.1, 1e-6),
    ("snyder_laea_sphere", "+proj=laea +R=3 +lat_0=40 +lon_0=-100", 100.0, -20.0, -4.2339303, 4.0257775, 1e-7, 1e-6),
    ("snyder_cea_ellipsoid", "+proj=cea %s +lat_ts=5 +lon_0=-75" % CLARKE, -78.0, -5.0, -332699.8, -554248.5, 0.1,
     1e-6),
    ("ease2_global_half_extent", "EPSG:6933", 180.0, 85.0445664, 17367530.45, 7314540.83, 0.02, 1e-7),
]


@pytest.mark.parametrize("name,srs,lon,lat,ex,ey,bar,bar_deg", EXAMPLES, ids=[e[0] for e in EXAMPLES])
def test_published_worked_example(name, srs, lon, lat, ex, ey, bar, bar_deg):
    x, y, ok = crs_transform("EPSG:4326", srs, [lon], [lat])
    assert ok[0]
    print("%s forward: x %.7f y %.7f (published %r %r)" % (name, x[0], y[0], ex, ey))
    assert abs(x[0] - ex) <= bar and abs(y[0] - ey) <= bar
    lo, la, ok = crs_transform(srs, "EPSG:4326", [ex], [ey])
    assert ok[0]
    # 180 E and 180 W are one meridian: the rounded half extent lies a millimetre beyond it
    dlon = (lo[0] - lon + 180.0) % 360.0 - 180.0
    print("%s inverse: lon %.9f lat %.9f" % (name, lo[0], la[0]))
    assert abs(dlon) <= bar_deg and abs(la[0] - lat) <= bar_deg


# ---------------------------------------------------------------- the formulation
def points_around(lat0, lon0, n=2000, max_angle=150.0, seed=24):
    """n seeded longitude / latitude points within max_angle degrees of arc of (lat0, lon0)."""
    rng = np.random.default_rng(seed)
    ang = np.radians(max_angle) * np.sqrt(rng.uniform(0, 1, n))
    az = rng.uniform(0, 2 * np.pi, n)
    p0 = math.radians(lat0)
    lat = np.arcsin(np.clip(math.sin(p0) * np.cos(ang) + math.cos(p0) * np.sin(ang) * np.cos(az), -1, 1))
    lon = np.arctan2(np.sin(az) * np.sin(ang) * math.cos(p0), np.cos(ang) - math.sin(p0) * np.sin(lat))
    return (lon0 + np.degrees(lon) + 180.0) % 360.0 - 180.0, np.degrees(lat)


def check_against(name, srs, lon, lat, fx, fy):
    """Forward against the formulation to 1e-6 m (both closed forms in fp64 at
    up to 2e7 m), fwd(inv) to 1e-3 m, inv(fwd) to 1e-8 degree."""
    x, y, ok = crs_transform("EPSG:4326", srs, lon, lat)
    assert ok.all()
    err = float(np.maximum(np.abs(x - fx), np.abs(y - fy)).max())
    lo2, la2, ok2 = crs_transform(srs, "EPSG:4326", x, y)
    assert ok2.all()
    x2, y2, ok3 = crs_transform("EPSG:4326", srs, lo2, la2)
    assert ok3.all()
    rt_m = float(np.maximum(np.abs(x2 - x), np.abs(y2 - y)).max())
    rt_deg = float(np.maximum(np.abs((lo2 - lon + 180.0) % 360.0 - 180.0), np.abs(la2 - lat)).max())
    print("%s: forward vs formulation %.3e m, fwd(inv) %.3e m, inv(fwd) %.3e deg over %d points" % (
        name, err, rt_m, rt_deg, lon.size))
    assert err <= 1e-6
    assert rt_m <= 1e-3
    assert rt_deg <= 1e-8


LAEA_CASES = [(lat0, ell) for lat0 in (90.0, -90.0, 0.0, 52.0) for ell in ("GRS80", "sphere")]


@pytest.mark.parametrize("lat0,ell", LAEA_CASES)
def test_laea_against_snyder(lat0, ell):
    a, rf = GRS80 if ell == "GRS80" else (EASE_R, 0.0)
    lon0 = 10.0
    srs = "+proj=laea +lat_0=%r +lon_0=%r +x_0=4321000 +y_0=3210000 %s" % (
        lat0, lon0, "+ellps=GRS80" if ell == "GRS80" else "+R=%r" % a)
    assert parse_crs(srs).kind == 8
    lon, lat = points_around(lat0, lon0)
    fx, fy = snyder_laea(lon, lat, lat0, lon0, a, _es(rf), 4321000.0, 3210000.0)
    check_against("laea %g %s" % (lat0, ell), srs, lon, lat, fx, fy)


@pytest.mark.parametrize("ell", ["WGS84", "sphere"])
@pytest.mark.parametrize("lat_ts", [0.0, 30.0])
def test_cea_against_snyder(ell, lat_ts):
    a, rf = WGS84 if ell == "WGS84" else (EASE_R, 0.0)
    srs = "+proj=cea +lat_ts=%r +lon_0=0 %s" % (lat_ts, "+datum=WGS84" if ell == "WGS84" else "+R=%r" % a)
    assert parse_crs(srs).kind == 9
    rng = np.random.default_rng(10)
    lon, lat = rng.uniform(-180, 180, 2000), rng.uniform(-89.9, 89.9, 2000)
    fx, fy = snyder_cea(lon, lat, lat_ts, 0.0, a, _es(rf))
    check_against("cea %g %s" % (lat_ts, ell), srs, lon, lat, fx, fy)


def test_polar_inverse_next_to_the_pole():
    """The polar inverse takes the authalic colatitude by its half angle, so it
    loses nothing next to the pole; the forward keeps PROJ's qp - q, whose
    rounding is about 3 cm over the distance from the pole in metres: from 50 m
    on, a point comes back to a millimetre."""
    for srs in ("EPSG:6931", "EPSG:6932", "EPSG:3408"):
        x = np.array([200.0, 0.0, -30.0, 1000.0, 0.0])
        y = np.array([0.0, -100.0, 40.0, 1000.0, 0.0])
        lo, la, ok = crs_transform(srs, "EPSG:4326", x, y)
        assert ok.all()
        assert abs(abs(la[4]) - 90.0) < 1e-12
        x2, y2, ok = crs_transform("EPSG:4326", srs, lo, la)
        assert ok.all()
        assert float(np.maximum(np.abs(x2 - x), np.abs(y2 - y)).max()) <= 1e-3


# ---------------------------------------------------------------- failure rules
SHORT = 1e-9   # degrees


@pytest.mark.parametrize("srs,lat0,lon0", [("EPSG:3035", 52.0, 10.0), ("EPSG:6931", 90.0, 0.0), ("EPSG:6932", -90.0, 0.0),
                                           ("EPSG:3408", 90.0, 0.0), ("+proj=laea +lat_0=0 +lon_0=10 +ellps=GRS80", 0.0, 10.0),
                                           ("+proj=laea +lat_0=52 +lon_0=10 +R=6371228", 52.0, 10.0)])
def test_laea_forward_fails_at_the_antipode(srs, lat0, lon0):
    alon, alat = lon0 - 180.0, -lat0
    near = alat + SHORT if alat < 0 else alat - SHORT
    x, y, ok = crs_transform("EPSG:4326", srs, [alon, alon, lon0], [alat, near, lat0])
    assert ok.tolist() == [False, True, True]
    assert np.isfinite(x[1:]).all() and np.isfinite(y[1:]).all()
    if abs(lat0) == 90.0:   # any longitude at the opposite pole
        assert not crs_transform("EPSG:4326", srs, [33.0], [alat])[2][0]


@pytest.mark.parametrize("srs,a,rf,lat0", [("EPSG:3035", 6378137.0, 298.257222101, 52.0), ("EPSG:6931", 6378137.0, 298.257223563, 90.0),
                                           ("EPSG:3409", EASE_R, 0.0, -90.0),
                                           ("+proj=laea +lat_0=0 +lon_0=0 +R=6371228", EASE_R, 0.0, 0.0)])
def test_laea_inverse_fails_outside_the_disc(srs, a, rf, lat0):
    """The disc's radius is 2 Rq (sphere: 2 R); along the x axis the
    ellipsoidal oblique map scales it by D (Snyder 24-20)."""
    es = _es(rf)
    c = parse_crs(srs)
    rq = a * math.sqrt(float(q_of(np.float64(math.pi / 2), es)) / 2.0)
    p1 = math.radians(lat0)
    D = 1.0
    if es and abs(lat0) != 90.0:
        qp = float(q_of(np.float64(math.pi / 2), es))
        b1 = math.asin(float(q_of(np.float64(p1), es)) / qp)
        D = a * math.cos(p1) / math.sqrt(1 - es * math.sin(p1) ** 2) / (rq * math.cos(b1))
    r = 2.0 * rq * D
    xs = [c.x0 + r * (1 - 1e-9), c.x0 + r * (1 + 1e-9), c.x0 + 3 * r, c.x0]
    lo, la, ok = crs_transform(srs, "EPSG:4326", xs, [c.y0] * 4)
    assert ok.tolist() == [True, False, False, True]
    assert np.isfinite(lo[[0, 3]]).all() and np.isfinite(la[[0, 3]]).all()


@pytest.mark.parametrize("srs", ["EPSG:6933", "EPSG:3410"])
def test_cea_inverse_fails_beyond_the_pole_line(srs):
    _, yp, ok = crs_transform("EPSG:4326", srs, [0.0], [90.0])
    assert ok[0]
    ys = [yp[0] * (1 - 1e-9), yp[0], yp[0] * (1 + 1e-9), -yp[0] * (1 + 1e-9), 2 * yp[0]]
    lo, la, ok = crs_transform(srs, "EPSG:4326", [0.0] * 5, ys)
    assert ok.tolist() == [True, True, False, False, False]
    assert abs(la[1] - 90.0) < 1e-5 and 89.9 < la[0] < 90.0


# ---------------------------------------------------------------- longitude wrap
def test_polar_laea_wraps_the_longitude_difference():
    for srs in ("EPSG:6931", "+proj=laea +lat_0=90 +lon_0=-45 +datum=WGS84"):
        x, y, ok = crs_transform("EPSG:4326", srs, [179.9, -179.9], [60.0, 60.0])
        assert ok.all()
        rho = math.hypot(x[0], y[0])
        arc = math.degrees(2 * math.asin(math.hypot(x[1] - x[0], y[1] - y[0]) / (2 * rho)))
        assert abs(arc - 0.2) < 1e-9, (srs, arc)
    # lon_0 = -45: 135 E is straight up the map (x = 0), and 179.9 E / 179.9 W are on either side of nothing special
    x, y, ok = crs_transform("EPSG:4326", "+proj=laea +lat_0=90 +lon_0=-45 +datum=WGS84", [135.0, -45.0], [60.0, 60.0])
    assert abs(x[0]) < 1e-6 and y[0] > 0 and abs(x[1]) < 1e-6 and y[1] < 0


# ---------------------------------------------------------------- parser
def wkt(projection, params, a, rf, authority=None):
    s = ('PROJCS["unnamed",GEOGCS["unknown",DATUM["unknown",SPHEROID["unknown",%r,%r]],PRIMEM["Greenwich",0],'
         'UNIT["degree",0.0174532925199433,AUTHORITY["EPSG","9122"]]],PROJECTION["%s"],' % (a, rf, projection))
    s += "".join('PARAMETER["%s",%r],' % kv for kv in params)
    s += 'UNIT["metre",1,AUTHORITY["EPSG","9001"]]'
    if authority:
        s += ',AUTHORITY["EPSG","%d"]' % authority
    return s + "]"


def write_cf_nc(path, data, x, y, cf):
    from scipy.io import netcdf_file
    ny, nx = data.shape
    with netcdf_file(path, "w") as f:
        f.createDimension("y", ny)
        f.createDimension("x", nx)
        vx = f.createVariable("x", "f8", ("x",))
        vx[:] = x
        vy = f.createVariable("y", "f8", ("y",))
        vy[:] = y
        crs = f.createVariable("crs", "i", ())
        for k, val in cf.items():
            setattr(crs, k, val if isinstance(val, str) else np.atleast_1d(np.float64(val)))
        v = f.createVariable("band", data.dtype.char, ("y", "x"))
        v.grid_mapping = "crs"
        v._FillValue = data.dtype.type(-999)
        v[:] = data


NX, NY, RES = 6, 5, 1000.0
DATA = np.arange(NX * NY, dtype=np.int16).reshape(NY, NX)


def grid_axes(x0, y0):
    return x0 + RES * (np.arange(NX) + 0.5), y0 - RES * (np.arange(NY) + 0.5), (x0, RES, 0.0, y0, 0.0, -RES)


def cf_srs(tmp_path, cf, name="c.nc", origin=(4000000.0, 3000000.0)):
    """The SRS the ingest reports for a classic netCDF file with this CF grid mapping."""
    p = str(tmp_path / name)
    xs, ys, gt = grid_axes(*origin)
    write_cf_nc(p, DATA, xs, ys, cf)
    inf = ingest.info(p)
    assert (inf.xsize, inf.ysize) == (NX, NY)
    assert np.allclose(inf.geot, gt, rtol=0, atol=1e-6), (inf.geot, gt)
    assert np.array_equal(ingest.read_host(p, 1).view(np.int16), DATA)
    srs = ingest.netcdf_srs(p, 1)
    assert ingest.netcdf_srs(p, 0) == srs
    return srs


def same_transform(srs_a, srs_b, lon, lat, tol=1e-9):
    xa, ya, oka = crs_transform("EPSG:4326", srs_a, lon, lat)
    xb, yb, okb = crs_transform("EPSG:4326", srs_b, lon, lat)
    assert oka.all() and okb.all()
    assert float(np.maximum(np.abs(xa - xb), np.abs(ya - yb)).max()) <= tol, (srs_a, srs_b)
    la, pa, oka = crs_transform(srs_a, "EPSG:4326", xa, ya)
    lb, pb, okb = crs_transform(srs_b, "EPSG:4326", xa, ya)
    assert oka.all() and okb.all()
    assert float(np.maximum(np.abs(la - lb), np.abs(pa - pb)).max()) <= tol / 1e5 + 1e-13   # degrees: 1 m ~ 1e-5


def test_laea_parser_forms_agree(tmp_path):
    lon, lat = points_around(52.0, 10.0, 200, 60.0)
    proj = "+proj=laea +lat_0=52 +lon_0=10 +x_0=4321000 +y_0=3210000 +ellps=GRS80 +units=m +no_defs"
    params = [("latitude_of_center", 52.0), ("longitude_of_center", 10.0), ("false_easting", 4321000.0),
              ("false_northing", 3210000.0)]
    cf = cf_srs(tmp_path, {"grid_mapping_name": "lambert_azimuthal_equal_area", "latitude_of_projection_origin": 52.0,
                           "longitude_of_projection_origin": 10.0, "false_easting": 4321000.0,
                           "false_northing": 3210000.0, "semi_major_axis": GRS80[0], "inverse_flattening": GRS80[1]})
    assert cf.startswith("+proj=laea ")
    for other in (proj, proj.replace("+ellps=GRS80", "+a=6378137 +rf=298.257222101"),
                  wkt("Lambert_Azimuthal_Equal_Area", params, *GRS80),
                  wkt("Lambert_Azimuthal_Equal_Area", [], 1.0, 0.0, authority=3035), cf):
        assert parse_crs(other).kind == 8
        same_transform("EPSG:3035", other, lon, lat)
    # +a +b: the semi-minor axis rounds once more (an ulp of b is 1e-9 m; es moves by a few 1e-16, the map by 1e-8 m)
    same_transform("EPSG:3035", proj.replace("+ellps=GRS80", "+a=6378137 +b=%r" % (6378137.0 * (1 - 1 / GRS80[1]))), lon, lat,
                   1e-6)
    # the polar and spherical codes
    lon, lat = points_around(90.0, 0.0, 200, 80.0)
    same_transform("EPSG:6931", "+proj=laea +lat_0=90 +lon_0=0 +datum=WGS84", lon, lat)
    same_transform("EPSG:6932", "+proj=laea +lat_0=-90 +lon_0=0 +ellps=WGS84", lon, -lat)
    same_transform("EPSG:3408", "+proj=laea +lat_0=90 +lon_0=0 +R=6371228", lon, lat)
    same_transform("EPSG:3409", wkt("Lambert_Azimuthal_Equal_Area", [("latitude_of_center", -90.0)], EASE_R, 0.0), lon, -lat)
    c = parse_crs("EPSG:6932")
    assert (c.kind, c.phi2, c.es > 0) == (8, 1.0, True) and parse_crs("EPSG:3409").es == 0.0


def test_cea_parser_forms_agree(tmp_path):
    rng = np.random.default_rng(3)
    lon, lat = rng.uniform(-180, 180, 200), rng.uniform(-85, 85, 200)
    proj = "+proj=cea +lat_ts=30 +lon_0=0 +x_0=0 +y_0=0 +datum=WGS84 +units=m +no_defs"
    params = [("standard_parallel_1", 30.0), ("central_meridian", 0.0), ("false_easting", 0.0), ("false_northing", 0.0)]
    base = {"longitude_of_central_meridian": 0.0, "standard_parallel": 30.0, "false_easting": 0.0, "false_northing": 0.0,
            "semi_major_axis": WGS84[0], "inverse_flattening": WGS84[1]}
    cf = cf_srs(tmp_path, dict(base, grid_mapping_name="lambert_cylindrical_equal_area"), "a.nc")
    alias = cf_srs(tmp_path, dict(base, grid_mapping_name="cylindrical_equal_area"), "b.nc")
    assert cf == alias and cf.startswith("+proj=cea +lat_ts=30 ")
    k0 = parse_crs("EPSG:6933").k0
    assert abs(k0 - math.cos(math.radians(30)) / math.sqrt(1 - _es(WGS84[1]) * 0.25)) < 1e-15
    by_scale = {k: v for k, v in base.items() if k != "standard_parallel"}
    cf_k = cf_srs(tmp_path, dict(by_scale, grid_mapping_name="lambert_cylindrical_equal_area",
                                 scale_factor_at_projection_origin=k0), "k.nc")
    assert "+k_0=" in cf_k
    for other in (proj, "+proj=cea +k_0=%r +datum=WGS84" % k0, wkt("Cylindrical_Equal_Area", params, *WGS84),
                  wkt("Cylindrical_Equal_Area", [], 1.0, 0.0, authority=6933), cf, cf_k):
        assert parse_crs(other).kind == 9
        same_transform("EPSG:6933", other, lon, lat)
    same_transform("EPSG:3410", "+proj=cea +lat_ts=30 +R=6371228", lon, lat)
    x, y, _ = crs_transform("EPSG:4326", "+proj=cea +lat_ts=30 +lon_0=20 +x_0=1000 +y_0=-2000 +datum=WGS84", [20.0], [0.0])
    assert abs(x[0] - 1000.0) < 1e-9 and abs(y[0] + 2000.0) < 1e-9


@pytest.mark.parametrize("srs", ["+proj=laea +lat_0=91 +datum=WGS84", "+proj=laea +lat_0=-100 +R=6371228",
                                 "+proj=cea +lat_ts=90 +datum=WGS84", "+proj=cea +lat_ts=-95 +R=6371228",
                                 "+proj=cea +k_0=0 +datum=WGS84", "+proj=cea +k_0=-1 +datum=WGS84"])
def test_parser_rejects(srs):
    with pytest.raises(GskyError) as e:
        parse_crs(srs)
    assert e.value.code == E_CRS


def test_wkt_rejects_a_latitude_beyond_the_pole():
    with pytest.raises(GskyError):
        parse_crs(wkt("Lambert_Azimuthal_Equal_Area", [("latitude_of_center", 95.0)], *GRS80))
    with pytest.raises(GskyError):
        parse_crs(wkt("Cylindrical_Equal_Area", [("standard_parallel_1", 90.0)], *WGS84))


def test_crs_of_different_parameters_differ():
    """The planner's same-CRS shortcut compares the defining parameters: two
    CRSs of one new kind that differ in any of them differ there."""
    names = ("kind", "a", "es", "lam0", "phi0", "phi1", "phi2", "x0", "y0", "k0")
    key = lambda s: tuple(getattr(parse_crs(s), n) for n in names)
    laea = ["EPSG:3035", "EPSG:6931", "EPSG:6932", "EPSG:3408", "+proj=laea +lat_0=52 +lon_0=11 +x_0=4321000 +y_0=3210000 "
            "+ellps=GRS80", "+proj=laea +lat_0=51 +lon_0=10 +x_0=4321000 +y_0=3210000 +ellps=GRS80",
            "+proj=laea +lat_0=52 +lon_0=10 +x_0=0 +y_0=3210000 +ellps=GRS80",
            "+proj=laea +lat_0=52 +lon_0=10 +x_0=4321000 +y_0=3210000 +datum=WGS84"]
    cea = ["EPSG:6933", "EPSG:3410", "+proj=cea +lat_ts=31 +datum=WGS84", "+proj=cea +lat_ts=30 +lon_0=1 +datum=WGS84"]
    keys = [key(s) for s in laea + cea]
    assert len(set(keys)) == len(keys)
    assert key("EPSG:3035") == key("+proj=laea +lat_0=52 +lon_0=10 +x_0=4321000 +y_0=3210000 +ellps=GRS80")


# ---------------------------------------------------------------- netCDF
def test_ingest_netcdf4_laea(tmp_path):
    from .h5write import Var, write_nc4
    xs, ys, gt = grid_axes(4000000.0, 3000000.0)
    cf = {"grid_mapping_name": "lambert_azimuthal_equal_area", "latitude_of_projection_origin": 52.0,
          "longitude_of_projection_origin": 10.0, "false_easting": 4321000.0, "false_northing": 3210000.0,
          "semi_major_axis": GRS80[0], "inverse_flattening": GRS80[1]}
    p = str(tmp_path / "n4.nc")
    variables = [Var("y", ("y",), ys, filters=()), Var("x", ("x",), xs, filters=()),
                 Var("crs", (), np.array(0, np.int32), filters=(), atts=cf),
                 Var("band", ("y", "x"), DATA, atts={"grid_mapping": "crs", "_FillValue": np.int16(-999)}, chunks=(NY, NX))]
    write_nc4(p, [("y", NY), ("x", NX)], variables, {"Conventions": "CF-1.6"})
    inf = ingest.info(p)
    assert (inf.xsize, inf.ysize) == (NX, NY) and np.allclose(inf.geot, gt, rtol=0, atol=1e-6)
    assert np.array_equal(ingest.read_host(p, 1).view(np.int16), DATA)
    lon, lat = points_around(52.0, 10.0, 100, 40.0)
    same_transform("EPSG:3035", ingest.netcdf_srs(p, 1), lon, lat)


def _crs_bytes(c):
    return bytes(c)


@pytest.mark.parametrize("epsg,mapping", [(3035, b"lambert_azimuthal_equal_area"), (6933, b"lambert_cylindrical_equal_area"),
                                          (3395, b"mercator")])
def test_netcdf_output_round_trip(tmp_path, epsg, mapping):
    """A coverage written in the CRS and ingested again: the same gskyhip_crs
    (through the code the writer records), and through the CF attributes alone
    the same transform (degrees and the flattening went through text-free
    doubles: a few ulps, 1e-6 m leaves orders of slack)."""
    from gsky_amd.encode import encode_netcdf_host
    xs, ys, gt = grid_axes(4000000.0, 3000000.0)
    p = str(tmp_path / "o.nc")
    with open(p, "wb") as f:
        f.write(encode_netcdf_host([DATA], gt, epsg, nodata=[-999.0]))
    inf = ingest.info(p)
    assert (inf.xsize, inf.ysize) == (NX, NY) and np.allclose(inf.geot, gt, rtol=0, atol=1e-6)
    assert np.array_equal(ingest.read_host(p, 1).view(np.int16), DATA)
    assert _crs_bytes(parse_crs(ingest.netcdf_srs(p, 0))) == _crs_bytes(parse_crs("EPSG:%d" % epsg))
    got = ingest.netcdf_srs(p, 1)
    assert parse_crs(got).kind == parse_crs("EPSG:%d" % epsg).kind
    rng = np.random.default_rng(5)
    same_transform("EPSG:%d" % epsg, got, rng.uniform(-20, 40, 100), rng.uniform(30, 70, 100), tol=1e-6)
    raw = open(p, "rb").read()
    for name in (b"grid_mapping_name", mapping, b"false_easting", b"false_northing", b"semi_major_axis",
                 b"inverse_flattening"):
        assert name in raw, name


# ---------------------------------------------------------------- drill geometry
def test_drill_window_over_an_ease2_global_granule():
    """getDrillFileDescriptor's window (drill.go:363-423) of a WGS 84 polygon
    against an EPSG:6933 dataset: the envelope of the vertices projected by
    the formulation, through the inverse geotransform, truncated as Go's int()."""
    from gsky_amd.drill import drill_descriptors
    res = 36032.220840584
    gt = [-17367530.45, res, 0.0, 7314540.83, 0.0, -res]
    ring = [(100.0, 10.0), (150.0, 12.0), (152.5, -35.0), (103.0, -33.0), (100.0, 10.0)]
    geo = json.dumps({"type": "Polygon", "coordinates": [[list(p) for p in ring]]})
    win, off, buf, st = drill_descriptors([geo], "EPSG:6933", gt, 964, 406)
    assert st[0] == 0
    fx, fy = snyder_cea([p[0] for p in ring], [p[1] for p in ring], 30.0, 0.0, WGS84[0], _es(WGS84[1]))
    px0, px1 = (fx.min() - gt[0]) / res, (fx.max() - gt[0]) / res
    py0, py1 = (fy.max() - gt[3]) / -res, (fy.min() - gt[3]) / -res
    for v in (px0, px1, py0, py1):   # no expected value on a truncation step (the two sides agree to 1e-9 m)
        assert abs(v - round(v)) > 1e-6
    exp = [int(px0), int(py0), int(px1) - int(px0), int(py1) - int(py0)]
    assert win[0].tolist() == exp, (win[0].tolist(), exp)
    assert exp[2] > 100 and exp[3] > 100
