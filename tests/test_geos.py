"""Geostationary satellite CRS (+proj=geos, WKT1 Geostationary_Satellite, CF
geostationary): host-side checks, no GPU and no oracle (the oracle does not
know this family).

The product restates PROJ 6.1.1's geos.cpp.  It is pinned here by
  * the GOES-R Product User Guide's worked example (GRS80, H 42164160 m, sub-
    satellite longitude -75, sweep x: lat 33.846162, lon -84.690932 <-> scan
    angles x -0.024052 rad, y 0.095340 rad), and
  * an independent formulation written below from the CGMS LRIT/HRIT Global
    Specification 4.4.3.2 (also the GOES-R PUG's form) -- geocentric latitude,
    the satellite-to-point vector (s_x, s_y, s_z), visibility, then the scan
    angles of either sweep -- not taken from PROJ's code.
Projected coordinates are the scan angles times the satellite height h above
the ellipsoid (H = h + r_eq from the Earth's centre)."""
import json
import math

import numpy as np
import pytest

from gsky_amd import GskyError, ingest
from gsky_amd.tiles import crs_transform, parse_crs

HIMAWARI = "+proj=geos +lon_0=140.7 +h=35785863 +a=6378137 +b=6356752.3 +sweep=y"
H8 = dict(lon0=140.7, h=35785863.0, r_eq=6378137.0, r_pol=6356752.3)
E_CRS = -4


def cgms(lon, lat, lon0, h, r_eq, r_pol, sweep="y"):
    """CGMS 4.4.3.2: geodetic degrees -> (x, y) metres, visible, margin (the
    visibility expression over H^2)."""
    lon, lat = np.radians(np.asarray(lon, np.float64)), np.radians(np.asarray(lat, np.float64))
    H = h + r_eq
    phi_c = np.arctan((r_pol / r_eq) ** 2 * np.tan(lat))
    e2 = 1.0 - (r_pol / r_eq) ** 2
    r_c = r_pol / np.sqrt(1.0 - e2 * np.cos(phi_c) ** 2)
    dl = lon - math.radians(lon0)
    s_x = H - r_c * np.cos(phi_c) * np.cos(dl)
    s_y = -r_c * np.cos(phi_c) * np.sin(dl)
    s_z = r_c * np.sin(phi_c)
    margin = (H * (H - s_x) - s_y * s_y - (r_eq / r_pol) ** 2 * s_z * s_z) / (H * H)
    s = np.sqrt(s_x * s_x + s_y * s_y + s_z * s_z)
    if sweep == "x":
        y = np.arctan(s_z / s_x)
        x = np.arcsin(-s_y / s)
    else:
        x = np.arctan(-s_y / s_x)
        y = np.arcsin(s_z / s)
    return x * h, y * h, margin >= 0, margin


# ---------------------------------------------------------------- published pin
PUG = dict(lon0=-75.0, h=35786023.0, r_eq=6378137.0, r_pol=6356752.31414)
PUG_SRS = "+proj=geos +lon_0=-75 +h=35786023 +a=6378137 +b=6356752.31414 +sweep=x"
PUG_LAT, PUG_LON, PUG_X, PUG_Y = 33.846162, -84.690932, -0.024052, 0.095340


def test_goes_r_pug_worked_example_forward():
    x, y, ok = crs_transform("EPSG:4326", PUG_SRS, [PUG_LON], [PUG_LAT])
    assert ok[0]
    print("PUG forward: x %.9f rad, y %.9f rad" % (x[0] / PUG["h"], y[0] / PUG["h"]))
    # half the last printed digit of the published angles
    assert abs(x[0] / PUG["h"] - PUG_X) <= 5e-7
    assert abs(y[0] / PUG["h"] - PUG_Y) <= 5e-7


def test_goes_r_pug_worked_example_inverse():
    lon, lat, ok = crs_transform(PUG_SRS, "EPSG:4326", [PUG_X * PUG["h"]], [PUG_Y * PUG["h"]])
    assert ok[0]
    # ground shift of +-5e-7 rad in x and y, by finite differences of the formulation
    d = 1e-6   # degrees
    x0, y0, _, _ = cgms(PUG_LON, PUG_LAT, sweep="x", **PUG)
    xa, ya, _, _ = cgms(PUG_LON + d, PUG_LAT, sweep="x", **PUG)
    xb, yb, _, _ = cgms(PUG_LON, PUG_LAT + d, sweep="x", **PUG)
    J = np.array([[(xa - x0) / d, (xb - x0) / d], [(ya - y0) / d, (yb - y0) / d]]) / PUG["h"]   # rad per degree
    Ji = np.abs(np.linalg.inv(J))
    tol_lon = (Ji[0, 0] + Ji[0, 1]) * 5e-7 + 5e-7
    tol_lat = (Ji[1, 0] + Ji[1, 1]) * 5e-7 + 5e-7
    print("PUG inverse: lon %.7f lat %.7f (tolerances %.2e, %.2e deg)" % (lon[0], lat[0], tol_lon, tol_lat))
    assert abs(lon[0] - PUG_LON) <= tol_lon
    assert abs(lat[0] - PUG_LAT) <= tol_lat


# ---------------------------------------------------------------- the formulation
def _disc_points(lon0, n=2000, max_angle=75.0):
    """About n longitude / latitude points within max_angle degrees of central
    angle from the sub-satellite point."""
    rng = np.random.default_rng(8)
    ang = np.radians(max_angle) * np.sqrt(rng.uniform(0, 1, n))
    az = rng.uniform(0, 2 * np.pi, n)
    lat = np.arcsin(np.sin(ang) * np.cos(az))
    lon = np.arctan2(np.sin(az) * np.sin(ang), np.cos(ang))
    return lon0 + np.degrees(lon), np.degrees(lat)


@pytest.mark.parametrize("name,srs,par,sweep", [
    ("himawari", HIMAWARI, H8, "y"),
    ("sweep_x", HIMAWARI.replace("+sweep=y", "+sweep=x"), H8, "x"),
    ("sphere", "+proj=geos +lon_0=140.7 +h=35785863 +R=6378137", dict(H8, r_pol=6378137.0), "y"),
])
def test_against_the_cgms_formulation(name, srs, par, sweep):
    lon, lat = _disc_points(par["lon0"])
    fx, fy, vis, _ = cgms(lon, lat, sweep=sweep, **par)
    assert vis.all()
    x, y, ok = crs_transform("EPSG:4326", srs, lon, lat)
    assert ok.all()
    err = float(np.maximum(np.abs(x - fx), np.abs(y - fy)).max())
    # inverse: round trip in projected space
    lo2, la2, ok2 = crs_transform(srs, "EPSG:4326", x, y)
    assert ok2.all()
    x2, y2, ok3 = crs_transform("EPSG:4326", srs, lo2, la2)
    assert ok3.all()
    rt = float(np.maximum(np.abs(x2 - x), np.abs(y2 - y)).max())
    print("%s: forward vs formulation %.3e m, round trip %.3e m over %d points" % (name, err, rt, lon.size))
    # both sides fp64 at 4e7 m magnitudes (rounding < 1e-6 m): 1e-3 m catches any wrong constant
    assert err <= 1e-3
    assert rt <= 1e-3


def test_default_sweep_is_y():
    lon, lat = _disc_points(140.7, 50)
    a = crs_transform("EPSG:4326", HIMAWARI, lon, lat)
    b = crs_transform("EPSG:4326", HIMAWARI.replace(" +sweep=y", ""), lon, lat)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---------------------------------------------------------------- failure rule
def test_forward_fails_beyond_the_limb():
    """At the equator the limb sits near 81.3 degrees from the sub-satellite longitude."""
    lon0 = H8["lon0"]
    lon = [lon0 + 81, lon0 - 81, lon0 + 82, lon0 - 82, lon0 + 180]
    x, y, ok = crs_transform("EPSG:4326", HIMAWARI, lon, [0.0] * 5)
    assert ok.tolist() == [True, True, False, False, False]
    assert cgms(lon, [0.0] * 5, **H8)[2].tolist() == ok.tolist()


def test_inverse_fails_off_the_disc():
    x, y, ok = crs_transform(HIMAWARI, "EPSG:4326", [5.40e6, 5.45e6, 5.5e6], [0.0, 0.0, 5.5e6])
    assert ok.tolist() == [True, False, False]
    assert np.isfinite(x[0]) and np.isfinite(y[0])


# ---------------------------------------------------------------- parser
def _wkt(lon0, h, a=6378137.0, rf=298.25722356300003, ext=None, fe=0.0, fn=0.0):
    s = ('PROJCS["unnamed",GEOGCS["unknown",DATUM["unknown",SPHEROID["unknown",%r,%r]],PRIMEM["Greenwich",0],'
         'UNIT["degree",0.0174532925199433]],PROJECTION["Geostationary_Satellite"],'
         'PARAMETER["central_meridian",%r],PARAMETER["satellite_height",%r],PARAMETER["false_easting",%r],'
         'PARAMETER["false_northing",%r],UNIT["metre",1]' % (a, rf, lon0, h, fe, fn))
    if ext:
        s += ',EXTENSION["PROJ4","%s"]' % ext
    return s + "]"


def _same_transform(srs_a, srs_b, lon0, tol=1e-9):
    lon, lat = _disc_points(lon0, 200)
    xa, ya, oka = crs_transform("EPSG:4326", srs_a, lon, lat)
    xb, yb, okb = crs_transform("EPSG:4326", srs_b, lon, lat)
    assert oka.all() and okb.all()
    assert float(np.maximum(np.abs(xa - xb), np.abs(ya - yb)).max()) <= tol
    la, pa, oka = crs_transform(srs_a, "EPSG:4326", xa, ya)
    lb, pb, okb = crs_transform(srs_b, "EPSG:4326", xa, ya)
    assert oka.all() and okb.all()
    if tol <= 1e-9:   # the same constants: the same bits
        assert np.array_equal(la, lb) and np.array_equal(pa, pb)
    else:
        assert float(np.maximum(np.abs(la - lb), np.abs(pa - pb)).max()) <= tol / 1e5   # degrees: 1 m ~ 1e-5


def test_parser_forms_agree():
    proj_y = "+proj=geos +lon_0=140.7 +h=35785863 +x_0=0 +y_0=0 +a=6378137 +rf=298.25722356300003 +sweep=y"
    proj_x = proj_y.replace("+sweep=y", "+sweep=x")
    assert parse_crs(proj_y).kind == 7
    _same_transform(proj_y, _wkt(140.7, 35785863.0), 140.7)
    # the sweep in an EXTENSION node, as GDAL's netCDF driver carries it: the full PROJ string or the flag alone
    full = "+proj=geos +lon_0=140.7 +h=35785863 +x_0=0 +y_0=0 +datum=WGS84 +units=m +no_defs +sweep=x"
    _same_transform(proj_x, _wkt(140.7, 35785863.0, ext=full), 140.7)
    _same_transform(proj_x, _wkt(140.7, 35785863.0, ext="+sweep=x"), 140.7)
    assert parse_crs(_wkt(140.7, 35785863.0)).phi2 == 0.0 and parse_crs(_wkt(140.7, 35785863.0, ext=full)).phi2 == 1.0
    # +ellps / +datum, and false easting / northing
    _same_transform(proj_y, "+proj=geos +lon_0=140.7 +h=35785863 +datum=WGS84", 140.7)
    x, y, _ = crs_transform("EPSG:4326", proj_y, [150.0], [-30.0])
    x2, y2, _ = crs_transform("EPSG:4326", proj_y.replace("+x_0=0 +y_0=0", "+x_0=1000 +y_0=-2000"), [150.0], [-30.0])
    assert abs(x2[0] - x[0] - 1000.0) <= 1e-8 and abs(y2[0] - y[0] + 2000.0) <= 1e-8


@pytest.mark.parametrize("srs", ["+proj=geos +lon_0=140.7 +a=6378137 +b=6356752.3", "+proj=geos +h=0 +lon_0=0",
                                 "+proj=geos +h=-5 +lon_0=0", "+proj=geos +h=35785863 +sweep=z"])
def test_parser_rejects(srs):
    with pytest.raises(GskyError) as e:
        parse_crs(srs)
    assert e.value.code == E_CRS
    with pytest.raises(GskyError):
        parse_crs(_wkt(140.7, 0.0))


# ---------------------------------------------------------------- ingest
def _cf(**kw):
    cf = {"grid_mapping_name": "geostationary", "longitude_of_projection_origin": np.array([140.7]),
          "perspective_point_height": np.array([35785863.0]), "semi_major_axis": np.array([6378137.0]),
          "inverse_flattening": np.array([298.257223563]), "false_easting": np.array([0.0]),
          "false_northing": np.array([0.0])}
    cf.update(kw)
    return {k: v for k, v in cf.items() if v is not None}


def _write_nc(path, data, x, y, cf, xunits=None, yunits=None, xpack=None):
    from scipy.io import netcdf_file
    ny, nx = data.shape
    with netcdf_file(path, "w") as f:
        f.createDimension("y", ny)
        f.createDimension("x", nx)
        vx = f.createVariable("x", "f8", ("x",))
        vx[:] = x
        vy = f.createVariable("y", "f8", ("y",))
        vy[:] = y
        if xunits:
            vx.units = xunits
        if yunits:
            vy.units = yunits
        if xpack:
            vx.scale_factor, vx.add_offset = np.float64(xpack[0]), np.float64(xpack[1])
        crs = f.createVariable("crs", "i", ())
        for k, val in cf.items():
            setattr(crs, k, val)
        v = f.createVariable("band", data.dtype.char, ("y", "x"))
        v.grid_mapping = "crs"
        v._FillValue = data.dtype.type(-999)
        v[:] = data


NX, NY, RES = 6, 5, 2000.0
X_M = -2700000.0 + RES * (np.arange(NX) + 0.5)
Y_M = 100000.0 - RES * (np.arange(NY) + 0.5)
GT_M = (-2700000.0, RES, 0.0, 100000.0, 0.0, -RES)
DATA = np.arange(NX * NY, dtype=np.int16).reshape(NY, NX)


def _check_file(path, h, sweep, rtol=1e-12):
    inf = ingest.info(path)
    assert (inf.xsize, inf.ysize) == (NX, NY)
    for got, exp in zip(inf.geot, GT_M):
        assert abs(got - exp) <= rtol * 3e6, (inf.geot, GT_M)
    srs = ingest.netcdf_srs(path, 1)
    assert ingest.netcdf_srs(path, 0) == srs
    c = parse_crs(srs)
    assert c.kind == 7 and c.phi2 == (1.0 if sweep == "x" else 0.0)
    _same_transform(srs, "+proj=geos +lon_0=140.7 +h=%r +a=6378137 +rf=298.257223563 +sweep=%s" % (h, sweep), 140.7)
    assert np.array_equal(ingest.read_host(path, 1).view(np.int16), DATA)


@pytest.mark.parametrize("units,scale", [(None, 1.0), ("m", 1.0), ("rad", 35785863.0), ("Rad", 35785863.0),
                                         ("microradian", 35785863.0 * 1e-6), ("MICRORADIAN", 35785863.0 * 1e-6)])
def test_ingest_axis_units(tmp_path, units, scale):
    """x / y in metres, radians or microradians (case-insensitive): the
    geotransform is in metres (netcdfdataset.cpp:3578-3626)."""
    p = str(tmp_path / "u.nc")
    _write_nc(p, DATA, X_M / scale, Y_M / scale, _cf(sweep_angle_axis="y"), units, units)
    _check_file(p, 35785863.0, "y", rtol=1e-9)


def test_ingest_axis_units_per_axis_and_after_scale_offset(tmp_path):
    """The rule is per axis, and applies after scale_factor / add_offset."""
    h = 35785863.0
    p = str(tmp_path / "p.nc")
    xr = X_M / h
    sf, ao = 1e-5, xr[0]
    _write_nc(p, DATA, (xr - ao) / sf, Y_M, _cf(), xunits="rad", yunits="m", xpack=(sf, ao))
    _check_file(p, h, "y", rtol=1e-9)


@pytest.mark.parametrize("axis,sweep", [("x", "x"), ("y", "y"), (None, "y"), ("X", "x"), ("z", "y")])
def test_ingest_sweep_angle_axis(tmp_path, axis, sweep):
    p = str(tmp_path / "s.nc")
    _write_nc(p, DATA, X_M, Y_M, _cf(sweep_angle_axis=axis))
    _check_file(p, 35785863.0, sweep)


def test_ingest_default_height(tmp_path):
    """No perspective_point_height: 35785831 m (netcdfdataset.cpp:3147), which
    also scales radian axes."""
    h = 35785831.0
    p = str(tmp_path / "h.nc")
    _write_nc(p, DATA, X_M / h, Y_M / h, _cf(perspective_point_height=None), "rad", "rad")
    _check_file(p, h, "y", rtol=1e-9)
    assert "+h=35785831 " in ingest.netcdf_srs(p, 1)


def test_ingest_netcdf4(tmp_path):
    from .h5write import Var, write_nc4
    h = 35785863.0
    cf = {k: (float(v[0]) if isinstance(v, np.ndarray) else v) for k, v in _cf(sweep_angle_axis="x").items()}
    p = str(tmp_path / "n4.nc")
    variables = [Var("y", ("y",), Y_M / h * 1e6, filters=(), atts={"units": "microradian"}),
                 Var("x", ("x",), X_M / h * 1e6, filters=(), atts={"units": "microradian"}),
                 Var("crs", (), np.array(0, np.int32), filters=(), atts=cf),
                 Var("band", ("y", "x"), DATA, atts={"grid_mapping": "crs", "_FillValue": np.int16(-999)},
                     chunks=(NY, NX))]
    write_nc4(p, [("y", NY), ("x", NX)], variables, {"Conventions": "CF-1.6"})
    _check_file(p, h, "x", rtol=1e-9)


def test_other_projections_ignore_radian_units(tmp_path):
    """For this projection only: an Albers file's axes are never rescaled."""
    from .test_ingest import ALBERS_CF
    p = str(tmp_path / "a.nc")
    _write_nc(p, DATA, X_M, Y_M, ALBERS_CF, "rad", "rad")
    inf = ingest.info(p)
    assert abs(inf.geot[0] - GT_M[0]) < 1e-6 and abs(inf.geot[1] - RES) < 1e-9


# ---------------------------------------------------------------- drill geometry
def _geojson(ring):
    return json.dumps({"type": "Polygon", "coordinates": [[list(p) for p in ring]]})


def test_drill_window_over_central_australia():
    """getDrillFileDescriptor's window (drill.go:363-423) of a WGS 84 polygon
    against a geostationary dataset: the envelope of the vertices projected by
    the formulation, through the inverse geotransform, truncated as Go's int()."""
    from gsky_amd.drill import drill_descriptors
    n, res = 2200, 2000.0
    gt = [-2700000.0, res, 0.0, 100000.0, 0.0, -res]
    ring = [(130.0, -22.0), (136.0, -22.0), (136.5, -27.0), (130.5, -27.5), (130.0, -22.0)]
    win, off, buf, st = drill_descriptors([_geojson(ring)], HIMAWARI, gt, n, n)
    assert st[0] == 0
    fx, fy, vis, _ = cgms([p[0] for p in ring], [p[1] for p in ring], **H8)
    assert vis.all()
    px0, px1 = (fx.min() - gt[0]) / res, (fx.max() - gt[0]) / res
    py0, py1 = (fy.max() - gt[3]) / -res, (fy.min() - gt[3]) / -res
    for v in (px0, px1, py0, py1):   # no expected value on a truncation step (the two sides agree to 1e-9 m)
        assert abs(v - round(v)) > 1e-6
    exp = [int(px0), int(py0), int(px1) - int(px0), int(py1) - int(py0)]
    assert win[0].tolist() == exp, (win[0].tolist(), exp)
    assert exp[2] > 200 and exp[3] > 200


def test_drill_vertex_beyond_the_limb():
    from gsky_amd.drill import drill_descriptors
    gt = [-5500000.0, 10000.0, 0.0, 5500000.0, 0.0, -10000.0]
    ring = [(130.0, -22.0), (136.0, -22.0), (40.0, -27.0), (130.0, -22.0)]   # 40 E: 100 degrees west of 140.7
    win, off, buf, st = drill_descriptors([_geojson(ring)], HIMAWARI, gt, 1100, 1100)
    assert st[0] == E_CRS


# ---------------------------------------------------------------- netCDF output
@pytest.mark.parametrize("sweep", ["y", "x"])
def test_netcdf_output_writes_the_geostationary_mapping(tmp_path, sweep):
    """A geostationary destination CRS: the CF `geostationary` mapping with all
    its attributes (sweep_angle_axis always, netcdfdataset.cpp:4192-4200), read
    back with the product's own reader."""
    from gsky_amd.encode import encode_netcdf_host
    srs = "+proj=geos +lon_0=140.7 +h=35785863 +x_0=100 +y_0=-200 +a=6378137 +rf=298.257223563 +sweep=%s" % sweep
    p = str(tmp_path / "o.nc")
    with open(p, "wb") as f:
        f.write(encode_netcdf_host([DATA], GT_M, 0, nodata=[-999.0], srs=srs))
    inf = ingest.info(p)
    assert (inf.xsize, inf.ysize) == (NX, NY)
    assert np.allclose(inf.geot, GT_M, rtol=0, atol=1e-6)
    assert np.array_equal(ingest.read_host(p, 1).view(np.int16), DATA)
    for cf in (0, 1):
        got = ingest.netcdf_srs(p, cf)
        assert got.startswith("+proj=geos +lon_0=") and "+h=35785863 " in got and got.endswith("+sweep=%s" % sweep)
        assert abs(float(got.split("+lon_0=")[1].split()[0]) - 140.7) < 1e-12
        assert "+x_0=100 " in got and "+y_0=-200 " in got
        # the written attributes went through radians -> degrees and es -> inverse flattening, a few
        # ulps each (1e-15 of 4e7 m): 1e-6 m leaves two orders of slack and catches any wrong attribute
        _same_transform(got, srs, 140.7, tol=1e-6)
    raw = open(p, "rb").read()
    for name in (b"grid_mapping_name", b"geostationary", b"longitude_of_projection_origin", b"perspective_point_height",
                 b"sweep_angle_axis", b"false_easting", b"false_northing", b"semi_major_axis", b"inverse_flattening",
                 b"Geostationary_Satellite"):
        assert name in raw, name
    # an SRS outside the supported families stays an error
    with pytest.raises(GskyError) as e:
        encode_netcdf_host([DATA], GT_M, 0, srs="+proj=robin")
    assert e.value.code == E_CRS
