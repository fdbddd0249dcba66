"""Record what the SRS parser (gskyhip_crs_from_srs) makes of a corpus of SRS
strings into tests/golden/srs_corpus.json.gz: for every string the return
code and, where that is 0, the raw bytes of the gskyhip_crs it filled (from
a zero-initialised struct).  tests/test_srs_corpus.py replays the fixture, so
any change to the parser that moves one bit of one struct shows there.

The strings are derived from the parser's branches: every EPSG code and range
end crs_epsg knows, every +proj= branch of crs_proj4 with each ellipsoid and
scale spelling it reads, and every WKT1 PROJECTION name of parse_srs with
each parameter present and absent.  The fixture is a record of one commit
(its hash is stored in it): regenerate it only to extend the corpus, from a
build of the commit that the parser last changed in, never to make a failing
replay pass.

    python tests/make_srs_corpus.py
"""
import ctypes
import gzip
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(HERE, "golden", "srs_corpus.json.gz")

WGS84 = ("WGS 84", 6378137, 298.257223563)
GRS80 = ("GRS 1980", 6378137, 298.257222101)
BESSEL = ("Bessel 1841", 6377397.155, 299.1528128)
SPHERE = ("Sphere", 6371228, 0)


def wkt(projection, params, spheroid=WGS84, authority=None, tail=""):
    """A GDAL-style WKT1 PROJCS.  spheroid: (name, a, rf), (name, a) for a node
    without the flattening, or None for no SPHEROID node.  params: (name,
    value) pairs in order, so one may appear twice."""
    sph = ""
    if spheroid is not None:
        sph = ',SPHEROID["%s",%s]' % (spheroid[0], ",".join(repr(v) for v in spheroid[1:]))
    s = 'PROJCS["corpus",GEOGCS["g",DATUM["d"%s],PRIMEM["Greenwich",0],UNIT["degree",0.0174532925199433]]' % sph
    if projection:
        s += ',PROJECTION["%s"]' % projection
    s += "".join(',PARAMETER["%s",%r]' % (n, v) for n, v in params)
    s += ',UNIT["metre",1]' + tail
    if authority is not None:
        s += ',AUTHORITY["EPSG","%s"]' % authority
    return s + "]"


def each_absent(params):
    """params whole, then with each one left out in turn."""
    yield list(params)
    for i in range(len(params)):
        yield params[:i] + params[i + 1:]


def epsg_strings():
    singles = [4326, 4283, 3857, 900913, 3577, 3031, 3413, 3976, 32661, 32761, 3112, 7845, 3035, 6931, 6932, 3408,
               3409, 6933, 3410, 3395, 3832]
    ranges = [(32601, 32660), (32701, 32760), (28348, 28358), (7846, 7859)]
    codes = list(singles)
    for lo, hi in ranges:   # every zone, and the outside neighbour of each end
        codes += list(range(lo - 1, hi + 2))
    out = ["EPSG:%d" % c for c in dict.fromkeys(codes)]
    return out + ["epsg:4326", "Epsg:3857", "EPSG:", "EPSG:0", "EPSG:9999", "EPSG:-1", "EPSG: 4326", "EPSG:4326abc",
                  "EPSG:abc", "EPSG:32755.5", "EPSG:04326", "EPSG"]


def name_strings():
    return ["MODIS", "modis", "Modis", "SR-ORG:6842", "sr-org:6842", "", " ", "garbage", "MODIS ", "SR-ORG:6974",
            "WGS84", "CRS:84", "urn:ogc:def:crs:EPSG::4326", "+", "+proj", "+proj=", "proj=longlat"]


ELLPS = ["", "+ellps=GRS80", "+ellps=WGS84", "+datum=WGS84", "+a=6377397.155 +rf=299.1528128", "+R=6371228"]
AB = "+a=6378137 +b=6356752.314245"
AES = "+a=6378137 +es=0.00669438"
K = ["", "+k_0=0.997", "+k=0.998", "+k_0=0.997 +k=0.998", "+k=0.998 +k_0=0.997"]
TS = ["", "+lat_ts=42"]


def join(*parts):
    return " ".join(p for p in parts if p)


def proj_strings():
    out = []
    # the ellipsoid spellings every branch shares (longlat keeps the struct small)
    for proj in ("longlat", "latlong"):
        out += [join("+proj=" + proj, e, "+no_defs") for e in ELLPS]
    out += [join("+proj=longlat", e) for e in (
        "+a=6378137", "+a=6378137 +rf=0", "+rf=298.3", "+R=0", "+R=-5", "+R=6371228 +ellps=GRS80",
        "+ellps=GRS80 +a=1 +rf=2", "+ellps=GRS67", "+ellps=sphere", "+ellps=GRS80xyz", "+datum=WGS84 +ellps=GRS80",
        "+datum=NAD83", "+towgs84=0,0,0 +a=6378160 +rf=298.25", "x+a=5 +rf=7", "++a=6378160 +rf=298.25", AB, AES)]
    out += ["+proj=longlat +lon_0=10 +lat_0=20 +x_0=30 +y_0=40 +datum=WGS84", "+proj=longlat +proj=merc +R=6371228",
            "+datum=WGS84 +proj=longlat", "+proj=longlatx", "+proj=robin +datum=WGS84", "+proj= longlat",
            "+PROJ=longlat"]
    out += [join("+proj=webmerc", e) for e in ELLPS] + ["+proj=webmerc +lon_0=10 +x_0=5 +datum=WGS84"]
    # merc / cea: +lat_ts | +k_0 | +k, every ellipsoid form with and without +lat_ts
    for proj in ("merc", "cea"):
        base = "+proj=%s +lon_0=110 +x_0=3900000 +y_0=900000" % proj
        for e in ELLPS + [AB, AES]:
            out += [join(base, e, k, ts) for k, ts in (("", ""), ("+k_0=0.997", ""), ("", "+lat_ts=42"))]
        for e in ("+ellps=WGS84", "+R=6371228"):
            out += [join("+proj=" + proj, e, k, ts) for k in K for ts in TS if k or ts]
        out += [join("+proj=" + proj, e) for e in (
            "+lat_ts=90 +datum=WGS84", "+lat_ts=-90 +R=6371228", "+lat_ts=120 +datum=WGS84", "+k_0=0 +datum=WGS84",
            "+k_0=-0.5 +datum=WGS84", "+k=0 +R=6371228", "+lat_ts=-42 +datum=WGS84", "+lat_ts=0 +R=6378137",
            "+lat_ts=0 +k_0=0.5 +R=6378137", "+lat_0=30 +datum=WGS84", "+a=6378137 +b=0", "+a=6378137 +b=-1",
            "+a=6378137 +b=6378137", "+a=6378137 +es=1.5 +b=6356752.314245", "+a=6378137 +es=-0.1",
            "+a=6378137 +es=0", "+a=6378137 +es=0.00669438 +b=6300000", "+a=6378137 +rf=298.3 +b=6300000",
            "+R=6371228 +b=6300000", "+b=6356752.314245", "+es=0.00669438", "+ellps=WGS84 +es=0.1")]
    out += ["+proj=merc +a=6378137 +b=6378137 +lat_ts=0.0 +lon_0=0.0 +x_0=0.0 +y_0=0 +k=1.0 +units=m +nadgrids=@null "
            "+wktext +no_defs", "+proj=merc +lon_0=0 +k=1 +x_0=0 +y_0=0 +R=6378137 +units=m +nadgrids=@null +no_defs",
            "+proj=merc +lon_0=150 +k=1 +x_0=0 +y_0=0 +datum=WGS84 +units=m +no_defs",
            "+proj=merc +lon_0=150 +k_0=1 +a=6378137 +rf=298.257223563", "+proj=merc +R=6371228 +lat_ts=30 +lon_0=-60",
            "+proj=merc +a=6378245 +rf=298.3 +lat_ts=42 +lon_0=51", "+proj=merc +R=6378137 +k_0=1 +lon_0=20 +x_0=7"]
    # laea: the aspect from +lat_0
    base = "+proj=laea +lat_0=52 +lon_0=10 +x_0=4321000 +y_0=3210000"
    out += [join(base, e) for e in ELLPS + [AB, AES]]
    for lat0 in ("90", "-90", "0", "1e-11", "89.99999999999", "90.000000001", "90.1", "95", "-100", "-45"):
        out += [join("+proj=laea +lat_0=" + lat0, e) for e in ("+ellps=GRS80", "+R=6371228")]
    out += ["+proj=laea", "+proj=laea +proj=cea +lat_ts=30", "+proj=laea +lat_0=52 +k_0=0.5 +lat_ts=10 +datum=WGS84"]
    # aea
    base = "+proj=aea +lat_1=-18 +lat_2=-36 +lat_0=0 +lon_0=132 +x_0=0 +y_0=0"
    out += [join(base, e) for e in ELLPS]
    out += [join("+proj=aea", p, e) for e in ("+ellps=GRS80", "+R=6371228") for p in (
        "+lat_1=-18 +lat_2=18", "+lat_1=-25 +lat_2=-25 +lat_0=-10", "+lat_1=-25", "+lat_2=-25", "",
        "+lat_1=29.5 +lat_2=45.5 +lat_0=23 +lon_0=-96", "+lat_1=-18 +lat_1=-20 +lat_2=-36")]
    # sinu: the sphere only
    out += [join("+proj=sinu +lon_0=0 +x_0=0 +y_0=0", e, "+units=m") for e in ELLPS]
    out += ["+proj=sinu +R=6371007.181", "+proj=sinu +lon_0=15 +x_0=100 +y_0=-200 +R=6371007.181",
            "+proj=sinu +a=6371007.181 +b=6371007.181", "+proj=sinu +a=6371007.181"]
    # utm
    out += [join("+proj=utm +zone=55 +south", e) for e in ELLPS]
    out += [join("+proj=utm", p, "+ellps=GRS80") for p in (
        "", "+zone=55", "+zone=55.5", "+zone=0", "+zone=1", "+zone=60", "+zone=61", "+zone=-3", "+zone=33 +south",
        "+south", "+zone=55 +zone=56", "+zone=55 +lon_0=3 +k_0=1 +x_0=0 +y_0=5 +lat_0=10", "+zone=55 +southern",
        "+zone=1e1", "+zone=abc")]
    out += ["+proj=utm +zone=55 +R=6371228", "+south +zone=50 +proj=utm +datum=WGS84"]
    # ups
    out += [join("+proj=ups", s, e) for s in ("", "+south") for e in ELLPS]
    out += ["+proj=ups +lon_0=30 +k_0=1 +x_0=0 +y_0=0 +lat_0=45 +lat_ts=70 +datum=WGS84"]
    # stere: the polar aspects; the name at the end of the string, or before a space
    base = "+proj=stere +lat_0=90 +lat_ts=70 +lon_0=-45 +x_0=0 +y_0=0"
    out += [join(base, e) for e in ELLPS]
    for lat0 in ("90", "-90"):
        out += [join("+proj=stere +lat_0=" + lat0, k, ts, "+datum=WGS84") for k in K
                for ts in ("", "+lat_ts=-71", "+lat_ts=90")]
    out += ["+lat_0=90 +lat_ts=70 +lon_0=-45 +datum=WGS84 +proj=stere", "+proj=stere", "+proj=stere ",
            "+proj=stere +lat_0=45 +datum=WGS84", "+proj=stere +lat_0=0 +datum=WGS84", "+proj=stere +datum=WGS84",
            "+proj=stere +lat_0=-90 +lat_ts=-71 +k_0=0.9 +datum=WGS84",
            "+proj=sterea +lat_0=52.15616055555555 +lon_0=5.38763888888889 +k=0.9999079 +ellps=WGS84",
            "+lat_0=90 +datum=WGS84 +proj=sterea", "+proj=stere\t+lat_0=90", "+lat_0=90 +proj=stere +proj=lcc +lat_1=5",
            "+lat_1=5 +proj=lcc +lat_0=90 +lat_ts=70 +proj=stere", "+proj=stere +lat_0=90 +proj=ups +south",
            "+proj=stere +lat_0=89.99999999999 +lat_ts=70 +datum=WGS84", "+proj=stere +lat_0=100 +datum=WGS84"]
    # geos
    base = "+proj=geos +lon_0=140.7 +h=35785863 +x_0=0 +y_0=0"
    out += [join(base, e, "+sweep=y") for e in ELLPS + [AB, AES]]
    out += [join(base, AB, sw) for sw in ("", "+sweep=x", "+sweep=y", "+sweep=z", "+sweep=xy", "+sweep=x +units=m",
                                          "+sweep=X", "+sweep=", "+sweep= x", "+sweep=y +sweep=x")]
    out += [join("+proj=geos", p) for p in (
        "+lon_0=0 +a=6378137 +b=6356752.3", "+h=0 +datum=WGS84", "+h=-1 +datum=WGS84", "+h=35785831",
        "+h=35785831 +a=6378137 +b=0", "+h=35785831 +a=6378137 +b=-2", "+h=35785831 +a=6378137 +b=6378137",
        "+h=35785831 +a=6378137 +rf=298.257 +b=0", "+h=35785831 +R=6371228 +b=0", "+h=35785831 +b=6356752.3",
        "+h=35785831 +datum=WGS84 +b=6300000", "+h=35785831 +a=6378137 +es=0.1 +b=6356752.3", "+h=35785831 +sweep=x",
        "+h=35786023 +lon_0=-75 +x_0=1 +y_0=2 +lat_0=5 +k_0=3 +ellps=GRS80 +sweep=x +no_defs", "+h=35785831 +h=1",
        "+hh=35785831 +datum=WGS84", "+sweep=x +h=35785831 +a=6378169 +b=6356583.8")]
    # lcc
    base = "+proj=lcc +lat_1=-18 +lat_2=-36 +lat_0=0 +lon_0=134 +x_0=0 +y_0=0"
    out += [join(base, e) for e in ELLPS]
    out += [join("+proj=lcc", p, k, "+ellps=GRS80") for k in K for p in (
        "+lat_1=-30 +lon_0=134", "+lat_1=-30 +lat_0=-25 +lon_0=134", "+lat_1=-18 +lat_2=-36 +lat_0=-27")]
    out += [join("+proj=lcc", p, "+datum=WGS84") for p in (
        "", "+lat_2=-36", "+lat_0=40", "+lat_1=-18 +lat_2=18", "+lat_1=90", "+lat_1=-90 +lat_2=-90 +lat_0=-90",
        "+lat_1=33 +lat_2=45 +lat_0=90", "+lat_1=33 +lat_2=33 +lat_0=23", "+lat_1=33 +lat_1=45 +lat_2=45",
        "+lat_1=49 +lat_2=49.0000000000001 +lat_0=49")]
    # tmerc / etmerc
    for proj in ("tmerc", "etmerc"):
        base = "+proj=%s +lat_0=0 +lon_0=147 +k_0=0.9996 +x_0=500000 +y_0=10000000" % proj
        out += [join(base, e) for e in ELLPS]
        out += [join("+proj=" + proj, "+lat_0=49 +lon_0=-2 +x_0=400000 +y_0=-100000", k, "+ellps=GRS80") for k in K]
        out += [join(base, "+ellps=GRS80 +approx"), "+proj=%s" % proj]
    out += ["+proj=tmerc +lon_0=147 +lon_0=153 +k=0.9996 +k=1 +ellps=GRS80", "+approx +proj=etmerc +datum=WGS84",
            "+proj=tmerc +approximate +datum=WGS84", "+proj=tmerc +lat_0=90 +datum=WGS84"]
    # a key inside another token, a key that is the suffix of another, a key twice
    out += ["+proj=lcc foo+lat_1=10 +lat_1=-18 +lat_2=-36 +ellps=GRS80", "+proj=lcc +nlat_1=10 +lat_2=-36 +ellps=GRS80",
            "+proj=lcc +lat_1x=10 +lat_2=-36 +ellps=GRS80", "+proj=lcc ++lat_1=-18 +lat_2=-36 +ellps=GRS80",
            "+proj=lcc +lat_1=-18+lat_2=-36 +ellps=GRS80", "+proj=lcc +lat_1 =-18 +lat_2=-36 +ellps=GRS80",
            "+proj=tmerc +k_0=0.9996 +ellps=GRS80", "+proj=tmerc +k=0.9996 +ellps=GRS80",
            "+proj=tmerc +sk=0.5 +ellps=GRS80", "+proj=tmerc +sk_0=0.5 +k=0.9 +ellps=GRS80",
            "+proj=tmerc +k_0=abc +k=0.9 +ellps=GRS80", "+proj=tmerc +k_0= +k=0.9 +ellps=GRS80",
            "+proj=cea +lat_ts=30 +lat_ts=45 +ellps=WGS84", "+proj=cea +xlat_ts=30 +ellps=WGS84",
            "+proj=aea +lat_1=-18 +lat_2=-36 +lon_0=132 +lon_0=140 +x_0=1 +x_0=2 +ellps=GRS80",
            "lat_1=-18 +proj=aea +lat_2=-36 +ellps=GRS80", "+proj=longlat +R=6371228 +rf=298",
            "+proj=longlat +a=6378137 +rf=298.257223563 +R=1", "+proj=longlat +a=1e400 +rf=nan",
            "+proj=longlat +a=inf", "+proj=longlat +a=0x10 +rf=1e2"]
    return out


def wkt_strings():
    out = []
    fe = [("false_easting", 4321000.5), ("false_northing", -3210000.25)]
    families = [
        ("Polar_Stereographic", [("latitude_of_origin", -71.0), ("central_meridian", 15.0), ("scale_factor", 0.98)] + fe),
        ("Geostationary_Satellite", [("central_meridian", 140.7), ("satellite_height", 35785831.0)] + fe),
        ("Lambert_Azimuthal_Equal_Area", [("latitude_of_center", 52.0), ("longitude_of_center", 10.0)] + fe),
        ("Cylindrical_Equal_Area", [("standard_parallel_1", 30.0), ("central_meridian", 20.0)] + fe),
        ("Mercator_1SP", [("central_meridian", 110.0), ("scale_factor", 0.997)] + fe),
        ("Mercator_2SP", [("standard_parallel_1", 42.0), ("central_meridian", 51.0)] + fe),
        ("Lambert_Conformal_Conic_1SP", [("latitude_of_origin", -30.0), ("central_meridian", 134.0),
                                         ("scale_factor", 0.999)] + fe),
        ("Lambert_Conformal_Conic_2SP", [("standard_parallel_1", -18.0), ("standard_parallel_2", -36.0),
                                         ("latitude_of_origin", -27.0), ("central_meridian", 134.0)] + fe),
        ("Transverse_Mercator", [("latitude_of_origin", 49.0), ("central_meridian", -2.0),
                                 ("scale_factor", 0.9996012717)] + fe),
    ]
    for name, params in families:
        out += [wkt(name, p, BESSEL) for p in each_absent(params)]
        out += [wkt(name, params, sph) for sph in (WGS84, GRS80, SPHERE, None, ("a only", 6377397.155))]
        twice = params[:1] + [(params[0][0], params[0][1] / 2)] + params[1:] + [(params[-1][0], 7.0)]
        out.append(wkt(name, twice, BESSEL))
        # two SPHEROID nodes: the first counts
        out.append(wkt(name, params, BESSEL, tail=',SPHEROID["second",6378137,298.257223563]'))
        # a top-level code crs_epsg knows (each family's own, and a foreign one), and one it does not
        out += [wkt(name, params, BESSEL, authority=a) for a in ("3035", "4326", "9999", "0", "abc")]
        out.append(wkt(name, [], GRS80))
    out += [wkt("Lambert_Conformal_Conic_2SP", [("standard_parallel_1", -18.0), ("standard_parallel_2", -36.0),
                                                ("latitude_of_origin", 0.0), ("central_meridian", 134.0)], GRS80, "3112"),
            wkt("Lambert_Conformal_Conic_2SP", [("standard_parallel_1", -18.0), ("standard_parallel_2", 18.0)], GRS80),
            wkt("Lambert_Conformal_Conic_1SP", [("latitude_of_origin", 0.0)], GRS80),
            wkt("Lambert_Conformal_Conic_2SP", [("standard_parallel_1", -18.0), ("standard_parallel_2", -36.0)], SPHERE),
            wkt("Mercator_1SP", [("scale_factor", 1)], WGS84, "3857"),
            wkt("Mercator_1SP", [("central_meridian", 0.0), ("scale_factor", 1.0)], ("s", 6378137, 0)),
            wkt("Mercator_1SP", [("central_meridian", 150.0), ("scale_factor", 1.0)], WGS84, "3832"),
            wkt("Mercator_1SP", [("scale_factor", 0.0)], WGS84), wkt("Mercator_1SP", [("scale_factor", -1.0)], SPHERE),
            wkt("Mercator_2SP", [("standard_parallel_1", 0.0)], SPHERE),
            wkt("Mercator_2SP", [("standard_parallel_1", 90.0)], WGS84),
            wkt("Mercator_2SP", [("standard_parallel_1", -42.0), ("scale_factor", 0.5)], WGS84),
            wkt("Cylindrical_Equal_Area", [("standard_parallel_1", 30.0)], WGS84, "6933"),
            wkt("Cylindrical_Equal_Area", [("standard_parallel_1", 90.0)], WGS84),
            wkt("Cylindrical_Equal_Area", [("standard_parallel_1", 30.0), ("scale_factor", 0.5)], SPHERE),
            wkt("Lambert_Azimuthal_Equal_Area", [("latitude_of_center", 90.0)], WGS84, "6931"),
            wkt("Lambert_Azimuthal_Equal_Area", [("latitude_of_center", -90.0)], SPHERE),
            wkt("Lambert_Azimuthal_Equal_Area", [("latitude_of_center", 0.0), ("longitude_of_center", -100.0)], SPHERE),
            wkt("Lambert_Azimuthal_Equal_Area", [("latitude_of_center", 90.5)], WGS84),
            wkt("Lambert_Azimuthal_Equal_Area", [("latitude_of_center", -91.0)], WGS84),
            wkt("Lambert_Azimuthal_Equal_Area", [("latitude_of_origin", 52.0), ("central_meridian", 10.0)], GRS80)]
    for ts in (90.0, -90.0, 70.0, -71.0, 0.0, 89.9999999999999, 90.0000000000001, -60.0):
        out.append(wkt("Polar_Stereographic", [("latitude_of_origin", ts), ("central_meridian", -45.0)], WGS84))
    out += [wkt("Polar_Stereographic", [("latitude_of_origin", -71.0)], WGS84, "3031"),
            wkt("Polar_Stereographic", [("latitude_of_origin", 70.0)], SPHERE),
            wkt("Polar_Stereographic", [("latitude_of_origin", 90.0), ("scale_factor", 0.994),
                                        ("false_easting", 2000000.0), ("false_northing", 2000000.0)], WGS84, "32661")]
    # Transverse Mercator nodes that are UTM zones, and ones that miss by one condition each
    utm = {"latitude_of_origin": 0.0, "central_meridian": 147.0, "scale_factor": 0.9996, "false_easting": 500000.0,
           "false_northing": 10000000.0}
    for change in ({}, {"false_northing": 0.0}, {"central_meridian": -177.0}, {"central_meridian": 177.0},
                   {"central_meridian": 183.0}, {"central_meridian": -183.0}, {"scale_factor": 0.9995},
                   {"scale_factor": 1.0}, {"false_easting": 500001.0}, {"false_northing": 5.0},
                   {"central_meridian": 146.0}, {"central_meridian": 147.5}, {"latitude_of_origin": 1.0}):
        p = dict(utm, **change)
        out.append(wkt("Transverse_Mercator", list(p.items()), GRS80))
    out += [wkt("Transverse_Mercator", list(utm.items()), GRS80, "28355"),
            wkt("Transverse_Mercator", list(utm.items()), GRS80, "4326"),
            wkt("Transverse_Mercator", list(dict(utm, false_northing=0.0, central_meridian=15.0).items()), WGS84,
                "32633"),
            wkt("Transverse_Mercator", list(utm.items()), SPHERE),
            wkt("Transverse_Mercator", [("latitude_of_origin", 49.0), ("central_meridian", -2.0)], SPHERE)]
    # Sinusoidal: the semi-major axis of the first SPHEROID as a sphere; nothing else is read
    out += [wkt("Sinusoidal", [("longitude_of_center", 0.0), ("false_easting", 0.0), ("false_northing", 0.0)], sph)
            for sph in (("MODIS", 6371007.181, 0), ("no rf", 6371007.181), WGS84, None, ("zero", 0, 0),
                        ("negative", -6371007.181, 0))]
    out += [wkt("Sinusoidal", [("longitude_of_center", 15.0), ("false_easting", 100.0)], ("MODIS", 6371007.181, 0),
                "4326"),
            'PROJCS["x",PROJECTION["Sinusoidal"],SPHEROID[', 'PROJCS["x",PROJECTION["Sinusoidal"],SPHEROID["a,b",5,6]']
    # Geostationary: the sweep axis from the EXTENSION["PROJ4", ...] node only
    geos = [("central_meridian", 140.7), ("satellite_height", 35785831.0), ("false_easting", 0.0),
            ("false_northing", 0.0)]
    himawari = ("h8", 6378137, 298.2572221)
    for tail in ('', ',EXTENSION["PROJ4","+proj=geos +lon_0=140.7 +h=35785831 +x_0=0 +y_0=0 +a=6378137 +b=6356752.3 '
                 '+units=m +sweep=x +no_defs"]',
                 ',EXTENSION["PROJ4","+proj=geos +lon_0=140.7 +h=35785831 +sweep=y +no_defs"]',
                 ',EXTENSION["PROJ4","+proj=geos +h=35785831 +no_defs"],NOTE["+sweep=x"]',
                 ',EXTENSION["PROJ4","+proj=geos +h=35785831 +sweep=xy"]', ',NOTE["+sweep=x"]',
                 ',NOTE["+sweep=x"],EXTENSION["PROJ4","+proj=geos +h=1"]',
                 ',EXTENSION["PROJ4","+proj=geos +h=35785831 +sweep=x'):
        out.append(wkt("Geostationary_Satellite", geos, himawari, tail=tail))
    out += [wkt("Geostationary_Satellite", [("satellite_height", 0.0)], himawari),
            wkt("Geostationary_Satellite", [("satellite_height", -5.0)], himawari),
            wkt("Geostationary_Satellite", geos, SPHERE),
            wkt("Geostationary_Satellite", geos + [("scale_factor", 0.5), ("latitude_of_origin", 10.0)], himawari)]
    # a WKT that carries a PROJ string and is not geostationary goes to crs_proj4 whole
    out += [wkt("Lambert_Conformal_Conic_2SP", [("standard_parallel_1", -18.0), ("standard_parallel_2", -36.0)], GRS80,
                tail=',EXTENSION["PROJ4","+proj=lcc +lat_1=-10 +lat_2=-40 +lon_0=134 +ellps=GRS80 +no_defs"]'),
            wkt("Mercator_1SP", [("scale_factor", 1)], WGS84, "3857",
                tail=',EXTENSION["PROJ4","+proj=merc +a=6378137 +b=6378137 +lat_ts=0.0 +lon_0=0.0 +x_0=0.0 +y_0=0 '
                     '+k=1.0 +units=m +nadgrids=@null +wktext +no_defs"]'),
            wkt("Transverse_Mercator", list(utm.items()), GRS80, "28355", tail=',EXTENSION["PROJ4","+proj="]'),
            wkt("Sinusoidal", [], ("MODIS", 6371007.181, 0), tail=',EXTENSION["PROJ4","+proj=sinu +R=6371007.181"]')]
    # no projection the parser knows: the last EPSG authority, else a WKT2 ID
    geogcs = ('GEOGCS["WGS 84",DATUM["WGS_1984",SPHEROID["WGS 84",6378137,298.257223563,AUTHORITY["EPSG","7030"]],'
              'AUTHORITY["EPSG","6326"]],PRIMEM["Greenwich",0],UNIT["degree",0.0174532925199433]%s]')
    out += [geogcs % ',AUTHORITY["EPSG","4326"]', geogcs % ',AUTHORITY["EPSG","4283"]', geogcs % "",
            geogcs % ',AUTHORITY["EPSG",4326]', geogcs % ',AUTHORITY["epsg","4326"]', geogcs % ',AUTHORITY["EPSG","',
            'GEOGCRS["WGS 84",DATUM["World Geodetic System 1984",ELLIPSOID["WGS 84",6378137,298.257223563]],'
            'CS[ellipsoidal,2],ID["EPSG",4326]]',
            'PROJCRS["x",BASEGEOGCRS["WGS 84",ID["EPSG",4326]],CONVERSION["UTM zone 55S",ID["EPSG",17055]],'
            'ID["EPSG",32755]]', 'GEOGCRS["x",ID["EPSG","4326"]]', 'GEOGCRS["x",ID["EPSG",]]',
            geogcs % ',AUTHORITY["EPSG","0"],ID["EPSG",4326]', geogcs % ',AUTHORITY["EPSG","9999"],ID["EPSG",4326]',
            'GEOGCS["x",ID["EPSG",4326],AUTHORITY["EPSG","3857"]]',
            wkt("Albers_Conic_Equal_Area", [("standard_parallel_1", -18.0), ("standard_parallel_2", -36.0),
                                            ("longitude_of_center", 132.0)], GRS80),
            wkt("Albers_Conic_Equal_Area", [("standard_parallel_1", -18.0), ("standard_parallel_2", -36.0),
                                            ("longitude_of_center", 132.0)], GRS80, "3577"),
            wkt("Albers_Conic_Equal_Area", [], GRS80, "102003"), wkt("Oblique_Stereographic", [], BESSEL, "28992"),
            wkt("", [], WGS84, "32755"), wkt("", [], WGS84), 'PROJECTION["Transverse_Mercator"]',
            'PROJECTION["Mercator_1SP"]', 'PROJECTION["Geostationary_Satellite"]', 'PROJECTION["Sinusoidal"]',
            'PROJECTION["Polar_Stereographic"]', 'PROJECTION["transverse_mercator"]',
            'PROJECTION["Lambert_Conformal_Conic_1SP"],PROJECTION["Polar_Stereographic"],SPHEROID["x",6378137,298.25]',
            'PROJECTION["Mercator_2SP"],PROJECTION["Lambert_Azimuthal_Equal_Area"],PARAMETER["latitude_of_center",45]',
            'PROJECTION["Transverse_Mercator"],PROJECTION["Lambert_Conformal_Conic_2SP"],'
            'PARAMETER["standard_parallel_1",-18],PARAMETER["standard_parallel_2",-36]',
            'PROJECTION["Transverse_Mercator"],PARAMETER["scale_factor",],PARAMETER["false_easting",abc]',
            'PROJECTION["Transverse_Mercator"],PARAMETER["scale_factor", 0.5],PARAMETER["Scale_Factor",0.25]',
            'PROJECTION["Transverse_Mercator"],XPARAMETER["scale_factor",0.5],SPHEROID["x" , 6377397.155 , 299.15]']
    return out


def corpus_strings():
    out = epsg_strings() + name_strings() + proj_strings() + wkt_strings()
    return list(dict.fromkeys(out))


def record(strings):
    from gsky_amd import _lib
    L = _lib.lib()
    cases = []
    for s in strings:
        c = _lib.Crs()
        rc = L.gskyhip_crs_from_srs(s.encode(), ctypes.byref(c))
        cases.append([s, rc, bytes(c).hex() if rc == 0 else None])
    return cases


def main():
    from gsky_amd import _lib
    dirty = subprocess.check_output(["git", "status", "--porcelain", "--", "gsky_amd", "include"], cwd=ROOT).strip()
    if dirty:
        sys.exit("gsky_amd/ or include/ differ from HEAD: record the corpus from a clean build of a commit")
    commit = subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=ROOT).decode().strip()
    cases = record(corpus_strings())
    doc = {"commit": commit, "struct_size": ctypes.sizeof(_lib.Crs), "cases": cases}
    with open(OUT, "wb") as f:
        f.write(gzip.compress(json.dumps(doc, indent=0).encode("utf-8"), 9, mtime=0))
    ok = sum(1 for c in cases if c[1] == 0)
    print("%d strings (%d parsed, %d rejected) at %s -> %s (%d bytes)"
          % (len(cases), ok, len(cases) - ok, commit[:12], os.path.relpath(OUT, ROOT), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
