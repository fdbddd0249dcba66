// crs.cpp -- SRS text -> gskyhip_crs (crs.h): EPSG codes, PROJ strings and
// WKT1, and the set-up constants of every projection family.
//
// Host only, plain C++: nothing here needs the GPU, so tools/srs_check.cpp
// runs it under the host sanitizers.  The projections themselves (the
// forward / inverse of each kind) are gsky_device.h's; this file fills the
// struct they read, as include/gskyhip.h documents field by field.
#include "crs.h"

#include <strings.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

namespace gsky {
namespace {

constexpr double kD2R_h = 0.017453292519943295769236907684886;
constexpr double kHalfPi = 1.57079632679489661923;
constexpr double kPi = 3.14159265358979323846;
// the laea aspect in gskyhip_crs.phi2 (include/gskyhip.h, GSKYHIP_CRS_LAEA)
constexpr int kLaeaNPole = 0, kLaeaSPole = 1, kLaeaEquit = 2, kLaeaObliq = 3;

// tm_gatg / tm_clens / lcc_tsfn of gsky_device.h restated for the host (as
// h_qsfn below restates qsfn): the set-up needs them once per parsed string.
double tm_gatg(const double *p1, int len, double B) {
  const double cos_2B = 2 * std::cos(2 * B);
  const double *p = p1 + len;
  double h = 0, h1 = *--p, h2 = 0;
  while (p - p1) {
    h = -h2 + cos_2B * h1 + *--p;
    h2 = h1;
    h1 = h;
  }
  return B + h * std::sin(2 * B);
}

double tm_clens(const double *a, int size, double arg_r) {
  const double *p = a + size;
  const double r = 2 * std::cos(arg_r);
  double hr1 = 0, hr = *--p, hr2;
  for (; a - p;) {
    hr2 = hr1;
    hr1 = hr;
    hr = -hr2 + r * hr1 + *--p;
  }
  return std::sin(arg_r) * hr;
}

double lcc_tsfn(double phi, double sinphi, double e) {
  sinphi *= e;
  return std::tan(.5 * (kHalfPi - phi)) / std::pow((1. - sinphi) / (1. + sinphi), .5 * e);
}

void set_ellps(gskyhip_crs *c, double a, double rf) {
  c->a = a;
  c->ra = 1.0 / a;
  if (rf == 0.0) c->es = 0.0;
  else { double f = 1.0 / rf; c->es = 2 * f - f * f; }
  c->e = std::sqrt(c->es);
  c->one_es = 1.0 - c->es;
}

double h_qsfn(double sinphi, double e, double one_es) {
  if (e >= 1.0e-7) {
    double con = e * sinphi;
    double div1 = 1.0 - con * con;
    double div2 = 1.0 + con;
    if (div1 == 0.0 || div2 == 0.0) return HUGE_VAL;
    return one_es * (sinphi / div1 - (.5 / e) * std::log((1. - con) / div2));
  }
  return sinphi + sinphi;
}

// aea.cpp setup() of PROJ 6.1.1
int aea_setup(gskyhip_crs *c) {
  const double phi1 = c->phi1, phi2 = c->phi2;
  if (std::fabs(phi1 + phi2) < 1e-10) return GSKYHIP_E_CRS;
  double sinphi = std::sin(phi1), cosphi = std::cos(phi1);
  c->n = sinphi;
  const bool secant = std::fabs(phi1 - phi2) >= 1e-10;
  if (c->es > 0.) {
    const double m1 = cosphi / std::sqrt(1. - c->es * sinphi * sinphi);
    const double ml1 = h_qsfn(sinphi, c->e, c->one_es);
    if (secant) {
      const double s2 = std::sin(phi2), c2 = std::cos(phi2);
      const double m2 = c2 / std::sqrt(1. - c->es * s2 * s2);
      const double ml2 = h_qsfn(s2, c->e, c->one_es);
      if (ml2 == ml1) return GSKYHIP_E_CRS;
      c->n = (m1 * m1 - m2 * m2) / (ml2 - ml1);
    }
    c->ec = 1. - .5 * c->one_es * std::log((1. - c->e) / (1. + c->e)) / c->e;
    c->c = m1 * m1 + c->n * ml1;
    c->dd = 1. / c->n;
    c->rho0 = c->dd * std::sqrt(c->c - c->n * h_qsfn(std::sin(c->phi0), c->e, c->one_es));
  } else {
    if (secant) c->n = .5 * (c->n + std::sin(phi2));
    const double n2 = c->n + c->n;
    c->c = cosphi * cosphi + n2 * sinphi;
    c->dd = 1. / c->n;
    c->rho0 = c->dd * std::sqrt(c->c - n2 * std::sin(c->phi0));
  }
  return 0;
}

// tmerc.cpp setup_exact() of PROJ 6.1.1 (the Poder / Engsager series,
// gsky_device.h tm_fwd / tm_inv): third flattening n, the 6th-order series
// coefficients, the normalised meridian quadrant Qn and the northing of the
// origin latitude Zb.  Ellipsoids only (the spherical tmerc is not carried).
int tmerc_setup(gskyhip_crs *c) {
  if (!(c->es > 0)) return GSKYHIP_E_CRS;
  c->kind = GSKYHIP_CRS_TMERC;
  const double f = c->es / (1 + std::sqrt(1 - c->es));
  const double n = f / (2 - f);
  double np = n;
  double *cgb = c->tm_cgb, *cbg = c->tm_cbg, *utg = c->tm_utg, *gtu = c->tm_gtu;
  cgb[0] = n * (2 + n * (-2 / 3.0 + n * (-2 + n * (116 / 45.0 + n * (26 / 45.0 + n * (-2854 / 675.0))))));
  cbg[0] = n * (-2 + n * (2 / 3.0 + n * (4 / 3.0 + n * (-82 / 45.0 + n * (32 / 45.0 + n * (4642 / 4725.0))))));
  np *= n;
  cgb[1] = np * (7 / 3.0 + n * (-8 / 5.0 + n * (-227 / 45.0 + n * (2704 / 315.0 + n * (2323 / 945.0)))));
  cbg[1] = np * (5 / 3.0 + n * (-16 / 15.0 + n * (-13 / 9.0 + n * (904 / 315.0 + n * (-1522 / 945.0)))));
  np *= n;
  cgb[2] = np * (56 / 15.0 + n * (-136 / 35.0 + n * (-1262 / 105.0 + n * (73814 / 2835.0))));
  cbg[2] = np * (-26 / 15.0 + n * (34 / 21.0 + n * (8 / 5.0 + n * (-12686 / 2835.0))));
  np *= n;
  cgb[3] = np * (4279 / 630.0 + n * (-332 / 35.0 + n * (-399572 / 14175.0)));
  cbg[3] = np * (1237 / 630.0 + n * (-12 / 5.0 + n * (-24832 / 14175.0)));
  np *= n;
  cgb[4] = np * (4174 / 315.0 + n * (-144838 / 6237.0));
  cbg[4] = np * (-734 / 315.0 + n * (109598 / 31185.0));
  np *= n;
  cgb[5] = np * (601676 / 22275.0);
  cbg[5] = np * (444337 / 155925.0);
  np = n * n;
  c->tm_qn = c->k0 / (1 + n) * (1 + np * (1 / 4.0 + np * (1 / 64.0 + np / 256.0)));
  utg[0] = n * (-0.5 + n * (2 / 3.0 + n * (-37 / 96.0 + n * (1 / 360.0 + n * (81 / 512.0 + n * (-96199 / 604800.0))))));
  gtu[0] = n * (0.5 + n * (-2 / 3.0 + n * (5 / 16.0 + n * (41 / 180.0 + n * (-127 / 288.0 + n * (7891 / 37800.0))))));
  utg[1] = np * (-1 / 48.0 + n * (-1 / 15.0 + n * (437 / 1440.0 + n * (-46 / 105.0 + n * (1118711 / 3870720.0)))));
  gtu[1] = np * (13 / 48.0 + n * (-3 / 5.0 + n * (557 / 1440.0 + n * (281 / 630.0 + n * (-1983433 / 1935360.0)))));
  np *= n;
  utg[2] = np * (-17 / 480.0 + n * (37 / 840.0 + n * (209 / 4480.0 + n * (-5569 / 90720.0))));
  gtu[2] = np * (61 / 240.0 + n * (-103 / 140.0 + n * (15061 / 26880.0 + n * (167603 / 181440.0))));
  np *= n;
  utg[3] = np * (-4397 / 161280.0 + n * (11 / 504.0 + n * (830251 / 7257600.0)));
  gtu[3] = np * (49561 / 161280.0 + n * (-179 / 168.0 + n * (6601661 / 7257600.0)));
  np *= n;
  utg[4] = np * (-4583 / 161280.0 + n * (108847 / 3991680.0));
  gtu[4] = np * (34729 / 80640.0 + n * (-3418889 / 1995840.0));
  np *= n;
  utg[5] = np * (-20648693 / 638668800.0);
  gtu[5] = np * (212378941 / 319334400.0);
  const double Z = tm_gatg(cbg, 6, c->phi0);   // Gaussian latitude of the origin
  c->tm_zb = -c->tm_qn * (Z + tm_clens(gtu, 6, 2 * Z));
  return 0;
}

// lcc.cpp setup() of PROJ 6.1.1 for an ellipsoid (pj_msfn / pj_tsfn): the
// cone constant n (one standard parallel: its sine; two: the secant form),
// c and rho0.  phi1 / phi2 / phi0 / k0 set by the caller.
int lcc_setup(gskyhip_crs *c) {
  if (!(c->es > 0)) return GSKYHIP_E_CRS;   // the spherical lcc is not carried
  c->kind = GSKYHIP_CRS_LCC;
  const double phi1 = c->phi1, phi2 = c->phi2;
  if (std::fabs(phi1 + phi2) < 1e-10) return GSKYHIP_E_CRS;
  double sinphi = std::sin(phi1);
  const double cosphi = std::cos(phi1);
  c->n = sinphi;
  const bool secant = std::fabs(phi1 - phi2) >= 1e-10;
  auto msfn = [&](double s, double co) { return co / std::sqrt(1. - c->es * s * s); };
  const double m1 = msfn(sinphi, cosphi);
  const double ml1 = lcc_tsfn(phi1, sinphi, c->e);
  if (secant) {
    sinphi = std::sin(phi2);
    c->n = std::log(m1 / msfn(sinphi, std::cos(phi2)));
    c->n /= std::log(ml1 / lcc_tsfn(phi2, sinphi, c->e));
  }
  c->c = c->rho0 = m1 * std::pow(ml1, -c->n) / c->n;
  c->rho0 *= (std::fabs(std::fabs(c->phi0) - kHalfPi) < 1e-10) ? 0.
                                                                : std::pow(lcc_tsfn(c->phi0, std::sin(c->phi0), c->e), c->n);
  return 0;
}

// stere.cpp setup() of PROJ 6.1.1, polar aspects on an ellipsoid: phi0 =
// +-pi/2 picks the pole, |lat_ts| the true-scale parallel (pi/2: k0 at the
// pole); akm1 into c->c.
int stere_polar_setup(gskyhip_crs *c, double phi0, bool has_ts, double lat_ts) {
  if (!(c->es > 0)) return GSKYHIP_E_CRS;   // the spherical stere is not carried
  if (std::fabs(std::fabs(phi0) - kHalfPi) >= 1e-10) return GSKYHIP_E_CRS;   // oblique / equatorial: not carried
  c->kind = GSKYHIP_CRS_STERE_POLAR;
  c->phi0 = phi0 < 0 ? -kHalfPi : kHalfPi;
  const double phits = std::fabs(has_ts ? lat_ts : kHalfPi);
  c->phi1 = phits;
  const double e = c->e;
  if (std::fabs(phits - kHalfPi) < 1e-10) {
    c->c = 2. * c->k0 / std::sqrt(std::pow(1 + e, 1 + e) * std::pow(1 - e, 1 - e));
  } else {
    double t = std::sin(phits);
    c->c = std::cos(phits) / lcc_tsfn(phits, t, e);
    t *= e;
    c->c /= std::sqrt(1. - t * t);
  }
  return 0;
}

// geos.cpp setup() of PROJ 6.1.1: the satellite height above the ellipsoid
// and the sweep axis; constants in units of the semi-major axis, assigned as
// gsky_device.h geos_fwd / geos_inv (and include/gskyhip.h) document.  A
// sphere (es == 0) runs the same expressions with radius_p = 1.
int geos_setup(gskyhip_crs *c, double h, bool sweep_x) {
  if (!(h > 0.)) return GSKYHIP_E_CRS;
  c->kind = GSKYHIP_CRS_GEOS;
  c->phi0 = 0.0;
  c->k0 = 1.0;
  c->phi1 = h / c->a;                  // radius_g_1
  c->phi2 = sweep_x ? 1.0 : 0.0;       // flip_axis
  c->n = 1. + c->phi1;                 // radius_g
  c->c = c->n * c->n - 1.0;            // C
  if (c->es != 0.0) {
    c->dd = std::sqrt(c->one_es);      // radius_p
    c->rho0 = c->one_es;               // radius_p2
    c->ec = 1. / c->one_es;            // radius_p_inv2
  } else {
    c->dd = c->rho0 = c->ec = 1.0;
  }
  return 0;
}

// pj_authset() of PROJ 6.1.1: the three-term series authalic -> geodetic
// latitude (Snyder 3-18), into tm_cgb[0..2] (gsky_device.h ea_authlat).
void authalic_setup(gskyhip_crs *c) {
  const double es = c->es, es2 = es * es, es3 = es2 * es;
  c->tm_cgb[0] = es * (1 / 3.0) + es2 * (31 / 180.0) + es3 * (517 / 5040.0);
  c->tm_cgb[1] = es2 * (23 / 360.0) + es3 * (251 / 3780.0);
  c->tm_cgb[2] = es3 * (761 / 45360.0);
}

// laea.cpp setup() of PROJ 6.1.1: the aspect from lat_0, and on an ellipsoid
// qp, rq, dd, xmf, ymf and the authalic latitude of the centre; assigned as
// include/gskyhip.h documents.  phi0 / lam0 / x0 / y0 set by the caller.
int laea_setup(gskyhip_crs *c) {
  const double t = std::fabs(c->phi0);
  if (!(t <= kHalfPi + 1e-10)) return GSKYHIP_E_CRS;
  c->kind = GSKYHIP_CRS_LAEA;
  c->k0 = 1.0;
  c->phi1 = 0.0;
  int mode;
  if (std::fabs(t - kHalfPi) < 1e-10) {
    mode = c->phi0 < 0 ? kLaeaSPole : kLaeaNPole;
    c->phi0 = c->phi0 < 0 ? -kHalfPi : kHalfPi;
  } else if (t < 1e-10) {
    mode = kLaeaEquit;
  } else {
    mode = kLaeaObliq;
  }
  c->phi2 = mode;
  c->n = 2.0; c->c = 1.0; c->dd = 1.0; c->rho0 = 1.0; c->ec = 1.0;
  c->tm_qn = 0.0; c->tm_zb = 1.0;   // sinb1, cosb1 (equatorial)
  if (c->es != 0.) {
    c->n = h_qsfn(1., c->e, c->one_es);   // qp
    authalic_setup(c);
    if (mode == kLaeaEquit) {
      c->c = std::sqrt(.5 * c->n);
      c->dd = 1. / c->c;
      c->rho0 = 1.;
      c->ec = .5 * c->n;
    } else if (mode == kLaeaObliq) {
      c->c = std::sqrt(.5 * c->n);
      const double sinphi = std::sin(c->phi0);
      c->tm_qn = h_qsfn(sinphi, c->e, c->one_es) / c->n;
      c->tm_zb = std::sqrt(1. - c->tm_qn * c->tm_qn);
      c->dd = std::cos(c->phi0) / (std::sqrt(1. - c->es * sinphi * sinphi) * c->c * c->tm_zb);
      c->ec = c->c / c->dd;
      c->rho0 = c->c * c->dd;
    }
  } else if (mode == kLaeaObliq) {
    c->tm_qn = std::sin(c->phi0);
    c->tm_zb = std::cos(c->phi0);
  }
  return 0;
}

// k0 of a cylindrical projection true to scale at lat_ts (pj_msfn).
double ts_k0(const gskyhip_crs *c, double lat_ts) {
  const double s = std::sin(lat_ts);
  return std::cos(lat_ts) / std::sqrt(1. - c->es * s * s);
}

// cea.cpp setup() of PROJ 6.1.1: k0 from +lat_ts, else +k_0; qp.
int cea_setup(gskyhip_crs *c, bool has_ts, double lat_ts, double k0) {
  if (has_ts && !(std::fabs(lat_ts) < kHalfPi)) return GSKYHIP_E_CRS;
  if (!has_ts && !(k0 > 0)) return GSKYHIP_E_CRS;
  c->kind = GSKYHIP_CRS_CEA;
  c->phi0 = 0.0; c->phi2 = 0.0;
  c->phi1 = has_ts ? lat_ts : 0.0;
  c->k0 = has_ts ? ts_k0(c, lat_ts) : k0;
  c->n = 2.0;
  if (c->es != 0.) {
    c->n = h_qsfn(1., c->e, c->one_es);
    authalic_setup(c);
  }
  return 0;
}

// merc.cpp setup() of PROJ 6.1.1: k0 from +lat_ts (2SP), else +k_0 (1SP).
// The sphere with k0 = 1 stays GSKYHIP_CRS_WEBMERC (the callers see to it).
int merc_setup(gskyhip_crs *c, bool has_ts, double lat_ts, double k0) {
  if (has_ts && !(std::fabs(lat_ts) < kHalfPi)) return GSKYHIP_E_CRS;
  if (!has_ts && !(k0 > 0)) return GSKYHIP_E_CRS;
  c->kind = GSKYHIP_CRS_MERC;
  c->phi0 = 0.0; c->phi2 = 0.0;
  c->phi1 = has_ts ? std::fabs(lat_ts) : 0.0;
  c->k0 = has_ts ? ts_k0(c, c->phi1) : k0;
  return 0;
}

// Mercator on a sphere, true to scale at the equator: the web-mercator kind.
bool merc_is_web(const gskyhip_crs *c, bool has_ts, double lat_ts, double k0) {
  return c->es == 0.0 && (!has_ts || lat_ts == 0.0) && k0 == 1.0;
}

// utm.cpp setup: zone -> central meridian, k0 0.9996, false easting 500 km,
// false northing 10,000 km in the south.
int utm_setup(gskyhip_crs *c, int zone, bool south) {
  if (zone < 1 || zone > 60) return GSKYHIP_E_CRS;
  c->lam0 = (zone - 0.5) * (kPi / 30.0) - kPi;   // PROJ: (zone - .5) * M_PI / 30. - M_PI
  c->phi0 = 0.0;
  c->k0 = 0.9996;
  c->x0 = 500000.0;
  c->y0 = south ? 10000000.0 : 0.0;
  return tmerc_setup(c);
}

double proj_param(const std::string &s, const char *key, double dflt, bool *found = nullptr) {
  const std::string k = std::string(key) + "=";
  size_t pos = 0;
  while ((pos = s.find(k, pos)) != std::string::npos) {
    if (pos == 0 || s[pos - 1] == ' ' || s[pos - 1] == '+') {
      if (found) *found = true;
      return std::strtod(s.c_str() + pos + k.size(), nullptr);
    }
    pos += k.size();
  }
  if (found) *found = false;
  return dflt;
}

int crs_epsg(int code, gskyhip_crs *c) {
  std::memset(c, 0, sizeof(*c));
  c->k0 = 1.0;
  switch (code) {
    case 4326: c->kind = GSKYHIP_CRS_LONGLAT; set_ellps(c, 6378137.0, 298.257223563); return 0;
    case 4283: c->kind = GSKYHIP_CRS_LONGLAT; set_ellps(c, 6378137.0, 298.257222101); return 0;
    case 3857: case 900913: c->kind = GSKYHIP_CRS_WEBMERC; set_ellps(c, 6378137.0, 0.0); return 0;
    case 3577:
      c->kind = GSKYHIP_CRS_AEA;
      set_ellps(c, 6378137.0, 298.257222101);
      c->lam0 = 132.0 * kD2R_h; c->phi0 = 0.0; c->phi1 = -18.0 * kD2R_h; c->phi2 = -36.0 * kD2R_h;
      return aea_setup(c);
    default: break;
  }
  // Transverse Mercator zones: WGS 84 / UTM north (326zz) and south (327zz),
  // GDA94 / MGA (283zz, zones 48-58) and GDA2020 / MGA (78zz, zones 46-59);
  // both GDA datums on GRS80, taken without a datum shift like EPSG:3577
  if (code >= 32601 && code <= 32660) { set_ellps(c, 6378137.0, 298.257223563); return utm_setup(c, code - 32600, false); }
  if (code >= 32701 && code <= 32760) { set_ellps(c, 6378137.0, 298.257223563); return utm_setup(c, code - 32700, true); }
  if (code >= 28348 && code <= 28358) { set_ellps(c, 6378137.0, 298.257222101); return utm_setup(c, code - 28300, true); }
  if (code >= 7846 && code <= 7859) { set_ellps(c, 6378137.0, 298.257222101); return utm_setup(c, code - 7800, true); }
  if (code == 3031 || code == 3413 || code == 3976) {   // WGS 84 polar stereographic (Antarctic, NSIDC)
    set_ellps(c, 6378137.0, 298.257223563);
    c->lam0 = (code == 3413 ? -45.0 : 0.0) * kD2R_h;
    const double ts = code == 3031 ? -71.0 : code == 3413 ? 70.0 : -70.0;
    return stere_polar_setup(c, (ts < 0 ? -90.0 : 90.0) * kD2R_h, true, ts * kD2R_h);
  }
  if (code == 32661 || code == 32761) {   // WGS 84 / UPS North / South
    set_ellps(c, 6378137.0, 298.257223563);
    c->k0 = 0.994; c->x0 = 2000000.0; c->y0 = 2000000.0;
    return stere_polar_setup(c, (code == 32661 ? 90.0 : -90.0) * kD2R_h, false, 0.0);
  }
  if (code == 3112 || code == 7845) {   // GDA94 / GDA2020 Geoscience Australia Lambert
    set_ellps(c, 6378137.0, 298.257222101);
    c->phi1 = -18.0 * kD2R_h; c->phi2 = -36.0 * kD2R_h; c->phi0 = 0.0; c->lam0 = 134.0 * kD2R_h;
    return lcc_setup(c);
  }
  if (code == 3035) {   // ETRS89-extended / LAEA Europe
    set_ellps(c, 6378137.0, 298.257222101);
    c->phi0 = 52.0 * kD2R_h; c->lam0 = 10.0 * kD2R_h; c->x0 = 4321000.0; c->y0 = 3210000.0;
    return laea_setup(c);
  }
  if (code == 6931 || code == 6932 || code == 3408 || code == 3409) {   // EASE-Grid 2.0 / EASE-Grid North, South
    if (code > 6000) set_ellps(c, 6378137.0, 298.257223563);
    else set_ellps(c, 6371228.0, 0.0);
    c->phi0 = ((code == 6931 || code == 3408) ? 90.0 : -90.0) * kD2R_h;
    return laea_setup(c);
  }
  if (code == 6933 || code == 3410) {   // EASE-Grid 2.0 / EASE-Grid Global
    if (code == 6933) set_ellps(c, 6378137.0, 298.257223563);
    else set_ellps(c, 6371228.0, 0.0);
    return cea_setup(c, true, 30.0 * kD2R_h, 1.0);
  }
  if (code == 3395 || code == 3832) {   // WGS 84 / World Mercator, PDC Mercator
    set_ellps(c, 6378137.0, 298.257223563);
    c->lam0 = (code == 3832 ? 150.0 : 0.0) * kD2R_h;
    return merc_setup(c, false, 0.0, 1.0);
  }
  return GSKYHIP_E_CRS;
}

// The ellipsoid of a PROJ string of the equal-area / Mercator families: the
// forms crs_proj4 takes (+ellps / +datum, +a +rf, +R), and +a +b, +a +es
// (+proj=geos, whose operators publish +a +b, does not read +es).
void proj4_ellps(const std::string &s, gskyhip_crs *c, double a, double rf, double R, bool read_es = true) {
  set_ellps(c, a, rf);
  if (R > 0 || rf != 0) return;
  bool has_b = false, has_es = false;
  const double b = proj_param(s, "+b", 0, &has_b), es = read_es ? proj_param(s, "+es", 0, &has_es) : 0;
  if (has_es && es >= 0 && es < 1) c->es = es;
  else if (has_b && b > 0) c->es = 1.0 - (b * b) / (a * a);
  else return;
  c->e = std::sqrt(c->es);
  c->one_es = 1.0 - c->es;
}

// +k_0, else +k, else 1.
double proj4_k0(const std::string &s) {
  bool has_k = false;
  const double k0 = proj_param(s, "+k_0", 1.0, &has_k);
  return has_k ? k0 : proj_param(s, "+k", 1.0);
}

int crs_proj4(const std::string &s, gskyhip_crs *c) {
  std::memset(c, 0, sizeof(*c));
  c->k0 = 1.0;
  bool has_a = false;
  double a = proj_param(s, "+a", 0, &has_a);
  double R = proj_param(s, "+R", 0);
  double rf = proj_param(s, "+rf", 0);
  if (s.find("+ellps=GRS80") != std::string::npos) { a = 6378137.0; rf = 298.257222101; has_a = true; }
  else if (s.find("+ellps=WGS84") != std::string::npos || s.find("+datum=WGS84") != std::string::npos) {
    a = 6378137.0; rf = 298.257223563; has_a = true;
  }
  if (R > 0) { a = R; rf = 0; has_a = true; }
  if (!has_a) { a = 6378137.0; rf = 298.257223563; }
  c->lam0 = proj_param(s, "+lon_0", 0) * kD2R_h;
  c->phi0 = proj_param(s, "+lat_0", 0) * kD2R_h;
  c->x0 = proj_param(s, "+x_0", 0);
  c->y0 = proj_param(s, "+y_0", 0);
  bool has_ts = false;   // +lat_ts | +k_0 of the families that take them
  const double ts = proj_param(s, "+lat_ts", 0, &has_ts) * kD2R_h, k0 = proj4_k0(s);
  if (s.find("+proj=longlat") != std::string::npos || s.find("+proj=latlong") != std::string::npos) {
    c->kind = GSKYHIP_CRS_LONGLAT; set_ellps(c, a, rf); return 0;
  }
  if (s.find("+proj=webmerc") != std::string::npos) {
    c->kind = GSKYHIP_CRS_WEBMERC; set_ellps(c, a, 0.0); return 0;
  }
  if (s.find("+proj=merc") != std::string::npos) {   // merc.cpp; the k0 = 1 sphere is the web-mercator kind
    proj4_ellps(s, c, a, rf, R);
    if (merc_is_web(c, has_ts, ts, k0)) { c->kind = GSKYHIP_CRS_WEBMERC; set_ellps(c, a, 0.0); return 0; }
    return merc_setup(c, has_ts, ts, k0);
  }
  if (s.find("+proj=laea") != std::string::npos) {   // laea.cpp
    proj4_ellps(s, c, a, rf, R);
    if (!(std::fabs(c->phi0) <= kHalfPi + 1e-10)) return GSKYHIP_E_CRS;
    return laea_setup(c);
  }
  if (s.find("+proj=cea") != std::string::npos) {   // cea.cpp
    proj4_ellps(s, c, a, rf, R);
    return cea_setup(c, has_ts, ts, k0);
  }
  if (s.find("+proj=aea") != std::string::npos) {
    c->kind = GSKYHIP_CRS_AEA; set_ellps(c, a, rf);
    c->phi1 = proj_param(s, "+lat_1", 0) * kD2R_h;
    c->phi2 = proj_param(s, "+lat_2", 0) * kD2R_h;
    return aea_setup(c);
  }
  if (s.find("+proj=sinu") != std::string::npos) {
    c->kind = GSKYHIP_CRS_SINU; set_ellps(c, a, rf);
    return c->es == 0 ? 0 : GSKYHIP_E_CRS;  // only the spherical form (MODIS)
  }
  if (s.find("+proj=utm") != std::string::npos) {
    set_ellps(c, a, rf);
    bool has_zone = false;
    const double zone = proj_param(s, "+zone", 0, &has_zone);
    if (!has_zone || zone != std::floor(zone)) return GSKYHIP_E_CRS;   // PROJ guesses from lon_0: not carried
    return utm_setup(c, (int)zone, s.find("+south") != std::string::npos);
  }
  if (s.find("+proj=ups") != std::string::npos) {   // ups: stere at a pole, k0 0.994, false E / N 2000 km
    set_ellps(c, a, rf);
    c->k0 = 0.994; c->x0 = 2000000.0; c->y0 = 2000000.0; c->lam0 = 0.0;
    return stere_polar_setup(c, (s.find("+south") != std::string::npos ? -90.0 : 90.0) * kD2R_h, false, 0.0);
  }
  if (s.find("+proj=stere ") != std::string::npos ||
      (s.size() >= 11 && s.compare(s.size() - 11, 11, "+proj=stere") == 0)) {
    set_ellps(c, a, rf);
    c->k0 = k0;
    return stere_polar_setup(c, c->phi0, has_ts, ts);
  }
  if (s.find("+proj=geos") != std::string::npos) {   // geos.cpp: +h required and positive, +sweep x or y
    bool has_b = false, has_h = false;
    const double b = proj_param(s, "+b", 0, &has_b);
    if (has_b && rf == 0 && !(R > 0) && !(b > 0)) return GSKYHIP_E_CRS;   // (the other families ignore such a +b)
    proj4_ellps(s, c, a, rf, R, false);   // +a +b (the form satellite operators publish): es = 1 - b^2 / a^2
    const double h = proj_param(s, "+h", 0, &has_h);
    if (!has_h) return GSKYHIP_E_CRS;
    bool sweep_x = false;
    const size_t sw = s.find("+sweep=");
    if (sw != std::string::npos) {
      const char ax = s[sw + 7];
      const char nx = sw + 8 < s.size() ? s[sw + 8] : ' ';
      if ((ax != 'x' && ax != 'y') || (nx != ' ' && nx != '\0')) return GSKYHIP_E_CRS;
      sweep_x = ax == 'x';
    }
    return geos_setup(c, h, sweep_x);
  }
  if (s.find("+proj=lcc") != std::string::npos) {   // lcc.cpp: one parallel -> the tangent cone at it
    set_ellps(c, a, rf);
    bool has_l1 = false, has_l2 = false, has_l0 = false;
    c->phi1 = proj_param(s, "+lat_1", 0, &has_l1) * kD2R_h;
    c->phi2 = proj_param(s, "+lat_2", 0, &has_l2) * kD2R_h;
    proj_param(s, "+lat_0", 0, &has_l0);
    if (!has_l2) {
      c->phi2 = c->phi1;
      if (!has_l0) c->phi0 = c->phi1;
    }
    c->k0 = k0;
    return lcc_setup(c);
  }
  if (s.find("+proj=tmerc") != std::string::npos || s.find("+proj=etmerc") != std::string::npos) {
    if (s.find("+approx") != std::string::npos) return GSKYHIP_E_CRS;   // Evenden / Snyder series: not carried
    set_ellps(c, a, rf);
    c->k0 = k0;
    return tmerc_setup(c);
  }
  return GSKYHIP_E_CRS;
}

// The PROJECTION names the WKT1 reader knows, in the order it looks for them
// (a string that names two goes by the earlier one).
const char *const kWktProjections[] = {
    "Sinusoidal", "Polar_Stereographic", "Geostationary_Satellite", "Lambert_Azimuthal_Equal_Area",
    "Cylindrical_Equal_Area", "Mercator_2SP", "Mercator_1SP", "Lambert_Conformal_Conic_2SP",
    "Lambert_Conformal_Conic_1SP", "Transverse_Mercator"};

// What parse_srs reads of a WKT1 (GDAL) string, read once.  Nodes are found
// by their text, not their nesting: the first SPHEROID[ and the first
// PARAMETER["name", count.
struct Wkt1 {
  const std::string &s;
  std::string projection, proj4;   // of kWktProjections, else ""; EXTENSION["PROJ4" up to its closing bracket
  bool has_a = false, has_epsg = false;   // a SPHEROID[ with a comma after it; wkt_epsg_code
  double a = 6378137.0, rf = 298.257223563;   // of that SPHEROID: semi-major axis and, where one follows, 1 / f
  int epsg = 0;

  explicit Wkt1(const std::string &text) : s(text) {
    for (const char *name : kWktProjections)
      if (s.find(std::string("PROJECTION[\"") + name + "\"]") != std::string::npos) { projection = name; break; }
    const size_t p = s.find("SPHEROID["), q = p == std::string::npos ? p : s.find(',', p);
    if (q != std::string::npos) {
      char *end = nullptr;
      has_a = true;
      a = std::strtod(s.c_str() + q + 1, &end);
      if (end && *end == ',') rf = std::strtod(end + 1, nullptr);
    }
    has_epsg = wkt_epsg_code(s, &epsg);
    const size_t ext = s.find("EXTENSION[\"PROJ4\""), close = ext == std::string::npos ? ext : s.find(']', ext);
    if (ext != std::string::npos) proj4 = s.substr(ext, close == std::string::npos ? close : close - ext);
  }

  double param(const char *name, double dflt) const {
    const std::string k = std::string("PARAMETER[\"") + name + "\",";
    const size_t p = s.find(k);
    return p == std::string::npos ? dflt : std::strtod(s.c_str() + p + k.size(), nullptr);
  }
};

// A WKT1 node of a projection family: its parameters (each family's own
// names and defaults) into the struct, then the family's set-up.
int crs_wkt1(const Wkt1 &w, gskyhip_crs *c) {
  const std::string &p = w.projection;
  if (p == "Sinusoidal") {   // the sphere of the semi-major axis; nothing else is read
    char buf[96];
    std::snprintf(buf, sizeof(buf), "+proj=sinu +R=%.17g", w.has_a ? w.a : 6371007.181);
    return crs_proj4(buf, c);
  }
  const bool laea = p == "Lambert_Azimuthal_Equal_Area", cea = p == "Cylindrical_Equal_Area";
  const bool merc2 = p == "Mercator_2SP", merc = merc2 || p == "Mercator_1SP";
  // equal-area / Mercator: a known top-level code, else the parameters
  // (EPSG:3857 is a Mercator_1SP node over the WGS 84 spheroid)
  if ((laea || cea || merc) && w.has_epsg && crs_epsg(w.epsg, c) == 0) return 0;
  std::memset(c, 0, sizeof(*c));
  set_ellps(c, w.a, w.rf);
  const double lat0 = w.param("latitude_of_origin", 0), cm = w.param("central_meridian", 0);
  const double sp1 = w.param("standard_parallel_1", 0) * kD2R_h, k0 = w.param("scale_factor", 1.0);
  c->lam0 = cm * kD2R_h;
  c->x0 = w.param("false_easting", 0);
  c->y0 = w.param("false_northing", 0);
  c->k0 = 1.0;
  if (p == "Polar_Stereographic") {   // latitude_of_origin is lat_ts, the pole without it
    const double ts = w.param("latitude_of_origin", 90.0);
    c->k0 = k0;
    return stere_polar_setup(c, (ts < 0 ? -90.0 : 90.0) * kD2R_h, std::fabs(std::fabs(ts) - 90.0) > 1e-12,
                             ts * kD2R_h);
  }
  if (p == "Geostationary_Satellite")   // no sweep parameter in WKT1: GDAL carries +sweep=x in the PROJ4 extension
    return geos_setup(c, w.param("satellite_height", 0), w.proj4.find("+sweep=x") != std::string::npos);
  if (laea) {
    const double lat = w.param("latitude_of_center", 0);
    if (!(std::fabs(lat) <= 90.0)) return GSKYHIP_E_CRS;
    c->phi0 = lat * kD2R_h;
    c->lam0 = w.param("longitude_of_center", 0) * kD2R_h;
    return laea_setup(c);
  }
  if (cea) return cea_setup(c, true, sp1, 1.0);
  if (merc) {   // 2SP: the standard parallel; 1SP: the scale factor
    const double ts = merc2 ? sp1 : 0.0, k = merc2 ? 1.0 : k0;
    if (merc_is_web(c, merc2, ts, k)) { c->kind = GSKYHIP_CRS_WEBMERC; return 0; }
    return merc_setup(c, merc2, ts, k);
  }
  c->phi0 = lat0 * kD2R_h;
  if (p != "Transverse_Mercator") {   // Lambert_Conformal_Conic_2SP, or _1SP: the tangent cone at the origin
    const bool two = p == "Lambert_Conformal_Conic_2SP";
    c->k0 = two ? 1.0 : k0;
    c->phi1 = two ? sp1 : c->phi0;
    c->phi2 = two ? w.param("standard_parallel_2", 0) * kD2R_h : c->phi0;
    return lcc_setup(c);
  }
  // a UTM zone's parameters become +proj=utm in PROJ 6 (Conversion's isUTM
  // when exporting the PROJ string): the zone's own central meridian
  c->k0 = k0;
  const double zone = (cm + 183.0) / 6.0;
  if (lat0 == 0 && k0 == 0.9996 && c->x0 == 500000.0 && (c->y0 == 0 || c->y0 == 10000000.0) &&
      zone == std::floor(zone) && zone >= 1 && zone <= 60)
    return utm_setup(c, (int)zone, c->y0 != 0);
  return tmerc_setup(c);
}

}  // namespace

bool wkt_epsg_code(const std::string &text, int *code) {
  static const char key[] = "AUTHORITY[\"EPSG\",\"";
  const size_t p = text.rfind(key);
  if (p != std::string::npos) *code = std::atoi(text.c_str() + p + sizeof(key) - 1);
  return p != std::string::npos;
}

int parse_srs(const char *srs, gskyhip_crs *c) {
  if (!srs) return GSKYHIP_E_CRS;
  std::string s(srs);
  auto ieq = [](const std::string &a, const char *b) { return strcasecmp(a.c_str(), b) == 0; };
  if (ieq(s, "MODIS") || ieq(s, "SR-ORG:6842")) return crs_proj4("+proj=sinu +R=6371007.181", c);
  if (s.size() > 5 && strncasecmp(s.c_str(), "EPSG:", 5) == 0) return crs_epsg(std::atoi(s.c_str() + 5), c);
  // (a WKT1 Geostationary_Satellite node may carry a PROJ string in its EXTENSION: parsed as WKT below)
  if (s.find("+proj=") != std::string::npos && s.find("PROJECTION[\"Geostationary_Satellite\"]") == std::string::npos)
    return crs_proj4(s, c);
  // WKT: a projection family's node, else the top-level (last) EPSG authority
  const Wkt1 w(s);
  if (!w.projection.empty()) return crs_wkt1(w, c);
  if (w.has_epsg) return crs_epsg(w.epsg, c);
  const size_t pos = s.rfind("ID[\"EPSG\",");
  return pos == std::string::npos ? GSKYHIP_E_CRS : crs_epsg(std::atoi(s.c_str() + pos + 10), c);
}

}  // namespace gsky

extern "C" int gskyhip_crs_from_srs(const char *srs, gskyhip_crs *out) { return gsky::parse_srs(srs, out); }
