// resample.h -- the per-pixel resampling rules, each written once: the
// nearest-neighbour index rule (warp.go:271-300), GWKBilinearResample4Sample
// and GWKCubicResample4Sample (GDAL 3.0.1) in fp64, the cubic B-spline and
// Lanczos point kernels (after GWKResample), the area average and mode
// over a pixel's footprint (after GWKAverageOrMode), the exit conversion to
// the window's type, and the fp32 renormalised 2 x 2 of the float canvas
// kernels.  The fp64 rules take a tap accessor `double tap(int xx, int yy)`,
// called only for taps inside the band: what a kernel loads, and how (typed
// pointer, global address space, run-time source type), stays with the kernel.
// A new resampler is one more *_rule() here over the same accessor, one more
// branch in the callers' wrappers (render_common.h, render_generic.h) and one
// more case of with_resample().
#pragma once
#include <type_traits>

#include "gsky_device.h"

namespace gsky {

// A tap holds the band's nodata (a NaN nodata matches NaN taps).
__device__ __forceinline__ bool tap_is_nodata(double v, bool has_nodata, double nodata64) {
  return has_nodata && (v == nodata64 || (nodata64 != nodata64 && v != v));
}

// The nearest-neighbour index rule (warp.go:271-300): s < 0 -> no pixel,
// + 1e-10, >= 2147483647 (or NaN) -> no pixel, truncation, >= n -> no pixel.
constexpr double kNnEps = 1.0e-10;

// The rule along one axis of n source pixels, branch-free (bytesRead tests x
// alone, windows.hip); i is meaningful only where the result is true.
__device__ __forceinline__ bool nn_axis(double s, int n, int &i) {
  const double a = s + kNnEps;
  i = __double2int_rz(a);
  return !(s < 0) && a < 2147483647.0 && i < n;
}

// The nearest-neighbour source pixel of (sx, sy) in a bx x by band; false ->
// window fill (idx is then not to be used).
__device__ __forceinline__ bool nn_index(double sx, double sy, int bx, int by, long &idx) {
  if (sx < 0 || sy < 0) return false;
  const double ax = sx + kNnEps, ay = sy + kNnEps;
  if (!(ax < 2147483647.0) || !(ay < 2147483647.0)) return false;
  const int ix = (int)ax, iy = (int)ay;
  if (ix >= bx || iy >= by) return false;
  idx = (long)iy * bx + ix;
  return true;
}

// GWKBilinearResample4Sample up to and including the divide: the 2 x 2 taps
// at floor(s - 0.5) with the -1 edge rule, taps outside the band or holding
// its nodata dropped and the weights renormalised.  false -> no sample.
// Every operation in the written order (-ffp-contract=off; the numpy rule of
// tests/test_bilinear_edges.py evaluates the same sequence).
template <typename Tap>
__device__ __forceinline__ bool bilinear_rule(int bx, int by, bool has_nodata, double nodata64, double sx,
                                              double sy, Tap tap, double &r) {
  int iSrcX = (int)floor(sx - 0.5);
  int iSrcY = (int)floor(sy - 0.5);
  double rX = 1.5 - (sx - iSrcX);
  double rY = 1.5 - (sy - iSrcY);
  if (iSrcX == -1) { iSrcX = 0; rX = 1; }
  if (iSrcY == -1) { iSrcY = 0; rY = 1; }
  double accR = 0.0, accDiv = 0.0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int xx = iSrcX + (k & 1), yy = iSrcY + (k >> 1);
    const double w = ((k & 1) ? (1.0 - rX) : rX) * ((k >> 1) ? (1.0 - rY) : rY);
    if (xx < 0 || xx >= bx || yy < 0 || yy >= by) continue;
    const double d = tap(xx, yy);
    // tap_is_nodata(), written out: as a call its short circuits are folded to
    // selects before it is inlined, and render_lds_kernel then holds 4 more VGPRs
    if (has_nodata && (d == nodata64 || (nodata64 != nodata64 && d != d))) continue;
    accDiv += w;
    accR += d * w;
  }
  if (accDiv == 1.0) r = accR;
  else if (accDiv < 0.00001) return false;
  else r = accR / accDiv;
  return true;
}

// One 1-D cubic convolution of GWKCubicResample4Sample, every operation in
// the written order (the numpy rule of tests/test_cubic.py evaluates the same
// sequence).
__device__ __forceinline__ double cubic_conv(double t, double f0, double f1, double f2, double f3) {
  const double t2 = t * t;
  const double t3 = t2 * t;
  return f1 + 0.5 * (t * (f2 - f0) + t2 * (2.0 * f0 - 5.0 * f1 + 4.0 * f2 - f3) + t3 * (3.0 * (f1 - f2) + f3 - f0));
}

// The 4 x 4 taps of a cubic sample lie inside an nx x ny band (tested on the
// floored coordinates as doubles: no integer conversion of a far coordinate).
__device__ __forceinline__ bool cubic_inside(double fx, double fy, int nx, int ny) {
  return fx >= 1.0 && fx + 2.0 < (double)nx && fy >= 1.0 && fy + 2.0 < (double)ny;
}

// GWKCubicResample4Sample (GSKYHIP_RESAMPLE_CUBIC, gskyhip.h): the 4 x 4 taps
// around floor(s - 0.5), rows first; a tap outside the band or holding its
// nodata hands the pixel to bilinear_rule().  false -> no sample.
template <typename Tap>
__device__ __forceinline__ bool cubic_rule(int bx, int by, bool has_nodata, double nodata64, double sx, double sy,
                                           Tap tap, double &r) {
  const double fx = floor(sx - 0.5), fy = floor(sy - 0.5);
  if (!cubic_inside(fx, fy, bx, by)) return bilinear_rule(bx, by, has_nodata, nodata64, sx, sy, tap, r);
  const int iX = (int)fx, iY = (int)fy;
  const double tx = sx - 0.5 - fx, ty = sy - 0.5 - fy;
  double h[4];
  bool anynd = false;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    double f[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
      f[i] = tap(iX - 1 + i, iY - 1 + j);
      anynd = anynd || tap_is_nodata(f[i], has_nodata, nodata64);
    }
    h[j] = cubic_conv(tx, f[0], f[1], f[2], f[3]);
  }
  if (anynd) return bilinear_rule(bx, by, has_nodata, nodata64, sx, sy, tap, r);
  r = cubic_conv(ty, h[0], h[1], h[2], h[3]);
  return true;
}

// ------------------------------------------------------- the point kernels
// GSKYHIP_RESAMPLE_CUBICSPLINE / _LANCZOS (gskyhip.h), after GDAL's general
// GWKResample at scale 1 with GWKBSpline / GWKLanczosSinc as the weights:
// 2 R x 2 R taps around floor(s - 0.5), R = kernel_radius().
constexpr bool is_kernel(int res) { return res == GSKYHIP_RESAMPLE_CUBICSPLINE || res == GSKYHIP_RESAMPLE_LANCZOS; }
constexpr int kernel_radius(int res) { return res == GSKYHIP_RESAMPLE_LANCZOS ? 3 : 2; }

// The cubic B-spline at x: >= 0, zero at and beyond 2, its integer samples
// sum to 1.  Every operation in the written order (the numpy rule of
// tests/test_kernel_rule.py evaluates the same sequence).
__device__ __forceinline__ double bspline_weight(double x) {
  const double a = fabs(x);
  if (a < 1.0) {
    const double a2 = a * a;
    return ((4.0 - 6.0 * a2) + 3.0 * (a2 * a)) / 6.0;
  }
  if (a < 2.0) {
    const double u = 2.0 - a;
    return (u * u * u) / 6.0;
  }
  return 0.0;
}

// Lanczos, a = 3: sinc(x) sinc(x / 3), zero at and beyond 3.
__device__ __forceinline__ double lanczos_weight(double x) {
  if (x == 0.0) return 1.0;
  if (fabs(x) >= 3.0) return 0.0;
  const double p = M_PI * x;
  const double q = p / 3.0;
  return sin(p) * sin(q) / (p * q);
}

// The centre 2 x 2 of a point-kernel sample lies inside an nx x ny band
// (tested on the floored doubles, cubic_inside()'s reason).
__device__ __forceinline__ bool kernel_inside(double fx, double fy, int nx, int ny) {
  return fx >= 0.0 && fx + 1.0 < (double)nx && fy >= 0.0 && fy + 1.0 < (double)ny;
}

// The rule of radius R (2: spline, 3: Lanczos).  The centre 2 x 2 must lie
// inside the band and hold no nodata, else the pixel takes bilinear_rule();
// an outer tap outside the band or holding the nodata is dropped and the
// weights renormalised: w = wx * wy, accW += w, accR += d * w, rows outer,
// always divided.  false -> no sample.
template <int R, typename Tap>
__device__ __forceinline__ bool kernel_rule(int bx, int by, bool has_nodata, double nodata64, double sx, double sy,
                                            Tap tap, double &r) {
  static_assert(R == 2 || R == 3, "spline or Lanczos");
  const double fx = floor(sx - 0.5), fy = floor(sy - 0.5);
  if (!kernel_inside(fx, fy, bx, by)) return bilinear_rule(bx, by, has_nodata, nodata64, sx, sy, tap, r);
  const int iX = (int)fx, iY = (int)fy;
  bool anynd = false;
#pragma unroll
  for (int k = 0; k < 4; k++) anynd = anynd || tap_is_nodata(tap(iX + (k & 1), iY + (k >> 1)), has_nodata, nodata64);
  if (anynd) return bilinear_rule(bx, by, has_nodata, nodata64, sx, sy, tap, r);
  const double tx = sx - 0.5 - fx, ty = sy - 0.5 - fy;
  auto K = [](double x) { return R == 2 ? bspline_weight(x) : lanczos_weight(x); };
  double wx[2 * R];
#pragma unroll
  for (int i = 0; i < 2 * R; i++) wx[i] = K((double)(i + 1 - R) - tx);
  double accR = 0.0, accW = 0.0;
  // rows rolled (a row's weight is made where it is used), columns unrolled:
  // wx stays in registers and the body holds 2 R taps, not 4 R^2
#pragma unroll 1
  for (int j = 0; j < 2 * R; j++) {
    const int yy = iY + 1 - R + j;
    if (yy < 0 || yy >= by) continue;
    const double wyj = K((double)(j + 1 - R) - ty);
#pragma unroll
    for (int i = 0; i < 2 * R; i++) {
      const int xx = iX + 1 - R + i;
      if (xx < 0 || xx >= bx) continue;
      const double d = tap(xx, yy);
      if (tap_is_nodata(d, has_nodata, nodata64)) continue;
      const double w = wx[i] * wyj;
      accW += w;
      accR += d * w;
    }
  }
  r = accR / accW;
  return true;
}

// ---------------------------------------------------------------- area rules
// GSKYHIP_RESAMPLE_AVERAGE / _MODE (gskyhip.h), after GDAL's GWKAverageOrMode:
// a pixel's footprint in the source is the box [sx - hx, sx + hx] x [sy - hy,
// sy + hy] (hx, hy >= 0.5 from the pixel's neighbours: area_half(); the
// callers' wrappers take the neighbours' coordinates), its taps the outer
// product of area_taps() along x and y, rows outer.
constexpr int kAreaTaps = 8;   // taps per axis at the most (64 per pixel)

constexpr bool is_area(int res) { return res == GSKYHIP_RESAMPLE_AVERAGE || res == GSKYHIP_RESAMPLE_MODE; }
// The rule a raster of the mask layer warps by under the data's rule `res`:
// nearest neighbour under the area rules and the point kernels (bit fields
// are neither averaged, voted nor convolved), else the data's.
constexpr int mask_res(int res) { return (is_area(res) || is_kernel(res)) ? GSKYHIP_RESAMPLE_NEAREST : res; }

// Host side: the run-time rule r as a compile-time one.  Calls
// f(std::integral_constant<int, R>{}) for the GSKYHIP_RESAMPLE_* value r;
// false, and no call, when r is none of them.  Every launch of a kernel
// templated on the rule goes through here.
template <class F>
bool with_resample(int r, F &&f) {
  switch (r) {
    case GSKYHIP_RESAMPLE_NEAREST: f(std::integral_constant<int, GSKYHIP_RESAMPLE_NEAREST>{}); return true;
    case GSKYHIP_RESAMPLE_BILINEAR: f(std::integral_constant<int, GSKYHIP_RESAMPLE_BILINEAR>{}); return true;
    case GSKYHIP_RESAMPLE_CUBIC: f(std::integral_constant<int, GSKYHIP_RESAMPLE_CUBIC>{}); return true;
    case GSKYHIP_RESAMPLE_AVERAGE: f(std::integral_constant<int, GSKYHIP_RESAMPLE_AVERAGE>{}); return true;
    case GSKYHIP_RESAMPLE_MODE: f(std::integral_constant<int, GSKYHIP_RESAMPLE_MODE>{}); return true;
    case GSKYHIP_RESAMPLE_CUBICSPLINE: f(std::integral_constant<int, GSKYHIP_RESAMPLE_CUBICSPLINE>{}); return true;
    case GSKYHIP_RESAMPLE_LANCZOS: f(std::integral_constant<int, GSKYHIP_RESAMPLE_LANCZOS>{}); return true;
    default: return false;
  }
}

// Half extent of a footprint along one axis from that axis' component of
// u = S(i + 1, row) - S(i, row) and v = S(i, row + 1) - S(i, row).
__device__ __forceinline__ double area_half(double u, double v) { return fmax(0.5, 0.5 * (fabs(u) + fabs(v))); }

// The taps of [s - h, s + h] along an axis of n source pixels: lo, lo +
// stride, ... < hi, at most kAreaTaps of them; false -> none.  The bounds are
// compared as doubles (cubic_inside()'s reason); [x0, x1] is the interval.
struct AreaAxis {
  int lo, hi, stride;
  double x0, x1;
  __device__ __forceinline__ int count() const { return (hi - lo + stride - 1) / stride; }
  // covered length of tap xx; 1 once the taps are strided
  __device__ __forceinline__ double weight(int xx) const {
    return stride == 1 ? fmin((double)xx + 1.0, x1) - fmax((double)xx, x0) : 1.0;
  }
};
__device__ __forceinline__ bool area_taps(double s, double h, int n, AreaAxis &a) {
  a.x0 = s - h;
  a.x1 = s + h;
  if (!(fabs(a.x0) < INFINITY) || !(fabs(a.x1) < INFINITY)) return false;
  const double lo = fmax(floor(a.x0), 0.0), hi = fmin(ceil(a.x1), (double)n);
  if (hi <= lo) return false;
  a.lo = (int)lo;
  a.hi = (int)hi;
  a.stride = (a.hi - a.lo + kAreaTaps - 1) / kAreaTaps;
  return true;
}

// AVERAGE: the weighted mean of the taps that do not hold the band's nodata,
// w = wx * wy, accW += w and accR += d * w in scan order.  false -> no sample.
// With hx = hy = 0.5 the taps and weights are bilinear_rule()'s.
template <typename Tap>
__device__ __forceinline__ bool average_rule(int bx, int by, bool has_nodata, double nodata64, double sx, double sy,
                                             double hx, double hy, Tap tap, double &r) {
  AreaAxis ax, ay;
  if (!area_taps(sx, hx, bx, ax) || !area_taps(sy, hy, by, ay)) return false;
  double accR = 0.0, accW = 0.0;
  for (int yy = ay.lo; yy < ay.hi; yy += ay.stride) {
    const double wy = ay.weight(yy);
    for (int xx = ax.lo; xx < ax.hi; xx += ax.stride) {
      const double w = ax.weight(xx) * wy;
      const double d = tap(xx, yy);
      if (tap_is_nodata(d, has_nodata, nodata64) || !(w > 0.0)) continue;
      accW += w;
      accR += d * w;
    }
  }
  if (accW < 0.00001) return false;
  r = accR / accW;
  return true;
}

// MODE: taps of equal value form a class (a NaN tap that is not nodata is a
// class of its own), a class weighs the sum of its taps' w in scan order, the
// sample is the value of the heaviest class, the first in scan order among
// equals.  No tap storage: a tap whose value an earlier tap holds is skipped,
// any other sums its class over the taps after it.  false -> no sample.
template <typename Tap>
__device__ __forceinline__ bool mode_rule(int bx, int by, bool has_nodata, double nodata64, double sx, double sy,
                                          double hx, double hy, Tap tap, double &r) {
  AreaAxis ax, ay;
  if (!area_taps(sx, hx, bx, ax) || !area_taps(sy, hy, by, ay)) return false;
  const int nx = ax.count(), n = nx * ay.count();
  // tap k of the scan: its value, and its weight (0: dropped)
  auto at = [&](int k, double &d) {
    const int xx = ax.lo + (k % nx) * ax.stride, yy = ay.lo + (k / nx) * ay.stride;
    d = tap(xx, yy);
    const double w = ax.weight(xx) * ay.weight(yy);
    return (tap_is_nodata(d, has_nodata, nodata64) || !(w > 0.0)) ? 0.0 : w;
  };
  bool found = false;
  double best = 0.0;
  for (int k = 0; k < n; k++) {
    double d, o;
    double cw = at(k, d);
    if (cw == 0.0) continue;
    bool seen = false;
    for (int j = 0; j < k && !seen; j++) seen = at(j, o) != 0.0 && o == d;
    if (seen) continue;
    for (int j = k + 1; j < n; j++) {
      const double w = at(j, o);
      if (w != 0.0 && o == d) cw += w;
    }
    if (!found || cw > best) {
      found = true;
      best = cw;
      r = d;
    }
  }
  return found;
}

// The exit of a sample: (float)r into a float32 window, GDALCopyWords'
// rounding and clamp of floor(r + 0.5) into an integer one.  T: the window's
// element type (any integer T where only out_dtype tells the integer types
// apart); the Val form picks by out_dtype at run time.
template <typename T>
__device__ __forceinline__ auto resample_store(double r, int out_dtype) {
  if constexpr (std::is_same<T, float>::value) return (float)r;
  else return gdal_copy_to(floor(r + 0.5), out_dtype).i;
}
__device__ __forceinline__ Val resample_store(double r, int out_dtype) {
  Val o;
  if (out_dtype == GSKYHIP_FLOAT32) o.f = resample_store<float>(r, out_dtype);
  else o.i = resample_store<int32_t>(r, out_dtype);
  return o;
}

// The float canvas kernels' 2 x 2 with nodata taps dropped (render_bil.h,
// render_cub.h), weights and sums in WT: tv the taps x, x + 1 of the upper
// row then of the lower, wx / wy the weights of (x, x + 1) and (y, y + 1).
// All four taps are inside the band.  fillv where too little weight is left.
template <typename WT>
__device__ __forceinline__ float bil4_renorm(const float (&tv)[4], const WT (&wx)[2], const WT (&wy)[2], bool nd_nan,
                                             float ndf, float fillv) {
  WT aR = (WT)0.0, aD = (WT)0.0;
#pragma unroll
  for (int kk = 0; kk < 4; kk++) {
    const WT w = wx[kk & 1] * wy[kk >> 1];
    const bool use = !(nd_nan ? (tv[kk] != tv[kk]) : (tv[kk] == ndf));
    aD += use ? w : (WT)0.0;
    aR += use ? (WT)tv[kk] * w : (WT)0.0;
  }
  if (aD == (WT)1.0) return (float)aR;
  if (aD >= (WT)0.00001) return (float)(aR / aD);
  return fillv;
}

}  // namespace gsky
