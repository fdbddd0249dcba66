// stage_rules.h -- the per-value rules the stage kernels share: typed loads and
// stores of a canvas element, Go's math.Log10 and the utils.Scale pixel rule
// (raster_scaler.go:40-330).  One home for stages.hip and fuse.hip, which so
// compute the same bits -- but not the rule's only copy.  utils.Scale is
// written five times:
//   S1  scale_one() here, with host_scale_consts() and the scale_minmax /
//       scale_finalize / scale_apply kernels of stages.hip; fuse.hip's layers
//       and outer scale
//   S2  scale_px() + make_scale() + auto_minmax() (render_common.h): the
//       general kernel, canvas_rgba_kernel after an auto-scale fold, float32
//   S3  scale_t<T>() with go_u8_f32() (render_common.h): render_lds.h and the
//       typed generic kernels (render_generic.h)
//   S4  scale_int<T, SAFE>() (render_nn.h): the nearest-neighbour band kernel
//   S5  scale_legacy_kernel (stages.hip): processor/tile_scaler.go
// and Go's math.Log10 twice (go_log10_s here, go_log10 in render_common.h).
// The render copies differ for register and speed reasons; what
// holds all of them to the same bytes is tests/test_scale_edges.py, which
// drives each with the case table of tests/test_scale_rule.py.
#pragma once
#include "gsky_device.h"
#include "stages.h"

namespace gsky {

__device__ __forceinline__ Val load_typed(const void *p, int dtype, long idx) {
  Val v;
  switch (dtype) {
    case GSKYHIP_SIGNEDBYTE: v.i = ((const int8_t *)p)[idx]; break;
    case GSKYHIP_BYTE: v.i = ((const uint8_t *)p)[idx]; break;
    case GSKYHIP_INT16: v.i = ((const int16_t *)p)[idx]; break;
    case GSKYHIP_UINT16: v.i = ((const uint16_t *)p)[idx]; break;
    default: v.u = ((const uint32_t *)p)[idx]; break;
  }
  return v;
}
__device__ __forceinline__ void store_typed(void *p, int dtype, long idx, Val v) {
  switch (dtype) {
    case GSKYHIP_SIGNEDBYTE: case GSKYHIP_BYTE: ((uint8_t *)p)[idx] = (uint8_t)v.i; break;
    case GSKYHIP_INT16: case GSKYHIP_UINT16: ((uint16_t *)p)[idx] = (uint16_t)v.i; break;
    default: ((uint32_t *)p)[idx] = v.u; break;
  }
}

__device__ inline double go_log_s(double x) {
  const double Ln2Hi = 6.93147180369123816490e-01, Ln2Lo = 1.90821492927058770002e-10;
  const double L1 = 6.666666666666735130e-01, L2 = 3.999999999940941908e-01,
               L3 = 2.857142874366239149e-01, L4 = 2.222219843214978396e-01,
               L5 = 1.818357216161805012e-01, L6 = 1.531383769920937332e-01,
               L7 = 1.479819860511658591e-01;
  if (x != x || x == INFINITY) return x;
  if (x < 0) return NAN;
  if (x == 0) return -INFINITY;
  int ki;
  double f1 = frexp(x, &ki);
  if (f1 < 1.41421356237309504880168872420969808 / 2) { f1 *= 2; ki--; }
  double f = f1 - 1;
  double k = (double)ki;
  double s = f / (2 + f);
  double s2 = s * s;
  double s4 = s2 * s2;
  double t1 = s2 * (L1 + s4 * (L3 + s4 * (L5 + s4 * L7)));
  double t2 = s4 * (L2 + s4 * (L4 + s4 * L6));
  double R = t1 + t2;
  double hfsq = 0.5 * f * f;
  return k * Ln2Hi - ((hfsq - (s * (hfsq + R) + k * Ln2Lo)) - f);
}
__device__ inline double go_log10_s(double x) {
  int e;
  double frac = frexp(x, &e);
  double l2;
  if (frac == 0.5) l2 = (double)(e - 1);
  else l2 = go_log_s(frac) * (1.0 / 0.693147180559945309417232121458176568) + (double)e;
  return l2 * 0.301029995663981195213738894724493026768189881462108541310;
}

// utils.Scale of one value with the constants of host_scale_consts().
__device__ __forceinline__ uint8_t scale_one(const ScaleC &k, Val v) {
  if (k.dtype == GSKYHIP_FLOAT32) {
    float value = v.f;
    if (value == k.noData.f) return 0xFF;
    if (k.colour_scale > 0) {
      double d = (double)value;
      if (!(d == k.nodata64)) {
        if (k.colour_scale == 1) d = go_log10_s(d);
        if (isinf(d) || d != d) d = k.nodata64;
      }
      if (d == k.nodata64) return 0xFF;
      value = (float)d;
    }
    value += k.off.f;
    if (value > k.clp.f) value = k.clp.f;
    if (value < 0.0f) value = 0.0f;
    return go_f32_u8(value * k.sc);
  }
  int32_t value = v.i;
  if (value == k.noData.i) return 0xFF;
  switch (k.dtype) {
    case GSKYHIP_SIGNEDBYTE: value = (int8_t)(value + k.off.i); break;
    case GSKYHIP_BYTE: value = (uint8_t)(value + k.off.i); break;
    case GSKYHIP_INT16: value = (int16_t)(value + k.off.i); break;
    default: value = (uint16_t)(value + k.off.i); break;
  }
  if (value > k.clp.i) value = k.clp.i;
  if (value < 0) value = 0;
  return go_f32_u8((float)value * k.sc);
}

}  // namespace gsky
