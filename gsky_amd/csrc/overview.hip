// overview.hip -- overview pyramids built on the GPU for granules that come
// without any (netCDF, plain GeoTIFF, bands registered from HBM), so the
// warp's overview pick (warp.go:156-198) has levels to pick from.  What an
// operator otherwise does offline with gdaladdo.
//
// Semantics (include/gskyhip.h, DESIGN.md "Overview pyramids"):
//   level k is ceil(n / 2^k) per axis (GDAL's (n + f - 1) / f);
//   NEAREST: level k (i, j) = level k-1 (2i, 2j);
//   AVERAGE: cascaded -- level k (i, j) = mean of the valid pixels among
//     level k-1 (2i..2i+1, 2j..2j+1) clipped to the extent, taken from the
//     stored (already rounded) values of level k-1.  A pixel is invalid when
//     has_nodata and it equals the typed nodata (GDALCopyWords of the nodata
//     double: the value the warp's nodata fill writes, warp.go:247), or when
//     it is a float32 NaN.  No valid pixel: the typed nodata, or the quiet
//     NaN 0x7fc00000 without a nodata value.  Integer types: exact int32 sum,
//     sum / count rounded half away from zero in integer arithmetic; float32:
//     fp32 sum from +0.0f over the valid pixels in row-major box order, one
//     fp32 division by the count.  A result is stored as computed, also when
//     it happens to equal the nodata value.
//
// Kernel: bandwidth-bound, so each level is read once.  One workgroup of 256
// threads takes an aligned 64 x 64 tile of level k, reduces it to the 32 x 32
// tile of level k+1 straight from its loads (8- or 16-byte lane loads when the
// base and the row pitch allow, element loads otherwise), keeps that tile in
// LDS, and reduces it on to 16 x 16 (k+2) and 8 x 8 (k+3); all three are
// written, rows contiguous across lanes.  Tile origins are multiples of 64,
// so the 2 x 2 boxes nest and the in-tile cascade on typed values is
// bit-identical to a level-by-level one.  The next pass starts from the
// coarsest level written.  Offsets are 64-bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "../../include/gskyhip.h"
#include "gsky_device.h"

namespace gsky {
namespace {

constexpr int kOvrTile = 64;        // source tile side of one pass
constexpr int kOvrThreads = 256;
constexpr int kOvrPassLevels = 3;   // levels written by one pass

struct OvrPass {
  const void *src;
  int32_t sx, sy;                   // size of the source level
  void *out[kOvrPassLevels];
  int32_t ox[kOvrPassLevels], oy[kOvrPassLevels];
  int32_t n_out;                    // 1..3 levels this pass writes
  int32_t tiles_x;
  int32_t has_nodata;
  int32_t vec;                      // base and pitch allow the wide loads
  Val nd;                           // typed nodata
};

template <typename T> struct OvrTraits { static constexpr bool is_float = false; };
template <> struct OvrTraits<float> { static constexpr bool is_float = true; };

template <typename T>
__device__ __forceinline__ T ovr_nodata(const Val &nd) {
  if constexpr (OvrTraits<T>::is_float) return nd.f;
  else return (T)nd.i;
}

// One output pixel from its 2 x 2 box: get(dx, dy) reads the source pixel,
// in_x1 / in_y1 say whether the box's second column / row is inside the
// extent (the first always is).
template <typename T, int METHOD, typename Get>
__device__ __forceinline__ T ovr_box(Get get, bool in_x1, bool in_y1, bool has_nd, T nd) {
  if constexpr (METHOD == GSKYHIP_OVR_NEAREST) {
    return get(0, 0);
  } else if constexpr (OvrTraits<T>::is_float) {
    float sum = 0.0f;
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int dx = k & 1, dy = k >> 1;
      if ((dx && !in_x1) || (dy && !in_y1)) continue;
      const float v = get(dx, dy);
      if (v != v || (has_nd && v == nd)) continue;
      sum += v;
      cnt++;
    }
    if (cnt == 0) return has_nd ? nd : __uint_as_float(0x7fc00000u);
    return sum / (float)cnt;
  } else {
    int32_t sum = 0, cnt = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int dx = k & 1, dy = k >> 1;
      if ((dx && !in_x1) || (dy && !in_y1)) continue;
      const T v = get(dx, dy);
      if (has_nd && v == nd) continue;
      sum += (int32_t)v;
      cnt++;
    }
    if (cnt == 0) return nd;   // integer bands without a nodata value always have a valid pixel
    const int32_t a = sum < 0 ? -sum : sum;
    const int32_t q = (2 * a + cnt) / (2 * cnt);   // half away from zero
    return (T)(sum < 0 ? -q : q);
  }
}

template <int BYTES> struct OvrChunk;
template <> struct OvrChunk<8> { using type = uint2; };
template <> struct OvrChunk<16> { using type = uint4; };

template <typename T, int METHOD>
__global__ __launch_bounds__(kOvrThreads) void overview_pass_kernel(const OvrPass p) {
  // elements per wide load: 8 bytes for 1-byte types, 16 bytes otherwise
  constexpr int VEC = sizeof(T) == 4 ? 4 : 8;
  using Chunk = typename OvrChunk<VEC * sizeof(T)>::type;
  constexpr int H1 = kOvrTile / 2, H2 = kOvrTile / 4, H3 = kOvrTile / 8;
  __shared__ T l1[H1][H1 + 1];
  __shared__ T l2[H2][H2 + 1];

  const int tid = threadIdx.x;
  const int ty = (int)(blockIdx.x / (unsigned)p.tiles_x), tx = (int)(blockIdx.x % (unsigned)p.tiles_x);
  const int64_t x0 = (int64_t)tx * kOvrTile, y0 = (int64_t)ty * kOvrTile;   // tile origin in the source level
  const T *__restrict__ src = (const T *)p.src;
  const int64_t sx = p.sx, sy = p.sy;
  const bool has_nd = p.has_nodata != 0;
  const T nd = ovr_nodata<T>(p.nd);

  // ---- level +1 from global memory into l1
  if (p.vec) {
    constexpr int CH = kOvrTile / VEC;   // chunks per tile row
    for (int it = tid; it < CH * H1; it += kOvrThreads) {
      const int rp = it / CH, c = it % CH;
      const int64_t x = x0 + (int64_t)c * VEC, y = y0 + 2 * (int64_t)rp;
      if (x >= sx || y >= sy) continue;   // sx is a multiple of VEC here: a chunk is all in or all out
      const bool in_y1 = y + 1 < sy;
      union { Chunk c; T v[VEC]; } r0, r1;
      r0.c = *reinterpret_cast<const Chunk *>(src + y * sx + x);
      if (in_y1) r1.c = *reinterpret_cast<const Chunk *>(src + (y + 1) * sx + x);
      else r1.c = r0.c;
#pragma unroll
      for (int k = 0; k < VEC / 2; k++) {
        l1[rp][c * (VEC / 2) + k] = ovr_box<T, METHOD>(
            [&](int dx, int dy) { return dy ? r1.v[2 * k + dx] : r0.v[2 * k + dx]; }, true, in_y1, has_nd, nd);
      }
    }
  } else {
    for (int o = tid; o < H1 * H1; o += kOvrThreads) {
      const int r = o / H1, c = o % H1;
      const int64_t x = x0 + 2 * (int64_t)c, y = y0 + 2 * (int64_t)r;
      if (x >= sx || y >= sy) continue;
      const T *q = src + y * sx + x;
      l1[r][c] = ovr_box<T, METHOD>([&](int dx, int dy) { return q[(int64_t)dy * sx + dx]; }, x + 1 < sx,
                                    y + 1 < sy, has_nd, nd);
    }
  }
  __syncthreads();
  {
    T *__restrict__ out = (T *)p.out[0];
    const int64_t w = p.ox[0], h = p.oy[0];
    const int64_t bx = (int64_t)tx * H1, by = (int64_t)ty * H1;
    for (int o = tid; o < H1 * H1; o += kOvrThreads) {
      const int r = o / H1, c = o % H1;
      if (bx + c < w && by + r < h) out[(by + r) * w + bx + c] = l1[r][c];
    }
  }
  if (p.n_out < 2) return;   // uniform over the launch

  // ---- level +2 from l1 (its extent: level +1's size)
  {
    const int r = tid / H2, c = tid % H2;   // 256 threads, 16 x 16 outputs
    const int64_t w1 = p.ox[0], h1 = p.oy[0], w = p.ox[1], h = p.oy[1];
    const int64_t x = (int64_t)tx * H1 + 2 * c, y = (int64_t)ty * H1 + 2 * r;   // box origin in level +1
    if (x < w1 && y < h1) {
      const T v = ovr_box<T, METHOD>([&](int dx, int dy) { return l1[2 * r + dy][2 * c + dx]; }, x + 1 < w1,
                                     y + 1 < h1, has_nd, nd);
      l2[r][c] = v;
      ((T *)p.out[1])[((int64_t)ty * H2 + r) * w + (int64_t)tx * H2 + c] = v;
    }
  }
  if (p.n_out < 3) return;
  __syncthreads();

  // ---- level +3 from l2
  if (tid < H3 * H3) {
    const int r = tid / H3, c = tid % H3;
    const int64_t w2 = p.ox[1], h2 = p.oy[1], w = p.ox[2];
    const int64_t x = (int64_t)tx * H2 + 2 * c, y = (int64_t)ty * H2 + 2 * r;   // box origin in level +2
    if (x < w2 && y < h2) {
      const T v = ovr_box<T, METHOD>([&](int dx, int dy) { return l2[2 * r + dy][2 * c + dx]; }, x + 1 < w2,
                                     y + 1 < h2, has_nd, nd);
      ((T *)p.out[2])[((int64_t)ty * H3 + r) * w + (int64_t)tx * H3 + c] = v;
    }
  }
}

template <typename T>
int launch_pass(const OvrPass &p, int method, unsigned grid, hipStream_t s) {
  if (method == GSKYHIP_OVR_AVERAGE)
    hipLaunchKernelGGL((overview_pass_kernel<T, GSKYHIP_OVR_AVERAGE>), dim3(grid), dim3(kOvrThreads), 0, s, p);
  else
    hipLaunchKernelGGL((overview_pass_kernel<T, GSKYHIP_OVR_NEAREST>), dim3(grid), dim3(kOvrThreads), 0, s, p);
  return hipGetLastError() == hipSuccess ? 0 : GSKYHIP_E_HIP;
}

// Levels one pass writes: 3; the A/B build takes GSKYHIP_OVR_PASS_LEVELS
// (1..3) to time the one-launch-per-level variant of the same kernel.
int pass_levels() {
#ifdef GSKYHIP_AB
  if (const char *e = getenv("GSKYHIP_OVR_PASS_LEVELS")) return std::max(1, std::min(kOvrPassLevels, atoi(e)));
#endif
  return kOvrPassLevels;
}

}  // namespace
}  // namespace gsky

using namespace gsky;

extern "C" int gskyhip_overview_levels(int xsize, int ysize, int min_size, int32_t *ovr_xsize, int32_t *ovr_ysize) {
  if (xsize <= 0 || ysize <= 0) return GSKYHIP_E_ARG;
  if (min_size <= 0) min_size = 256;
  int n = 0, w = xsize, h = ysize;
  while (std::max(w, h) > min_size && n < GSKYHIP_MAX_OVR) {
    w = (int)(((int64_t)w + 1) / 2);
    h = (int)(((int64_t)h + 1) / 2);
    if (ovr_xsize) ovr_xsize[n] = w;
    if (ovr_ysize) ovr_ysize[n] = h;
    n++;
  }
  return n;
}

extern "C" int gskyhip_build_overviews(const void *src, int dtype, int signed_byte, int xsize, int ysize,
                                       int has_nodata, double nodata, int method, int n_levels,
                                       void *const *ovr_out, const int32_t *ovr_xsize, const int32_t *ovr_ysize,
                                       void *stream) {
  // every check before any HIP call
  if (!src || xsize <= 0 || ysize <= 0 || n_levels < 0 || n_levels > GSKYHIP_MAX_OVR) return GSKYHIP_E_ARG;
  if (method != GSKYHIP_OVR_NEAREST && method != GSKYHIP_OVR_AVERAGE) return GSKYHIP_E_ARG;
  if (n_levels > 0 && (!ovr_out || !ovr_xsize || !ovr_ysize)) return GSKYHIP_E_ARG;
  for (int k = 0, w = xsize, h = ysize; k < n_levels; k++) {
    w = (int)(((int64_t)w + 1) / 2);
    h = (int)(((int64_t)h + 1) / 2);
    if (!ovr_out[k] || ovr_xsize[k] != w || ovr_ysize[k] != h) return GSKYHIP_E_ARG;
  }
  if (dtype == GSKYHIP_SIGNEDBYTE || (dtype == GSKYHIP_BYTE && signed_byte)) dtype = GSKYHIP_SIGNEDBYTE;
  switch (dtype) {
    case GSKYHIP_BYTE: case GSKYHIP_SIGNEDBYTE: case GSKYHIP_INT16: case GSKYHIP_UINT16: case GSKYHIP_FLOAT32: break;
    case GSKYHIP_UINT32: case GSKYHIP_INT32: case GSKYHIP_FLOAT64: return GSKYHIP_E_TYPE;
    default: return GSKYHIP_E_ARG;
  }
  const int ts = type_size(dtype);
  const int per_pass = pass_levels();
  const void *cur = src;
  int cw = xsize, ch = ysize;
  if (n_levels > 0) (void)hipGetLastError();   // an earlier call's error is not this launch's
  for (int k = 0; k < n_levels;) {
    OvrPass p;
    p.src = cur;
    p.sx = cw;
    p.sy = ch;
    p.n_out = std::min(per_pass, n_levels - k);
    for (int j = 0; j < kOvrPassLevels; j++) {
      const int q = std::min(k + j, k + p.n_out - 1);   // unused slots repeat the last level (never written)
      p.out[j] = ovr_out[q];
      p.ox[j] = ovr_xsize[q];
      p.oy[j] = ovr_ysize[q];
    }
    p.tiles_x = (cw + kOvrTile - 1) / kOvrTile;
    const int64_t tiles = (int64_t)p.tiles_x * ((ch + kOvrTile - 1) / kOvrTile);
    if (tiles > 0x7fffffff) return GSKYHIP_E_ARG;
    p.has_nodata = has_nodata ? 1 : 0;
    p.nd = gdal_copy_to(nodata, dtype);
    const int chunk = ts == 1 ? 8 : 16;   // bytes of one wide load
    p.vec = ((uintptr_t)cur % chunk == 0 && ((int64_t)cw * ts) % chunk == 0) ? 1 : 0;
    int rc;
    switch (dtype) {
      case GSKYHIP_BYTE: rc = launch_pass<uint8_t>(p, method, (unsigned)tiles, (hipStream_t)stream); break;
      case GSKYHIP_SIGNEDBYTE: rc = launch_pass<int8_t>(p, method, (unsigned)tiles, (hipStream_t)stream); break;
      case GSKYHIP_INT16: rc = launch_pass<int16_t>(p, method, (unsigned)tiles, (hipStream_t)stream); break;
      case GSKYHIP_UINT16: rc = launch_pass<uint16_t>(p, method, (unsigned)tiles, (hipStream_t)stream); break;
      default: rc = launch_pass<float>(p, method, (unsigned)tiles, (hipStream_t)stream); break;
    }
    if (rc) return rc;
    k += p.n_out;
    cur = ovr_out[k - 1];
    cw = ovr_xsize[k - 1];
    ch = ovr_ysize[k - 1];
  }
  return 0;
}
