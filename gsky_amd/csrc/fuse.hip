// fuse.hip -- layer fusion (input_layers): TilePipeline.processDeps
// (processor/tile_pipeline.go:196-324) with getFlexRaster (482-632), the
// RasterMerger fold of the fuse<j> rasters (tile_merger.go:38-225), and for
// fuse_render the outer utils.Scale (raster_scaler.go:30-332) and the EncodePNG
// pixel loop (ogc_encoders.go:86-133), in one pass over the layer canvases.
// The rule is written out in include/gskyhip.h.
//
// A pure HBM stream: one lane per 4 consecutive pixels of a row, vector loads
// of 4 elements where the address allows, one 16-byte RGBA store.  Layer
// descriptors and their Scale constants travel in the kernel arguments, so a
// call allocates nothing, copies nothing and never synchronises.
#include <cstring>

#include "gsky_device.h"
#include "stages.h"
#include "stage_rules.h"

namespace gsky {

// One input layer as the kernels see it.
struct FuseLayerD {
  const uint8_t *canvases;   // (n_tiles, n_ns) slots of max_w * max_h * 4 bytes
  const uint8_t *present;    // per tile, or NULL: present everywhere
  ScaleC k;                  // the layer's own Scale constants (scaled layers)
  int32_t dtype;             // value type of the canvases
  int32_t scaled;            // 1: utils.Scale to Byte, nodata 0xFF
  int32_t norm;              // 1: unscaled, and T(n_0) != T(n_l) against an unscaled layer 0
  int32_t esize;
  Val nd_own, nd_norm;       // T(n_l), T(n_0) in the layer's type
  double nodata, nodata_norm;   // n_l, n_0
};

struct FuseArgs {
  FuseLayerD layer[GSKYHIP_FUSE_MAX_LAYERS];
  const gskyhip_tile *tiles;
  int32_t n_layers, n_ns, max_w, max_h;
  int32_t post_dtype;        // the one post-stage type of every layer
  int32_t groups;            // lanes per row: ceil(max_w / 4)
  int32_t tile0;             // first tile of this launch
  int32_t _pad;
};

// The post-stage nodata of layer l on a tile where layer 0 is (not) present.
__device__ __forceinline__ void fuse_post_nodata(const FuseLayerD &L, bool norm_ok, Val &nd, double &nd64) {
  if (L.scaled) { nd.i = 0xFF; nd64 = 255.0; }
  else if (L.norm && norm_ok) { nd = L.nd_norm; nd64 = L.nodata_norm; }
  else { nd = L.nd_own; nd64 = L.nodata; }
}

// 4 consecutive elements of a row, `nvalid` of them inside the tile.
__device__ __forceinline__ void fuse_load4(const uint8_t *row, int dtype, int esize, int x0, int nvalid,
                                           Val v[4]) {
  const uint8_t *p = row + (size_t)x0 * esize;
  if (nvalid == 4 && (((uintptr_t)p) & (uintptr_t)(4 * esize - 1)) == 0) {
    if (esize == 1) {
      const uint32_t u = *(const uint32_t *)p;
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const uint32_t b = (u >> (8 * q)) & 0xFFu;
        v[q].i = dtype == GSKYHIP_SIGNEDBYTE ? (int32_t)(int8_t)b : (int32_t)b;
      }
    } else if (esize == 2) {
      const uint2 u = *(const uint2 *)p;
      const uint32_t h[4] = {u.x & 0xFFFFu, u.x >> 16, u.y & 0xFFFFu, u.y >> 16};
#pragma unroll
      for (int q = 0; q < 4; q++) v[q].i = dtype == GSKYHIP_INT16 ? (int32_t)(int16_t)h[q] : (int32_t)h[q];
    } else {
      const uint4 u = *(const uint4 *)p;
      v[0].u = u.x; v[1].u = u.y; v[2].u = u.z; v[3].u = u.w;
    }
    return;
  }
#pragma unroll
  for (int q = 0; q < 4; q++) {
    v[q].u = 0;
    if (q < nvalid) v[q] = load_typed(row, dtype, x0 + q);
  }
}

__device__ __forceinline__ void fuse_store4(uint8_t *row, int dtype, int esize, int x0, int nvalid,
                                            const Val v[4]) {
  uint8_t *p = row + (size_t)x0 * esize;
  if (nvalid == 4 && (((uintptr_t)p) & (uintptr_t)(4 * esize - 1)) == 0) {
    if (esize == 1) {
      *(uint32_t *)p = ((uint32_t)v[0].i & 0xFFu) | (((uint32_t)v[1].i & 0xFFu) << 8) |
                       (((uint32_t)v[2].i & 0xFFu) << 16) | (((uint32_t)v[3].i & 0xFFu) << 24);
    } else if (esize == 2) {
      uint2 u;
      u.x = ((uint32_t)v[0].i & 0xFFFFu) | (((uint32_t)v[1].i & 0xFFFFu) << 16);
      u.y = ((uint32_t)v[2].i & 0xFFFFu) | (((uint32_t)v[3].i & 0xFFFFu) << 16);
      *(uint2 *)p = u;
    } else {
      uint4 u;
      u.x = v[0].u; u.y = v[1].u; u.z = v[2].u; u.w = v[3].u;
      *(uint4 *)p = u;
    }
    return;
  }
#pragma unroll
  for (int q = 0; q < 4; q++)
    if (q < nvalid) store_typed(row, dtype, x0 + q, v[q]);
}

// Which layers are present on tile t (bit l), read once per lane: wave-uniform.
__device__ __forceinline__ uint32_t fuse_present_mask(const FuseArgs &a, int t) {
  uint32_t m = 0;
  for (int l = 0; l < a.n_layers; l++) {
    const uint8_t *p = a.layer[l].present;
    if (!p || p[t]) m |= 1u << l;
  }
  return m;
}

// The fused canvas nodata of a tile: the first present layer's post-stage
// nodata; layer 0's where no layer is present.
__device__ __forceinline__ void fuse_canvas_nodata(const FuseArgs &a, uint32_t pres, Val &C, double &C64) {
  const int p0 = pres ? __ffs((int)pres) - 1 : 0;
  fuse_post_nodata(a.layer[p0], (pres & 1u) && !a.layer[0].scaled, C, C64);
}

// The fold of one namespace slot for this lane's 4 pixels.  Every lane of the
// wave calls it (inactive ones with nvalid = 0): the layer loop votes.
__device__ __forceinline__ void fuse_fold4(const FuseArgs &a, uint32_t pres, int t, int s, int x0, int y,
                                           int nvalid, Val C, Val c[4]) {
  const bool isf = a.post_dtype == GSKYHIP_FLOAT32;
  const bool norm_ok = (pres & 1u) && !a.layer[0].scaled;
  const size_t slot = ((size_t)t * a.n_ns + s) * (size_t)a.max_w * a.max_h * 4;
#pragma unroll
  for (int q = 0; q < 4; q++) c[q] = C;
  bool first = true;
  for (int l = 0; l < a.n_layers; l++) {
    if (!((pres >> l) & 1u)) continue;
    const FuseLayerD &L = a.layer[l];
    Val nd;
    double nd64;
    fuse_post_nodata(L, norm_ok, nd, nd64);
    // the pixels this layer may still write: all of them for the first
    // present layer, afterwards those where the canvas equals its nodata
    bool open[4];
    bool need = false;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      open[q] = q < nvalid && (first || val_eq(c[q], nd, isf));
      need = need || open[q];
    }
    first = false;
    // every lane's pixels are filled: the wave skips the layer's reads.  With
    // one nodata for all layers this holds for every later layer too, which
    // is the early stop the reference meant (tile_pipeline.go:300-305).
    if (!__any(need)) continue;
    if (!need) continue;
    Val v[4];
    fuse_load4(L.canvases + slot + (size_t)y * a.max_w * L.esize, L.dtype, L.esize, x0, nvalid, v);
    if (L.scaled) {
#pragma unroll
      for (int q = 0; q < 4; q++) v[q].i = scale_one(L.k, v[q]);
    } else if (L.norm && norm_ok) {
#pragma unroll
      for (int q = 0; q < 4; q++)
        if (val_eq(v[q], L.nd_own, isf)) v[q] = L.nd_norm;
    }
#pragma unroll
    for (int q = 0; q < 4; q++)
      if (open[q] && !val_eq(v[q], nd, isf)) c[q] = v[q];
  }
}

// Lane -> (tile, row, first column); false outside the tile.
__device__ __forceinline__ bool fuse_lane(const FuseArgs &a, int t, int &x0, int &y, int &nvalid) {
  const gskyhip_tile &tl = a.tiles[t];
  const int w = min(tl.width, a.max_w), h = min(tl.height, a.max_h);
  const int gid = blockIdx.x * blockDim.x + threadIdx.x;
  y = gid / a.groups;
  x0 = (gid - y * a.groups) * 4;
  nvalid = 0;
  if (y >= h || x0 >= w) return false;
  nvalid = min(4, w - x0);
  return true;
}

__global__ __launch_bounds__(256) void fuse_layers_kernel(const FuseArgs a, uint8_t *canvas_out,
                                                          double *nodata_out) {
  const int t = a.tile0 + (int)blockIdx.y / a.n_ns, s = (int)blockIdx.y % a.n_ns;
  int x0, y, nvalid;
  fuse_lane(a, t, x0, y, nvalid);
  const uint32_t pres = fuse_present_mask(a, t);
  Val C;
  double C64;
  fuse_canvas_nodata(a, pres, C, C64);
  if (s == 0 && blockIdx.x == 0 && threadIdx.x == 0) nodata_out[t] = C64;
  Val c[4];
  fuse_fold4(a, pres, t, s, x0, y, nvalid, C, c);
  if (nvalid == 0) return;
  const int es = type_size(a.post_dtype);
  const size_t slot = ((size_t)t * a.n_ns + s) * (size_t)a.max_w * a.max_h * 4;
  fuse_store4(canvas_out + slot + (size_t)y * a.max_w * es, a.post_dtype, es, x0, nvalid, c);
}

__global__ __launch_bounds__(256) void fuse_render_kernel(const FuseArgs a, ScaleC outer, const uint32_t *ramp,
                                                          uint32_t *rgba_out, uint8_t *canvas_out,
                                                          double *nodata_out) {
  __shared__ uint32_t s_ramp[256];
  if (ramp) s_ramp[threadIdx.x] = ramp[threadIdx.x];   // blockDim.x == 256
  __syncthreads();
  const int t = a.tile0 + (int)blockIdx.y;
  int x0, y, nvalid;
  fuse_lane(a, t, x0, y, nvalid);
  const uint32_t pres = fuse_present_mask(a, t);
  Val C;
  double C64;
  fuse_canvas_nodata(a, pres, C, C64);
  if (nodata_out && blockIdx.x == 0 && threadIdx.x == 0) nodata_out[t] = C64;
  // host_scale_consts(post type, C, outer_sp): only the nodata depends on the tile
  outer.noData = C;
  outer.nodata64 = C64;
  const int es = type_size(a.post_dtype);
  uint8_t b[3][4];
  for (int s = 0; s < a.n_ns; s++) {
    Val c[4];
    fuse_fold4(a, pres, t, s, x0, y, nvalid, C, c);
    if (canvas_out && nvalid) {
      const size_t slot = ((size_t)t * a.n_ns + s) * (size_t)a.max_w * a.max_h * 4;
      fuse_store4(canvas_out + slot + (size_t)y * a.max_w * es, a.post_dtype, es, x0, nvalid, c);
    }
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const uint8_t o = scale_one(outer, c[q]);
      if (s == 0) b[0][q] = o;
      else if (s == 1) b[1][q] = o;
      else b[2][q] = o;
    }
  }
  if (nvalid == 0) return;
  uint32_t px[4];
#pragma unroll
  for (int q = 0; q < 4; q++) {
    uint32_t o = 0;
    if (a.n_ns == 1) {
      const uint32_t v = b[0][q];
      if (v != 0xFF) o = ramp ? s_ramp[v] : (0xFF000000u | (v << 16) | (v << 8) | v);
    } else {
      const uint32_t r = b[0][q], g = b[1][q], bl = b[2][q];
      if (r != 0xFF || g != 0xFF || bl != 0xFF) o = 0xFF000000u | (bl << 16) | (g << 8) | r;
    }
    px[q] = o;
  }
  uint32_t *dst = rgba_out + ((size_t)t * a.max_h + y) * (size_t)a.max_w + x0;
  if (nvalid == 4 && (((uintptr_t)dst) & 15u) == 0) {
    uint4 u;
    u.x = px[0]; u.y = px[1]; u.z = px[2]; u.w = px[3];
    *(uint4 *)dst = u;
  } else {
    for (int q = 0; q < nvalid; q++) dst[q] = px[q];
  }
}

// ------------------------------------------------------------------------ host
static bool fuse_type_ok(int dtype) {
  return dtype == GSKYHIP_SIGNEDBYTE || dtype == GSKYHIP_BYTE || dtype == GSKYHIP_INT16 ||
         dtype == GSKYHIP_UINT16 || dtype == GSKYHIP_FLOAT32;
}

// Go's T(a) != T(b) on two nodata values (a NaN is always "different").
static bool fuse_val_differs(Val a, Val b, bool is_float) { return is_float ? !(a.f == b.f) : a.i != b.i; }

// Argument checks and descriptors, without any HIP call.
static int fuse_prepare(const gskyhip_fuse_layer *layers, int n_layers, int n_ns, const gskyhip_tile *tiles,
                        int n_tiles, int max_w, int max_h, int fusion_unscale, FuseArgs &a) {
  if (!layers || !tiles) return GSKYHIP_E_ARG;
  if (n_layers < 1 || n_layers > GSKYHIP_FUSE_MAX_LAYERS) return GSKYHIP_E_ARG;
  if (n_ns != 1 && n_ns != 3) return GSKYHIP_E_ARG;
  if (n_tiles < 0 || max_w < 1 || max_h < 1) return GSKYHIP_E_ARG;
  for (int l = 0; l < n_layers; l++) {
    if (!layers[l].canvases) return GSKYHIP_E_ARG;
  }
  for (int l = 0; l < n_layers; l++)
    if (!fuse_type_ok(layers[l].dtype)) return GSKYHIP_E_TYPE;   // raster_scaler.go:329-331
  std::memset(&a, 0, sizeof(a));
  a.tiles = tiles;
  a.n_layers = n_layers;
  a.n_ns = n_ns;
  a.max_w = max_w;
  a.max_h = max_h;
  a.groups = (max_w + 3) / 4;
  for (int l = 0; l < n_layers; l++) {
    const gskyhip_fuse_layer &in = layers[l];
    FuseLayerD &L = a.layer[l];
    const bool has_sp = !(in.sp.offset == 0.0 && in.sp.scale == 0.0 && in.sp.clip == 0.0);   // tile_pipeline.go:251
    L.canvases = (const uint8_t *)in.canvases;
    L.present = in.present;
    L.dtype = in.dtype;
    L.esize = type_size(in.dtype);
    L.scaled = (fusion_unscale == 0 && has_sp) ? 1 : 0;
    L.nodata = in.nodata;
    L.nd_own = go_conv_to(in.nodata, in.dtype);
    if (L.scaled) {
      gskyhip_scale_params sp = in.sp;
      sp.colour_scale = 0;                     // the inner ScaleParams carry none (254-257)
      L.k = host_scale_consts(in.dtype, in.nodata, sp);
    }
    const int post = L.scaled ? GSKYHIP_BYTE : in.dtype;
    if (l == 0) a.post_dtype = post;
    else if (post != a.post_dtype) return GSKYHIP_E_TYPE;   // the reference would reinterpret the bytes
  }
  // getFlexRaster's normalise against layer 0's raster (normRaster is only set
  // in the unscaled branch, 283-286)
  if (!a.layer[0].scaled) {
    for (int l = 1; l < n_layers; l++) {
      FuseLayerD &L = a.layer[l];
      if (L.scaled) continue;
      L.nodata_norm = a.layer[0].nodata;
      L.nd_norm = a.layer[0].nd_own;
      L.norm = fuse_val_differs(L.nd_norm, L.nd_own, L.dtype == GSKYHIP_FLOAT32) ? 1 : 0;
    }
  }
  return 0;
}

static inline unsigned fuse_blocks(const FuseArgs &a) {
  return (unsigned)(((int64_t)a.groups * a.max_h + 255) / 256);
}

}  // namespace gsky

using namespace gsky;

extern "C" {

int gskyhip_fuse_layers(const gskyhip_fuse_layer *layers, int n_layers, int n_ns, const gskyhip_tile *tiles,
                        int n_tiles, int max_w, int max_h, int fusion_unscale, void *canvas_out,
                        double *nodata_out, int32_t *dtype_out, void *stream) {
  if (!canvas_out || !nodata_out || !dtype_out) return GSKYHIP_E_ARG;
  FuseArgs a;
  const int r = fuse_prepare(layers, n_layers, n_ns, tiles, n_tiles, max_w, max_h, fusion_unscale, a);
  if (r) return r;
  *dtype_out = a.post_dtype;
  const int per = 65535 / n_ns;   // grid.y limit
  for (int t0 = 0; t0 < n_tiles; t0 += per) {
    const int nt = n_tiles - t0 < per ? n_tiles - t0 : per;
    a.tile0 = t0;
    hipLaunchKernelGGL(fuse_layers_kernel, dim3(fuse_blocks(a), (unsigned)(nt * n_ns)), dim3(256), 0,
                       (hipStream_t)stream, a, (uint8_t *)canvas_out, nodata_out);
    if (hipGetLastError() != hipSuccess) return GSKYHIP_E_HIP;
  }
  return 0;
}

int gskyhip_fuse_render(const gskyhip_fuse_layer *layers, int n_layers, int n_ns, const gskyhip_tile *tiles,
                        int n_tiles, int max_w, int max_h, int fusion_unscale,
                        const gskyhip_scale_params *outer_sp, const uint8_t *ramp, uint8_t *rgba_out,
                        void *canvas_out, double *nodata_out, void *stream) {
  if (!outer_sp || !rgba_out) return GSKYHIP_E_ARG;
  if (outer_sp->offset == 0.0 && outer_sp->scale == 0.0 && outer_sp->clip == 0.0)
    return GSKYHIP_E_ARG;   // auto-scale needs a reduction: gskyhip_fuse_layers, then gskyhip_scale
  FuseArgs a;
  const int r = fuse_prepare(layers, n_layers, n_ns, tiles, n_tiles, max_w, max_h, fusion_unscale, a);
  if (r) return r;
  const ScaleC outer = host_scale_consts(a.post_dtype, 0.0, *outer_sp);   // nodata: per tile, in the kernel
  for (int t0 = 0; t0 < n_tiles; t0 += 65535) {
    const int nt = n_tiles - t0 < 65535 ? n_tiles - t0 : 65535;
    a.tile0 = t0;
    hipLaunchKernelGGL(fuse_render_kernel, dim3(fuse_blocks(a), (unsigned)nt), dim3(256), 0, (hipStream_t)stream,
                       a, outer, (const uint32_t *)ramp, (uint32_t *)rgba_out, (uint8_t *)canvas_out, nodata_out);
    if (hipGetLastError() != hipSuccess) return GSKYHIP_E_HIP;
  }
  return 0;
}

}  // extern "C"
