// render.hip -- launch_render(): the batched GetMap / WCS render call on gfx950.
// It plans the batch (plan_all, plan.hip), picks the kernels for the call --
// a typed band kernel (band*.hip: render_nn.h, render_bil.h, render_cub.h,
// render_area.h, render_kern.h) where the batch has one value type, one
// namespace and no auto-scale, else the generic kernels (render_generic.h,
// instantiated in render_generic{1,3}.hip), which also take every complex
// tile -- and launches them on the call's stream.  The only kernels defined
// here are the two of the auto-scale path: minmax_init_kernel before the
// canvases are rendered and canvas_rgba_kernel (utils.Scale + palette / RGBA
// from the typed canvases) after.  No intermediate FlexRaster reaches HBM on
// the fused path.  The FlexRaster windows and the service's warp batch run
// on the same plan from windows.hip.
#include "plan.h"
#include "render_generic.h"
#include <cstdlib>

namespace gsky {

// Scale + RGBA from typed canvases (auto-scale second pass).
__global__ __launch_bounds__(256) void canvas_rgba_kernel(RenderArgs a) {
  __shared__ uint32_t s_ramp[256];
  const int tid = threadIdx.x;
  if (a.ramp) s_ramp[tid] = a.ramp[tid];
  __syncthreads();
  const int bands_per_tile = (a.max_h + a.rows_per_block - 1) / a.rows_per_block;
  const int t = blockIdx.x / bands_per_tile;
  const int band0 = (blockIdx.x % bands_per_tile) * a.rows_per_block;
  if (t >= a.n_tiles) return;
  const gskyhip_tile tile = a.tiles[t];
  const TilePlan tp = a.tplans[t];
  if (tp.status == GSKYHIP_E_ARG) return;   // tile outside the slot: never written
  const int W = tile.width, H = tile.height, n_out = a.n_out;
  ScaleK sk[3];
  bool all_created = true;
  for (int s = 0; s < n_out; s++) {
    const int ns = a.out_ns[s];
    all_created = all_created && tp.created[ns];
    if (!tp.created[ns]) continue;
    float mn = 0.0f, mx = 0.0f;
    if (a.autom) auto_minmax(a.minmax[t * 3 + s], mn, mx);
    sk[s] = make_scale(tp.dtype[ns], tp.nodata[ns], a.sp, a.autom != 0, mn, mx);
  }
  for (int r = band0; r < band0 + a.rows_per_block && r < H; r++) {
    for (int x = tid; x < W; x += 256) {
      const long idx = (long)r * a.max_w + x;
      uint8_t b[3] = {0xFF, 0xFF, 0xFF};
      if (all_created) {
        for (int s = 0; s < n_out; s++) {
          const int dt = tp.dtype[a.out_ns[s]];
          const uint8_t *cb = a.canvas + t * a.canvas_tile_stride + s * a.canvas_ns_stride;
          Val v;
          switch (dt) {
            case GSKYHIP_SIGNEDBYTE: v.i = ((const int8_t *)cb)[idx]; break;
            case GSKYHIP_BYTE: v.i = cb[idx]; break;
            case GSKYHIP_INT16: v.i = ((const int16_t *)cb)[idx]; break;
            case GSKYHIP_UINT16: v.i = ((const uint16_t *)cb)[idx]; break;
            default: v.u = ((const uint32_t *)cb)[idx]; break;
          }
          b[s] = scale_px(sk[s], v);
        }
      }
      uint32_t o = 0;
      if (all_created) {
        if (n_out == 1) {
          if (b[0] != 0xFF) o = a.ramp ? s_ramp[b[0]] : (0xFF000000u | ((uint32_t)b[0] << 16) | ((uint32_t)b[0] << 8) | b[0]);
        } else if (b[0] != 0xFF || b[1] != 0xFF || b[2] != 0xFF) {
          o = 0xFF000000u | ((uint32_t)b[2] << 16) | ((uint32_t)b[1] << 8) | b[0];
        }
      }
      ((uint32_t *)(a.rgba + (long)t * a.max_h * a.max_w * 4))[idx] = o;
    }
  }
}

__global__ void minmax_init_kernel(MinMax *m, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  m[i].mn = fenc(INFINITY);
  m[i].mx = fenc(-INFINITY);
  m[i].p0_valid = 0;
  m[i].p0 = 0.0f;
}

// One value type for the whole batch (bit mask of GSKYHIP_VT_*): the typed
// LDS band kernel, else 0.
static int single_value_type(uint32_t vt) {
  switch (vt) {
    case GSKYHIP_VT_BYTE: return GSKYHIP_BYTE;
    case GSKYHIP_VT_SIGNEDBYTE: return GSKYHIP_SIGNEDBYTE;
    case GSKYHIP_VT_INT16: return GSKYHIP_INT16;
    case GSKYHIP_VT_UINT16: return GSKYHIP_UINT16;
    case GSKYHIP_VT_FLOAT32: return GSKYHIP_FLOAT32;
    default: return 0;
  }
}

int launch_render(const RenderCall &rc, const int32_t *out_ns, int n_out, const gskyhip_scale_params &sp,
                  const uint8_t *ramp, uint8_t *rgba_out, void *canvas_out, int phase) {
  if (n_out != 1 && n_out != 3) return GSKYHIP_E_ARG;  // ogc_encoders.go:135-136
  for (int k = 0; k < n_out; k++) if (out_ns[k] < 0 || out_ns[k] >= 4) return GSKYHIP_E_ARG;
  if (rc.resample < GSKYHIP_RESAMPLE_NEAREST || rc.resample > GSKYHIP_RESAMPLE_LANCZOS) return GSKYHIP_E_ARG;
  // rgba_out == NULL: canvases only (WCS GetCoverage, FusionUnscale, ows.go:728)
  const bool autom = rgba_out && sp.offset == 0.0 && sp.scale == 0.0 && sp.clip == 0.0;
  if ((autom || !rgba_out) && !canvas_out) return GSKYHIP_E_ARG;
  if (rc.n_tiles <= 0) return 0;
  // One value type, one namespace, no auto-scale: the typed band kernel, for
  // RGBA output (GetMap) or typed canvases only (GetCoverage); complex tiles
  // (exact transforms, type promotion) still go to render_general_kernel.
  const int vt = single_value_type(rc.value_types);
  const bool mask = rc.mask_ns >= 0;
  const bool bil = rc.resample == GSKYHIP_RESAMPLE_BILINEAR;
  int lds_mode = -1;
  if (rc.resample == GSKYHIP_RESAMPLE_CUBIC) {
    // cubic: float32 canvases without a mask layer have a band kernel
    // (render_cub_kernel); every other combination runs the generic kernels
    if (vt == GSKYHIP_FLOAT32 && n_out == 1 && !rgba_out && canvas_out && !mask) lds_mode = kCanvas | kCubic;
  } else if (rc.resample == GSKYHIP_RESAMPLE_AVERAGE) {
    // average: the same combination has render_avg_kernel (render_area.h)
    if (vt == GSKYHIP_FLOAT32 && n_out == 1 && !rgba_out && canvas_out && !mask) lds_mode = kCanvas | kAverage;
  } else if (rc.resample == GSKYHIP_RESAMPLE_MODE) {
    // mode: the generic kernels
  } else if (is_kernel(rc.resample)) {
    // spline, Lanczos: the same combination has render_kern_kernel (render_kern.h)
    if (vt == GSKYHIP_FLOAT32 && n_out == 1 && !rgba_out && canvas_out && !mask)
      lds_mode = kCanvas | (rc.resample == GSKYHIP_RESAMPLE_LANCZOS ? kLanczos : kSpline);
  } else if (vt && n_out == 1 && !autom) {
    if (rgba_out && !canvas_out) lds_mode = bil ? kBilinear : 0;
    else if (!rgba_out && canvas_out) lds_mode = kCanvas | (bil ? kBilinear : 0);
  }
  // Pair-less tiles from the planner launches (fill_pairless): a whole call
  // (phase 0) of the nearest-neighbour RGBA band kernel without a mask layer
  // -- lds_mode 0 is RGBA out, no canvas, no auto-scale, one namespace -- that
  // has a pair (else neither carrier kernel runs).  Phase 1 never touches the
  // output and phase 2 alone writes every tile, as every other call does.
  bool fill = phase == 0 && lds_mode == 0 && !mask && rc.n_pairs > 0;
#ifdef GSKYHIP_AB
  if (const char *e = getenv("GSKYHIP_FILL")) fill = fill && atoi(e) != 0;
#endif
  bool filled = false;
  Carve cv;
  if (phase != 2) {  // 0: plan + render, 1: plan only, 2: render only (plan done)
    int rcode = plan_all(rc, cv, fill ? rgba_out : nullptr, &filled);
    if (rcode || phase == 1) return rcode;
  } else {
    if (!rc.workspace || rc.workspace_bytes < render_workspace_size(rc.n_tiles, rc.n_pairs, rc.max_h))
      return GSKYHIP_E_ARG;
    cv = carve(rc.workspace, rc.n_tiles, rc.n_pairs, rc.max_h);
  }
  RenderArgs a;
  a.pairs = cv.pairs; a.xforms = cv.xforms; a.tplans = cv.tplans; a.order = cv.order;
  a.tiles = rc.tiles; a.rows = cv.rows; a.rowfix = cv.rowfix; a.pool = cv.pool; a.counters = cv.counters;
  a.complex_list = cv.complex_list; a.max_h = rc.max_h; a.max_w = rc.max_w;
  a.n_tiles = rc.n_tiles; a.rows_per_block = 16; a.n_out = n_out;
  for (int k = 0; k < 3; k++) a.out_ns[k] = k < n_out ? out_ns[k] : -1;
  for (int k = 0; k < 4; k++) a.mask[k] = rc.mask_specs[k];
  a.sp = sp;
  a.autom = autom ? 1 : 0;
  a.ramp = (const uint32_t *)ramp;
  a.rgba = rgba_out;
  a.canvas = (uint8_t *)canvas_out;
  a.canvas_ns_stride = (long)rc.max_w * rc.max_h * 4;
  a.canvas_tile_stride = a.canvas_ns_stride * n_out;
  a.minmax = cv.minmax;
  a.entries = cv.entries;
  a.lds_mode = 0;
  a.cov_offsets = rc.cov_offsets;
  a.cov_stride = rc.cov_stride;
  a.skip_pairless = filled ? 1 : 0;
  const int bands = (rc.max_h + a.rows_per_block - 1) / a.rows_per_block;
  const dim3 grid((unsigned)(rc.n_tiles * bands));
  hipStream_t s = rc.stream;
  if (autom) {
    hipLaunchKernelGGL(minmax_init_kernel, dim3((rc.n_tiles * 3 + 255) / 256), dim3(256), 0, s, cv.minmax,
                       rc.n_tiles * 3);
    a.write_rgba = 0;
  } else {
    a.write_rgba = rgba_out ? 1 : 0;
  }
  if (lds_mode >= 0) {
    a.lds_mode = lds_mode;
    const int n_items = rc.n_tiles * ((rc.max_h + kLdsBandRows - 1) / kLdsBandRows) * ((rc.max_w + 511) / 512);
    launch_band_kernels(a, vt, mask, n_items, s);
    if (int e = dispatch_render_1(a, rc.resample, mask, grid, true, s)) return e;
  } else if (n_out == 1) {
    if (int e = dispatch_render_1(a, rc.resample, mask, grid, false, s)) return e;
  } else {
    if (int e = dispatch_render_3(a, rc.resample, mask, grid, false, s)) return e;
  }
  if (autom) {
    a.write_rgba = 1;
    hipLaunchKernelGGL(canvas_rgba_kernel, grid, dim3(256), 0, s, a);
  }
  return hipGetLastError() == hipSuccess ? 0 : GSKYHIP_E_HIP;
}

}  // namespace gsky
