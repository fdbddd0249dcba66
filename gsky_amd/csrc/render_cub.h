// render_cub.h -- cubic convolution band kernel for float32 typed canvases
// (WCS GetCoverage at GSKYHIP_RESAMPLE_CUBIC), shaped like render_bil_kernel
// (render_bil.h):
//
//   * a wave owns RPW consecutive rows of a 512-column block; a lane the 8
//     pixels lane, lane + 64, ..., lane + 448 of each row, so one row of one
//     entry is a single scalar chain (order -> descriptor -> row record) and
//     every tap load and canvas store instruction covers 64 consecutive
//     output columns; canvas rows leave through bil_store();
//   * per pixel GWKCubicResample4Sample (GDAL 3.0.1; the rule is written out
//     in gskyhip.h): the fp64 source coordinate of the row record gives iX =
//     floor(sx - 0.5), iY = floor(sy - 0.5) and the fractions tx, ty; the 16
//     taps arrive as four 16-byte buffer loads (columns iX - 1 .. iX + 2 of
//     source rows iY - 1 .. iY + 2, 4-byte aligned), issued for HP pixels
//     before the first wait;
//   * a pixel is cubic only where all 16 taps lie inside the band, decided
//     from the indices: such a pixel's four loads lie wholly inside the
//     buffer, every other pixel loads nothing (an offset past the band), so
//     no value ever depends on the buffer range check;
//   * the eight 1-D weights and the 16-term sum are fp32 (fused multiply-add:
//     one rounding per term); against the fp64 rule this stays within a few
//     1e-7 of the data's scale (the resampling bar is 1e-4);
//   * a cubic pixel with a nodata tap among the 16 takes the bilinear rule on
//     the centre 2 x 2 of the taps it already holds (fp32 weights, dropped
//     taps renormalised: bil4_renorm(), resample.h, as render_bil_kernel);
//   * a pixel with a tap outside the band takes the bilinear rule with its
//     edge cases (the -1 rule, taps outside dropped) through bilinear_rule()
//     (resample.h, fp64) behind a branch: only the band's two outer rows
//     and columns of source pixels reach it;
//   * a band whose nodata no float32 equals runs cub_fetch() (cubic_rule(),
//     resample.h, fp64) one pixel at a time, for render_bil_kernel's reason: a sample
//     over taps that all hold (float)nodata must be exactly that value.
#pragma once
#include "render_bil.h"

namespace gsky {

// fp32 weights of CC(t, f0..f3) = sum w[i] * f[i]:
//   2 w0 = -t + 2 t^2 - t^3, 2 w1 = 2 - 5 t^2 + 3 t^3,
//   2 w2 = t + 4 t^2 - 3 t^3, 2 w3 = t^3 - t^2.
__device__ __forceinline__ void cub_weights(float t, float (&w)[4]) {
  const float t2 = t * t, t3 = t2 * t;
  w[0] = 0.5f * (__builtin_fmaf(2.0f, t2, -t) - t3);
  w[1] = 0.5f * __builtin_fmaf(3.0f, t3, __builtin_fmaf(-5.0f, t2, 2.0f));
  w[2] = 0.5f * __builtin_fmaf(-3.0f, t3, __builtin_fmaf(4.0f, t2, t));
  w[3] = 0.5f * (t3 - t2);
}

// HP: pixels whose 16 taps are in flight together; WPS: waves per SIMD the
// register budget is sized for.
template <int RPW, int HP, int WPS>
__global__ __launch_bounds__(256, WPS) void render_cub_kernel(RenderArgs a, const EntryD *__restrict__ ents,
                                                            const int32_t *__restrict__ order,
                                                            const RowRec *__restrict__ rows,
                                                            const Leaf *__restrict__ pool,
                                                            const TilePlan *__restrict__ tplans,
                                                            const gskyhip_tile *__restrict__ tiles, int n_items) {
  static_assert(kNnPx % HP == 0, "HP divides the pixels of a lane");
  constexpr int kRowsBlk = 4 * RPW;
  const int item = blockIdx.x;
  if (item >= n_items) return;
  const int bands_per_tile = (a.max_h + kRowsBlk - 1) / kRowsBlk;
  const int col_blocks = (a.max_w + kBandCols - 1) / kBandCols;
  const int t = item / (bands_per_tile * col_blocks);
  const int in_tile = item - t * bands_per_tile * col_blocks;
  const TilePlan &tp = tplans[t];
  if (tp.complex || (tp.n_entries > 0 && tp.vt != GSKYHIP_FLOAT32)) return;   // empty tiles: written here
  const gskyhip_tile &tile = tiles[t];
  const int W = tile.width, H = tile.height;
  const int band0 = (in_tile / col_blocks) * kRowsBlk;
  const int xb = (in_tile % col_blocks) * kBandCols;
  if (band0 >= H || xb >= W) return;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int r0 = band0 + wave * RPW;
  if (r0 >= H) return;

  const int ns_out = a.out_ns[0];
  const float cnod = go_conv_to(tp.nodata[ns_out], tp.dtype[ns_out]).f;
  const int32_t *ord = order + tile.pair_begin;
  const int n_entries = tp.n_entries;
  const int ncols = min(kBandCols, W - xb);
  const bool full = ncols == kBandCols;
  const int xl = xb + lane;

#pragma unroll 1
  for (int j = 0; j < RPW; j++) {
    const int r = r0 + j;
    if (r >= H) break;
    float c[kNnPx];
#pragma unroll
    for (int q = 0; q < kNnPx; q++) c[q] = cnod;

#pragma unroll 1
    for (int k = 0; k < n_entries; k++) {
      const EntryD &e = ents[ord[k]];
      const int eyoff = e.yoff, eh = e.h, exoff = e.xoff, ew = e.w;
      if (e.ns != ns_out || ew <= 0) continue;
      const int ir = r - eyoff;
      if (ir < 0 || ir >= eh) continue;
      const int lim = max(0, min(ew, W - exoff));
      const int c0 = exoff - xb, c1 = exoff + lim - xb;
      if (c1 <= 0 || c0 >= ncols) continue;
      const RowRec *rr = rows + e.row_base + ir;
      const int kind = __builtin_amdgcn_readfirstlane(rr->kind);
      const int bx = e.band_x, by = e.band_y;
      const float nd = e.nd.f, fillv = e.fill.f;
      const bool fill_mode = e.fill_mode != 0;
      const bool hnd = e.has_nodata != 0;
      const double nd64 = e.nodata64;
      const bool nd_nan = nd64 != nd64;
      const int ic0 = xl - exoff;
      const double xs0 = rr->v[0], ys0 = rr->v[1], dX = rr->v[2], dY = rr->v[3];
      // the source coordinate of the lane's pixel q: the LINEAR row's fp64
      // expressions (src_coords()), or the leaf's (POOL rows); false: no sample
      auto coords = [&](int q, double &sx, double &sy) -> bool {
        const int ic = ic0 + 64 * q;
        const bool inw = (unsigned)ic < (unsigned)lim;
        if (kind == ROW_LINEAR) {
          const double dist = (double)ic;
          sy = ys0 + dY * dist;
          sx = xs0 + dX * dist;
          return inw;
        }
        sx = 0.0;
        sy = 0.0;
        return inw && lin_coords(*rr, pool, inw ? ic : 0, sx, sy);
      };
      auto fold = [&](int q, float v) {
        const int ic = ic0 + 64 * q;
        const bool take = ((unsigned)ic < (unsigned)lim) & (v != nd) & (!fill_mode | (c[q] == nd));
        c[q] = take ? v : c[q];
      };
      // the nodata test of a tap in float32 (exact: the band's nodata is a float32 value or NaN)
      const bool nd_f32 = !hnd || nd_nan || (double)(float)nd64 == nd64;
      const float ndf = (float)nd64;
      if (!nd_f32) {   // rare bands: the fp64 rule, one pixel at a time
#pragma unroll
        for (int q = 0; q < kNnPx; q++) {
          double sx, sy;
          float v = fillv, got;
          if (coords(q, sx, sy) && cub_fetch<float>(e, sx, sy, got)) v = got;
          fold(q, v);
        }
        continue;
      }
      const float *bandp = (const float *)uniform_ptr(e.band);
      const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
          (void *)bandp, (short)0, (int)((int64_t)bx * by * 4), 0x00020000);
      const uint32_t rowb = (uint32_t)bx * 4u;
#pragma unroll
      for (int h = 0; h < kNnPx; h += HP) {
        u32x4 tap[HP][4];
        float tx[HP], ty[HP];
        bool cub[HP];
#pragma unroll
        for (int q = 0; q < HP; q++) {
          double sx, sy;
          const bool ok = coords(h + q, sx, sy);
          const double fx = floor(sx - 0.5), fy = floor(sy - 0.5);
          cub[q] = ok && cubic_inside(fx, fy, bx, by);
          tx[q] = (float)(sx - 0.5 - fx);
          ty[q] = (float)(sy - 0.5 - fy);
          // cubic: 1 <= iX <= bx - 3, 1 <= iY <= by - 3, the four loads inside
          // the buffer; otherwise an offset past the band (< 2 GiB): no fetch
          const int iX = cub[q] ? (int)fx : 1, iY = cub[q] ? (int)fy : 1;
          const uint32_t o = cub[q] ? (uint32_t)((iY - 1) * bx + (iX - 1)) * 4u : 0x80000000u;
#pragma unroll
          for (int m = 0; m < 4; m++)
            tap[q][m] = __builtin_amdgcn_raw_buffer_load_b128(rs, cub[q] ? o + (uint32_t)m * rowb : 0x80000000u, 0, 0);
        }
#pragma unroll
        for (int q = 0; q < HP; q++) {
          float wx[4], wy[4];
          cub_weights(tx[q], wx);
          cub_weights(ty[q], wy);
          float acc = 0.0f;
          bool anynd = false;
#pragma unroll
          for (int m = 0; m < 4; m++) {
            const float f[4] = {__uint_as_float(tap[q][m].x), __uint_as_float(tap[q][m].y),
                                __uint_as_float(tap[q][m].z), __uint_as_float(tap[q][m].w)};
            float hrow = f[0] * wx[0];
#pragma unroll
            for (int i = 1; i < 4; i++) hrow = __builtin_fmaf(f[i], wx[i], hrow);
#pragma unroll
            for (int i = 0; i < 4; i++) anynd = anynd | (nd_nan ? (f[i] != f[i]) : (f[i] == ndf));
            acc = m == 0 ? hrow * wy[0] : __builtin_fmaf(hrow, wy[m], acc);
          }
          float v = acc;
          if (hnd & anynd) {
            // a nodata tap among the 16: the bilinear rule on the centre 2 x 2
            // (all four inside the band), nodata taps dropped and the weights
            // renormalised
            const float tv[4] = {__uint_as_float(tap[q][1].y), __uint_as_float(tap[q][1].z),
                                 __uint_as_float(tap[q][2].y), __uint_as_float(tap[q][2].z)};
            const float bwx[2] = {1.0f - tx[q], tx[q]}, bwy[2] = {1.0f - ty[q], ty[q]};
            v = bil4_renorm<float>(tv, bwx, bwy, nd_nan, ndf, fillv);
          }
          if (!cub[q]) {   // a tap outside the band (or no sample at all): the bilinear rule, fp64
            double sx, sy;
            float got;
            v = fillv;
            if (coords(h + q, sx, sy) && band_bil<float>(bandp, bx, by, hnd, nd64, GSKYHIP_FLOAT32, sx, sy, got))
              v = got;
          }
          fold(h + q, v);
        }
      }
    }

    bil_store(a, t, r, xl, lane, full, ncols, c);
  }
}

// Cubic float canvases (no mask layer): 4 rows per wave, 2 pixels' taps (32
// registers) in flight: 86 VGPRs, no scratch, 5 waves per SIMD.  Measured and
// not kept: 4 pixels in flight (125 VGPRs, 4 waves per SIMD,
// 1.37 vs 1.27 ms on C3); budgets of 6 and 8 waves per SIMD spill to scratch.
void launch_cub(const RenderArgs &a, hipStream_t s) {
  const int items = a.n_tiles * ((a.max_h + 15) / 16) * ((a.max_w + kBandCols - 1) / kBandCols);
  hipLaunchKernelGGL((render_cub_kernel<4, 2, 4>), dim3((unsigned)items), dim3(256), 0, s, a, a.entries, a.order,
                     a.rows, a.pool, a.tplans, a.tiles, items);
}

}  // namespace gsky
