// render_area.h -- area-average band kernel for float32 typed canvases (WCS
// GetCoverage at GSKYHIP_RESAMPLE_AVERAGE; the rule is written out in
// gskyhip.h), shaped like render_cub_kernel (render_cub.h):
//
//   * a wave owns RPW consecutive rows of a 512-column block; a lane the 8
//     pixels lane, lane + 64, ..., lane + 448 of each row, so one row of one
//     entry is a single scalar chain (order -> descriptor -> row record and
//     the record of the row beside it) and every tap load and canvas store
//     instruction covers 64 consecutive output columns; canvas rows leave
//     through bil_store();
//   * the footprint of a pixel of a LINEAR row: u is the row record's (dX,
//     dY), scalar per row (zero for a window one pixel wide); v is the
//     difference to the pixel of the same column on the next window row (the
//     previous one on the window's last row), from that row's record when it
//     is LINEAR too; half extents, interval bounds and the tap ranges
//     (area_taps(), resample.h) are fp64;
//   * a pixel whose taps are not strided (at most 8 per axis) sums them in
//     fp32: the weights are the covered lengths relative to the first tap
//     (exact differences of the fp64 bounds, rounded once), the sums run in
//     scan order with one fused multiply-add per tap; against the fp64 rule
//     this stays within a few 1e-7 of the data's scale (the resampling bar is
//     1e-4).  Taps arrive as 8-byte buffer loads (columns lo + 2k, lo + 2k +
//     1 of one source row), HP pixels' rows in flight together;
//   * the trip counts are wave-uniform: the wave's largest row count and
//     largest column-pair count, lanes with fewer taps predicated.  A tap
//     that is not the pixel's is dropped by its index, never by what the load
//     returned: a load of no tap at all has an offset past the band (no
//     fetch), the odd half of a pair may lie past the row's end, and neither
//     value is used -- no value depends on the buffer range check;
//   * behind a branch, through area_fetch() (render_common.h: the fp64 rule,
//     the footprint from the neighbours' coordinates): pixels whose taps are
//     strided (more than 8 source pixels per destination pixel along an axis),
//     rows that are not LINEAR or whose neighbour row is not, and bands whose
//     nodata no float32 equals (render_bil_kernel's reason).
#pragma once
#include "render_bil.h"

namespace gsky {

// HP: pixels whose tap rows are in flight together; WPS: waves per SIMD the
// register budget is sized for.
template <int RPW, int HP, int WPS>
__global__ __launch_bounds__(256, WPS) void render_avg_kernel(RenderArgs a, const EntryD *__restrict__ ents,
                                                            const int32_t *__restrict__ order,
                                                            const RowRec *__restrict__ rows,
                                                            const Leaf *__restrict__ pool,
                                                            const TilePlan *__restrict__ tplans,
                                                            const gskyhip_tile *__restrict__ tiles, int n_items) {
  static_assert(kNnPx % HP == 0, "HP divides the pixels of a lane");
  constexpr int kRowsBlk = 4 * RPW;
  constexpr int kPairs = kAreaTaps / 2;   // 8-byte loads per tap row
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
      // the window row that gives v: the next one, the previous one on the last row, this one (v = 0) alone
      const RowRec *rn = rr + (ir + 1 < eh ? 1 : (ir > 0 ? -1 : 0));
      const int kind = __builtin_amdgcn_readfirstlane(rr->kind);
      const int kindn = __builtin_amdgcn_readfirstlane(rn->kind);
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
      // the fp64 rule of the lane's pixel q (its footprint from the neighbours' coordinates)
      auto slow_px = [&](int q) -> float {
        double sx, sy;
        if (!coords(q, sx, sy)) return fillv;
        return area_fetch<float, GSKYHIP_RESAMPLE_AVERAGE>(e, rows, pool, ic0 + 64 * q, ir, sx, sy, fillv);
      };
      // the nodata test of a tap in float32 (exact: the band's nodata is a float32 value or NaN)
      const bool nd_f32 = !hnd || nd_nan || (double)(float)nd64 == nd64;
      const float ndf = (float)nd64;
      if (!nd_f32 || kind != ROW_LINEAR || kindn != ROW_LINEAR) {   // rare bands and rows: one pixel at a time
#pragma unroll
        for (int q = 0; q < kNnPx; q++) fold(q, slow_px(q));
        continue;
      }
      const double ux = ew > 1 ? dX : 0.0, uy = ew > 1 ? dY : 0.0;
      const double nxs0 = rn->v[0], nys0 = rn->v[1], ndX = rn->v[2], ndY = rn->v[3];
      const float *bandp = (const float *)uniform_ptr(e.band);
      const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
          (void *)bandp, (short)0, (int)((int64_t)bx * by * 4), 0x00020000);
#pragma unroll
      for (int h = 0; h < kNnPx; h += HP) {
        int cx[HP], cy[HP];         // taps along x and y; 0: no fp32 sample
        uint32_t o0[HP];            // byte offset of the first tap
        float ax0[HP], ax1[HP], ay0[HP], ay1[HP];   // the footprint's bounds relative to the first tap
        bool slow[HP];
        int mcx = 0, mcy = 0;
#pragma unroll
        for (int q = 0; q < HP; q++) {
          double sx, sy;
          const bool ok = coords(h + q, sx, sy);
          const double dist = (double)(ic0 + 64 * (h + q));
          const double vx = (nxs0 + ndX * dist) - sx, vy = (nys0 + ndY * dist) - sy;
          AreaAxis ax = {0, 0, 1, 0.0, 0.0}, ay = {0, 0, 1, 0.0, 0.0};
          const bool has = ok && area_taps(sx, area_half(ux, vx), bx, ax) && area_taps(sy, area_half(uy, vy), by, ay);
          slow[q] = has && (ax.stride > 1 || ay.stride > 1);
          const bool f32 = has && !slow[q];
          cx[q] = f32 ? ax.hi - ax.lo : 0;
          cy[q] = f32 ? ay.hi - ay.lo : 0;
          o0[q] = f32 ? ((uint32_t)ay.lo * (uint32_t)bx + (uint32_t)ax.lo) * 4u : 0u;
          ax0[q] = (float)(ax.x0 - (double)ax.lo);
          ax1[q] = (float)(ax.x1 - (double)ax.lo);
          ay0[q] = (float)(ay.x0 - (double)ay.lo);
          ay1[q] = (float)(ay.x1 - (double)ay.lo);
          mcx = max(mcx, cx[q]);
          mcy = max(mcy, cy[q]);
        }
        // the wave's trip counts: its largest row count and column-pair count
        int nyw = kAreaTaps, nxw = kPairs;
        while (nyw > 0 && !__any(mcy >= nyw)) nyw--;
        while (nxw > 0 && !__any(mcx > 2 * (nxw - 1))) nxw--;
        float aR[HP], aW[HP];
#pragma unroll
        for (int q = 0; q < HP; q++) aR[q] = aW[q] = 0.0f;
        const uint32_t rowb = (uint32_t)bx * 4u;
#pragma unroll 1
        for (int ty = 0; ty < nyw; ty++) {
          u32x2 tap[HP][kPairs];
#pragma unroll
          for (int q = 0; q < HP; q++)
#pragma unroll
            for (int p = 0; p < kPairs; p++)
              if (p < nxw) {
                // the pair's first tap is the pixel's, or nothing is fetched (an offset past the band, < 2 GiB)
                const bool in = (ty < cy[q]) & (2 * p < cx[q]);
                tap[q][p] = __builtin_amdgcn_raw_buffer_load_b64(
                    rs, in ? o0[q] + (uint32_t)ty * rowb + (uint32_t)p * 8u : 0x80000000u, 0, 0);
              }
#pragma unroll
          for (int q = 0; q < HP; q++) {
            const float fy = (float)ty;
            const float wy = fminf(fy + 1.0f, ay1[q]) - fmaxf(fy, ay0[q]);
#pragma unroll
            for (int p = 0; p < kPairs; p++)
              if (p < nxw) {
#pragma unroll
                for (int m = 0; m < 2; m++) {
                  const int tx = 2 * p + m;
                  const float fx = (float)tx;
                  const float w = (fminf(fx + 1.0f, ax1[q]) - fmaxf(fx, ax0[q])) * wy;
                  const float f = __uint_as_float(m ? tap[q][p].y : tap[q][p].x);
                  const bool isnd = hnd & (nd_nan ? (f != f) : (f == ndf));
                  // bitwise, not short-circuit: no per-tap exec-mask branches
                  const bool use = (ty < cy[q]) & (tx < cx[q]) & !isnd & (w > 0.0f);
                  aW[q] += use ? w : 0.0f;
                  aR[q] = use ? __builtin_fmaf(f, w, aR[q]) : aR[q];
                }
              }
          }
        }
#pragma unroll
        for (int q = 0; q < HP; q++) {
          float v = fillv;
          if (aW[q] >= 0.00001f) v = aR[q] / aW[q];
          if (slow[q]) v = slow_px(h + q);   // strided taps: the fp64 rule
          fold(h + q, v);
        }
      }
    }

    bil_store(a, t, r, xl, lane, full, ncols, c);
  }
}

// Average float canvases (no mask layer): 4 rows per wave, 2 pixels' tap rows
// in flight: 111 VGPRs, no scratch, 4 waves per SIMD.  Not built (compiler
// resource report only): every smaller register budget spills to scratch -- 5
// / 6 / 8 waves per SIMD 80 / 128 / 192 B per lane, one pixel in flight at 6 /
// 8 waves 48 / 96 B -- and 4 pixels in flight hold 128 VGPRs and 160 B.
void launch_avg(const RenderArgs &a, hipStream_t s) {
  const int items = a.n_tiles * ((a.max_h + 15) / 16) * ((a.max_w + kBandCols - 1) / kBandCols);
  hipLaunchKernelGGL((render_avg_kernel<4, 2, 4>), dim3((unsigned)items), dim3(256), 0, s, a, a.entries, a.order,
                     a.rows, a.pool, a.tplans, a.tiles, items);
}

}  // namespace gsky
