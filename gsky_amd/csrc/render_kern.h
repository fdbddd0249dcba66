// render_kern.h -- band kernel of the two point kernels, cubic B-spline and
// Lanczos, for float32 typed canvases (WCS GetCoverage at
// GSKYHIP_RESAMPLE_CUBICSPLINE / _LANCZOS), shaped like render_cub_kernel
// (render_cub.h):
//
//   * a wave owns RPW consecutive rows of a 512-column block; a lane the 8
//     pixels lane, lane + 64, ..., lane + 448 of each row: one scalar chain
//     (order -> descriptor -> row record) per entry row, every tap load and
//     canvas store covering 64 consecutive output columns; canvas rows leave
//     through bil_store();
//   * per pixel the rule of gskyhip.h with R = 2 (spline) or 3 (Lanczos): the
//     fp64 source coordinate gives iX = floor(sx - 0.5), iY = floor(sy - 0.5)
//     and the fractions tx, ty; the taps of columns iX + 1 - R .. iX + R come
//     in one source row at a time as one 16-byte buffer load (and one 8-byte
//     load for Lanczos), 4-byte aligned; a row's taps are summed with the
//     column weights and that sum folded into the vertical sum, so a pixel
//     holds one row of taps, not 4 R^2;
//   * weights and sums are fp32.  The Lanczos weights need no sine per tap:
//     sin(pi (i - t)) = -/+ sin(pi t), and sin(pi (i - t) / 3) takes three
//     values from s = sin(pi t / 3) and c = cos(pi t / 3); s and c are
//     polynomials on [0, pi / 6] (t folded to 1 - t past 1/2; truncation below 1e-9) and sin(pi t) = 3 s -
//     4 s^3, so an axis costs two polynomials and six reciprocals;
//   * an outer tap outside the band or holding the nodata has its weight
//     zeroed; the sample is sum(w d) / sum(w) over the others, always divided;
//   * a pixel whose centre 2 x 2 holds a nodata takes the bilinear rule on
//     those four taps (fp32 weights, dropped taps renormalised: bil4_renorm(),
//     resample.h);
//   * the fp32 path runs only where the centre 2 x 2 lies inside the band and
//     every row load lies wholly inside the buffer (a load may start in the
//     previous source row or end in the next: those taps carry no weight), so
//     no value depends on the buffer range check.  Every other pixel -- centre
//     across the band's edge (bilinear_rule() with its edge cases), the first
//     and last source row's overhanging corners -- and every pixel of a band
//     whose nodata no float32 equals runs kern_fetch() (kernel_rule(),
//     resample.h, fp64) in a rolled loop behind a branch.  Measured and not
//     kept: the edge pixels through band_bil() alone, with
//     kern_fetch() left for the corners (Lanczos 7.80 vs 6.78 ms on C3).
#pragma once
#include "render_bil.h"

namespace gsky {

// fp32 weights w[i + R - 1] = K(i - t), i = 1 - R .. R, t in [0, 1].
template <int R>
__device__ __forceinline__ void kern_weights(float t, float (&w)[2 * R]) {
  if constexpr (R == 2) {
    // |x| = 1 + t, t, 1 - t, 2 - t
    const float u = 1.0f - t;
    const float t2 = t * t, u2 = u * u;
    const float k6 = 1.0f / 6.0f;
    w[0] = (u2 * u) * k6;
    w[1] = __builtin_fmaf(3.0f, t2 * t, __builtin_fmaf(-6.0f, t2, 4.0f)) * k6;
    w[2] = __builtin_fmaf(3.0f, u2 * u, __builtin_fmaf(-6.0f, u2, 4.0f)) * k6;
    w[3] = (t2 * t) * k6;
  } else {
    // K is even: past t = 1/2 the weights are those of 1 - t (exact in fp32)
    // in reverse, which keeps h - g below free of cancellation
    const bool flip = t > 0.5f;
    const float tt = flip ? 1.0f - t : t;
    const float th = tt * 1.04719755119659775f;   // pi tt / 3 in [0, pi / 6]
    const float z = th * th;
    float ps = -2.50521083854417188e-8f;          // sin: th (1 - z / 3! + ... - z^5 / 11!)
    ps = __builtin_fmaf(ps, z, 2.75573192239858907e-6f);
    ps = __builtin_fmaf(ps, z, -1.98412698412698413e-4f);
    ps = __builtin_fmaf(ps, z, 8.33333333333333333e-3f);
    ps = __builtin_fmaf(ps, z, -1.66666666666666667e-1f);
    const float s = __builtin_fmaf(ps * z, th, th);
    float pc = 2.08767569878680990e-9f;           // cos: 1 - z / 2! + ... + z^6 / 12!
    pc = __builtin_fmaf(pc, z, -2.75573192239858907e-7f);
    pc = __builtin_fmaf(pc, z, 2.48015873015873016e-5f);
    pc = __builtin_fmaf(pc, z, -1.38888888888888889e-3f);
    pc = __builtin_fmaf(pc, z, 4.16666666666666667e-2f);
    pc = __builtin_fmaf(pc, z, -0.5f);
    const float c = __builtin_fmaf(pc, z, 1.0f);
    const float sp = s * __builtin_fmaf(-4.0f * s, s, 3.0f);   // sin(pi tt)
    const float h = 0.866025403784438647f * c, g = 0.5f * s;
    // sin(pi (i - tt) / 3), i = -2 .. 3; sin(pi (i - tt)) = -sp, sp, -sp, sp, -sp, sp
    const float sq[6] = {g - h, -h - g, -s, h - g, h + g, s};
    const float k = 3.0f / 9.86960440108935862f * sp;          // 3 sin(pi tt) / pi^2, its sign below
    float u[6];
#pragma unroll
    for (int i = 0; i < 6; i++) {
      const float x = (float)(i - 2) - tt;
      const float ax = __builtin_fabsf(x);
      const float v = ((i & 1) ? k : -k) * sq[i] * __builtin_amdgcn_rcpf(x * x);
      u[i] = ax < 0x1p-12f ? 1.0f : (ax >= 3.0f ? 0.0f : v);
    }
#pragma unroll
    for (int i = 0; i < 6; i++) w[i] = flip ? u[5 - i] : u[i];
  }
}

// HP: pixels whose taps are in flight together; WPS: waves per SIMD the
// register budget is sized for.
template <int R, int RPW, int HP, int WPS>
__global__ __launch_bounds__(256, WPS) void render_kern_kernel(RenderArgs a, const EntryD *__restrict__ ents,
                                                             const int32_t *__restrict__ order,
                                                             const RowRec *__restrict__ rows,
                                                             const Leaf *__restrict__ pool,
                                                             const TilePlan *__restrict__ tplans,
                                                             const gskyhip_tile *__restrict__ tiles, int n_items) {
  static_assert(kNnPx % HP == 0, "HP divides the pixels of a lane");
  constexpr int RES = R == 2 ? GSKYHIP_RESAMPLE_CUBICSPLINE : GSKYHIP_RESAMPLE_LANCZOS;
  constexpr int NT = 2 * R;
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
      // the nodata test of a tap in float32 (exact: the band's nodata is a
      // float32 value or NaN); other bands take the fp64 rule at every pixel
      const bool nd_f32 = !hnd || nd_nan || (double)(float)nd64 == nd64;
      const float ndf = (float)nd64;
      const float *bandp = (const float *)uniform_ptr(e.band);
      const int nelem = bx * by;   // < 2^29: the buffer's byte count fits an int
      const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
          (void *)bandp, (short)0, (int)((int64_t)bx * by * 4), 0x00020000);
      uint32_t slow = 0u;   // bit q: the lane's pixel q takes the fp64 rule
#pragma unroll
      for (int h = 0; h < kNnPx; h += HP) {
        float tx[HP], ty[HP];
        bool ok[HP], fast[HP];
        int iX[HP], iY[HP];
#pragma unroll
        for (int q = 0; q < HP; q++) {
          double sx, sy;
          ok[q] = coords(h + q, sx, sy);
          const double fx = floor(sx - 0.5), fy = floor(sy - 0.5);
          const bool ctr = ok[q] && nd_f32 && kernel_inside(fx, fy, bx, by);
          tx[q] = (float)(sx - 0.5 - fx);
          ty[q] = (float)(sy - 0.5 - fy);
          // ctr: 0 <= iX <= bx - 2, 0 <= iY <= by - 2
          iX[q] = ctr ? (int)fx : 0;
          iY[q] = ctr ? (int)fy : 0;
          // the first and the last row load lie inside the buffer (elements)
          const int x0 = iX[q] + 1 - R;
          const int ylo = max(iY[q] + 1 - R, 0), yhi = min(iY[q] + R, by - 1);
          fast[q] = ctr && ylo * bx + x0 >= 0 && yhi * bx + x0 + NT <= nelem;
          slow |= (ok[q] && !fast[q]) ? (1u << (h + q)) : 0u;
        }
        float wx[HP][NT], wy[HP][NT], accR[HP], accW[HP], tv[HP][4];
        bool cnd[HP];
#pragma unroll
        for (int q = 0; q < HP; q++) {
          kern_weights<R>(tx[q], wx[q]);
          kern_weights<R>(ty[q], wy[q]);
          accR[q] = 0.0f;
          accW[q] = 0.0f;
          cnd[q] = false;
        }
#pragma unroll
        for (int m = 0; m < NT; m++) {
          float f[HP][NT];
#pragma unroll
          for (int q = 0; q < HP; q++) {
            const int yy = iY[q] + 1 - R + m;
            const bool rowin = fast[q] && (unsigned)yy < (unsigned)by;
            // a row outside the band (or a pixel off the fp32 path): an offset
            // past the band (< 2 GiB), no fetch; its values are not used
            const uint32_t o = rowin ? (uint32_t)(yy * bx + iX[q] + 1 - R) * 4u : 0x80000000u;
            const u32x4 v4 = __builtin_amdgcn_raw_buffer_load_b128(rs, o, 0, 0);
            f[q][0] = __uint_as_float(v4.x); f[q][1] = __uint_as_float(v4.y);
            f[q][2] = __uint_as_float(v4.z); f[q][3] = __uint_as_float(v4.w);
            if constexpr (R == 3) {
              const u32x2 v2 = __builtin_amdgcn_raw_buffer_load_b64(rs, rowin ? o + 16u : 0x80000000u, 0, 0);
              f[q][4] = __uint_as_float(v2.x); f[q][5] = __uint_as_float(v2.y);
            }
          }
#pragma unroll
          for (int q = 0; q < HP; q++) {
            const int yy = iY[q] + 1 - R + m;
            const bool rowin = fast[q] && (unsigned)yy < (unsigned)by;
            float hR = 0.0f, hW = 0.0f;
#pragma unroll
            for (int i = 0; i < NT; i++) {
              const bool isnd = hnd & (nd_nan ? (f[q][i] != f[q][i]) : (f[q][i] == ndf));
              // a tap outside the band (its row, its column) or holding the nodata is dropped
              const bool use = rowin & ((unsigned)(iX[q] + 1 - R + i) < (unsigned)bx) & !isnd;
              hW += use ? wx[q][i] : 0.0f;
              hR = use ? __builtin_fmaf(f[q][i], wx[q][i], hR) : hR;
              if ((m == R - 1 || m == R) && (i == R - 1 || i == R)) {   // the centre 2 x 2
                cnd[q] = cnd[q] | isnd;
                tv[q][(m - (R - 1)) * 2 + (i - (R - 1))] = f[q][i];
              }
            }
            accW[q] = __builtin_fmaf(hW, wy[q][m], accW[q]);
            accR[q] = __builtin_fmaf(hR, wy[q][m], accR[q]);
          }
        }
#pragma unroll
        for (int q = 0; q < HP; q++) {
          float v = accR[q] / accW[q];
          if (cnd[q]) {
            // a nodata among the centre 2 x 2 (all four inside the band): the
            // bilinear rule on it, nodata taps dropped and the weights renormalised
            const float bwx[2] = {1.0f - tx[q], tx[q]}, bwy[2] = {1.0f - ty[q], ty[q]};
            v = bil4_renorm<float>(tv[q], bwx, bwy, nd_nan, ndf, fillv);
          }
          // a pixel without a sample folds the window fill; a slow one folds below
          if (fast[q] || !ok[q]) fold(h + q, fast[q] ? v : fillv);
        }
      }
      if (slow != 0u) {   // rolled: one body of the fp64 rule
#pragma unroll 1
        for (int qq = 0; qq < kNnPx; qq++) {
          if (((slow >> qq) & 1u) == 0u) continue;
          double sx, sy;
          float v = fillv, got;
          if (coords(qq, sx, sy) && kern_fetch<float, RES>(e, sx, sy, got)) v = got;
#pragma unroll
          for (int q = 0; q < kNnPx; q++)
            if (q == qq) fold(q, v);
        }
      }
    }

    bil_store(a, t, r, xl, lane, full, ncols, c);
  }
}

// Spline and Lanczos float canvases (no mask layer): 4 rows per wave; the
// resource reports are in DESIGN.md 4.
template <int R>
void launch_kern(const RenderArgs &a, hipStream_t s) {
  const int items = a.n_tiles * ((a.max_h + 15) / 16) * ((a.max_w + kBandCols - 1) / kBandCols);
  hipLaunchKernelGGL((render_kern_kernel<R, 4, R == 2 ? 2 : 1, 4>), dim3((unsigned)items), dim3(256), 0, s, a,
                     a.entries, a.order, a.rows, a.pool, a.tplans, a.tiles, items);
}
void launch_spline(const RenderArgs &a, hipStream_t s) { launch_kern<2>(a, s); }
void launch_lanczos(const RenderArgs &a, hipStream_t s) { launch_kern<3>(a, s); }

}  // namespace gsky
