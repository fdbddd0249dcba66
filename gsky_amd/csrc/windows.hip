// windows.hip -- what runs on a planned batch (plan_all, plan.hip) besides
// the GetMap / WCS render of render.hip, each with its host launcher:
//   launch_warp_windows    the warped window of every pair (FlexRaster data,
//                          any resampling rule) with its bbox / dtype / nodata.
//   launch_warp_jobs       the service's warp batch: per request its window
//                          and its bytesRead in one pass, then the reply record.
//   launch_pair_footprint, observability of a planned batch: the source
//   launch_pair_touched    footprint of each pair, and the source elements and
//                          128-byte lines the whole batch touches.
// The window kernels sample through render_generic.h's helpers.
#include "plan.h"
#include "render_generic.h"
#include <map>
#include <vector>
#include <cstdlib>

namespace gsky {

// Warped window of each pair (the FlexRaster data of tile_grpc.go:228-241).
template <int RES>
__global__ __launch_bounds__(256) void warp_window_kernel(const PairPlan *pairs, const Xform *xforms,
                                                          const RowRec *rows, const Leaf *pool, int max_h,
                                                          int max_w, int n_pairs, uint8_t *out, long stride) {
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long per = (long)max_h * max_w;
  const int p = (int)(gid / per);
  if (p >= n_pairs) return;
  const PairPlan &pp = pairs[p];
  const long k = gid % per;
  const int row = (int)(k / max_w), i = (int)(k % max_w);
  if (row >= pp.h || i >= pp.w) return;
  const RowRec &rr = rows[(long)p * max_h + row];
  const Val v = warped_value<true, RES>(pp, rr, pool, xforms + p, i, row);
  const int dsz = type_size(pp.out_dtype);
  uint8_t *o = out + p * stride;
  const long idx = (long)row * pp.w + i;
  if (dsz == 1) o[idx] = (uint8_t)v.i;
  else if (dsz == 2) ((uint16_t *)o)[idx] = (uint16_t)v.i;
  else ((uint32_t *)o)[idx] = v.u;
}

// bytesRead of the drop-in (warp.go:278-347) for every (single-pair) request
// of a warp batch, job = pair: per window pixel the reference's two tests --
// the cache heuristic's x test (success, dx >= 0, iSrcX < srcXSize; no dy
// test) and the full gather test -- give the source x (xsrc, for the cache
// decision), the first valid pixel, the valid count and the bits of the
// source blocks that valid pixels touch.  This kernel clears a job's bits and
// counters; warp_job_kernel fills them and warp_job_resolve_kernel reads them.
__global__ __launch_bounds__(256) void block_stats_init_kernel(const BlockStatsJob *jobs, char *scratch,
                                                               int32_t *stats) {
  const BlockStatsJob J = jobs[blockIdx.x];
  uint32_t *bits = (uint32_t *)(scratch + J.bits_off);
  for (int k = threadIdx.x; k < J.n_words; k += blockDim.x) bits[k] = 0u;
  if (threadIdx.x == 0) {
    int32_t *st = stats + 4 * blockIdx.x;
    st[0] = 0x7FFFFFFF; st[1] = 0; st[2] = 0; st[3] = 0;
  }
}

// One window pixel of a job from one evaluation of its source coordinates:
// its value (warped_value's: sampled_value() or the window fill) and the
// bytesRead inputs (warp.go:281-347): xs, the source x where the cache
// heuristic's x test passes (else -1), and valid with (ix, iy) where the full
// gather test does.
template <int RES>
__device__ __forceinline__ Val warp_job_pixel(const PairPlan &pp, const RowRec &rr, const Leaf *pool, const Xform *xf,
                                              int i, int row, int &xs, bool &valid, int &ix, int &iy) {
  double sx, sy;
  const bool ok = src_coords<true>(rr, pool, xf, pp.xoff, pp.yoff, pp.w, i, row, sx, sy);
  const bool okx = ok && nn_axis(sx, pp.band_x, ix);
  xs = okx ? ix : -1;
  valid = okx && nn_axis(sy, pp.band_y, iy);
  return ok ? sampled_value<RES>(pp, sx, sy) : pp.fill;
}

// The per-node service's warp batch (warp_batch_launch, host.cpp): for every
// request (job = pair) its window values AND its bytesRead inputs from ONE
// source-coordinate evaluation per pixel -- round 4 ran warp_window_kernel
// and a bytesRead kernel, each deriving the same coordinates again.  The
// window goes straight to the job's destination `outs[job]`: a device staging
// slot, or the requesting worker's shared reply arena (host memory registered
// with HIP, written over PCIe: no read-back copy).  PX pixels per thread
// (consecutive in the packed window): with PX = 4 a thread's values leave in
// one store of 4 * element bytes (wider writes over PCIe).
template <int RES, int PX = 1>
__global__ __launch_bounds__(256) void warp_job_kernel(const PairPlan *pairs, const Xform *xforms,
                                                       const RowRec *rows, const Leaf *pool, int max_h,
                                                       const BlockStatsJob *jobs, char *scratch, int32_t *stats,
                                                       uint8_t *const *outs) {
  const int job = blockIdx.y;
  const PairPlan &pp = pairs[job];
  const BlockStatsJob J = jobs[job];
  int32_t *xsrc = (int32_t *)(scratch + J.xsrc_off);
  uint32_t *bits = (uint32_t *)(scratch + J.bits_off);
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long n = (long)pp.w * pp.h;
  const long p0 = gid * PX;
  int bx = J.bx;
  if (bx <= 0) bx = pp.band_x;
  const int nxb = (pp.band_x + bx - 1) / bx;
  const int dsz = type_size(pp.out_dtype);
  uint8_t *o = outs[job];
  int first = 0x7FFFFFFF, count = 0;
  long long blk[PX];
  Val v[PX];
#pragma unroll
  for (int q = 0; q < PX; q++) {
    blk[q] = -1;
    v[q].u = 0;
    const long p = p0 + q;
    if (p >= n) continue;
    const int row = (int)(p / pp.w), i = (int)(p % pp.w);
    int xs, ix, iy;
    bool valid;
    v[q] = warp_job_pixel<RES>(pp, rows[(int64_t)job * max_h + row], pool, xforms + job, i, row, xs, valid, ix, iy);
    xsrc[p] = xs;
    if (valid) {
      first = min(first, (int)p);
      count++;
      blk[q] = (long long)(ix / bx) + (long long)(iy / J.by) * nxb;
    }
  }
  const int wbytes = PX * dsz;   // the thread's window bytes
  if (PX > 1 && p0 + PX <= n && ((uintptr_t)(o + p0 * dsz) & ((wbytes < 16 ? wbytes : 16) - 1)) == 0) {
    // packed into 32-bit words, stored 4, 8 or 16 bytes at a time
    uint32_t w[PX];
#pragma unroll
    for (int k = 0; k < PX; k++) {
      if (dsz == 1)
        w[k] = k < PX / 4 ? (v[4 * k].u & 0xFFu) | (v[4 * k + 1].u & 0xFFu) << 8 | (v[4 * k + 2].u & 0xFFu) << 16 |
                                v[4 * k + 3].u << 24
                          : 0u;
      else if (dsz == 2)
        w[k] = k < PX / 2 ? (v[2 * k].u & 0xFFFFu) | v[2 * k + 1].u << 16 : 0u;
      else
        w[k] = v[k].u;
    }
    uint8_t *d = o + p0 * dsz;
    if (wbytes == 4) {
      *(uint32_t *)d = w[0];
    } else if (wbytes == 8) {
      *(uint2 *)d = make_uint2(w[0], w[1]);
    } else {
#pragma unroll
      for (int k = 0; k + 3 < PX; k += 4)
        if (4 * k < wbytes) *(uint4 *)(d + 4 * k) = make_uint4(w[k], w[k + 1], w[k + 2], w[k + 3]);
    }
  } else {
#pragma unroll
    for (int q = 0; q < PX; q++) {
      const long p = p0 + q;
      if (p >= n) continue;
      if (dsz == 1) o[p] = (uint8_t)v[q].i;
      else if (dsz == 2) ((uint16_t *)o)[p] = (uint16_t)v[q].i;
      else ((uint32_t *)o)[p] = v[q].u;
    }
  }
  // touched blocks: a pixel ORs its block's bit where it differs from the
  // pixel before it (the previous lane's last pixel for the first)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  long long prev = __shfl_up(blk[PX - 1], 1, 64);
  if (lane == 0) prev = -2;
#pragma unroll
  for (int q = 0; q < PX; q++) {
    if (blk[q] >= 0 && blk[q] != prev) atomicOr(&bits[blk[q] >> 5], 1u << (blk[q] & 31));
    prev = blk[q];
  }
  // first valid pixel and valid count: per wave, then per workgroup
  for (int sft = 32; sft > 0; sft >>= 1) {
    first = min(first, __shfl_xor(first, sft, 64));
    count += __shfl_xor(count, sft, 64);
  }
  __shared__ int s_first[4], s_count[4];
  if (lane == 0) {
    s_first[wave] = first;
    s_count[wave] = count;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int f = s_first[0], c = s_count[0];
    for (int w = 1; w < 4; w++) { f = min(f, s_first[w]); c += s_count[w]; }
    if (c > 0) {
      atomicMin(&stats[4 * job], f);
      atomicAdd(&stats[4 * job + 1], c);
    }
  }
}

// bytesRead (warp.go:281-313: the cache decision at the first valid pixel,
// and 347) and the job's reply record (bbox, dtype, nodata, overview-rescaled
// geotransform): one thread per job.
__global__ void warp_job_resolve_kernel(const PairPlan *pairs, const BlockStatsJob *jobs, const char *scratch,
                                        int32_t *stats_all, int n_jobs, WarpResult *res) {
  const int job = blockIdx.x * blockDim.x + threadIdx.x;
  if (job >= n_jobs) return;
  const PairPlan &pp = pairs[job];
  const BlockStatsJob J = jobs[job];
  const int32_t *xsrc = (const int32_t *)(scratch + J.xsrc_off);
  const uint32_t *bits = (const uint32_t *)(scratch + J.bits_off);
  int32_t *stats = stats_all + 4 * job;
  int bx = J.bx;
  if (bx <= 0) bx = pp.band_x;
  const int i0 = stats[0];
  int32_t br = 0;
  if (i0 != 0x7FFFFFFF) {
    const int r0 = i0 / pp.w, c0 = i0 % pp.w;
    const int prev = xsrc[i0];
    int curr = -1;
    for (int c = c0 + 1; c < pp.w; c++) {
      const int v = xsrc[(long)r0 * pp.w + c];
      if (v >= 0) { curr = v; break; }
    }
    if (curr < prev) curr = prev;
    const int stride = curr - prev;
    const bool cache = stride >= 0 && stride < bx;
    long nread = 0;
    if (cache) {
      for (int k = 0; k < J.n_words; k++) nread += __popc(bits[k]);
    } else {
      nread = stats[1];   // one GDALReadBlock per valid pixel (warp.go:319-322)
    }
    // C int arithmetic of warp.go:347 (wraps like the reference's 32-bit int)
    const long long b = (long long)bx * J.by * type_size(pp.src_dtype) * nread;
    br = (int32_t)(uint32_t)(unsigned long long)b;
  }
  WarpResult &r = res[job];
  r.bbox[0] = pp.xoff; r.bbox[1] = pp.yoff; r.bbox[2] = pp.w; r.bbox[3] = pp.h;
  r.dtype = pp.out_dtype;
  r.bytes_read = br;
  r.nodata = pp.nodata;
  for (int k = 0; k < 6; k++) r.src_gt[k] = pp.src_gt[k];
}

// Source footprint of every planned pair (gskyhip_render_pair_info, an
// observability hook for the algorithmic bytes of a batch): the picked
// level, its element size and the bounding box of the source pixels the
// pair's LINEAR rows and linear leaves sample (first and last pixel of each
// row or leaf: the interpolation is linear along a row), clamped to the
// level.  One thread per pair.
__global__ void pair_footprint_kernel(const PairPlan *pairs, const RowRec *rows, const Leaf *pool, int n_pairs,
                                      int max_h, int32_t *out) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pairs) return;
  const PairPlan &pp = pairs[p];
  double x0 = INFINITY, y0 = INFINITY, x1 = -INFINITY, y1 = -INFINITY;
  auto take = [&](double xs, double ys, double dx, double dy, int n) {
    const double xe = xs + dx * (n - 1), ye = ys + dy * (n - 1);
    x0 = fmin(x0, fmin(xs, xe)); x1 = fmax(x1, fmax(xs, xe));
    y0 = fmin(y0, fmin(ys, ye)); y1 = fmax(y1, fmax(ys, ye));
  };
  for (int r = 0; r < pp.h && pp.w > 0; r++) {
    const RowRec &rr = rows[(int64_t)p * max_h + r];
    if (rr.kind == ROW_LINEAR) {
      take(rr.v[0], rr.v[1], rr.v[2], rr.v[3], pp.w);
    } else if (rr.kind == ROW_POOL) {
      const Leaf *lv = pool + rr.pool_off;
      for (int k = 0; k < rr.nleaf; k++) {
        const Leaf &L = lv[k];
        if (L.kind != LEAF_LINEAR) continue;
        const int end = k + 1 < rr.nleaf ? lv[k + 1].start : pp.w;
        if (end > L.start) take(L.xs0, L.ys0, L.dX, L.dY, end - L.start);
      }
    }
  }
  int32_t *o = out + 8 * p;
  o[0] = pp.granule; o[1] = pp.band_x; o[2] = pp.band_y; o[3] = type_size(pp.src_dtype);
  if (x0 <= x1 && y0 <= y1) {
    o[4] = (int32_t)fmax(0.0, fmin((double)pp.band_x, floor(x0)));
    o[5] = (int32_t)fmax(0.0, fmin((double)pp.band_y, floor(y0)));
    o[6] = (int32_t)fmax(0.0, fmin((double)pp.band_x, floor(x1) + 1.0));
    o[7] = (int32_t)fmax(0.0, fmin((double)pp.band_y, floor(y1) + 1.0));
  } else {
    o[4] = o[5] = o[6] = o[7] = 0;
  }
}

// Source elements and 128-byte lines the pairs of a planned batch touch
// (gskyhip_render_touched: the algorithmic bytes of a batch, SURVEY.md 8(d)
// "unique source bytes touched ... at the chosen overview level"): every
// window pixel of every pair -- data and mask rasters alike, as GDAL reads
// each granule's window -- picks its source element by the nearest-neighbour
// rule of warp.go:271-300 (lin_coords + truncation + bounds); the element and
// its line are set in per-level bitmaps (base[p]: bit offsets of pair p's
// level in the element / line maps).  ROW_LINEAR and ROW_POOL rows (what the
// band kernels render); rows computed exactly at render time are not counted.
// Block = (pair, 4 rows), 256 threads over the window columns.
__global__ void pair_touch_kernel(const PairPlan *pairs, const RowRec *rows, const Leaf *pool, int max_h,
                                  const int64_t *base, uint32_t *ebits, uint32_t *lbits) {
  const int p = blockIdx.x;
  const PairPlan &pp = pairs[p];
  const int64_t eb = base[2 * p], lb = base[2 * p + 1];
  if (eb < 0 || pp.w <= 0) return;
  const int es = type_size(pp.src_dtype);
  for (int r = blockIdx.y * 4; r < min(pp.h, (int)blockIdx.y * 4 + 4); r++) {
    const RowRec &rr = rows[(int64_t)p * max_h + r];
    if (rr.kind != ROW_LINEAR && rr.kind != ROW_POOL) continue;
    for (int ic = threadIdx.x; ic < pp.w; ic += blockDim.x) {
      double sx, sy;
      if (!lin_coords(rr, pool, ic, sx, sy) || sx < 0.0 || sy < 0.0) continue;
      const double ax = sx + 1.0e-10, ay = sy + 1.0e-10;
      if (ax >= (double)pp.band_x || ay >= (double)pp.band_y) continue;
      const int64_t idx = (int64_t)(int)ay * pp.band_x + (int)ax;
      const int64_t e = eb + idx, l = lb + idx * es / 128;
      atomicOr(&ebits[e >> 5], 1u << (e & 31));
      atomicOr(&lbits[l >> 5], 1u << (l & 31));
    }
  }
}

__global__ void popcount_kernel(const uint32_t *bits, int64_t n_words, const int64_t *word_es, int n_seg,
                                unsigned long long *out) {
  // word_es: n_seg x (first word, element bytes) of each level's segment
  unsigned long long acc = 0;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n_words; i += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t w = bits[i];
    if (!w) continue;
    int lo = 0, hi = n_seg - 1;   // the segment holding word i
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (word_es[2 * mid] <= i) lo = mid; else hi = mid - 1;
    }
    acc += (unsigned long long)__popc(w) * (unsigned long long)word_es[2 * lo + 1];
  }
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if ((threadIdx.x & 63) == 0 && acc) atomicAdd(out, acc);
}

__global__ void pair_meta_kernel(const PairPlan *pairs, int n_pairs, int32_t *bbox, int32_t *dtype, double *nodata) {
  int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_pairs) return;
  const PairPlan &pp = pairs[p];
  bbox[4 * p] = pp.xoff; bbox[4 * p + 1] = pp.yoff; bbox[4 * p + 2] = pp.w; bbox[4 * p + 3] = pp.h;
  dtype[p] = pp.out_dtype;
  nodata[p] = pp.nodata;
}

int launch_pair_footprint(void *workspace, int n_tiles, int n_pairs, int max_h, int32_t *out, hipStream_t s) {
  if (n_pairs <= 0) return 0;
  const Carve cv = carve(workspace, n_tiles, n_pairs, max_h);
  hipLaunchKernelGGL(pair_footprint_kernel, dim3((n_pairs + 63) / 64), dim3(64), 0, s, cv.pairs, cv.rows, cv.pool,
                     n_pairs, max_h, out);
  return hipGetLastError() == hipSuccess ? 0 : GSKYHIP_E_HIP;
}

int launch_pair_touched(void *workspace, int n_tiles, int n_pairs, int max_h, int64_t *out2, hipStream_t s) {
  out2[0] = out2[1] = 0;
  if (n_pairs <= 0) return 0;
  const Carve cv = carve(workspace, n_tiles, n_pairs, max_h);
  std::vector<PairPlan> hp(n_pairs);
  if (hipMemcpyAsync(hp.data(), cv.pairs, sizeof(PairPlan) * n_pairs, hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return GSKYHIP_E_HIP;
  // one element map and one line map per distinct level (band pointer), 32-bit aligned segments
  struct Seg { int64_t ebit, lbit; };
  std::map<const void *, Seg> segs;
  std::vector<int64_t> base(2 * (size_t)n_pairs, -1), ew, lw;   // ew / lw: (first word, bytes per bit)
  int64_t ebits = 0, lbits = 0;
  for (int p = 0; p < n_pairs; p++) {
    const PairPlan &pp = hp[p];
    if (!pp.band || pp.w <= 0 || pp.h <= 0 || pp.band_x <= 0 || pp.band_y <= 0) continue;
    auto it = segs.find(pp.band);
    if (it == segs.end()) {
      const int es = type_size(pp.src_dtype);
      const int64_t n = (int64_t)pp.band_x * pp.band_y, nl = (n * es + 127) / 128;
      ew.push_back(ebits / 32); ew.push_back(es);
      lw.push_back(lbits / 32); lw.push_back(128);
      it = segs.emplace(pp.band, Seg{ebits, lbits}).first;
      ebits += (n + 31) / 32 * 32;
      lbits += (nl + 31) / 32 * 32;
    }
    base[2 * p] = it->second.ebit;
    base[2 * p + 1] = it->second.lbit;
  }
  if (segs.empty()) return 0;
  const int64_t ew_words = ebits / 32, lw_words = lbits / 32;
  // (+ 8: the word that aligns dbase when the two maps hold an odd number of words)
  const size_t bytes = (size_t)(ew_words + lw_words) * 4 + 8 + base.size() * 8 + (ew.size() + lw.size()) * 8 + 16;
  char *dev = nullptr;
  if (hipMalloc((void **)&dev, bytes) != hipSuccess) return GSKYHIP_E_HIP;
  uint32_t *eb = (uint32_t *)dev, *lb = eb + ew_words;
  int64_t *dbase = (int64_t *)(lb + lw_words + ((ew_words + lw_words) & 1));
  int64_t *dew = dbase + base.size(), *dlw = dew + ew.size();
  unsigned long long *cnt = (unsigned long long *)(dlw + lw.size());
  int rc = 0;
  if (hipMemsetAsync(dev, 0, (size_t)(ew_words + lw_words) * 4, s) != hipSuccess ||
      hipMemsetAsync(cnt, 0, 16, s) != hipSuccess ||
      hipMemcpyAsync(dbase, base.data(), base.size() * 8, hipMemcpyHostToDevice, s) != hipSuccess ||
      hipMemcpyAsync(dew, ew.data(), ew.size() * 8, hipMemcpyHostToDevice, s) != hipSuccess ||
      hipMemcpyAsync(dlw, lw.data(), lw.size() * 8, hipMemcpyHostToDevice, s) != hipSuccess)
    rc = GSKYHIP_E_HIP;
  if (!rc) {
    hipLaunchKernelGGL(pair_touch_kernel, dim3((unsigned)n_pairs, (unsigned)((max_h + 3) / 4)), dim3(256), 0, s,
                       cv.pairs, cv.rows, cv.pool, max_h, dbase, eb, lb);
    hipLaunchKernelGGL(popcount_kernel, dim3(1024), dim3(256), 0, s, eb, ew_words, dew, (int)(ew.size() / 2), cnt);
    hipLaunchKernelGGL(popcount_kernel, dim3(1024), dim3(256), 0, s, lb, lw_words, dlw, (int)(lw.size() / 2), cnt + 1);
    unsigned long long h[2] = {0, 0};
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(h, cnt, 16, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
      rc = GSKYHIP_E_HIP;
    out2[0] = (int64_t)h[0];
    out2[1] = (int64_t)h[1];
  }
  (void)hipFree(dev);
  return rc;
}

int launch_warp_jobs(const RenderCall &rc, const BlockStatsJob *jobs, int64_t max_px, void *scratch,
                     int32_t *stats, uint8_t *const *outs, WarpResult *results) {
  if (rc.resample != GSKYHIP_RESAMPLE_NEAREST) return GSKYHIP_E_ARG;   // the service warps nearest only
  Carve cv;
  int rcode = plan_all(rc, cv);
  if (rcode || rc.n_pairs <= 0) return rcode;
  hipStream_t s = rc.stream;
  const int n = rc.n_pairs;
  hipLaunchKernelGGL(block_stats_init_kernel, dim3(n), dim3(256), 0, s, jobs, (char *)scratch, stats);
  if (max_px > 0) {
    // eight pixels per thread, 8-32 bytes in one or two stores (service leg,
    // 16 / 64 workers: 1 px 32.3k / 48.4k req/s, 4 px 42.1-43.4k / 61.3-66.2k,
    // 8 px 44.8k / 62.7-63.4k; profiles/r05f_svc.txt, r05g_svc.txt);
    // GSKYHIP_SVC_PX=1/4 selects the others
    static const int env_px = [] {
      const char *e = getenv("GSKYHIP_SVC_PX");
      const int v = e ? atoi(e) : 8;
      return v == 1 || v == 4 ? v : 8;
    }();
    const int px = env_px;
    const dim3 grid((unsigned)((max_px + 256 * px - 1) / (256 * px)), n);
    auto launch = [&](auto px_c) {
      hipLaunchKernelGGL((warp_job_kernel<GSKYHIP_RESAMPLE_NEAREST, decltype(px_c)::value>), grid, dim3(256), 0, s,
                         cv.pairs, cv.xforms, cv.rows, cv.pool, rc.max_h, jobs, (char *)scratch, stats, outs);
    };
    if (px == 4) launch(std::integral_constant<int, 4>{});
    else if (px == 8) launch(std::integral_constant<int, 8>{});
    else launch(std::integral_constant<int, 1>{});
  }
  hipLaunchKernelGGL(warp_job_resolve_kernel, dim3((n + 63) / 64), dim3(64), 0, s, cv.pairs, jobs,
                     (const char *)scratch, stats, n, results);
  return hipGetLastError() == hipSuccess ? 0 : GSKYHIP_E_HIP;
}

int launch_warp_windows(const RenderCall &rc, int32_t *bbox_out, int32_t *dtype_out, double *nodata_out,
                        void *win_out, int64_t win_stride) {
  if (rc.resample < GSKYHIP_RESAMPLE_NEAREST || rc.resample > GSKYHIP_RESAMPLE_LANCZOS) return GSKYHIP_E_ARG;
  Carve cv;
  int rcode = plan_all(rc, cv);
  if (rcode || rc.n_pairs <= 0) return rcode;
  hipStream_t s = rc.stream;
  hipLaunchKernelGGL(pair_meta_kernel, dim3((rc.n_pairs + 255) / 256), dim3(256), 0, s, cv.pairs, rc.n_pairs,
                     bbox_out, dtype_out, nodata_out);
  const int64_t nthreads = (int64_t)rc.n_pairs * rc.max_h * rc.max_w;
  const dim3 grid((unsigned)((nthreads + 255) / 256));
  const bool known = with_resample(rc.resample, [&](auto res) {
    hipLaunchKernelGGL(warp_window_kernel<decltype(res)::value>, grid, dim3(256), 0, s, cv.pairs, cv.xforms, cv.rows,
                       cv.pool, rc.max_h, rc.max_w, rc.n_pairs, (uint8_t *)win_out, (long)win_stride);
  });
  if (!known) return GSKYHIP_E_ARG;
  return hipGetLastError() == hipSuccess ? 0 : GSKYHIP_E_HIP;
}

}  // namespace gsky
