// deflate.hip -- independent blocks deflated on the GPU, the
// same encoder on host threads, and the block preparation and packing of its
// two coverage writers around it: the netCDF writer's chunks (shuffle) and
// the GeoTIFF writer's tiles (edge padding and the TIFF predictor).
//
// The encoder is deflate_core.h, compiled for both sides.  On the device:
//   * deflate_tokenize_kernel, a wave per 64 segments of a block, a lane per
//     segment of kSeg bytes: the segment's tokens (one dword each) into the
//     workspace, the lane's 3-byte hash table in LDS (lane-interleaved, so a
//     wave's accesses fall into different banks), the symbol counts into an
//     LDS histogram that is added to the block's histogram in the workspace.
//   * deflate_write_kernel, a wave per block: lane 0 builds the block's plan
//     (dynamic code, fixed code or stored blocks, whichever stream is the
//     shortest) in LDS; the wave sums Adler-32; the stream length is now
//     exact, so a block that does not fit its capacity ends here with
//     GSKYHIP_INFLATE_E_CAP and nothing written.  Stored streams are written
//     byte by byte straight into the output.  Huffman-coded streams are built
//     in a zeroed, word-aligned staging area of the workspace -- 64 segments
//     at a time: their bit counts, a wave scan for the bit offsets, the codes
//     (shared words by atomicOr) -- and then copied to the output, which may
//     start at any byte.
// Every segment reads only its block's input, writes at most kSeg tokens into
// its own kSeg dwords, and the staging area of a block holds stage_words(n)
// words, more than any stream the plan can choose (the stored stream bounds
// the others).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

#include "../../include/gskyhip.h"
#include "deflate.h"
#include "deflate_core.h"
#include "tiffwrite.h"

namespace gsky {
namespace {

namespace gd = deflate;

constexpr int64_t kMaxBlockLen = 1ll << 30;

static_assert(gd::kOk == GSKYHIP_INFLATE_OK && gd::kOutputFull == GSKYHIP_INFLATE_E_CAP,
              "status codes of the header and of the core");

struct BlockDesc {
  int64_t in_off, in_len, out_off, out_cap;
  int64_t tok_off;     // dwords: the sum of the lengths before
  int64_t seg_off;     // segments before
  int64_t stage_off;   // words
  int64_t pad;
};

struct Layout {   // byte offsets into the workspace, from (n_blocks, total input) alone
  int64_t desc, status, out_len, freq, grp, ntok, tok, stage, end;
};

int64_t al16(int64_t v) { return (v + 15) & ~(int64_t)15; }

Layout layout_of(int64_t n, int64_t total) {
  const int64_t segs = total / gd::kSeg + n, groups = total / (64 * gd::kSeg) + n;
  const int64_t stage_words = (total + 5 * (total / 65535) + 11 * n) / 4 + 2 * n + 1;
  Layout L;
  L.desc = 0;
  L.status = al16(L.desc + n * (int64_t)sizeof(BlockDesc));
  L.out_len = al16(L.status + n * 4);
  L.freq = al16(L.out_len + n * 8);
  L.grp = al16(L.freq + n * gd::kSymN * 4);
  L.ntok = al16(L.grp + groups * 8);
  L.tok = al16(L.ntok + segs * 2);
  L.stage = al16(L.tok + total * 4);
  L.end = al16(L.stage + stage_words * 4);
  return L;
}

__device__ inline uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off);
  return v;
}

// grp[2 g] = block of group g, grp[2 g + 1] = its first segment in the block
__global__ __launch_bounds__(64) void deflate_tokenize_kernel(const uint8_t *__restrict__ in,
                                                              const BlockDesc *__restrict__ desc,
                                                              const int32_t *__restrict__ grp, int n_groups,
                                                              uint32_t *__restrict__ tok, uint16_t *__restrict__ ntok,
                                                              uint32_t *__restrict__ freq) {
  __shared__ uint32_t s_freq[gd::kSymN];
  __shared__ uint16_t s_hash[gd::kHashN * 64];
  const int g = blockIdx.x, lane = threadIdx.x;
  if (g >= n_groups) return;
  const int b = grp[2 * g];
  const BlockDesc d = desc[b];
  const int64_t seg = (int64_t)grp[2 * g + 1] + lane;
  for (int i = lane; i < gd::kSymN; i += 64) s_freq[i] = 0;
  __syncthreads();
  const int64_t p0 = seg * gd::kSeg;
  if (p0 < d.in_len) {
    const int64_t p1 = p0 + gd::kSeg < d.in_len ? p0 + gd::kSeg : d.in_len;
    const int n = gd::tokenize_segment(in + d.in_off, p0, p1, tok + d.tok_off + p0, s_hash + lane, 64,
                                       [&](int sym) { atomicAdd(&s_freq[sym], 1u); });
    ntok[d.seg_off + seg] = (uint16_t)n;
  }
  __syncthreads();
  for (int i = lane; i < gd::kSymN; i += 64)
    if (s_freq[i]) atomicAdd(&freq[(int64_t)b * gd::kSymN + i], s_freq[i]);
}

__global__ __launch_bounds__(64) void deflate_write_kernel(const uint8_t *__restrict__ in,
                                                           const BlockDesc *__restrict__ desc, int n_blocks,
                                                           const uint32_t *__restrict__ tok,
                                                           const uint16_t *__restrict__ ntok,
                                                           const uint32_t *__restrict__ freq, uint32_t *stage,
                                                           uint8_t *out, int zlib_wrapper, int level,
                                                           int32_t *__restrict__ status, int64_t *__restrict__ out_len) {
  __shared__ uint32_t s_freq[gd::kSymN];
  __shared__ gd::Plan P;
  __shared__ gd::PlanScratch S;
  const int b = blockIdx.x, lane = threadIdx.x;
  if (b >= n_blocks) return;
  const BlockDesc d = desc[b];
  const uint8_t *src = in + d.in_off;
  const int64_t n = d.in_len;
  for (int i = lane; i < gd::kSymN; i += 64) s_freq[i] = freq[(int64_t)b * gd::kSymN + i];
  __syncthreads();
  if (lane == 0) gd::plan_block(s_freq, n, zlib_wrapper, level, P, S);
  __syncthreads();
  uint32_t adler = 1;
  if (zlib_wrapper) {
    uint32_t a = 1, bsum = 0;
    constexpr uint32_t kPiece = 4096;   // sum of (L - i) * 255 over a piece stays below 2^32
    for (int64_t base = 0; base < n; base += kPiece) {
      const uint32_t L = (uint32_t)(n - base < kPiece ? n - base : kPiece);
      uint32_t sa = 0, sb = 0;
      for (uint32_t i = (uint32_t)lane; i < L; i += 64u) {
        const uint32_t v = src[base + i];
        sa += v;
        sb += (L - i) * v;
      }
      sa = wave_sum(sa);
      sb = wave_sum(sb);
      bsum = (uint32_t)(((uint64_t)bsum + (uint64_t)L * a + sb) % gd::kAdlerMod);
      a = (a + sa) % gd::kAdlerMod;
    }
    adler = (bsum << 16) | a;
  }
  const int64_t total = P.stream_bytes;
  const bool fits = total <= d.out_cap;
  if (lane == 0) {
    status[b] = fits ? GSKYHIP_INFLATE_OK : GSKYHIP_INFLATE_E_CAP;
    out_len[b] = total;
  }
  if (!fits) return;
  uint8_t *dst = out + d.out_off;
  if (P.mode == gd::kStored) {
    for (int64_t j = lane; j < total; j += 64) dst[j] = gd::stored_byte(j, src, n, zlib_wrapper, adler);
    return;
  }
  uint32_t *words = stage + d.stage_off;
  const int64_t nw = (total + 3) / 4;
  for (int64_t i = lane; i < nw; i += 64) words[i] = 0;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  __syncthreads();
  if (lane == 0) gd::write_frame(P, zlib_wrapper, gd::kFlgDefault, adler, words);
  const int64_t nseg = (n + gd::kSeg - 1) / gd::kSeg;
  int64_t running = (zlib_wrapper ? 16 : 0) + P.hdr_bits;
  for (int64_t s0 = 0; s0 < nseg; s0 += 64) {
    const int64_t seg = s0 + lane;
    const bool live = seg < nseg;
    const uint32_t *tk = tok + d.tok_off + seg * gd::kSeg;
    const int nt = live ? (int)ntok[d.seg_off + seg] : 0;
    const uint32_t bits = live ? gd::segment_bits(tk, nt, P.len) : 0u;
    uint32_t incl = bits;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t up = (uint32_t)__shfl_up((int)incl, off);
      if (lane >= off) incl += up;
    }
    if (live) gd::write_segment(tk, nt, P.code, P.len, words, running + incl - bits);
    running += (uint32_t)__shfl((int)incl, 63);
  }
  // the words were completed by atomics of other lanes: publish, then read past the vector cache
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  __syncthreads();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  const uint8_t *sb = (const uint8_t *)words;
  for (int64_t j = lane; j < total; j += 64) dst[j] = sb[j];
}

bool args_ok(const int64_t *in_off, const int64_t *in_len, int n, const int64_t *out_off, const int64_t *out_cap) {
  for (int k = 0; k < n; k++)
    if (in_off[k] < 0 || in_len[k] < 0 || in_len[k] > kMaxBlockLen || out_off[k] < 0 || out_cap[k] < 0) return false;
  return true;
}

// The two kernels over blocks described by host arrays; status / out_len stay
// in the workspace (at layout_of(n, total).status / .out_len).
int deflate_launch(const uint8_t *dev_in, const int64_t *in_off, const int64_t *in_len, int n, uint8_t *dev_out,
                   const int64_t *out_off, const int64_t *out_cap, int zlib_wrapper, int level, uint8_t *ws,
                   int64_t ws_bytes, hipStream_t s, std::vector<uint8_t> &host_buf, Layout &L) {
  int64_t total = 0;
  for (int k = 0; k < n; k++) total += in_len[k];
  L = layout_of(n, total);
  if (!ws || ws_bytes < L.end) return GSKYHIP_E_ARG;
  // desc and the group map in one upload (host_buf must outlive the copy)
  std::vector<int32_t> grp;
  host_buf.assign((size_t)(n * sizeof(BlockDesc)), 0);
  BlockDesc *desc = (BlockDesc *)host_buf.data();
  int64_t tok_off = 0, seg_off = 0, stage_off = 0;
  for (int k = 0; k < n; k++) {
    const int64_t nseg = (in_len[k] + gd::kSeg - 1) / gd::kSeg;
    desc[k] = {in_off[k], in_len[k], out_off[k], out_cap[k], tok_off, seg_off, stage_off, 0};
    for (int64_t s0 = 0; s0 < nseg; s0 += 64) {
      grp.push_back(k);
      grp.push_back((int32_t)s0);
    }
    tok_off += in_len[k];
    seg_off += nseg;
    stage_off += gd::stage_words(in_len[k]);
  }
  const int n_groups = (int)(grp.size() / 2);
  const size_t desc_bytes = host_buf.size();
  host_buf.resize(desc_bytes + grp.size() * 4);
  if (!grp.empty()) std::memcpy(host_buf.data() + desc_bytes, grp.data(), grp.size() * 4);
  if (hipMemcpyAsync(ws + L.desc, host_buf.data(), desc_bytes, hipMemcpyHostToDevice, s) != hipSuccess)
    return GSKYHIP_E_HIP;
  if (n_groups > 0 && hipMemcpyAsync(ws + L.grp, host_buf.data() + desc_bytes, grp.size() * 4, hipMemcpyHostToDevice,
                                     s) != hipSuccess)
    return GSKYHIP_E_HIP;
  if (hipMemsetAsync(ws + L.freq, 0, (size_t)n * gd::kSymN * 4, s) != hipSuccess) return GSKYHIP_E_HIP;
  if (n_groups > 0 && level != 0)
    hipLaunchKernelGGL(deflate_tokenize_kernel, dim3((unsigned)n_groups), dim3(64), 0, s, dev_in,
                       (const BlockDesc *)(ws + L.desc), (const int32_t *)(ws + L.grp), n_groups,
                       (uint32_t *)(ws + L.tok), (uint16_t *)(ws + L.ntok), (uint32_t *)(ws + L.freq));
  hipLaunchKernelGGL(deflate_write_kernel, dim3((unsigned)n), dim3(64), 0, s, dev_in, (const BlockDesc *)(ws + L.desc),
                     n, (const uint32_t *)(ws + L.tok), (const uint16_t *)(ws + L.ntok),
                     (const uint32_t *)(ws + L.freq), (uint32_t *)(ws + L.stage), dev_out, zlib_wrapper ? 1 : 0, level,
                     (int32_t *)(ws + L.status), (int64_t *)(ws + L.out_len));
  return hipGetLastError() == hipSuccess ? GSKYHIP_OK : GSKYHIP_E_HIP;
}

// ---------------------------------------------------------------- netCDF chunks
// File rows [j0, j0 + rows) of a band as shuffled chunks: byte b of element e
// of file row j at chunks[(j - j0) * width * ES + b * width + e].
template <int SS, int ES>
__global__ __launch_bounds__(256) void nc_shuffle_kernel(const uint8_t *__restrict__ band, int width, int height,
                                                         int j0, int rows, uint8_t *__restrict__ chunks) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)rows * width) return;
  const int r = (int)(idx / width), e = (int)(idx % width);
  const int64_t src = ((int64_t)(height - 1 - (j0 + r)) * width + e) * SS;
  uint32_t v = 0;
#pragma unroll
  for (int q = 0; q < SS; q++) v |= (uint32_t)band[src + q] << (8 * q);   // UInt16 -> int32: zero extension
  uint8_t *dst = chunks + (int64_t)r * width * ES + e;
#pragma unroll
  for (int q = 0; q < ES; q++) dst[(int64_t)q * width] = (uint8_t)(v >> (8 * q));
}

// off[k] = the sum of len[i], i < k (k <= n): one workgroup
__global__ __launch_bounds__(256) void nc_pack_scan_kernel(const int64_t *__restrict__ len, int n,
                                                           int64_t *__restrict__ off) {
  __shared__ int64_t s_part[256];
  const int tid = threadIdx.x;
  const int per = (n + 255) / 256;
  const int k0 = tid * per, k1 = min(n, k0 + per);
  int64_t sum = 0;
  for (int k = k0; k < k1; k++) sum += len[k];
  s_part[tid] = sum;
  __syncthreads();
  int64_t at = 0;
  for (int t = 0; t < tid; t++) at += s_part[t];
  for (int k = k0; k < k1; k++) { off[k] = at; at += len[k]; }
  if (tid == 255) off[n] = at;
}

__global__ __launch_bounds__(64) void nc_pack_copy_kernel(const uint8_t *__restrict__ z, int64_t zstride,
                                                          const int64_t *__restrict__ len,
                                                          const int64_t *__restrict__ off, int n,
                                                          uint8_t *__restrict__ packed) {
  const int k = blockIdx.x;
  if (k >= n) return;
  const uint8_t *src = z + (int64_t)k * zstride;
  uint8_t *dst = packed + off[k];
  const int64_t L = len[k];
  for (int64_t j = threadIdx.x; j < L; j += 64) dst[j] = src[j];
}

// ---------------------------------------------------------------- GeoTIFF tiles
template <int SS> struct SampleOf;
template <> struct SampleOf<1> { typedef uint8_t type; };
template <> struct SampleOf<2> { typedef uint16_t type; };
template <> struct SampleOf<4> { typedef uint32_t type; };

// the bits of sample (gx, gy) of the band, `pad` outside the image (or without a band)
template <int SS>
__device__ __forceinline__ uint32_t tiff_sample_at(const uint8_t *__restrict__ band, int width, int height, int gx,
                                                   int gy, uint32_t pad) {
  typedef typename SampleOf<SS>::type T;
  if (!band || gx >= width || gy >= height) return pad;
  return (uint32_t)((const T *)band)[(int64_t)gy * width + gx];
}

// Tiles [tile0, tile0 + gridDim.y) of a band (row-major over ntx columns of
// tiles) as the compressor receives them, tile k at dst + k * tile_bytes:
// block_y rows of block_x samples of SS bytes, edge tiles padded, the TIFF
// predictor PRED applied.  PRED 1, 2: a thread per sample (2: its difference
// to the left neighbour in the tile row, wrapping in the sample width; the
// first kept).  PRED 3 (SS = 4): a thread per output byte i = p * block_x + x
// of a row -- byte 3 - p of sample x (the planes most significant first)
// minus the byte before it in the row, which at x = 0 is the last column of
// plane p - 1; byte 0 is kept.  Reads are coalesced along x, writes are
// consecutive.  `items` = threads a tile needs (< 2^31).
template <int SS, int PRED>
__global__ __launch_bounds__(256) void tiff_tile_predict_kernel(const uint8_t *__restrict__ band, int width,
                                                                int height, int block_x, int block_y, int ntx,
                                                                int64_t tile0, uint32_t items, uint32_t pad,
                                                                uint8_t *__restrict__ dst) {
  typedef typename SampleOf<SS>::type T;
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= items) return;
  const int64_t tile = tile0 + blockIdx.y;
  const int tx = (int)(tile % ntx), ty = (int)(tile / ntx);
  const int64_t tile_bytes = (int64_t)block_x * block_y * SS;
  uint8_t *out = dst + (int64_t)blockIdx.y * tile_bytes;
  if (PRED == 3) {
    const uint32_t row_bytes = 4u * (uint32_t)block_x;
    const uint32_t r = i / row_bytes, c = i - r * row_bytes;
    const uint32_t p = c / (uint32_t)block_x, x = c - p * (uint32_t)block_x;
    const int gy = ty * block_y + (int)r, gx0 = tx * block_x;
    const uint32_t cur = (tiff_sample_at<SS>(band, width, height, gx0 + (int)x, gy, pad) >> (8 * (3 - p))) & 0xFFu;
    uint32_t prev = 0;
    if (x > 0) prev = (tiff_sample_at<SS>(band, width, height, gx0 + (int)x - 1, gy, pad) >> (8 * (3 - p))) & 0xFFu;
    else if (p > 0) prev = (tiff_sample_at<SS>(band, width, height, gx0 + block_x - 1, gy, pad) >> (8 * (4 - p))) & 0xFFu;
    out[i] = (uint8_t)(cur - prev);
  } else {
    const uint32_t r = i / (uint32_t)block_x, x = i - r * (uint32_t)block_x;
    const int gy = ty * block_y + (int)r, gx = tx * block_x + (int)x;
    uint32_t v = tiff_sample_at<SS>(band, width, height, gx, gy, pad);
    if (PRED == 2 && x > 0) v -= tiff_sample_at<SS>(band, width, height, gx - 1, gy, pad);
    ((T *)out)[i] = (T)v;
  }
}

struct NcLayout {
  int64_t chunks, z, off, packed, dws, end, zstride;
};

NcLayout nc_layout(int64_t row_bytes, int rows) {
  NcLayout N;
  N.zstride = (gd::bound(row_bytes) + 7) & ~(int64_t)7;
  N.chunks = 0;
  N.z = al16(N.chunks + row_bytes * rows);
  N.off = al16(N.z + N.zstride * rows);
  N.packed = al16(N.off + 8 * ((int64_t)rows + 1));
  N.dws = al16(N.packed + N.zstride * rows);
  N.end = N.dws + layout_of(rows, row_bytes * rows).end;
  return N;
}

// The n blocks of block_bytes each at ws + N.chunks (N = nc_layout(block_bytes,
// n)) deflated into zlib streams and packed end to end at ws + N.packed:
// lens[k] = the length of stream k, *total their sum.  Two small copies
// (lengths, statuses) and a synchronise; a block whose status is not OK fails
// the slab.
int deflate_pack_slab(const NcLayout &N, int64_t block_bytes, int n, int level, uint8_t *ws, int64_t ws_bytes,
                      int64_t *lens, int64_t *total, hipStream_t s) {
  std::vector<int64_t> in_off((size_t)n), in_len((size_t)n, block_bytes), out_off((size_t)n),
      out_cap((size_t)n, N.zstride);
  for (int k = 0; k < n; k++) {
    in_off[k] = (int64_t)k * block_bytes;
    out_off[k] = (int64_t)k * N.zstride;
  }
  std::vector<uint8_t> host_buf;
  Layout L;
  int rc = deflate_launch(ws + N.chunks, in_off.data(), in_len.data(), n, ws + N.z, out_off.data(), out_cap.data(), 1,
                          level, ws + N.dws, ws_bytes - N.dws, s, host_buf, L);
  const int64_t *d_len = (const int64_t *)(ws + N.dws + L.out_len);
  int64_t *d_off = (int64_t *)(ws + N.off);
  if (!rc) {
    hipLaunchKernelGGL(nc_pack_scan_kernel, dim3(1), dim3(256), 0, s, d_len, n, d_off);
    hipLaunchKernelGGL(nc_pack_copy_kernel, dim3((unsigned)n), dim3(64), 0, s, ws + N.z, N.zstride, d_len, d_off, n,
                       ws + N.packed);
    if (hipGetLastError() != hipSuccess) rc = GSKYHIP_E_HIP;
  }
  std::vector<int32_t> st((size_t)n);
  if (!rc && (hipMemcpyAsync(lens, d_len, 8 * (size_t)n, hipMemcpyDeviceToHost, s) != hipSuccess ||
              hipMemcpyAsync(st.data(), ws + N.dws + L.status, 4 * (size_t)n, hipMemcpyDeviceToHost, s) != hipSuccess))
    rc = GSKYHIP_E_HIP;
  if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = GSKYHIP_E_HIP;   // host_buf must outlive its upload
  if (rc) return rc;
  *total = 0;
  for (int k = 0; k < n; k++) {
    if (st[k] != GSKYHIP_INFLATE_OK || lens[k] <= 0 || lens[k] > N.zstride) return GSKYHIP_E_HIP;
    *total += lens[k];
  }
  return GSKYHIP_OK;
}

}  // namespace

int tiff_slab_tiles(int64_t tile_bytes, int64_t tiles_per_band, int slab_tiles) {
  int64_t t = slab_tiles > 0 ? slab_tiles : std::max<int64_t>(1, tiff::kSlabRawBytes / std::max<int64_t>(1, tile_bytes));
  t = std::min<int64_t>(t, tiff::kSlabMaxTiles);
  return (int)std::min<int64_t>(t, tiles_per_band);
}

int64_t tiff_deflate_workspace(int64_t tile_bytes, int tiles) { return nc_layout(tile_bytes, tiles).end; }

int tiff_deflate_slab(const void *dev_band, int ts, int predictor, int width, int height, int block_x, int block_y,
                      int ntx, int64_t tile0, int tiles, uint32_t pad, int level, uint8_t *ws, int64_t ws_bytes,
                      uint8_t *dst, int64_t dst_cap, int64_t *lens, int64_t *copied, hipStream_t s) {
  const int64_t tile_bytes = (int64_t)block_x * block_y * ts;
  if (width <= 0 || height <= 0 || block_x <= 0 || block_y <= 0 || ntx <= 0 || tile0 < 0 || tiles <= 0 ||
      tiles > tiff::kSlabMaxTiles || tile_bytes > tiff::kMaxTileBytes || !dst || !lens)
    return GSKYHIP_E_ARG;
  const int64_t nty = ((int64_t)height + block_y - 1) / block_y;
  // the tiles lie in the band's grid, and pixel coordinates of padded tiles stay below 2^31
  if ((int64_t)ntx * block_x > INT32_MAX || nty * block_y > INT32_MAX || tile0 + tiles > ntx * nty)
    return GSKYHIP_E_ARG;
  const NcLayout N = nc_layout(tile_bytes, tiles);
  if (!ws || ws_bytes < N.end) return GSKYHIP_E_ARG;
  const uint32_t items = (uint32_t)(predictor == 3 ? tile_bytes : tile_bytes / ts);
  const dim3 grid((items + 255u) / 256u, (unsigned)tiles);
  const uint8_t *band = (const uint8_t *)dev_band;
  uint8_t *raw = ws + N.chunks;
#define GSKY_TIFF_PREDICT(SS, PRED)                                                                             \
  hipLaunchKernelGGL((tiff_tile_predict_kernel<SS, PRED>), grid, dim3(256), 0, s, band, width, height, block_x, \
                     block_y, ntx, tile0, items, pad, raw)
  if (predictor == 3 && ts == 4) GSKY_TIFF_PREDICT(4, 3);
  else if (predictor == 2 && ts == 4) GSKY_TIFF_PREDICT(4, 2);
  else if (predictor == 2 && ts == 2) GSKY_TIFF_PREDICT(2, 2);
  else if (predictor == 2 && ts == 1) GSKY_TIFF_PREDICT(1, 2);
  else if (predictor == 1 && ts == 4) GSKY_TIFF_PREDICT(4, 1);
  else if (predictor == 1 && ts == 2) GSKY_TIFF_PREDICT(2, 1);
  else if (predictor == 1 && ts == 1) GSKY_TIFF_PREDICT(1, 1);
  else return GSKYHIP_E_ARG;
#undef GSKY_TIFF_PREDICT
  if (hipGetLastError() != hipSuccess) return GSKYHIP_E_HIP;
  int64_t total = 0;
  const int rc = deflate_pack_slab(N, tile_bytes, tiles, level, ws, ws_bytes, lens, &total, s);
  if (rc) return rc;
  if (total > dst_cap) return GSKYHIP_E_ARG;
  if (hipMemcpyAsync(dst, ws + N.packed, (size_t)total, hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return GSKYHIP_E_HIP;
  if (copied) *copied += total;
  return GSKYHIP_OK;
}

int nc_slab_rows(int64_t row_bytes, int height, int slab_rows) {
  int64_t r = slab_rows > 0 ? slab_rows : std::max<int64_t>(1, kNcSlabRawBytes / std::max<int64_t>(1, row_bytes));
  r = std::min<int64_t>(r, kNcSlabMaxRows);
  return (int)std::min<int64_t>(r, height);
}

int64_t nc_deflate_workspace(int64_t row_bytes, int rows) { return nc_layout(row_bytes, rows).end; }

int nc_deflate_slab(const void *dev_band, int src_size, int elem_size, int width, int height, int j0, int rows,
                    int level, uint8_t *ws, int64_t ws_bytes, std::vector<std::vector<uint8_t>> &z, int64_t *copied,
                    hipStream_t s) {
  const int64_t row_bytes = (int64_t)width * elem_size;
  const NcLayout N = nc_layout(row_bytes, rows);
  if (!ws || ws_bytes < N.end || j0 < 0 || rows <= 0 || j0 + rows > height || row_bytes > kMaxBlockLen)
    return GSKYHIP_E_ARG;
  const int64_t items = (int64_t)rows * width;
  const dim3 grid((unsigned)((items + 255) / 256));
  const uint8_t *band = (const uint8_t *)dev_band;
  uint8_t *chunks = ws + N.chunks;
  if (src_size == 1 && elem_size == 1)
    hipLaunchKernelGGL((nc_shuffle_kernel<1, 1>), grid, dim3(256), 0, s, band, width, height, j0, rows, chunks);
  else if (src_size == 2 && elem_size == 2)
    hipLaunchKernelGGL((nc_shuffle_kernel<2, 2>), grid, dim3(256), 0, s, band, width, height, j0, rows, chunks);
  else if (src_size == 2 && elem_size == 4)
    hipLaunchKernelGGL((nc_shuffle_kernel<2, 4>), grid, dim3(256), 0, s, band, width, height, j0, rows, chunks);
  else if (src_size == 4 && elem_size == 4)
    hipLaunchKernelGGL((nc_shuffle_kernel<4, 4>), grid, dim3(256), 0, s, band, width, height, j0, rows, chunks);
  else
    return GSKYHIP_E_ARG;
  if (hipGetLastError() != hipSuccess) return GSKYHIP_E_HIP;
  std::vector<int64_t> lens((size_t)rows);
  int64_t total = 0;
  const int rc = deflate_pack_slab(N, row_bytes, rows, level, ws, ws_bytes, lens.data(), &total, s);
  if (rc) return rc;
  std::vector<uint8_t> packed((size_t)total);
  if (hipMemcpyAsync(packed.data(), ws + N.packed, (size_t)total, hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return GSKYHIP_E_HIP;
  int64_t at = 0;
  for (int k = 0; k < rows; k++) {
    z[(size_t)(j0 + k)].assign(packed.begin() + at, packed.begin() + at + lens[k]);
    at += lens[k];
  }
  if (copied) *copied += total;
  return GSKYHIP_OK;
}

}  // namespace gsky

using namespace gsky;

extern "C" int64_t gskyhip_deflate_bound(int64_t in_len) { return in_len < 0 ? -1 : deflate::bound(in_len); }

extern "C" int64_t gskyhip_deflate_workspace_size(int n_blocks, int64_t total_in_len) {
  if (n_blocks < 0 || total_in_len < 0) return -1;
  return layout_of(n_blocks, total_in_len).end;
}

static int deflate_blocks_impl(const uint8_t *dev_in, const int64_t *in_off, const int64_t *in_len, int n_blocks,
                               uint8_t *dev_out, const int64_t *out_off, const int64_t *out_cap, int zlib_wrapper,
                               int level, void *workspace, int64_t workspace_bytes, int32_t *status, int64_t *out_len,
                               void *stream) {
  if (n_blocks < 0 || level < 0 || level > 9) return GSKYHIP_E_ARG;
  if (n_blocks == 0) return GSKYHIP_OK;
  if (!dev_in || !dev_out || !in_off || !in_len || !out_off || !out_cap || !status || !out_len || !workspace)
    return GSKYHIP_E_ARG;
  if (!args_ok(in_off, in_len, n_blocks, out_off, out_cap)) return GSKYHIP_E_ARG;
  hipStream_t s = (hipStream_t)stream;
  uint8_t *ws = (uint8_t *)workspace;
  std::vector<uint8_t> host_buf;
  Layout L;
  int rc = deflate_launch(dev_in, in_off, in_len, n_blocks, dev_out, out_off, out_cap, zlib_wrapper, level, ws,
                          workspace_bytes, s, host_buf, L);
  if (rc == GSKYHIP_E_ARG) return rc;   // nothing was enqueued
  if (!rc && (hipMemcpyAsync(out_len, ws + L.out_len, 8 * (size_t)n_blocks, hipMemcpyDeviceToHost, s) != hipSuccess ||
              hipMemcpyAsync(status, ws + L.status, 4 * (size_t)n_blocks, hipMemcpyDeviceToHost, s) != hipSuccess))
    rc = GSKYHIP_E_HIP;
  if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = GSKYHIP_E_HIP;   // host_buf must outlive its upload
  return rc;
}

static int deflate_blocks_host_impl(const uint8_t *in, const int64_t *in_off, const int64_t *in_len, int n_blocks,
                                    uint8_t *out, const int64_t *out_off, const int64_t *out_cap, int zlib_wrapper,
                                    int level, int32_t *status, int64_t *out_len) {
  if (n_blocks < 0 || level < 0 || level > 9) return GSKYHIP_E_ARG;
  if (n_blocks == 0) return GSKYHIP_OK;
  if (!in || !out || !in_off || !in_len || !out_off || !out_cap || !status || !out_len) return GSKYHIP_E_ARG;
  if (!args_ok(in_off, in_len, n_blocks, out_off, out_cap)) return GSKYHIP_E_ARG;
  std::atomic<int> next(0);
  auto work = [&]() {
    for (int k = next++; k < n_blocks; k = next++)
      deflate::encode_block_host(in + in_off[k], in_len[k], out + out_off[k], out_cap[k], zlib_wrapper ? 1 : 0, level,
                                 &status[k], &out_len[k], nullptr);
  };
  const unsigned nth = std::max(1u, std::min({16u, std::thread::hardware_concurrency(), (unsigned)n_blocks}));
  std::vector<std::thread> th;
  for (unsigned k = 1; k < nth; k++) th.emplace_back(work);
  work();
  for (auto &x : th) x.join();
  return GSKYHIP_OK;
}

extern "C" int gskyhip_deflate_blocks(const uint8_t *dev_in, const int64_t *in_off, const int64_t *in_len, int n_blocks,
                                      uint8_t *dev_out, const int64_t *out_off, const int64_t *out_cap,
                                      int zlib_wrapper, int level, void *workspace, int64_t workspace_bytes,
                                      int32_t *status, int64_t *out_len, void *stream) {
  try {
    return deflate_blocks_impl(dev_in, in_off, in_len, n_blocks, dev_out, out_off, out_cap, zlib_wrapper, level,
                               workspace, workspace_bytes, status, out_len, stream);
  } catch (...) {
    return GSKYHIP_E_ARG;
  }
}

extern "C" int gskyhip_deflate_blocks_host(const uint8_t *in, const int64_t *in_off, const int64_t *in_len, int n_blocks,
                                           uint8_t *out, const int64_t *out_off, const int64_t *out_cap,
                                           int zlib_wrapper, int level, int32_t *status, int64_t *out_len) {
  try {
    return deflate_blocks_host_impl(in, in_off, in_len, n_blocks, out, out_off, out_cap, zlib_wrapper, level, status,
                                    out_len);
  } catch (...) {
    return GSKYHIP_E_ARG;
  }
}
