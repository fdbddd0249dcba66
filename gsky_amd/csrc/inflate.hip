// inflate.hip -- Deflate / zlib streams decoded on the GPU, one wave64 per
// stream, and the same decoder on host threads.
//
// The decoder is inflate_core.h, compiled for both sides.  On the device one
// workgroup is one wave and owns one stream (blockIdx.x <-> block):
//   * lane 0 walks the bit stream (gsky::inflate::produce) and fills a ring of
//     up to 64 tokens in LDS; the Huffman tables are in LDS too (about 4.6 KiB
//     per wave together, so LDS never limits the waves of a CU);
//   * all 64 lanes then resolve the batch byte by byte: output byte j of the
//     batch belongs to the token found by a binary search over the tokens'
//     offsets, and is a literal, an input byte (stored run) or an earlier
//     output byte (match; distance < length repeats with period distance).
//     The producer closes a batch before a match that would read the batch's
//     own bytes, so the bytes of one batch never depend on each other.
//   * the window is the stream's own output in global memory.  Lanes read
//     bytes other lanes stored in earlier batches: a workgroup-scope release
//     fence follows the stores of a batch and a workgroup-scope acquire fence
//     precedes the loads of the next, with the barrier between them.
//   * Adler-32 over the finished output by the whole wave: two sums per 4 KiB
//     piece, reduced across the wave.
// Every bound is checked by the producer before a token exists (see the
// header), so the resolve phase only touches [0, out_cap) of its own output
// and [0, in_len) of its own input.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <thread>
#include <vector>

#include "../../include/gskyhip.h"
#include "inflate_core.h"

namespace gsky {
namespace {

namespace gi = inflate;

static_assert(gi::kOk == GSKYHIP_INFLATE_OK && gi::kInputTruncated == GSKYHIP_INFLATE_E_INPUT &&
                  gi::kBadBlock == GSKYHIP_INFLATE_E_BLOCK && gi::kBadCodes == GSKYHIP_INFLATE_E_CODES &&
                  gi::kBadDistance == GSKYHIP_INFLATE_E_DIST && gi::kOutputFull == GSKYHIP_INFLATE_E_CAP &&
                  gi::kBadChecksum == GSKYHIP_INFLATE_E_CHECKSUM && gi::kOutputShort == GSKYHIP_INFLATE_E_SHORT,
              "status codes of the header and of the core");

struct BlockDesc {
  int64_t in_off, in_len, out_off, out_cap, out_need;
};

__device__ inline uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off);
  return v;
}

__global__ __launch_bounds__(64) void inflate_kernel(const uint8_t *__restrict__ in, const BlockDesc *__restrict__ desc,
                                                     int n_blocks, uint8_t *out, int zlib_wrapper,
                                                     int32_t *__restrict__ status, int64_t *__restrict__ out_len) {
  __shared__ gi::Tables tables;
  __shared__ gi::Token ring[gi::kMaxBatch];
  __shared__ int sh_n, sh_rc, sh_phase;
  __shared__ unsigned long long sh_start, sh_end;
  __shared__ uint32_t sh_adler;
  const int b = blockIdx.x;
  if (b >= n_blocks) return;
  const int lane = threadIdx.x;
  const BlockDesc d = desc[b];
  const uint8_t *src = in + d.in_off;
  uint8_t *dst = out + d.out_off;
  gi::State s;
  gi::init(s, src, (uint64_t)d.in_len, (uint64_t)d.out_cap, zlib_wrapper);
  int rc = gi::kOk;
  uint64_t end = 0;
  for (;;) {
    if (lane == 0) {
      sh_start = s.pos;
      int n = 0;
      sh_rc = gi::produce(s, tables, ring, gi::kMaxBatch, &n);
      sh_n = n;
      sh_end = s.pos;
      sh_phase = s.phase;
      sh_adler = s.adler_want;
    }
    __syncthreads();
    const int n = sh_n;
    rc = sh_rc;
    const int phase = sh_phase;
    const uint64_t start = sh_start;
    end = sh_end;
    // the loads below read bytes that other lanes stored in earlier batches
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    const uint32_t total = (uint32_t)(end - start);
    if (n > 0) {
      for (uint32_t j = (uint32_t)lane; j < total; j += 64u) {
        int lo = 0, hi = n - 1;
        while (lo < hi) {   // the last token with rel <= j
          const int mid = (lo + hi + 1) >> 1;
          if (ring[mid].rel <= j) lo = mid; else hi = mid - 1;
        }
        const gi::Token tk = ring[lo];
        dst[start + j] = gi::token_byte(tk, j - tk.rel, src, dst, start + tk.rel);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();   // the ring is free again; the batch's bytes are published
    if (rc != gi::kOk || phase == 5) break;
  }
  if (rc == gi::kOk) {
    uint32_t a = 1, bsum = 0;
    if (zlib_wrapper) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      constexpr uint32_t kPiece = 4096;   // sum of (L - i) * 255 over a piece stays below 2^32
      for (uint64_t base = 0; base < end; base += kPiece) {
        const uint32_t L = (uint32_t)(end - base < kPiece ? end - base : kPiece);
        uint32_t sa = 0, sb = 0;
        for (uint32_t i = (uint32_t)lane; i < L; i += 64u) {
          const uint32_t v = dst[base + i];
          sa += v;
          sb += (L - i) * v;
        }
        sa = wave_sum(sa);
        sb = wave_sum(sb);
        bsum = (uint32_t)(((uint64_t)bsum + (uint64_t)L * a + sb) % gi::kAdlerMod);
        a = (a + sa) % gi::kAdlerMod;
      }
    }
    if (zlib_wrapper && ((bsum << 16) | a) != sh_adler) rc = gi::kBadChecksum;
    else if (end < (uint64_t)d.out_need) rc = gi::kOutputShort;
  }
  if (lane == 0) {
    status[b] = rc;
    out_len[b] = (int64_t)end;
  }
}

bool args_ok(const int64_t *in_off, const int64_t *in_len, int n, const int64_t *out_off, const int64_t *out_cap,
             const int64_t *out_need) {
  for (int k = 0; k < n; k++)
    if (in_off[k] < 0 || in_len[k] < 0 || in_len[k] > 0xFFFFFFFFll || out_off[k] < 0 || out_cap[k] < 0 ||
        out_need[k] < 0 || out_need[k] > out_cap[k])
      return false;
  return true;
}

}  // namespace
}  // namespace gsky

using namespace gsky;

static int inflate_blocks_impl(const uint8_t *dev_in, const int64_t *in_off, const int64_t *in_len, int n_blocks,
                               uint8_t *dev_out, const int64_t *out_off, const int64_t *out_cap,
                               const int64_t *out_need, int zlib_wrapper, int32_t *status, int64_t *out_len,
                               void *stream) {
  if (n_blocks < 0) return GSKYHIP_E_ARG;
  if (n_blocks == 0) return GSKYHIP_OK;
  if (!dev_in || !dev_out || !in_off || !in_len || !out_off || !out_cap || !out_need || !status || !out_len)
    return GSKYHIP_E_ARG;
  if (!args_ok(in_off, in_len, n_blocks, out_off, out_cap, out_need)) return GSKYHIP_E_ARG;
  std::vector<BlockDesc> desc((size_t)n_blocks);
  for (int k = 0; k < n_blocks; k++) desc[k] = {in_off[k], in_len[k], out_off[k], out_cap[k], out_need[k]};
  hipStream_t s = (hipStream_t)stream;
  const size_t desc_bytes = sizeof(BlockDesc) * (size_t)n_blocks;
  const size_t len_at = (desc_bytes + 15) & ~(size_t)15;
  const size_t st_at = len_at + sizeof(int64_t) * (size_t)n_blocks;
  const size_t bytes = st_at + sizeof(int32_t) * (size_t)n_blocks;
  uint8_t *ws = nullptr;
  if (hipMalloc((void **)&ws, bytes) != hipSuccess) return GSKYHIP_E_HIP;
  int rc = GSKYHIP_OK;
  if (hipMemcpyAsync(ws, desc.data(), desc_bytes, hipMemcpyHostToDevice, s) != hipSuccess) rc = GSKYHIP_E_HIP;
  if (!rc) {
    hipLaunchKernelGGL(inflate_kernel, dim3((unsigned)n_blocks), dim3(64), 0, s, dev_in, (const BlockDesc *)ws, n_blocks,
                       dev_out, zlib_wrapper ? 1 : 0, (int32_t *)(ws + st_at), (int64_t *)(ws + len_at));
    if (hipGetLastError() != hipSuccess) rc = GSKYHIP_E_HIP;
  }
  if (!rc && hipMemcpyAsync(out_len, ws + len_at, sizeof(int64_t) * (size_t)n_blocks, hipMemcpyDeviceToHost, s) != hipSuccess)
    rc = GSKYHIP_E_HIP;
  if (!rc && hipMemcpyAsync(status, ws + st_at, sizeof(int32_t) * (size_t)n_blocks, hipMemcpyDeviceToHost, s) != hipSuccess)
    rc = GSKYHIP_E_HIP;
  if (hipStreamSynchronize(s) != hipSuccess && !rc) rc = GSKYHIP_E_HIP;   // desc must outlive the copy
  (void)hipFree(ws);
  return rc;
}

static int inflate_blocks_host_impl(const uint8_t *in, const int64_t *in_off, const int64_t *in_len, int n_blocks,
                                    uint8_t *out, const int64_t *out_off, const int64_t *out_cap,
                                    const int64_t *out_need, int zlib_wrapper, int32_t *status, int64_t *out_len) {
  if (n_blocks < 0) return GSKYHIP_E_ARG;
  if (n_blocks == 0) return GSKYHIP_OK;
  if (!in || !out || !in_off || !in_len || !out_off || !out_cap || !out_need || !status || !out_len)
    return GSKYHIP_E_ARG;
  if (!args_ok(in_off, in_len, n_blocks, out_off, out_cap, out_need)) return GSKYHIP_E_ARG;
  std::atomic<int> next(0);
  auto work = [&]() {
    for (int k = next++; k < n_blocks; k = next++) {
      uint64_t got = 0;
      status[k] = inflate::inflate_serial(in + in_off[k], (uint64_t)in_len[k], out + out_off[k], (uint64_t)out_cap[k],
                                          (uint64_t)out_need[k], zlib_wrapper, &got);
      out_len[k] = (int64_t)got;
    }
  };
  const unsigned nth = std::max(1u, std::min({16u, std::thread::hardware_concurrency(), (unsigned)n_blocks}));
  std::vector<std::thread> th;
  for (unsigned k = 1; k < nth; k++) th.emplace_back(work);
  work();
  for (auto &x : th) x.join();
  return GSKYHIP_OK;
}

extern "C" int gskyhip_inflate_blocks(const uint8_t *dev_in, const int64_t *in_off, const int64_t *in_len, int n_blocks,
                                      uint8_t *dev_out, const int64_t *out_off, const int64_t *out_cap,
                                      const int64_t *out_need, int zlib_wrapper, int32_t *status, int64_t *out_len,
                                      void *stream) {
  try {
    return inflate_blocks_impl(dev_in, in_off, in_len, n_blocks, dev_out, out_off, out_cap, out_need, zlib_wrapper,
                               status, out_len, stream);
  } catch (...) {
    return GSKYHIP_E_ARG;
  }
}

extern "C" int gskyhip_inflate_blocks_host(const uint8_t *in, const int64_t *in_off, const int64_t *in_len, int n_blocks,
                                           uint8_t *out, const int64_t *out_off, const int64_t *out_cap,
                                           const int64_t *out_need, int zlib_wrapper, int32_t *status,
                                           int64_t *out_len) {
  try {
    return inflate_blocks_host_impl(in, in_off, in_len, n_blocks, out, out_off, out_cap, out_need, zlib_wrapper, status,
                                    out_len);
  } catch (...) {
    return GSKYHIP_E_ARG;
  }
}
