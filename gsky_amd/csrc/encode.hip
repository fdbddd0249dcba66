// encode.hip -- output codecs: EncodePNG's png.Encode (utils/ogc_encoders.go:
// 139; Go 1.12 image/png) for batches of RGBA tiles in HBM.
//
// Go's encoder on the *image.RGBA canvas of EncodePNG (ogc_encoders.go:82):
//   * colour type: truecolour RGB (cbTC8) when every alpha is 0xff
//     (image.RGBA.Opaque), else RGBA (cbTCA8) whose bytes are the
//     color.NRGBAModel conversion of each premultiplied pixel (a = 0 ->
//     0,0,0,0; a = 0xffff -> the bytes; else r * 0xffff / a in 16 bits, high
//     byte, wrapping like Go's uint8()) -- image.RGBA stores the palette
//     colours as they are, so a palette entry with r > a wraps;
//   * per row the filter of writer.go filter(): the sums of |int8(byte)| of the
//     Up, Paeth, None, Sub and Average residuals, tried in that order, the
//     first strictly smaller sum wins (the early exits there never change the
//     choice); the previous row of the first row is zero;
//   * zlib at DefaultCompression (level 6) over the filtered rows, written
//     through a 32 KiB bufio.Writer: IDAT chunks of exactly 32768 bytes, the
//     last one shorter; IHDR / IDAT / IEND with their CRC-32.
// Here the colour-type test, the NRGBA conversion and the filter selection run
// on the GPU (one workgroup per row), and so does the deflate of each tile
// ("GPU deflate" below: the encoder of deflate_core.h, one final Huffman-coded
// block per tile) and the CRC-32 of its IDAT chunks; host threads only frame
// the PNGs.  Tiles of more than 4096 rows, and every tile under
// GSKYHIP_PNG_ZLIB=1, are deflated by zlib (level 6, 32 KiB window, default
// strategy) on host threads instead.  The filtered rows -- every byte the
// deflate receives -- are Go's exactly; the compressed bytes are this
// encoder's (or zlib's), not Go's compress/flate (all DEFLATE: the decoded
// image and the filter bytes are identical, byte identity with Go is parity
// unpinned).
//
// Beside it, opt-in and beyond the reference, the indexed-colour encoder for
// one-band tiles (gskyhip_encode_png_indexed): EncodePNG expands
// the ByteRaster of utils.Scale through the 256-entry ramp of
// GradientRGBAPalette, or to grey, before png.Encode ever sees it; here the
// index bytes themselves are the image data of a colour type 3 PNG --
//   * IHDR (w, h, 8, 3, 0, 0, 0), PLTE, tRNS, IDAT..., IEND;
//   * PLTE / tRNS entry i < 255: the color.NRGBAModel conversion above of
//     ramp[i] (grey: i, i, i, 255); entry 255, the nodata byte 0xFF, is
//     transparent black (ogc_encoders.go:96, 105), so every decoder gives the
//     RGBA of the truecolour PNG of the same tile;
//   * every row the filter byte 0 (None) and its w index bytes, no filter
//     selection; the same GPU deflate with one byte a pixel, the same 32 KiB
//     IDAT chunks, GSKYHIP_PNG_FIXED / GSKYHIP_PNG_ZLIB and the 4096-row limit.
// Go's encoder never sees an image.Paletted on this path: the format is
// defined here and parity with png.Encode of one is unpinned.  What ships:
// two front ends -- png_opaque_kernel + png_filter_kernel for RGBA tiles,
// png_index_rows_kernel for index tiles, which stages the rows, and PLTE /
// tRNS framed once per call on the host -- over one back end (png_finish: the
// tokenise / count / write kernels with the bytes a pixel per tile, 1, 3 or
// 4, the IDAT CRC kernel, one copy of the compressed bytes, host framing),
// and the indexed path's host twin gskyhip_encode_png_indexed_host.
#include <hip/hip_runtime.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/gskyhip.h"
#include "deflate.h"
#include "deflate_core.h"
#include "tiffwrite.h"

namespace gsky {
namespace {

// ------------------------------------------------------------------ GPU pass
// bytes a pixel of tile t: 3 when it is opaque (image.RGBA.Opaque over its
// w x h rectangle: truecolour), else 4 (truecolour + alpha)
__global__ __launch_bounds__(256) void png_opaque_kernel(const uint8_t *__restrict__ rgba, int64_t tile_stride,
                                                         int64_t row_stride, const int32_t *__restrict__ wh,
                                                         int32_t *__restrict__ px_bytes) {
  const int t = blockIdx.x;
  const int w = wh[2 * t], h = wh[2 * t + 1];
  const uint8_t *base = rgba + (int64_t)t * tile_stride;
  int bad = 0;
  for (int64_t i = threadIdx.x; i < (int64_t)w * h; i += blockDim.x) {
    const int y = (int)(i / w), x = (int)(i % w);
    bad |= base[(int64_t)y * row_stride + 4 * x + 3] != 0xFF;
  }
  bad = __syncthreads_or(bad);
  if (threadIdx.x == 0) px_bytes[t] = bad ? 4 : 3;
}

// byte k of row y of the image data Go's writeImage feeds the filter: RGB of
// an opaque canvas, else NRGBA; the row above row 0 is zero
__device__ __forceinline__ uint32_t png_byte(const uint8_t *__restrict__ tile, int64_t row_stride, int y, int k,
                                             bool opq) {
  if (y < 0 || k < 0) return 0u;
  const int bpp = opq ? 3 : 4;
  const int x = k / bpp, c = k - x * bpp;
  const uint8_t *px = tile + (int64_t)y * row_stride + 4 * x;
  if (opq) return px[c];
  const uint32_t a = px[3];
  if (a == 0xFF) return px[c];
  if (a == 0) return 0u;
  if (c == 3) return a;
  const uint32_t a16 = a | (a << 8);
  const uint32_t v16 = (uint32_t)px[c] | ((uint32_t)px[c] << 8);
  return ((v16 * 0xFFFFu) / a16 >> 8) & 0xFFu;   // color.nrgbaModel, uint8() truncation
}

__device__ __forceinline__ uint32_t abs8(uint32_t d) { d &= 0xFFu; return d < 128u ? d : 256u - d; }

__device__ __forceinline__ uint32_t paeth(uint32_t a, uint32_t b, uint32_t c) {   // writer.go paeth()
  const int pc0 = (int)c;
  int pa = (int)b - pc0;
  int pb = (int)a - pc0;
  int pc = abs(pa + pb);
  pa = abs(pa);
  pb = abs(pb);
  if (pa <= pb && pa <= pc) return a;
  if (pb <= pc) return b;
  return c;
}

// One workgroup per (tile, row): out row = [filter byte][filtered bytes].
__global__ __launch_bounds__(256) void png_filter_kernel(const uint8_t *__restrict__ rgba, int64_t tile_stride,
                                                         int64_t row_stride, const int32_t *__restrict__ wh,
                                                         const int32_t *__restrict__ px_bytes, int max_h,
                                                         const int64_t *__restrict__ out_off,
                                                         uint8_t *__restrict__ out) {
  const int t = blockIdx.x / max_h, y = blockIdx.x % max_h;
  const int w = wh[2 * t], h = wh[2 * t + 1];
  if (y >= h) return;
  const bool opq = px_bytes[t] == 3;
  const int bpp = opq ? 3 : 4;
  const int n = bpp * w;
  const uint8_t *tile = rgba + (int64_t)t * tile_stride;
  __shared__ uint32_t s_sum[5][4];
  uint32_t sum[5] = {0, 0, 0, 0, 0};
  for (int k = threadIdx.x; k < n; k += blockDim.x) {
    const uint32_t cur = png_byte(tile, row_stride, y, k, opq), up = png_byte(tile, row_stride, y - 1, k, opq);
    const uint32_t left = k >= bpp ? png_byte(tile, row_stride, y, k - bpp, opq) : 0u;
    const uint32_t ul = k >= bpp ? png_byte(tile, row_stride, y - 1, k - bpp, opq) : 0u;
    sum[0] += abs8(cur - up);                                        // Up
    sum[1] += abs8(k >= bpp ? cur - paeth(left, up, ul) : cur - up);   // Paeth (first bpp bytes: Up)
    sum[2] += abs8(cur);                                             // None
    sum[3] += abs8(cur - left);                                      // Sub
    sum[4] += abs8(k >= bpp ? cur - ((left + up) >> 1) : cur - (up >> 1));   // Average
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int f = 0; f < 5; f++) {
    uint32_t s = sum[f];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) s_sum[f][wv] = s;
  }
  __syncthreads();
  // tried in the order Up, Paeth, None, Sub, Average; a strictly smaller sum wins
  const int order[5] = {2, 4, 0, 1, 3};   // their PNG filter types
  uint32_t best = 0;
  int ft = 2;
#pragma unroll
  for (int f = 0; f < 5; f++) {
    const uint32_t s = s_sum[f][0] + s_sum[f][1] + s_sum[f][2] + s_sum[f][3];
    if (f == 0 || s < best) { best = s; ft = order[f]; }
  }
  uint8_t *row = out + out_off[t] + (int64_t)y * (1 + n);
  if (threadIdx.x == 0) row[0] = (uint8_t)ft;
  for (int k = threadIdx.x; k < n; k += blockDim.x) {
    const uint32_t cur = png_byte(tile, row_stride, y, k, opq), up = png_byte(tile, row_stride, y - 1, k, opq);
    const uint32_t left = k >= bpp ? png_byte(tile, row_stride, y, k - bpp, opq) : 0u;
    const uint32_t ul = k >= bpp ? png_byte(tile, row_stride, y - 1, k - bpp, opq) : 0u;
    uint32_t v;
    switch (ft) {
      case 0: v = cur; break;
      case 1: v = cur - left; break;
      case 2: v = cur - up; break;
      case 3: v = k >= bpp ? cur - ((left + up) >> 1) : cur - (up >> 1); break;
      default: v = k >= bpp ? cur - paeth(left, up, ul) : cur - up; break;
    }
    row[1 + k] = (uint8_t)v;
  }
}

// Indexed colour: the image data of tile t -- h rows of [filter byte 0][the
// row's w index bytes] -- packed at out + t * per, from a tile whose rows lie
// row_stride bytes apart.  A thread per aligned dword of the packed stream
// (per is a multiple of 4 and out 4-byte aligned, so the store is one dword
// and a wave stores 256 consecutive bytes): where the four bytes are pixels of
// one row they are one load, the filter byte having shifted them by y + 1
// bytes against the source row, hence unaligned; a dword that holds a filter
// byte, straddles two rows or ends the stream is put together from bytes.
// Bytes of the last dword past the stream are zero.  Reads stay inside the
// tile's w x h rectangle, writes below out + t * per + per.
__global__ __launch_bounds__(256) void png_index_rows_kernel(const uint8_t *__restrict__ index, int64_t tile_stride,
                                                             int64_t row_stride, const int32_t *__restrict__ wh,
                                                             int blocks_per_tile, int64_t per,
                                                             uint8_t *__restrict__ out) {
  const int t = (int)(blockIdx.x / (unsigned)blocks_per_tile);
  const int64_t q = ((int64_t)(blockIdx.x % (unsigned)blocks_per_tile) * 256 + threadIdx.x) * 4;
  const int w = wh[2 * t], h = wh[2 * t + 1];
  const int stride = 1 + w;
  const int64_t n = (int64_t)h * stride;
  if (q >= n) return;
  const uint8_t *tile = index + (int64_t)t * tile_stride;
  // row and column (0: the filter byte) of stream byte q; 32-bit division where the stream allows
  int64_t y = n <= 0x7FFFFFFF ? (int64_t)((uint32_t)q / (uint32_t)stride) : q / stride;
  int c = (int)(q - y * stride);
  uint32_t v = 0;
  if (c >= 1 && c + 3 < stride) {
    v = deflate::ld_u32(tile + y * row_stride + (c - 1));
  } else {
    for (int k = 0; k < 4 && q + k < n; k++) {
      if (c != 0) v |= (uint32_t)tile[y * row_stride + (c - 1)] << (8 * k);
      if (++c == stride) { c = 0; y++; }
    }
  }
  *(uint32_t *)(out + (int64_t)t * per + q) = v;
}

// ------------------------------------------------------------------ GPU deflate
// The zlib stream of each tile's filtered rows built on the GPU: one final
// block -- Huffman codes built for the tile from its symbol frequencies
// (RFC 1951 3.2.7), or the fixed codes (3.2.6) where those come out shorter
// -- whose LZ77 matches are searched at the distances a PNG row offers --
// runs, pixels to the left, rows above and the diagonals (tokenize_row) --
// within the row (so rows are encoded independently: a thread per row, matches
// may reach back into earlier rows).  Pass 1 counts each row's bits; their
// prefix sums place every row in the tile's bit stream and every tile in one
// packed buffer (so only the compressed bytes cross PCIe); pass 2 writes the
// codes (the words two rows share by OR).  Adler-32 from per-row sums.  The
// stream is valid DEFLATE / zlib; its bytes are neither zlib's nor Go's
// compress/flate (parity unpinned; the tests inflate it, compare the rows, and
// hold the bytes to tests/golden/png_streams.json).
//
// The encoder is deflate_core.h, shared with the block encoder
// of deflate.hip and with the host twin gskyhip_png_deflate_rows_host: its row
// tokeniser, Huffman construction, block plan (plan_png: fixed or dynamic,
// never stored), bit sink and frame writer.  PNG's own are the geometry below,
// the per-row Adler-32 and the 4-byte aligned packing of the streams.
namespace gd = deflate;

constexpr int kPngMaxRows = 4096;    // rows of a tile the deflate kernels handle (LDS scan)

// Pass 0, a thread per row (a wave per 64 rows of a tile, so every CU holds
// many rows in flight): the row's tokens, one dword each, kept for pass 1's
// bit count and pass 2 (a row has at most `stride` tokens), and -- for a
// dynamic code -- their symbol frequencies, summed per workgroup in LDS and
// added to the tile's global histogram.
__global__ __launch_bounds__(64) void png_tokenize_kernel(const uint8_t *__restrict__ filt,
                                                          const int64_t *__restrict__ off,
                                                          const int32_t *__restrict__ wh,
                                                          const int32_t *__restrict__ px_bytes, int max_h,
                                                          uint32_t *__restrict__ tok, int32_t *__restrict__ ntok,
                                                          int64_t per, uint32_t *__restrict__ freq, int dynamic) {
  const int groups = (max_h + 63) / 64;
  const int t = (int)(blockIdx.x / groups), tid = threadIdx.x, y = (int)(blockIdx.x % groups) * 64 + tid;
  const int h = wh[2 * t + 1];
  const int bpp = px_bytes[t];
  const int stride = 1 + bpp * wh[2 * t];
  __shared__ uint32_t s_freq[gd::kSymN];
  for (int i = tid; i < gd::kSymN; i += 64) s_freq[i] = 0;
  __syncthreads();
  if (y < h) {
    const int64_t p0 = (int64_t)y * stride;
    ntok[(int64_t)t * max_h + y] =
        gd::tokenize_row(filt + off[t], p0, p0 + stride, bpp, stride, tok + (int64_t)t * per + p0, [&](int sym) {
          if (dynamic) atomicAdd(&s_freq[sym], 1u);
        });
  }
  __syncthreads();
  if (dynamic)
    for (int i = tid; i < gd::kSymN; i += 64)
      if (s_freq[i]) atomicAdd(&freq[(int64_t)t * gd::kSymN + i], s_freq[i]);
}

static_assert(sizeof(gd::Plan) % 4 == 0, "a tile's plan is copied in dwords");

// Pass 1, a workgroup per tile: the rows' Adler-32 sums; the tile's plan from
// pass 0's frequencies (thread 0: the dynamic code, or the fixed one where
// that is not longer, header included); each row's bits under it; the stream
// length; the plan into tab[t] for pass 2.  Tile stream: zlib header (2 B),
// block header, rows, end of block, pad to a byte, Adler-32 (4 B).
__global__ __launch_bounds__(256) void png_deflate_count_kernel(const uint8_t *__restrict__ filt,
                                                                const int64_t *__restrict__ off,
                                                                const int32_t *__restrict__ wh,
                                                                const int32_t *__restrict__ px_bytes, int max_h,
                                                                int32_t *__restrict__ row_bits,
                                                                uint32_t *__restrict__ adler,
                                                                int64_t *__restrict__ zlen, gd::Plan *__restrict__ tab,
                                                                int dynamic, const uint32_t *__restrict__ tok,
                                                                const int32_t *__restrict__ ntok, int64_t per,
                                                                const uint32_t *__restrict__ freq) {
  const int t = blockIdx.x, tid = threadIdx.x;
  const int w = wh[2 * t], h = wh[2 * t + 1];
  const int bpp = px_bytes[t];
  const int stride = 1 + bpp * w;
  const uint8_t *data = filt + off[t];
  __shared__ uint32_t s_a[kPngMaxRows], s_b[kPngMaxRows];
  __shared__ int64_t s_bits[256];
  __shared__ uint32_t s_freq[gd::kSymN];
  __shared__ gd::Plan P;
  __shared__ gd::PlanScratch S;
  for (int i = tid; i < gd::kSymN; i += blockDim.x) s_freq[i] = dynamic ? freq[(int64_t)t * gd::kSymN + i] : 0u;
  for (int y = tid; y < h; y += blockDim.x) {
    const int64_t p0 = (int64_t)y * stride;
    uint64_t a = 0, bb = 0;   // sum of bytes, sum of (n - i) * byte (exact: < 2^40), then mod 65521
    int i = 0;
    for (; i + 4 <= stride; i += 4) {
      const uint32_t v = gd::ld_u32(data + p0 + i);
      const uint32_t c0 = v & 0xFFu, c1 = (v >> 8) & 0xFFu, c2 = (v >> 16) & 0xFFu, c3 = v >> 24;
      a += c0 + c1 + c2 + c3;
      bb += (uint64_t)(stride - i) * c0 + (uint64_t)(stride - i - 1) * c1 + (uint64_t)(stride - i - 2) * c2 +
            (uint64_t)(stride - i - 3) * c3;
    }
    for (; i < stride; i++) {
      a += data[p0 + i];
      bb += (uint64_t)(stride - i) * data[p0 + i];
    }
    s_a[y] = (uint32_t)(a % gd::kAdlerMod);
    s_b[y] = (uint32_t)(bb % gd::kAdlerMod);
  }
  __syncthreads();
  if (tid == 0) gd::plan_png(s_freq, !dynamic, P, S);
  __syncthreads();
  int64_t mine = 0;
  for (int y = tid; y < h; y += blockDim.x) {
    const uint32_t b = gd::segment_bits(tok + (int64_t)t * per + (int64_t)y * stride, ntok[(int64_t)t * max_h + y], P.len);
    row_bits[(int64_t)t * max_h + y] = (int32_t)b;
    mine += b;
  }
  s_bits[tid] = mine;
  __syncthreads();
  if (tid == 0) {
    int64_t total = 0;
    for (int k = 0; k < (int)blockDim.x; k++) total += s_bits[k];
    uint32_t A = 1, B = 0;   // adler32 of the rows in order
    for (int y = 0; y < h; y++) {
      B = (uint32_t)((B + (uint64_t)stride * A + s_b[y]) % gd::kAdlerMod);
      A = (A + s_a[y]) % gd::kAdlerMod;
    }
    adler[t] = (B << 16) | A;
    gd::set_body(P, total, 6);
    zlen[t] = P.stream_bytes;
  }
  __syncthreads();
  for (int i = tid; i < (int)(sizeof(gd::Plan) / 4); i += blockDim.x)
    ((uint32_t *)&tab[t])[i] = ((const uint32_t *)&P)[i];
}

// Pass 2: the frame (thread 0) and the codes of every row at its bit offset
// in the tile's stream, at the tile's byte offset zoff[t] of the packed buffer
// (zeroed; 4-byte aligned, so the stream is the sink's words).
__global__ __launch_bounds__(256) void png_deflate_write_kernel(const int32_t *__restrict__ wh,
                                                                const int32_t *__restrict__ px_bytes, int max_h,
                                                                const int32_t *__restrict__ row_bits,
                                                                const uint32_t *__restrict__ adler,
                                                                const int64_t *__restrict__ zoff,
                                                                uint8_t *__restrict__ packed,
                                                                const gd::Plan *__restrict__ tab,
                                                                const uint32_t *__restrict__ tok,
                                                                const int32_t *__restrict__ ntok, int64_t per) {
  const int t = blockIdx.x;
  const int w = wh[2 * t], h = wh[2 * t + 1];
  const int stride = 1 + px_bytes[t] * w;
  uint32_t *words = (uint32_t *)(packed + zoff[t]);
  __shared__ int64_t s_start[kPngMaxRows];
  __shared__ uint16_t s_code[gd::kSymN];
  __shared__ uint8_t s_len[gd::kSymN];
  const gd::Plan &T = tab[t];
  for (int i = threadIdx.x; i < gd::kSymN; i += blockDim.x) { s_code[i] = T.code[i]; s_len[i] = T.len[i]; }
  if (threadIdx.x == 0) {   // row bit offsets (serial: h <= 4096 adds)
    int64_t b = 16 + T.hdr_bits;
    for (int y = 0; y < h; y++) { s_start[y] = b; b += row_bits[(int64_t)t * max_h + y]; }
  }
  __syncthreads();
  // every shared word by OR into the zeroed buffer, so no write order matters
  if (threadIdx.x == 0) gd::write_frame(T, 1, gd::kFlgFastest, adler[t], words);
  for (int y = threadIdx.x; y < h; y += blockDim.x)
    gd::write_segment(tok + (int64_t)t * per + (int64_t)y * stride, ntok[(int64_t)t * max_h + y], s_code, s_len, words,
                      s_start[y]);
}

// CRC-32 (PNG / zlib polynomial 0xEDB88320) of each 32 KiB IDAT chunk of
// every tile's stream, type bytes "IDAT" included: a thread per chunk,
// slicing by 4 over dword loads (the stream starts 4-byte aligned and so
// does every chunk), tables in LDS.
__global__ __launch_bounds__(256) void png_idat_crc_kernel(const uint8_t *__restrict__ packed,
                                                           const int64_t *__restrict__ zoff,
                                                           const int64_t *__restrict__ zlen, int n_tiles,
                                                           int max_chunks, uint32_t *__restrict__ crc) {
  __shared__ uint32_t T[4][256];
  for (int i = threadIdx.x; i < 256; i += blockDim.x) {
    uint32_t c = (uint32_t)i;
    for (int k = 0; k < 8; k++) c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
    T[0][i] = c;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 256; i += blockDim.x) {
    uint32_t c = T[0][i];
    for (int k = 1; k < 4; k++) { c = T[0][c & 0xFFu] ^ (c >> 8); T[k][i] = c; }
  }
  __syncthreads();
  const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (int64_t)n_tiles * max_chunks) return;
  const int t = (int)(g / max_chunks), ch = (int)(g % max_chunks);
  const int64_t n_all = zlen[t], p0 = (int64_t)ch * 32768;
  if (p0 >= n_all) return;
  const int64_t n = min((int64_t)32768, n_all - p0);
  const uint8_t *d = packed + zoff[t] + p0;
  uint32_t c = 0xFFFFFFFFu;
  const uint8_t idat[4] = {'I', 'D', 'A', 'T'};
  for (int k = 0; k < 4; k++) c = T[0][(c ^ idat[k]) & 0xFFu] ^ (c >> 8);
  int64_t i = 0;
  for (; i + 4 <= n; i += 4) {
    c ^= *(const uint32_t *)(d + i);
    c = T[3][c & 0xFFu] ^ T[2][(c >> 8) & 0xFFu] ^ T[1][(c >> 16) & 0xFFu] ^ T[0][c >> 24];
  }
  for (; i < n; i++) c = T[0][(c ^ d[i]) & 0xFFu] ^ (c >> 8);
  crc[g] = c ^ 0xFFFFFFFFu;
}

// ------------------------------------------------------------------ GeoTIFF
// One thread per (band, tile, row of the tile): the row's samples (edge
// tiles padded with `pad`) PackBits-encoded into its slot.
__global__ __launch_bounds__(256) void tiff_rows_kernel(const uint8_t *const *__restrict__ bands, int ts, int width,
                                                        int height, int bx, int by, int ntx, int nty,
                                                        const uint8_t *__restrict__ pad, int64_t slot,
                                                        uint8_t *__restrict__ raw, uint8_t *__restrict__ enc,
                                                        int32_t *__restrict__ len, int64_t n_rows) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_rows) return;
  const int row = (int)(r % by);
  const int64_t tb = r / by;
  const int tile = (int)(tb % ((int64_t)ntx * nty));
  const int b = (int)(tb / ((int64_t)ntx * nty));
  const int tx = tile % ntx, ty = tile / ntx;
  const int y = ty * by + row;
  const int rb = bx * ts;
  uint8_t *line = raw + r * (int64_t)rb;
  const uint8_t *src = bands[b];
  for (int x = 0; x < bx; x++) {
    const int gx = tx * bx + x;
    const bool in = src && gx < width && y < height;   // no source: an EmptyTile band, all `pad`
    for (int k = 0; k < ts; k++) line[x * ts + k] = in ? src[((int64_t)y * width + gx) * ts + k] : pad[b * 8 + k];
  }
  len[r] = tiff::packbits_row(line, rb, enc + r * slot);
}

// ------------------------------------------------------------------ host framing
void put32(std::vector<uint8_t> &o, uint32_t v) {
  o.push_back((uint8_t)(v >> 24)); o.push_back((uint8_t)(v >> 16));
  o.push_back((uint8_t)(v >> 8)); o.push_back((uint8_t)v);
}

void chunk(std::vector<uint8_t> &o, const char *type, const uint8_t *data, size_t n) {
  put32(o, (uint32_t)n);
  const size_t at = o.size();
  o.insert(o.end(), type, type + 4);
  if (n) o.insert(o.end(), data, data + n);
  put32(o, (uint32_t)crc32(0L, o.data() + at, (uInt)(n + 4)));
}

// How a call's tiles are framed.  Truecolour (gskyhip_encode_png): pal is
// NULL and a tile's colour type follows its bytes a pixel, 3 -> RGB (2),
// 4 -> RGBA (6).  Indexed (gskyhip_encode_png_indexed): colour type 3, and
// pal is the PLTE and tRNS chunks that follow every IHDR, framed once.
int png_colour_type(int px_bytes) { return px_bytes == 1 ? 3 : px_bytes == 3 ? 2 : 6; }

// byte c (0..2) of the color.NRGBAModel conversion of a premultiplied RGBA
// entry: png_byte()'s rule on the host
uint8_t nrgba_byte(const uint8_t *px, int c) {
  const uint32_t a = px[3];
  if (a == 0xFF) return px[c];
  if (a == 0) return 0;
  const uint32_t a16 = a | (a << 8);
  const uint32_t v16 = (uint32_t)px[c] | ((uint32_t)px[c] << 8);
  return (uint8_t)(((v16 * 0xFFFFu) / a16 >> 8) & 0xFFu);
}

// PLTE and tRNS of an indexed call, with length, type and CRC-32: entry i <
// 255 is the NRGBA of ramp[i] (256 x RGBA as GradientRGBAPalette leaves it),
// or (i, i, i, 255) without a ramp (grey); entry 255, the nodata index, is
// transparent black (ogc_encoders.go:96, 105).
void png_palette_chunks(const uint8_t *ramp, std::vector<uint8_t> &o) {
  uint8_t plte[768], trns[256];
  for (int i = 0; i < 255; i++) {
    for (int c = 0; c < 3; c++) plte[3 * i + c] = ramp ? nrgba_byte(ramp + 4 * i, c) : (uint8_t)i;
    trns[i] = ramp ? ramp[4 * i + 3] : 0xFF;
  }
  plte[765] = plte[766] = plte[767] = 0;
  trns[255] = 0;
  o.clear();
  chunk(o, "PLTE", plte, 768);
  chunk(o, "tRNS", trns, 256);
}

// PNG signature + IHDR of a w x h 8-bit image of px_bytes a pixel, then the
// call's palette chunks, if any.
void png_head(int w, int h, int px_bytes, const std::vector<uint8_t> *pal, std::vector<uint8_t> &o) {
  static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1A, '\n'};
  o.assign(sig, sig + 8);
  uint8_t ihdr[13];
  const uint32_t ww = (uint32_t)w, hh = (uint32_t)h;
  ihdr[0] = ww >> 24; ihdr[1] = ww >> 16; ihdr[2] = ww >> 8; ihdr[3] = ww;
  ihdr[4] = hh >> 24; ihdr[5] = hh >> 16; ihdr[6] = hh >> 8; ihdr[7] = hh;
  ihdr[8] = 8;                 // bit depth
  ihdr[9] = (uint8_t)png_colour_type(px_bytes);   // truecolour / truecolour + alpha / indexed
  ihdr[10] = 0; ihdr[11] = 0; ihdr[12] = 0;
  chunk(o, "IHDR", ihdr, 13);
  if (pal) o.insert(o.end(), pal->begin(), pal->end());
}

// A whole PNG around a finished zlib stream, written straight into dst
// (cap bytes): 32 KiB IDAT chunks (Go's bufio.Writer size), IEND; returns
// its size, 0 when it does not fit.
size_t png_frame(const uint8_t *z, size_t zn, int w, int h, int px_bytes, const std::vector<uint8_t> *pal,
                 uint8_t *dst, size_t cap, const uint32_t *idat_crc) {
  std::vector<uint8_t> head;
  png_head(w, h, px_bytes, pal, head);
  const size_t need = head.size() + (zn + 32767) / 32768 * 12 + zn + 12;
  if (need > cap) return 0;
  uint8_t *o = dst;
  std::memcpy(o, head.data(), head.size());
  o += head.size();
  auto be32 = [&](uint32_t v) { o[0] = v >> 24; o[1] = v >> 16; o[2] = v >> 8; o[3] = v; o += 4; };
  const uLong crc_idat = crc32(0L, (const Bytef *)"IDAT", 4);
  for (size_t p = 0; p < zn; p += 32768) {
    const size_t n = std::min<size_t>(32768, zn - p);
    be32((uint32_t)n);
    std::memcpy(o, "IDAT", 4);
    o += 4;
    std::memcpy(o, z + p, n);
    o += n;
    be32(idat_crc ? idat_crc[p / 32768] : (uint32_t)crc32(crc_idat, z + p, (uInt)n));
  }
  be32(0);
  std::memcpy(o, "IEND", 4);
  o += 4;
  be32((uint32_t)crc32(0L, (const Bytef *)"IEND", 4));
  return (size_t)(o - dst);
}

// One tile through host zlib: PNG signature, IHDR, the palette chunks, the
// zlib stream in 32 KiB IDAT chunks, IEND.
int png_tile(const uint8_t *filtered, size_t n_filtered, int w, int h, int px_bytes, const std::vector<uint8_t> *pal,
             std::vector<uint8_t> &o) {
  png_head(w, h, px_bytes, pal, o);
  std::vector<uint8_t> z(compressBound((uLong)n_filtered) + 64);
  z_stream s;
  std::memset(&s, 0, sizeof(s));
  if (deflateInit2(&s, 6, Z_DEFLATED, 15, 8, Z_DEFAULT_STRATEGY) != Z_OK) return GSKYHIP_E_ARG;
  s.next_in = (Bytef *)filtered;
  s.avail_in = (uInt)n_filtered;
  s.next_out = z.data();
  s.avail_out = (uInt)z.size();
  const int rc = ::deflate(&s, Z_FINISH);   // zlib's, not the namespace of deflate_core.h
  const size_t zn = z.size() - s.avail_out;
  deflateEnd(&s);
  if (rc != Z_STREAM_END) return GSKYHIP_E_ARG;
  for (size_t p = 0; p < zn; p += 32768) chunk(o, "IDAT", z.data() + p, std::min<size_t>(32768, zn - p));
  chunk(o, "IEND", nullptr, 0);
  return 0;
}

}  // namespace
}  // namespace gsky

using namespace gsky;

extern "C" {

int gskyhip_png_deflate_rows_host(const uint8_t *rows, int h, int stride, int bpp, int fixed_only, uint8_t *out,
                                  int64_t cap, int64_t *out_len) {
  if (!rows || !out || !out_len || h <= 0 || stride <= 0 || (bpp != 3 && bpp != 4) || cap < 0 ||
      (int64_t)h * stride > (1ll << 30))
    return GSKYHIP_E_ARG;
  try {
    return deflate::encode_rows_host(rows, h, stride, bpp, fixed_only ? 1 : 0, out, cap, out_len);
  } catch (...) {
    return GSKYHIP_E_ARG;
  }
}

// Workspace: the rows (filtered, or staged index rows) | per-tile offsets,
// sizes, bytes a pixel | per-row bit counts | Adler-32, zlib lengths and
// offsets | per-tile codes | the packed zlib streams (at most 9/8 of the
// rows' bytes + 16 per tile: a dynamic block is only used where it is
// shorter than the fixed one) | the rows' tokens (a dword per byte at most)
// and token counts.  `per` is a tile's slot of row bytes: max_h * (1 + 4 *
// max_w) for truecolour, max_h * (1 + max_w) in whole dwords for indexed.
static int64_t png_deflate_cap(int64_t per) { return (per * 9 + 7) / 8 + 64 + (per / 32768 + 1) * 4 + 256; }

static int64_t png_workspace(int n_tiles, int max_h, int64_t per) {
  const int64_t a = ((int64_t)n_tiles * per + 255) / 256 * 256 + (int64_t)n_tiles * (8 + 8 + 4) + 1024;
  const int64_t b = ((int64_t)n_tiles * max_h * 4 + 255) / 256 * 256 + (int64_t)n_tiles * (4 + 8 + 8) + 1024 +
                    (int64_t)n_tiles * (int64_t)sizeof(deflate::Plan) + 256;
  const int64_t c = (int64_t)n_tiles * per * 4 + (int64_t)n_tiles * max_h * 4 + 1024 +   // tokens, counts,
                    (int64_t)n_tiles * deflate::kSymN * 4 + 256;                                 // symbol frequencies
  return a + b + (int64_t)n_tiles * png_deflate_cap(per) + 1024 + c;
}

// the most bytes of a PNG over `raw` bytes of rows, `extra` bytes of chunks between IHDR and IDAT
static int64_t png_bound(int64_t raw, int64_t extra) {
  const uLong z = std::max<uLong>(compressBound((uLong)raw) + 64, (uLong)png_deflate_cap(raw));
  return 8 + 25 + extra + (int64_t)(z / 32768 + 1) * 12 + (int64_t)z + 12;
}

int64_t gskyhip_png_workspace_size(int n_tiles, int max_w, int max_h) {
  if (n_tiles <= 0 || max_w <= 0 || max_h <= 0) return 0;
  return png_workspace(n_tiles, max_h, (int64_t)max_h * (1 + 4 * (int64_t)max_w));
}

int64_t gskyhip_png_bound(int width, int height) {
  if (width <= 0 || height <= 0) return 0;
  return png_bound((int64_t)height * (1 + 4 * (int64_t)width), 0);
}

// An indexed tile's slot of the workspace: its rows of 1 + w bytes, rounded up
// to whole dwords (png_index_rows_kernel stores dwords)
static int64_t png_indexed_per(int max_w, int max_h) { return ((int64_t)max_h * (1 + (int64_t)max_w) + 3) & ~(int64_t)3; }

int64_t gskyhip_png_indexed_workspace_size(int n_tiles, int max_w, int max_h) {
  if (n_tiles <= 0 || max_w <= 0 || max_h <= 0) return 0;
  return png_workspace(n_tiles, max_h, png_indexed_per(max_w, max_h));
}

int64_t gskyhip_png_indexed_bound(int width, int height) {
  if (width <= 0 || height <= 0) return 0;
  return png_bound((int64_t)height * (1 + (int64_t)width), (12 + 768) + (12 + 256));   // + PLTE, tRNS
}

// What both encoders hand to png_finish: the call's arguments and the head of
// its workspace -- the rows of tile t at filt + t * per, then (d_off) the
// tiles' offsets, sizes and bytes a pixel.
struct PngCall {
  int n_tiles, max_h;
  int64_t per;
  const int32_t *sizes;
  const std::vector<uint8_t> *pal;   // PLTE + tRNS (indexed), or NULL
  char *ws;
  int64_t workspace_bytes;
  uint8_t *png_out;
  int64_t png_capacity;
  int64_t *png_sizes;
  int n_threads;
  hipStream_t s;
  uint8_t *filt;
  char *tail;
  int64_t *d_off;
  int32_t *d_wh, *d_px;
  std::vector<char> meta;            // the upload's source, alive until the call has synchronised
};

// carves the head of the workspace and uploads the offsets and sizes; px_bytes
// != 0: also that value as every tile's bytes a pixel (else a kernel sets them)
static int png_begin(PngCall &c, int px_bytes) {
  const int n_tiles = c.n_tiles;
  c.filt = (uint8_t *)c.ws;
  c.tail = c.ws + ((int64_t)n_tiles * c.per + 255) / 256 * 256;
  c.d_off = (int64_t *)c.tail;
  c.d_wh = (int32_t *)(c.d_off + n_tiles);
  c.d_px = c.d_wh + 2 * n_tiles;
  std::vector<char> &meta = c.meta;
  meta.resize((size_t)n_tiles * (8 + 8 + (px_bytes ? 4 : 0)));
  int64_t *off = (int64_t *)meta.data();
  for (int t = 0; t < n_tiles; t++) off[t] = (int64_t)t * c.per;
  std::memcpy(meta.data() + (size_t)n_tiles * 8, c.sizes, (size_t)n_tiles * 8);
  if (px_bytes) {
    int32_t *px = (int32_t *)(meta.data() + (size_t)n_tiles * 16);
    for (int t = 0; t < n_tiles; t++) px[t] = px_bytes;
  }
  return hipMemcpyAsync(c.d_off, meta.data(), meta.size(), hipMemcpyHostToDevice, c.s) == hipSuccess ? 0
                                                                                                       : GSKYHIP_E_HIP;
}

// Everything behind the rows: the GPU deflate of every tile, the CRC-32 of its
// IDAT chunks, one copy of the compressed bytes and the framing on host
// threads; or, for tiles of more than kPngMaxRows rows and under
// GSKYHIP_PNG_ZLIB=1, a copy of the rows and host zlib.
static int png_finish(const PngCall &c) {
  const int n_tiles = c.n_tiles, max_h = c.max_h, n_threads = c.n_threads;
  const int64_t per = c.per, workspace_bytes = c.workspace_bytes, png_capacity = c.png_capacity;
  const int32_t *sizes = c.sizes;
  const std::vector<uint8_t> *pal = c.pal;
  char *ws = c.ws, *tail = c.tail;
  uint8_t *png_out = c.png_out, *filt = c.filt;
  int64_t *png_sizes = c.png_sizes, *d_off = c.d_off;
  int32_t *d_wh = c.d_wh, *d_px = c.d_px;
  hipStream_t s = c.s;
  // GSKYHIP_PNG_ZLIB=1: deflate with zlib level 6 on host threads (round 3)
  const char *zl = std::getenv("GSKYHIP_PNG_ZLIB");
  const bool host_zlib = zl && std::atoi(zl) != 0;
  const bool trace = std::getenv("GSKYHIP_PNG_TRACE") != nullptr;
  auto now_us = [] {
    return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
  };
  const double t_start = now_us();
  if (!host_zlib && max_h <= kPngMaxRows) {
    char *b = tail + (int64_t)n_tiles * (8 + 8 + 4) + 1024;
    b = (char *)(((uintptr_t)b + 255) & ~(uintptr_t)255);
    int32_t *d_rowbits = (int32_t *)b;
    b += ((int64_t)n_tiles * max_h * 4 + 255) / 256 * 256;
    uint32_t *d_adler = (uint32_t *)b;
    int64_t *d_zlen = (int64_t *)(b + (((int64_t)n_tiles * 4 + 7) & ~(int64_t)7));
    int64_t *d_zoff = d_zlen + n_tiles;
    deflate::Plan *d_tab = (deflate::Plan *)(((uintptr_t)(d_zoff + n_tiles) + 255) & ~(uintptr_t)255);
    uint8_t *d_packed = (uint8_t *)(((uintptr_t)(d_tab + n_tiles) + 255) & ~(uintptr_t)255);
    // per-tile dynamic Huffman codes where they are shorter (GSKYHIP_PNG_FIXED=1: fixed codes only)
    const char *fx = std::getenv("GSKYHIP_PNG_FIXED");
    const int dynamic = (fx && std::atoi(fx) != 0) ? 0 : 1;
    uint32_t *d_tok = (uint32_t *)(((uintptr_t)(d_packed + (int64_t)n_tiles * png_deflate_cap(per)) + 255) &
                                   ~(uintptr_t)255);
    int32_t *d_ntok = (int32_t *)(d_tok + (int64_t)n_tiles * per);
    uint32_t *d_freq = (uint32_t *)(((uintptr_t)(d_ntok + (int64_t)n_tiles * max_h) + 255) & ~(uintptr_t)255);
    if ((char *)(d_freq + (int64_t)n_tiles * deflate::kSymN) > ws + workspace_bytes) return GSKYHIP_E_ARG;
    if (hipMemsetAsync(d_freq, 0, (size_t)n_tiles * deflate::kSymN * 4, s) != hipSuccess) return GSKYHIP_E_HIP;
    hipLaunchKernelGGL(png_tokenize_kernel, dim3((unsigned)((int64_t)n_tiles * ((max_h + 63) / 64))), dim3(64), 0, s, filt,
                       d_off, d_wh, d_px, max_h, d_tok, d_ntok, per, d_freq, dynamic);
    hipLaunchKernelGGL(png_deflate_count_kernel, dim3((unsigned)n_tiles), dim3(256), 0, s, filt, d_off, d_wh, d_px,
                       max_h, d_rowbits, d_adler, d_zlen, d_tab, dynamic, d_tok, d_ntok, per, d_freq);
    std::vector<int64_t> zlen(n_tiles), zoff(n_tiles);
    std::vector<int32_t> px(n_tiles);
    if (hipGetLastError() != hipSuccess ||
        hipMemcpyAsync(zlen.data(), d_zlen, (size_t)n_tiles * 8, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemcpyAsync(px.data(), d_px, (size_t)n_tiles * 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess)
      return GSKYHIP_E_HIP;
    const double t_count = now_us();
    int64_t total = 0, max_zlen = 0;
    for (int t = 0; t < n_tiles; t++) {
      zoff[t] = total;
      total += (zlen[t] + 3) & ~(int64_t)3;
      max_zlen = std::max(max_zlen, zlen[t]);
    }
    const int max_chunks = (int)((max_zlen + 32767) / 32768);
    if (hipMemcpyAsync(d_zoff, zoff.data(), (size_t)n_tiles * 8, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemsetAsync(d_packed, 0, (size_t)std::max<int64_t>(total, 4), s) != hipSuccess)
      return GSKYHIP_E_HIP;
    hipLaunchKernelGGL(png_deflate_write_kernel, dim3((unsigned)n_tiles), dim3(256), 0, s, d_wh, d_px, max_h,
                       d_rowbits, d_adler, d_zoff, d_packed, d_tab, d_tok, d_ntok, per);
    // IDAT CRCs behind the packed streams (the pinned read-back holds both)
    const int64_t crc_at = (total + 255) & ~(int64_t)255;
    const int64_t n_crc = (int64_t)n_tiles * max_chunks;
    if (crc_at + n_crc * 4 > (int64_t)n_tiles * png_deflate_cap(per)) return GSKYHIP_E_ARG;
    uint32_t *d_crc = (uint32_t *)(d_packed + crc_at);
    if (n_crc > 0)
      hipLaunchKernelGGL(png_idat_crc_kernel, dim3((unsigned)((n_crc + 255) / 256)), dim3(256), 0, s, d_packed, d_zoff,
                         d_zlen, n_tiles, max_chunks, d_crc);
    uint8_t *zhost = nullptr;
    const int64_t back = crc_at + n_crc * 4;
    if (hipGetLastError() != hipSuccess || hipHostMalloc((void **)&zhost, (size_t)std::max<int64_t>(back, 4),
                                                         hipHostMallocDefault) != hipSuccess)
      return GSKYHIP_E_HIP;
    if (hipStreamSynchronize(s) != hipSuccess) { hipHostFree(zhost); return GSKYHIP_E_HIP; }
    const double t_write = now_us();
    if (hipMemcpyAsync(zhost, d_packed, (size_t)back, hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess) {
      hipHostFree(zhost);
      return GSKYHIP_E_HIP;
    }
    const double t_copy = now_us();
    // PNG framing on host threads: IHDR, 32 KiB IDAT chunks with CRC-32, IEND
    std::atomic<int> next(0), err(0);
    auto frame = [&]() {
      for (;;) {
        const int t = next++;
        if (t >= n_tiles) return;
        const size_t n = png_frame(zhost + zoff[t], (size_t)zlen[t], sizes[2 * t], sizes[2 * t + 1], px[t], pal,
                                   png_out + (int64_t)t * png_capacity, (size_t)png_capacity,
                                   (const uint32_t *)(zhost + crc_at) + (int64_t)t * max_chunks);
        if (!n) err = GSKYHIP_E_ARG;
        png_sizes[t] = (int64_t)n;
      }
    };
    const int nt = std::max(1, std::min(n_threads > 0 ? n_threads : 1, n_tiles));
    std::vector<std::thread> pool;
    for (int i = 1; i < nt; i++) pool.emplace_back(frame);
    frame();
    for (auto &th : pool) th.join();
    hipHostFree(zhost);
    if (trace)
      std::fprintf(stderr, "png tiles=%d filter+count_us=%.0f write_us=%.0f d2h_us=%.0f (%.1f MB) frame_us=%.0f\n",
                   n_tiles, t_count - t_start, t_write - t_count, t_copy - t_write, total / 1e6, now_us() - t_copy);
    return err.load();
  }
  std::vector<uint8_t> host((size_t)n_tiles * per);
  std::vector<int32_t> px(n_tiles);
  if (hipMemcpyAsync(host.data(), filt, host.size(), hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipMemcpyAsync(px.data(), d_px, (size_t)n_tiles * 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return GSKYHIP_E_HIP;
  // deflate + framing per tile on host threads
  std::atomic<int> next(0), err(0);
  auto work = [&]() {
    std::vector<uint8_t> o;
    for (;;) {
      const int t = next++;
      if (t >= n_tiles) return;
      const int w = sizes[2 * t], h = sizes[2 * t + 1];
      const size_t n = (size_t)h * (1 + (size_t)px[t] * (size_t)w);
      const int rc = png_tile(host.data() + (int64_t)t * per, n, w, h, px[t], pal, o);
      if (rc || (int64_t)o.size() > png_capacity) { err = rc ? rc : GSKYHIP_E_ARG; png_sizes[t] = 0; continue; }
      std::memcpy(png_out + (int64_t)t * png_capacity, o.data(), o.size());
      png_sizes[t] = (int64_t)o.size();
    }
  };
  const int nt = std::max(1, std::min(n_threads > 0 ? n_threads : 1, n_tiles));
  std::vector<std::thread> pool;
  for (int i = 1; i < nt; i++) pool.emplace_back(work);
  work();
  for (auto &th : pool) th.join();
  return err.load();
}

int gskyhip_encode_png(const uint8_t *rgba, int n_tiles, int max_w, int max_h, int64_t tile_stride,
                       int64_t row_stride, const int32_t *sizes, void *workspace, int64_t workspace_bytes,
                       uint8_t *png_out, int64_t png_capacity, int64_t *png_sizes, int n_threads, void *stream) {
  if (n_tiles <= 0) return 0;
  if (!rgba || !sizes || !png_out || !png_sizes || max_w <= 0 || max_h <= 0 || row_stride < 4LL * max_w ||
      tile_stride < row_stride * max_h)
    return GSKYHIP_E_ARG;
  if (!workspace || workspace_bytes < gskyhip_png_workspace_size(n_tiles, max_w, max_h)) return GSKYHIP_E_ARG;
  for (int t = 0; t < n_tiles; t++) {
    const int w = sizes[2 * t], h = sizes[2 * t + 1];
    if (w <= 0 || h <= 0 || w > max_w || h > max_h || png_capacity < gskyhip_png_bound(w, h)) return GSKYHIP_E_ARG;
  }
  PngCall c;
  c.n_tiles = n_tiles; c.max_h = max_h; c.per = (int64_t)max_h * (1 + 4 * (int64_t)max_w);
  c.sizes = sizes; c.pal = nullptr; c.ws = (char *)workspace; c.workspace_bytes = workspace_bytes;
  c.png_out = png_out; c.png_capacity = png_capacity; c.png_sizes = png_sizes; c.n_threads = n_threads;
  c.s = (hipStream_t)stream;
  if (png_begin(c, 0)) return GSKYHIP_E_HIP;
  hipLaunchKernelGGL(png_opaque_kernel, dim3((unsigned)n_tiles), dim3(256), 0, c.s, rgba, tile_stride, row_stride,
                     c.d_wh, c.d_px);
  hipLaunchKernelGGL(png_filter_kernel, dim3((unsigned)((int64_t)n_tiles * max_h)), dim3(256), 0, c.s, rgba,
                     tile_stride, row_stride, c.d_wh, c.d_px, max_h, c.d_off, c.filt);
  if (hipGetLastError() != hipSuccess) return GSKYHIP_E_HIP;
  return png_finish(c);
}

// The indexed encoder: png_index_rows_kernel stages the rows, PLTE and tRNS
// are framed once on the host, and png_finish does the rest with one byte a
// pixel.
int gskyhip_encode_png_indexed(const uint8_t *index, int n_tiles, int max_w, int max_h, int64_t tile_stride,
                               int64_t row_stride, const int32_t *sizes, const uint8_t *ramp, void *workspace,
                               int64_t workspace_bytes, uint8_t *png_out, int64_t png_capacity,
                               int64_t *png_sizes, int n_threads, void *stream) {
  if (n_tiles <= 0) return 0;
  if (!index || !sizes || !png_out || !png_sizes || max_w <= 0 || max_h <= 0 || row_stride < (int64_t)max_w ||
      tile_stride < row_stride * max_h)
    return GSKYHIP_E_ARG;
  if (!workspace || ((uintptr_t)workspace & 7) ||
      workspace_bytes < gskyhip_png_indexed_workspace_size(n_tiles, max_w, max_h))
    return GSKYHIP_E_ARG;
  for (int t = 0; t < n_tiles; t++) {
    const int w = sizes[2 * t], h = sizes[2 * t + 1];
    if (w <= 0 || h <= 0 || w > max_w || h > max_h || png_capacity < gskyhip_png_indexed_bound(w, h))
      return GSKYHIP_E_ARG;
  }
  std::vector<uint8_t> pal;
  png_palette_chunks(ramp, pal);
  PngCall c;
  c.n_tiles = n_tiles; c.max_h = max_h; c.per = png_indexed_per(max_w, max_h);
  c.sizes = sizes; c.pal = &pal; c.ws = (char *)workspace; c.workspace_bytes = workspace_bytes;
  c.png_out = png_out; c.png_capacity = png_capacity; c.png_sizes = png_sizes; c.n_threads = n_threads;
  c.s = (hipStream_t)stream;
  const int64_t blocks_per_tile = (c.per / 4 + 255) / 256;
  if (blocks_per_tile * n_tiles > 0x7FFFFFFF) return GSKYHIP_E_ARG;
  if (png_begin(c, 1)) return GSKYHIP_E_HIP;
  hipLaunchKernelGGL(png_index_rows_kernel, dim3((unsigned)(blocks_per_tile * n_tiles)), dim3(256), 0, c.s, index,
                     tile_stride, row_stride, c.d_wh, (int)blocks_per_tile, c.per, c.filt);
  if (hipGetLastError() != hipSuccess) return GSKYHIP_E_HIP;
  return png_finish(c);
}

int gskyhip_encode_png_indexed_host(const uint8_t *index, int w, int h, const uint8_t *ramp, int fixed_only,
                                    uint8_t *out, int64_t cap, int64_t *out_len) {
  if (!index || !out || !out_len || w <= 0 || h <= 0 || cap < 0 || (int64_t)h * (1 + (int64_t)w) > (1ll << 30))
    return GSKYHIP_E_ARG;
  try {
    const int stride = 1 + w;
    const int64_t n = (int64_t)h * stride;
    std::vector<uint8_t> rows((size_t)n), pal;
    for (int y = 0; y < h; y++) {
      rows[(size_t)y * stride] = 0;
      std::memcpy(rows.data() + (size_t)y * stride + 1, index + (size_t)y * w, (size_t)w);
    }
    std::vector<uint8_t> z((size_t)png_deflate_cap(n));
    int64_t zn = 0;
    if (deflate::encode_rows_host(rows.data(), h, stride, 1, fixed_only ? 1 : 0, z.data(), (int64_t)z.size(), &zn))
      return GSKYHIP_E_ARG;
    png_palette_chunks(ramp, pal);
    *out_len = 8 + 25 + (int64_t)pal.size() + (zn + 32767) / 32768 * 12 + zn + 12;
    if (*out_len > cap) return GSKYHIP_E_ARG;
    const size_t wrote = png_frame(z.data(), (size_t)zn, w, h, 1, &pal, out, (size_t)cap, nullptr);
    if (!wrote) return GSKYHIP_E_ARG;
    *out_len = (int64_t)wrote;
    return 0;
  } catch (...) {
    return GSKYHIP_E_ARG;
  }
}

// ---- GeoTIFF (EncodeGdalOpen / EncodeGdal, utils/ogc_encoders.go:277-450)
int64_t gskyhip_geotiff_workspace_size(int width, int height, int n_bands, int dtype, int block_x, int block_y) {
  int ts;
  uint16_t fmt;
  if (width <= 0 || height <= 0 || n_bands <= 0 || block_x <= 0 || block_y <= 0 || tiff::sample(dtype, ts, fmt))
    return 0;
  const int64_t ntx = (width + block_x - 1) / block_x, nty = (height + block_y - 1) / block_y;
  const int64_t rows = (int64_t)n_bands * ntx * nty * block_y;
  const int64_t rb = (int64_t)block_x * ts;
  const int64_t slot = rb + rb / 128 + 2;
  return rows * (rb + slot + 4) + 8 * (int64_t)n_bands + 64 * (int64_t)n_bands + 4096;
}

// (gskyhip_geotiff_bound, the band rules and the framing: tiffwrite.cpp)
int gskyhip_encode_geotiff(const void *const *bands, int n_bands, int dtype, int width, int height,
                           const double *geot, int epsg, const double *nodata, const char *const *names,
                           int block_x, int block_y, void *workspace, int64_t workspace_bytes, uint8_t *out,
                           int64_t capacity, int64_t *size, void *stream) {
  if (!bands || !geot || !out || !size || n_bands <= 0 || n_bands > 4096) return GSKYHIP_E_ARG;
  tiff::Spec sp;
  sp.n_bands = n_bands; sp.dtype = dtype; sp.width = width; sp.height = height;
  sp.geot = geot; sp.epsg = epsg; sp.nodata = nodata; sp.names = names;
  sp.block_x = block_x; sp.block_y = block_y;
  const int bad = sp.check();
  if (bad) return bad;
  if (!workspace || workspace_bytes < gskyhip_geotiff_workspace_size(width, height, n_bands, dtype, block_x, block_y))
    return GSKYHIP_E_ARG;
  if (capacity < gskyhip_geotiff_bound(width, height, n_bands, dtype, block_x, block_y)) return GSKYHIP_E_ARG;
  const int ts = sp.ts, ntx = sp.ntx, nty = sp.nty;
  const int64_t n_tiles = sp.n_tiles();
  const int64_t n_rows = n_tiles * block_y;
  const int64_t rb = (int64_t)block_x * ts;
  const int64_t slot = rb + rb / 128 + 2;
  char *ws = (char *)workspace;
  uint8_t *raw = (uint8_t *)ws;
  uint8_t *enc = raw + n_rows * rb;
  int32_t *len = (int32_t *)(enc + n_rows * slot);
  const uint8_t **d_bands = (const uint8_t **)(((uintptr_t)(len + n_rows) + 15) & ~(uintptr_t)15);
  uint8_t *d_pad = (uint8_t *)(d_bands + n_bands);
  // the band pointers (none for an EmptyTile band: all pad) and the pad samples in one upload
  std::vector<char> meta((size_t)n_bands * 8 + (size_t)n_bands * 8, 0);
  std::memcpy(meta.data(), bands, (size_t)n_bands * 8);
  for (int b = 0; b < n_bands; b++)
    if (sp.empty[b]) std::memset(meta.data() + 8 * (size_t)b, 0, 8);
  std::memcpy(meta.data() + (size_t)n_bands * 8, sp.pad.data(), (size_t)n_bands * 8);
  hipStream_t s = (hipStream_t)stream;
  if (hipMemcpyAsync(d_bands, meta.data(), meta.size(), hipMemcpyHostToDevice, s) != hipSuccess) return GSKYHIP_E_HIP;
  hipLaunchKernelGGL(tiff_rows_kernel, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, s, d_bands, ts, width,
                     height, block_x, block_y, ntx, nty, d_pad, slot, raw, enc, len, n_rows);
  if (hipGetLastError() != hipSuccess) return GSKYHIP_E_HIP;
  std::vector<int32_t> lens((size_t)n_rows);
  std::vector<uint8_t> encs((size_t)(n_rows * slot));
  if (hipMemcpyAsync(lens.data(), len, (size_t)n_rows * 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipMemcpyAsync(encs.data(), enc, encs.size(), hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return GSKYHIP_E_HIP;
  // file: header | tile data (band-major, tiles row-major) | IFD | out-of-line tag data
  tiff::Writer W(out, capacity, n_tiles);
  for (int64_t t = 0; t < n_tiles; t++) {
    W.begin_tile();
    for (int r = 0; r < block_y; r++) {
      const int64_t i = t * block_y + r;
      W.append(encs.data() + i * slot, lens[i]);
    }
    W.end_tile();
  }
  return W.finish(sp, size);
}

// The Deflate file with the tiles predicted and deflated in HBM, a band at a
// time in slabs of tiles (deflate.hip): each slab's packed streams are copied
// straight to their place in the file.  A band without samples (EmptyTile, or
// no pointer) is one tile compressed once by the encoder's host twin (the
// same bytes) and repeated.
static int encode_geotiff_device(const tiff::Spec &sp, const void *const *bands, int zlevel, int slab_tiles,
                                 uint8_t *out, int64_t capacity, int64_t *size, int64_t *stats, hipStream_t s) {
  const int64_t tpb = sp.tiles_per_band();
  const int slab = tiff_slab_tiles(sp.tile_bytes, tpb, slab_tiles);
  const int64_t ws_bytes = tiff_deflate_workspace(sp.tile_bytes, slab);
  uint8_t *ws = nullptr;
  if (hipMalloc((void **)&ws, (size_t)ws_bytes) != hipSuccess) return GSKYHIP_E_HIP;
  int64_t st[4] = {0, 0, 0, ws_bytes};
  tiff::Writer W(out, capacity, sp.n_tiles());
  std::vector<int64_t> lens((size_t)slab);
  std::vector<uint8_t> pad_z;
  uint32_t pad_of = 0;
  int rc = 0;
  for (int b = 0; b < sp.n_bands && !rc; b++) {
    const void *band = sp.empty[b] ? nullptr : bands[b];
    if (!band) {
      if (pad_z.empty() || pad_of != sp.pad_bits(b)) {
        rc = tiff::deflate_tile(sp, nullptr, b, 0, 0, zlevel, pad_z);
        pad_of = sp.pad_bits(b);
      }
      for (int64_t t = 0; t < tpb && !rc; t++) {
        W.begin_tile();
        W.append(pad_z.data(), (int64_t)pad_z.size());
        W.end_tile();
      }
      continue;
    }
    for (int64_t t0 = 0; t0 < tpb && !rc; t0 += slab) {
      const int n = (int)std::min<int64_t>(slab, tpb - t0);
      rc = tiff_deflate_slab(band, sp.ts, sp.predictor, sp.width, sp.height, sp.block_x, sp.block_y, sp.ntx, t0, n,
                             sp.pad_bits(b), zlevel, ws, ws_bytes, W.cursor(), W.left(), lens.data(), &st[2], s);
      for (int k = 0; k < n && !rc; k++) {
        W.begin_tile();
        if (!W.room(lens[(size_t)k])) rc = GSKYHIP_E_ARG;
        W.end_tile();
      }
      st[0] += n;
    }
    st[1] += (int64_t)sp.width * sp.height * sp.ts;
  }
  (void)hipStreamSynchronize(s);
  (void)hipFree(ws);
  if (!rc) rc = W.finish(sp, size);
  if (!rc && stats) std::memcpy(stats, st, sizeof(st));
  return rc;
}

static int encode_geotiff_opts(const void *const *bands, int n_bands, int dtype, int width, int height,
                               const double *geot, int epsg, const double *nodata, const char *const *names,
                               int block_x, int block_y, int compression, int predictor, int zlevel, int deflate,
                               int slab_tiles, int n_threads, uint8_t *out, int64_t capacity, int64_t *size,
                               int64_t *stats, hipStream_t s) {
  if (stats) std::memset(stats, 0, 4 * sizeof(int64_t));
  if (!bands || !geot || !out || !size || n_bands <= 0 || n_bands > 4096) return GSKYHIP_E_ARG;
  tiff::Spec sp;
  sp.n_bands = n_bands; sp.dtype = dtype; sp.width = width; sp.height = height;
  sp.geot = geot; sp.epsg = epsg; sp.nodata = nodata; sp.names = names;
  sp.block_x = block_x; sp.block_y = block_y; sp.compression = compression; sp.predictor = predictor;
  const int bad = sp.check();
  if (bad) return bad;
  if (zlevel < 0 || zlevel > 9 || (deflate != GSKYHIP_DEFLATE_HOST && deflate != GSKYHIP_DEFLATE_DEVICE) ||
      slab_tiles < 0)
    return GSKYHIP_E_ARG;
  if (capacity < gskyhip_geotiff_bound_opts(width, height, n_bands, dtype, block_x, block_y, compression))
    return GSKYHIP_E_ARG;
  if (deflate == GSKYHIP_DEFLATE_HOST) {   // one copy of every band to the host, then the host writer
    const size_t nb = (size_t)width * height * sp.ts;
    std::vector<std::vector<uint8_t>> host((size_t)n_bands);
    std::vector<const void *> ptrs((size_t)n_bands, nullptr);
    for (int b = 0; b < n_bands; b++) {
      if (!bands[b] || sp.empty[b]) continue;
      host[b].resize(nb);
      if (hipMemcpyAsync(host[b].data(), bands[b], nb, hipMemcpyDeviceToHost, s) != hipSuccess) return GSKYHIP_E_HIP;
      ptrs[b] = host[b].data();
    }
    if (hipStreamSynchronize(s) != hipSuccess) return GSKYHIP_E_HIP;
    return tiff::encode_host(sp, ptrs.data(), zlevel, n_threads, out, capacity, size);
  }
  if (compression == GSKYHIP_TIFF_PACKBITS) {   // the unchanged writer, on a workspace of this call's
    const int64_t ws_bytes = gskyhip_geotiff_workspace_size(width, height, n_bands, dtype, block_x, block_y);
    void *ws = nullptr;
    if (hipMalloc(&ws, (size_t)ws_bytes) != hipSuccess) return GSKYHIP_E_HIP;
    const int rc = gskyhip_encode_geotiff(bands, n_bands, dtype, width, height, geot, epsg, nodata, names, block_x,
                                          block_y, ws, ws_bytes, out, capacity, size, s);
    (void)hipStreamSynchronize(s);
    (void)hipFree(ws);
    if (!rc && stats) stats[3] = ws_bytes;
    return rc;
  }
  return encode_geotiff_device(sp, bands, zlevel, slab_tiles, out, capacity, size, stats, s);
}

int gskyhip_encode_geotiff_opts(const void *const *bands, int n_bands, int dtype, int width, int height,
                                const double *geot, int epsg, const double *nodata, const char *const *names,
                                int block_x, int block_y, int compression, int predictor, int zlevel, int deflate,
                                int slab_tiles, int n_threads, uint8_t *out, int64_t capacity, int64_t *size,
                                int64_t *stats, void *stream) {
  try {
    return encode_geotiff_opts(bands, n_bands, dtype, width, height, geot, epsg, nodata, names, block_x, block_y,
                               compression, predictor, zlevel, deflate, slab_tiles, n_threads, out, capacity, size,
                               stats, (hipStream_t)stream);
  } catch (...) {
    return GSKYHIP_E_HIP;
  }
}

}  // extern "C"
