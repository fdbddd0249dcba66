// deflate_core.h -- the one Deflate encoder (RFC 1950 / 1951), compiled for
// the host and for the device: two tokenisers (a segment of an
// independent block; a row of a PNG image), the length-limited Huffman
// construction, the block plan in parts (build_dynamic, finish_plan) with each
// user's choice of block type on top (plan_block: the smallest of dynamic /
// fixed / stored; plan_png: fixed or dynamic), the header writer and the bit
// sink.  deflate.hip runs these functions with a lane per segment and a wave
// per block, encode.hip with a thread per image row and a workgroup per tile;
// the host twins (encode_block_host, encode_rows_host) run the same functions
// in a loop, so each gives its device's bytes.
//
// A block of n bytes is cut into segments of kSeg bytes.  A segment's tokens
// depend only on the block's bytes: a match starts and ends inside its
// segment and may reach back to any earlier byte of the block (the encoder
// looks at distance 1 -- runs -- and at the last position of the same 3-byte
// hash inside the segment, so no distance exceeds kSeg).  The tokens are
// kept one dword each; the block's code comes from their histogram; every
// segment's bits then go to its own bit offset of a zeroed word buffer, the
// words two segments share by OR.
//
// Bounds: a segment reads data[0, n) only (match compares stay below the
// segment end), writes at most kSeg tokens, and the sink writes only words
// below (stream bytes + 3) / 4 of its buffer.
#ifndef GSKY_DEFLATE_CORE_H
#define GSKY_DEFLATE_CORE_H

#include <stdint.h>
#include <string.h>

#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GSKY_DF_HD __host__ __device__ inline
#else
#define GSKY_DF_HD inline
#endif

namespace gsky {
namespace deflate {

constexpr int kSeg = 256;        // bytes of a segment (one lane)
constexpr int kHashBits = 6;     // per-segment table of 3-byte hashes
constexpr int kHashN = 1 << kHashBits;
constexpr int kLitN = 286, kDistN = 30, kClN = 19, kSymN = kLitN + kDistN;
constexpr int kHdrWords = 160;   // room of a dynamic block header (at most 4.5 kbit)
constexpr uint32_t kAdlerMod = 65521u;
constexpr int kStoredMax = 65535;
// FLG of the zlib header after CMF 0x78, (0x78 * 256 + FLG) % 31 == 0: default level / fastest
constexpr uint32_t kFlgDefault = 0x9C, kFlgFastest = 0x01;

enum Mode { kDynamic = 0, kFixed = 1, kStored = 2 };
enum Status { kOk = 0, kOutputFull = 5 };   // GSKYHIP_INFLATE_OK, GSKYHIP_INFLATE_E_CAP

// RFC 1951 3.2.5 as functions (no tables: the same text serves both sides)
GSKY_DF_HD int len_extra(int lc) { return lc < 4 || lc == 28 ? 0 : (lc - 4) >> 2; }
GSKY_DF_HD int len_base(int lc) {
  if (lc < 8) return 3 + lc;
  if (lc == 28) return 258;
  const int e = (lc - 4) >> 2;
  return 3 + ((4 + (lc & 3)) << e);
}
GSKY_DF_HD int len_code(int l) {   // 3 <= l <= 258
  if (l < 11) return l - 3;
  if (l == 258) return 28;
  const int v = l - 3;
  const int e = 29 - __builtin_clz((unsigned)v);   // floor(log2 v) - 2
  return 4 * e + 4 + ((v >> e) & 3);
}
GSKY_DF_HD int dist_extra(int dc) { return dc < 2 ? 0 : (dc - 2) >> 1; }
GSKY_DF_HD int dist_base(int dc) {
  if (dc < 4) return 1 + dc;
  const int e = (dc - 2) >> 1;
  return 1 + ((2 + (dc & 1)) << e);
}
GSKY_DF_HD int dist_code(int d) {   // 1 <= d <= 32768
  if (d < 5) return d - 1;
  const int v = d - 1;
  const int e = 30 - __builtin_clz((unsigned)v);   // floor(log2 v) - 1
  return 2 * e + 2 + ((v >> e) & 1);
}

GSKY_DF_HD uint32_t rev_bits(uint32_t code, int len) {
  uint32_t r = 0;
  for (int i = 0; i < len; i++) r |= ((code >> i) & 1u) << (len - 1 - i);
  return r;
}

// fixed code of a literal / length symbol (3.2.6), not yet reversed
GSKY_DF_HD void fixed_lit(int v, uint32_t &code, int &len) {
  if (v < 144) { code = 0x30 + v; len = 8; }
  else if (v < 256) { code = 0x190 + (v - 144); len = 9; }
  else if (v < 280) { code = v - 256; len = 7; }
  else { code = 0xC0 + (v - 280); len = 8; }
}

typedef uint32_t u32_unaligned __attribute__((aligned(1)));
GSKY_DF_HD uint32_t ld_u32(const uint8_t *p) { return *(const u32_unaligned *)p; }

// token: symbol (9 bits) | distance code + 1 (5) | length extra (5) | distance extra (13)
GSKY_DF_HD uint32_t tok_pack(int sym, uint32_t lx, int dc, uint32_t dx) {
  return (uint32_t)sym | ((uint32_t)(dc + 1) << 9) | (lx << 14) | (dx << 19);
}

// the token of a literal byte / of a match of length l at distance d; add(sym)
// counts a literal / length symbol, add(kLitN + dc) a distance symbol
template <class Add> GSKY_DF_HD uint32_t literal_token(uint8_t byte, Add &&add) {
  add((int)byte);
  return tok_pack((int)byte, 0u, -1, 0u);
}
template <class Add> GSKY_DF_HD uint32_t match_token(int l, int d, Add &&add) {
  const int lc = len_code(l), dc = dist_code(d);
  add(257 + lc);
  add(kLitN + dc);
  return tok_pack(257 + lc, (uint32_t)(l - len_base(lc)), dc, (uint32_t)(d - dist_base(dc)));
}

// length of the match of data[p ..) with data[p - d ..), at most lim
GSKY_DF_HD int match_len(const uint8_t *data, int64_t p, int d, int lim) {
  int l = 0;
  while (l + 4 <= lim) {
    const uint32_t x = ld_u32(data + p + l) ^ ld_u32(data + p + l - d);
    if (x) return l + (__builtin_ctz(x) >> 3);
    l += 4;
  }
  while (l < lim && data[p + l] == data[p + l - d]) l++;
  return l;
}

GSKY_DF_HD uint32_t hash3(const uint8_t *p) {
  const uint32_t v = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
  return (v * 0x9E3779B1u) >> (32 - kHashBits);
}

// The tokens of segment [p0, p1) of a block data[0, n): tok[0 .. return).
// hash[i * hstride], i < kHashN, is the caller's table for this segment
// (positions relative to p0, plus one; any content on entry).  add(sym)
// counts a literal / length symbol, add(kLitN + dc) a distance symbol.
template <class Add>
GSKY_DF_HD int tokenize_segment(const uint8_t *data, int64_t p0, int64_t p1, uint32_t *tok, uint16_t *hash,
                                int hstride, Add &&add) {
  for (int i = 0; i < kHashN; i++) hash[i * hstride] = 0;
  int n = 0;
  int64_t p = p0;
  while (p < p1) {
    const int lim = (int)(p1 - p < 258 ? p1 - p : 258);
    int best = 0, bd = 0;
    if (lim >= 3) {
      if (p >= 1) {
        best = match_len(data, p, 1, lim);
        bd = 1;
      }
      uint16_t *slot = &hash[hash3(data + p) * hstride];
      const int q = (int)*slot - 1;
      *slot = (uint16_t)(p - p0 + 1);
      if (q >= 0 && best < lim) {
        const int d = (int)(p - p0) - q;
        const int l = match_len(data, p, d, lim);
        if (l > best) { best = l; bd = d; }
      }
    }
    if (best >= 3) {
      tok[n++] = match_token(best, bd, add);
      if (best <= 16)   // short matches keep the table fresh; long runs need no entries
        for (int64_t r = p + 1; r < p + best && r + 3 <= p1; r++) hash[hash3(data + r) * hstride] = (uint16_t)(r - p0 + 1);
      p += best;
    } else {
      tok[n++] = literal_token(data[p], add);
      p++;
    }
  }
  return n;
}

// The PNG encoder's matcher, over rows of `stride` filtered bytes (bpp bytes a
// pixel): the candidates at p are the distances a PNG of upsampled tiles
// repeats at -- runs (1), the pixel to the left and 2-3 pixels back, the
// pixels above (1-3 rows) and the diagonals --, the one saving the most bits
// by a static estimate wins (6.5 bits per literal byte against ~7 bits of
// length code plus the distance code and its extra bits).  A match ends
// before p1 and reaches back to data[0] at most, never past the window.
GSKY_DF_HD void row_best_match(const uint8_t *data, int64_t p, int64_t p1, int bpp, int stride, int &best, int &bd) {
  best = 0;
  bd = 0;
  int bscore = -(1 << 30);
  const int dists[11] = {1, bpp, stride, 2 * bpp, 3 * bpp, 2 * stride, stride - bpp, stride + bpp,
                         2 * stride - bpp, 2 * stride + bpp, 3 * stride};
  const int lim = (int)(p1 - p < 258 ? p1 - p : 258);
#pragma unroll
  for (int c = 0; c < 11; c++) {
    const int d = dists[c];
    if (d < 1 || p - d < 0 || d > 32768) continue;   // (d < 1: only rows shorter than a pixel)
    const int l = match_len(data, p, d, lim);
    if (l < 3) continue;
    const int score = 13 * l - 2 * (7 + 5 + dist_extra(dist_code(d)));   // 2x the bits saved
    if (score > bscore) { bscore = score; best = l; bd = d; }
  }
}

// The tokens of row [p0, p1) of an image data[0 ..): tok[0 .. return), at
// most p1 - p0 of them; add() as in tokenize_segment.  One step of lazy
// matching: a match starting one byte later that is 2+ bytes longer wins, the
// byte going out as a literal.
template <class Add>
GSKY_DF_HD int tokenize_row(const uint8_t *data, int64_t p0, int64_t p1, int bpp, int stride, uint32_t *tok,
                            Add &&add) {
  int n = 0;
  int64_t p = p0;
  while (p < p1) {
    int best, bd;
    row_best_match(data, p, p1, bpp, stride, best, bd);
    if (best >= 3 && p + 1 < p1) {
      int b2, d2;
      row_best_match(data, p + 1, p1, bpp, stride, b2, d2);
      if (b2 > best + 1) {
        tok[n++] = literal_token(data[p], add);
        p++;
        best = b2;
        bd = d2;
      }
    }
    if (best >= 3) {
      tok[n++] = match_token(best, bd, add);
      p += best;
    } else {
      tok[n++] = literal_token(data[p], add);
      p++;
    }
  }
  return n;
}

// ---------------------------------------------------------------- Huffman
struct HuffScratch {
  uint32_t weight[2 * kLitN];
  int16_t sorted[kLitN];
  int16_t parent[2 * kLitN];
  uint8_t depth[2 * kLitN];
  int32_t bl_count[16], next[16];   // codes per length, next code of a length (not on a lane's stack)
};

// Code lengths <= maxbits for n symbols (n <= kLitN): a Huffman tree by the
// two-queue merge over the leaves sorted by (frequency, symbol), lengths past
// maxbits folded back as zlib's gen_bitlen does, the least frequent symbols
// taking the longest codes.  A code needs two leaves: unused symbols are
// given weight 1 until there are two.  Returns 1 if the lengths are a
// complete prefix code; *limited is set when the fold ran.
GSKY_DF_HD int huff_lengths(const uint32_t *freq, int n, int maxbits, uint8_t *len, HuffScratch &H, int *limited) {
  int m = 0;
  for (int s = 0; s < n; s++) {
    len[s] = 0;
    if (freq[s]) m++;
  }
  int forced0 = -1, forced1 = -1;
  for (int s = 0; m < 2 && s < n; s++)
    if (!freq[s]) {
      if (forced0 < 0) forced0 = s; else forced1 = s;
      m++;
    }
  auto wf = [&](int s) -> uint32_t { return freq[s] ? freq[s] : ((s == forced0 || s == forced1) ? 1u : 0u); };
  // the leaves sorted by (weight, symbol): a Shell sort (gaps 121, 40, 13, 4,
  // 1), since one thread sorts up to 286 leaves; no two keys are equal, so the
  // order is the only one
  int k = 0;
  for (int s = 0; s < n; s++)
    if (wf(s)) { H.weight[k] = wf(s); H.sorted[k++] = (int16_t)s; }
  for (int gap = 121; gap > 0; gap /= 3)
    for (int j = gap; j < m; j++) {
      const uint32_t w = H.weight[j];
      const int16_t s = H.sorted[j];
      int i = j;
      for (; i >= gap && (H.weight[i - gap] > w || (H.weight[i - gap] == w && H.sorted[i - gap] > s)); i -= gap) {
        H.weight[i] = H.weight[i - gap];
        H.sorted[i] = H.sorted[i - gap];
      }
      H.weight[i] = w;
      H.sorted[i] = s;
    }
  int il = 0, in = m, nx = m;
  for (int j = 0; j < m - 1; j++) {
    int a, b;
    if (il < m && (in >= nx || H.weight[il] <= H.weight[in])) a = il++; else a = in++;
    if (il < m && (in >= nx || H.weight[il] <= H.weight[in])) b = il++; else b = in++;
    H.weight[nx] = H.weight[a] + H.weight[b];
    H.parent[a] = (int16_t)nx;
    H.parent[b] = (int16_t)nx;
    nx++;
  }
  const int root = nx - 1;
  int32_t *bl_count = H.bl_count;
  // (the loops over code lengths stay rolled: unrolled, they hold the counters in ~40 registers a lane)
#pragma nounroll
  for (int b = 0; b < 16; b++) bl_count[b] = 0;
  int overflow = 0;
  H.depth[root] = 0;
  for (int i = root - 1; i >= 0; i--) {
    const int d = H.depth[H.parent[i]] + 1;
    H.depth[i] = (uint8_t)(d < 255 ? d : 255);
    // every node past maxbits counts, internal ones too: k leaves under a node
    // at maxbits come with k - 2 internal nodes and need k - 1 moves
    if (d > maxbits) overflow++;
    if (i < m) bl_count[d < maxbits ? d : maxbits]++;
  }
  if (overflow > 0 && limited) *limited = 1;
  while (overflow > 0) {
    int bits = maxbits - 1;
    while (bits > 0 && bl_count[bits] == 0) bits--;
    if (bits == 0) break;
    bl_count[bits]--;
    bl_count[bits + 1] += 2;
    bl_count[maxbits]--;
    overflow -= 2;
  }
  int i = 0;
#pragma nounroll
  for (int bits = maxbits; bits >= 1; bits--)
    for (int c = bl_count[bits]; c > 0 && i < m; c--) len[H.sorted[i++]] = (uint8_t)bits;
  uint64_t kraft = 0;
  for (int s = 0; s < n; s++)
    if (len[s]) kraft += 1ull << (maxbits - len[s]);
  return (i == m && kraft == (1ull << maxbits)) ? 1 : 0;
}

// canonical codes (3.2.2), bit-reversed for LSB-first output
GSKY_DF_HD void huff_codes(const uint8_t *len, int n, uint16_t *code, HuffScratch &H) {
  int32_t *bl = H.bl_count, *next = H.next;
#pragma nounroll
  for (int b = 0; b < 16; b++) bl[b] = 0;
  for (int s = 0; s < n; s++) bl[len[s]]++;
  bl[0] = 0;
  int c = 0;
  next[0] = 0;
#pragma nounroll
  for (int b = 1; b < 16; b++) { c = (c + bl[b - 1]) << 1; next[b] = c; }
  for (int s = 0; s < n; s++) code[s] = len[s] ? (uint16_t)rev_bits((uint32_t)next[len[s]]++, len[s]) : 0;
}

// ---------------------------------------------------------------- the block plan
struct Plan {
  uint32_t hdr[kHdrWords];   // block header, LSB-first: BFINAL, BTYPE and (dynamic) the code lengths
  uint16_t code[kSymN];      // literal / length codes, then distance codes, bit-reversed
  uint8_t len[kSymN];
  int32_t hdr_bits;
  int32_t mode;              // Mode
  int32_t limited;           // the length limiter ran (diagnostic)
  int64_t body_bits;         // the tokens' bits under the chosen code, end of block excluded
  int64_t stream_bytes;      // the whole stream, wrapper included
};

struct PlanScratch {
  HuffScratch H;
  uint32_t clf[kClN];
  uint8_t cll[kClN];
  uint16_t clc[kClN];
  uint8_t rs[kSymN], rx[kSymN];   // the code lengths run-length coded: symbols, extra values
};

GSKY_DF_HD int64_t stored_bytes(int64_t n) {
  const int64_t nb = n == 0 ? 1 : (n + kStoredMax - 1) / kStoredMax;
  return n + 5 * nb;
}

GSKY_DF_HD int cl_order(int k) {
  const uint8_t o[kClN] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  return o[k];
}

// What the dynamic code of a histogram costs, beside the fixed code: bits of
// the tokens with the end of block (the extra bits in both), bits of the
// dynamic header, and what finish_plan needs to write that header.
struct DynCode {
  int64_t dyn_bits, fix_bits, hdr_bits;
  int32_t ok;        // the lengths are complete prefix codes and the header fits Plan::hdr
  int32_t limited;   // the length limiter ran
  int32_t hlit, hdist, hclen, nr;
};

// The dynamic code of the histogram freq (freq[256] is set to 1 here: the end
// of block): its lengths into P.len, the code-length code and the run-length
// coded lengths into S.
GSKY_DF_HD DynCode build_dynamic(uint32_t *freq, Plan &P, PlanScratch &S) {
  freq[256] = 1;
  int64_t extra = 0;
  for (int lc = 0; lc < 29; lc++) extra += (int64_t)freq[257 + lc] * len_extra(lc);
  for (int dc = 0; dc < kDistN; dc++) extra += (int64_t)freq[kLitN + dc] * dist_extra(dc);
  int limited = 0;
  int ok = huff_lengths(freq, kLitN, 15, P.len, S.H, &limited);
  ok &= huff_lengths(freq + kLitN, kDistN, 15, P.len + kLitN, S.H, &limited);
  int hlit = kLitN, hdist = kDistN;
  while (hlit > 257 && !P.len[hlit - 1]) hlit--;
  while (hdist > 1 && !P.len[kLitN + hdist - 1]) hdist--;
  for (int k = 0; k < kClN; k++) S.clf[k] = 0;
  const int N = hlit + hdist;
  int nr = 0;
  for (int i = 0; i < N;) {
    auto L = [&](int j) { return (int)(j < hlit ? P.len[j] : P.len[kLitN + j - hlit]); };
    auto emit = [&](int sym, int x) { S.rs[nr] = (uint8_t)sym; S.rx[nr] = (uint8_t)x; nr++; S.clf[sym]++; };
    const int v = L(i);
    int run = 1;
    while (i + run < N && L(i + run) == v) run++;
    int r = run;
    if (v == 0) {
      while (r >= 11) { const int k = r < 138 ? r : 138; emit(18, k - 11); r -= k; }
      if (r >= 3) { emit(17, r - 3); r = 0; }
      while (r > 0) { emit(0, 0); r--; }
    } else {
      emit(v, 0); r--;
      while (r >= 3) { const int k = r < 6 ? r : 6; emit(16, k - 3); r -= k; }
      while (r > 0) { emit(v, 0); r--; }
    }
    i += run;
  }
  ok &= huff_lengths(S.clf, kClN, 7, S.cll, S.H, &limited);
  int hclen = kClN;
  while (hclen > 4 && !S.cll[cl_order(hclen - 1)]) hclen--;
  int64_t hb = 3 + 5 + 5 + 4 + 3 * hclen;
  for (int k = 0; k < nr; k++) {
    const int sym = S.rs[k];
    hb += S.cll[sym] + (sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0);
  }
  int64_t dyn = extra, fix = extra;
  for (int v = 0; v < kLitN; v++) {
    uint32_t c;
    int l;
    fixed_lit(v, c, l);
    dyn += (int64_t)freq[v] * P.len[v];
    fix += (int64_t)freq[v] * l;
  }
  for (int d = 0; d < kDistN; d++) {
    dyn += (int64_t)freq[kLitN + d] * P.len[kLitN + d];
    fix += (int64_t)freq[kLitN + d] * 5;
  }
  return {dyn, fix, hb, ok && hb <= (int64_t)kHdrWords * 32, limited, hlit, hdist, hclen, nr};
}

// The plan of a block in `mode` (kDynamic after build_dynamic, which D comes
// from, or kFixed): the codes and the block header.  The body's bits and the
// stream's length are the caller's to set (set_body).
GSKY_DF_HD void finish_plan(Plan &P, PlanScratch &S, const DynCode &D, int mode) {
  P.mode = mode;
  if (mode == kFixed) {
    for (int v = 0; v < kLitN; v++) {
      uint32_t c;
      int l;
      fixed_lit(v, c, l);
      P.code[v] = (uint16_t)rev_bits(c, l);
      P.len[v] = (uint8_t)l;
    }
    for (int d = 0; d < kDistN; d++) { P.code[kLitN + d] = (uint16_t)rev_bits((uint32_t)d, 5); P.len[kLitN + d] = 5; }
    P.hdr[0] = 0x3u;   // BFINAL 1, BTYPE 01
    P.hdr_bits = 3;
    P.limited = 0;
    return;
  }
  P.limited = D.limited;
  huff_codes(P.len, kLitN, P.code, S.H);
  huff_codes(P.len + kLitN, kDistN, P.code + kLitN, S.H);
  huff_codes(S.cll, kClN, S.clc, S.H);
  uint64_t acc = 0;
  int nacc = 0, word = 0;
  auto put = [&](uint32_t bits, int nb) {
    acc |= (uint64_t)bits << nacc;
    nacc += nb;
    if (nacc >= 32) { P.hdr[word++] = (uint32_t)acc; acc >>= 32; nacc -= 32; }
  };
  put(0x5u, 3);   // BFINAL 1, BTYPE 10
  put((uint32_t)(D.hlit - 257), 5);
  put((uint32_t)(D.hdist - 1), 5);
  put((uint32_t)(D.hclen - 4), 4);
  for (int k = 0; k < D.hclen; k++) put(S.cll[cl_order(k)], 3);
  for (int k = 0; k < D.nr; k++) {
    const int sym = S.rs[k];
    put(S.clc[sym], S.cll[sym]);
    if (sym == 16) put(S.rx[k], 2);
    else if (sym == 17) put(S.rx[k], 3);
    else if (sym == 18) put(S.rx[k], 7);
  }
  if (nacc > 0) P.hdr[word] = (uint32_t)acc;
  P.hdr_bits = (int32_t)D.hdr_bits;
}

// body_bits: the tokens' bits under the plan's code; wrap: bytes around the block (zlib: 6)
GSKY_DF_HD void set_body(Plan &P, int64_t body_bits, int64_t wrap) {
  P.body_bits = body_bits;
  P.stream_bytes = wrap + (P.hdr_bits + body_bits + P.len[256] + 7) / 8;
}

// The plan of an independent block of n bytes whose tokens have the histogram
// freq: the shortest stream in bytes of stored, fixed and dynamic, ties in
// that order.  level 0: stored blocks.
GSKY_DF_HD void plan_block(uint32_t *freq, int64_t n, int zlib_wrapper, int level, Plan &P, PlanScratch &S) {
  const int64_t wrap = zlib_wrapper ? 6 : 0;
  DynCode D = {};
  if (level != 0) D = build_dynamic(freq, P, S);
  // the three candidates in bytes (the bodies include the end of block)
  const int64_t stored = stored_bytes(n);
  const int64_t dyn_bytes = D.ok ? (D.hdr_bits + D.dyn_bits + 7) / 8 : INT64_MAX;
  const int64_t fix_bytes = level != 0 ? (3 + D.fix_bits + 7) / 8 : INT64_MAX;
  if (stored <= dyn_bytes && stored <= fix_bytes) {
    P.mode = kStored;
    P.limited = 0;
    P.hdr_bits = 0;
    P.body_bits = 0;
    P.stream_bytes = stored + wrap;
  } else if (fix_bytes <= dyn_bytes) {
    finish_plan(P, S, D, kFixed);
    set_body(P, D.fix_bits - 7, wrap);
  } else {
    finish_plan(P, S, D, kDynamic);
    set_body(P, D.dyn_bits - P.len[256], wrap);
  }
}

// The PNG encoder's plan of a tile: never stored; the fixed code iff it is
// asked for, the dynamic code is unusable, or the fixed block is not longer
// in bits, header included.  The body's bits come with the rows (set_body).
GSKY_DF_HD void plan_png(uint32_t *freq, int fixed_only, Plan &P, PlanScratch &S) {
  DynCode D = {};
  if (!fixed_only) D = build_dynamic(freq, P, S);
  finish_plan(P, S, D, !D.ok || 3 + D.fix_bits <= D.hdr_bits + D.dyn_bits ? kFixed : kDynamic);
}

// ---------------------------------------------------------------- the bit sink
// LSB-first bit writer over the 32-bit words of a zeroed buffer; the first
// and the last word of a piece are shared with its neighbours and go in by
// OR (atomic on the device, where the neighbours are other lanes).
GSKY_DF_HD void or_word(uint32_t *p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicOr(p, v);
#else
  *p |= v;
#endif
}

struct BitSink {
  uint32_t *out;
  uint64_t acc;
  int nacc;
  int64_t word;
  bool first;
  GSKY_DF_HD void init(uint32_t *o, int64_t bitpos) {
    out = o; word = bitpos >> 5; nacc = (int)(bitpos & 31); acc = 0; first = true;
  }
  GSKY_DF_HD void put(uint32_t bits, int n) {
    acc |= (uint64_t)bits << nacc;
    nacc += n;
    if (nacc >= 32) {
      if (first) { or_word(out + word, (uint32_t)acc); first = false; }
      else out[word] = (uint32_t)acc;
      acc >>= 32;
      nacc -= 32;
      word++;
    }
  }
  GSKY_DF_HD void finish() {
    if (nacc > 0) or_word(out + word, (uint32_t)acc);
  }
};

// bits of a segment's tokens under the plan's code
GSKY_DF_HD uint32_t segment_bits(const uint32_t *tok, int n, const uint8_t *len) {
  uint32_t b = 0;
  for (int i = 0; i < n; i++) {
    const uint32_t v = tok[i];
    const int sym = (int)(v & 511u), dc = (int)((v >> 9) & 31u) - 1;
    b += len[sym];
    if (dc >= 0) b += (uint32_t)len_extra(sym - 257) + len[kLitN + dc] + (uint32_t)dist_extra(dc);
  }
  return b;
}

// a segment's tokens at bit `bitpos` of the stream's words
GSKY_DF_HD void write_segment(const uint32_t *tok, int n, const uint16_t *code, const uint8_t *len, uint32_t *words,
                              int64_t bitpos) {
  BitSink bs;
  bs.init(words, bitpos);
  for (int i = 0; i < n; i++) {
    const uint32_t v = tok[i];
    const int sym = (int)(v & 511u), dc = (int)((v >> 9) & 31u) - 1;
    bs.put(code[sym], len[sym]);
    if (dc >= 0) {
      const int le = len_extra(sym - 257), de = dist_extra(dc);
      if (le) bs.put((v >> 14) & 31u, le);
      bs.put(code[kLitN + dc], len[kLitN + dc]);
      if (de) bs.put(v >> 19, de);
    }
  }
  bs.finish();
}

GSKY_DF_HD void or_byte(uint32_t *words, int64_t pos, uint32_t v) {
  or_word(words + (pos >> 2), (v & 0xFFu) << (8 * (int)(pos & 3)));
}

// What one writer adds around the segments of a Huffman-coded stream: the
// zlib header (CMF 0x78: deflate, 32 KiB window; then flg, a kFlg* value),
// the block header, the end of block and the Adler-32.
GSKY_DF_HD void write_frame(const Plan &P, int zlib_wrapper, uint32_t flg, uint32_t adler, uint32_t *words) {
  const int64_t base = zlib_wrapper ? 16 : 0;
  if (zlib_wrapper) {
    or_byte(words, 0, 0x78);
    or_byte(words, 1, flg);
  }
  BitSink bs;
  bs.init(words, base);
  int k = 0;
  for (; k + 32 <= P.hdr_bits; k += 32) bs.put(P.hdr[k >> 5], 32);
  if (k < P.hdr_bits) bs.put(P.hdr[k >> 5] & ((1u << (P.hdr_bits - k)) - 1u), P.hdr_bits - k);
  bs.finish();
  const int64_t eob = base + P.hdr_bits + P.body_bits;
  bs.init(words, eob);
  bs.put(P.code[256], P.len[256]);
  bs.finish();
  if (zlib_wrapper) {
    const int64_t end = (eob + P.len[256] + 7) / 8;
    or_byte(words, end, adler >> 24);
    or_byte(words, end + 1, adler >> 16);
    or_byte(words, end + 2, adler >> 8);
    or_byte(words, end + 3, adler);
  }
}

// byte j of the stream of stored blocks over data[0, n)
GSKY_DF_HD uint8_t stored_byte(int64_t j, const uint8_t *data, int64_t n, int zlib_wrapper, uint32_t adler) {
  if (zlib_wrapper) {
    if (j == 0) return 0x78;
    if (j == 1) return kFlgDefault;
    j -= 2;
  }
  const int64_t body = stored_bytes(n);
  if (j >= body) return (uint8_t)(adler >> (8 * (3 - (int)(j - body))));
  const int64_t q = j / (kStoredMax + 5), r = j % (kStoredMax + 5);
  if (r >= 5) return data[q * kStoredMax + r - 5];
  const int64_t left = n - q * kStoredMax;
  const uint32_t L = (uint32_t)(left < kStoredMax ? left : kStoredMax);
  const bool last = left <= kStoredMax;
  switch ((int)r) {
    case 0: return last ? 1 : 0;   // BFINAL, BTYPE 00, padding
    case 1: return (uint8_t)L;
    case 2: return (uint8_t)(L >> 8);
    case 3: return (uint8_t)~L;
    default: return (uint8_t)(~L >> 8);
  }
}

GSKY_DF_HD uint32_t adler32_serial(const uint8_t *data, int64_t n) {
  uint32_t a = 1, b = 0;
  int64_t i = 0;
  while (i < n) {
    const int64_t e = n - i < 5552 ? n : i + 5552;
    for (; i < e; i++) { a += data[i]; b += a; }
    a %= kAdlerMod;
    b %= kAdlerMod;
  }
  return (b << 16) | a;
}

GSKY_DF_HD int64_t bound(int64_t n) { return n + 5 * (n / 65535 + 1) + 6; }

// words of the staging buffer a block's Huffman-coded stream needs
GSKY_DF_HD int64_t stage_words(int64_t n) { return (bound(n) + 3) / 4 + 1; }

// One block on the host: the functions above, segment after segment.
// *out_len is the stream's length; kOutputFull (nothing written) when it
// exceeds cap.  *limited (may be NULL) is set when the code-length limiter
// shaped the code that was used.
inline void encode_block_host(const uint8_t *src, int64_t n, uint8_t *dst, int64_t cap, int zlib_wrapper, int level,
                              int32_t *status, int64_t *out_len, int *limited) {
  const int64_t nseg = (n + kSeg - 1) / kSeg;
  std::vector<uint32_t> tok((size_t)(level ? n : 0));
  std::vector<uint16_t> ntok((size_t)(level ? nseg : 0));
  std::vector<uint32_t> freq(kSymN, 0u);
  uint16_t hash[kHashN];
  if (level)
    for (int64_t seg = 0; seg < nseg; seg++) {
      const int64_t p0 = seg * kSeg, p1 = p0 + kSeg < n ? p0 + kSeg : n;
      ntok[(size_t)seg] =
          (uint16_t)tokenize_segment(src, p0, p1, tok.data() + p0, hash, 1, [&](int sym) { freq[(size_t)sym]++; });
    }
  std::vector<Plan> Pv(1);
  std::vector<PlanScratch> Sv(1);
  Plan &P = Pv[0];
  plan_block(freq.data(), n, zlib_wrapper, level, P, Sv[0]);
  if (limited) *limited = P.limited;
  const uint32_t adler = zlib_wrapper ? adler32_serial(src, n) : 1u;
  const int64_t total = P.stream_bytes;
  *out_len = total;
  if (total > cap) {
    *status = kOutputFull;
    return;
  }
  *status = kOk;
  if (P.mode == kStored) {
    for (int64_t j = 0; j < total; j++) dst[j] = stored_byte(j, src, n, zlib_wrapper, adler);
    return;
  }
  std::vector<uint32_t> words((size_t)((total + 3) / 4), 0u);   // exactly the stream: a write past it is out of bounds
  write_frame(P, zlib_wrapper, kFlgDefault, adler, words.data());
  int64_t at = (zlib_wrapper ? 16 : 0) + P.hdr_bits;
  for (int64_t seg = 0; seg < nseg; seg++) {
    const uint32_t *tk = tok.data() + seg * kSeg;
    write_segment(tk, ntok[(size_t)seg], P.code, P.len, words.data(), at);
    at += segment_bits(tk, ntok[(size_t)seg], P.len);
  }
  memcpy(dst, words.data(), (size_t)total);
}

// The PNG encoder's zlib stream of h rows of `stride` filtered bytes on the
// host: the functions the PNG kernels run, row after row.  Status and *out_len
// as in encode_block_host.
inline int32_t encode_rows_host(const uint8_t *rows, int h, int stride, int bpp, int fixed_only, uint8_t *dst,
                                int64_t cap, int64_t *out_len) {
  const int64_t n = (int64_t)h * stride;
  std::vector<uint32_t> tok((size_t)n), freq(kSymN, 0u);
  std::vector<int32_t> ntok((size_t)h);
  for (int y = 0; y < h; y++) {
    const int64_t p0 = (int64_t)y * stride;
    ntok[(size_t)y] = tokenize_row(rows, p0, p0 + stride, bpp, stride, tok.data() + p0, [&](int sym) {
      if (!fixed_only) freq[(size_t)sym]++;
    });
  }
  std::vector<Plan> Pv(1);
  std::vector<PlanScratch> Sv(1);
  Plan &P = Pv[0];
  plan_png(freq.data(), fixed_only, P, Sv[0]);
  int64_t body = 0;
  for (int y = 0; y < h; y++) body += segment_bits(tok.data() + (int64_t)y * stride, ntok[(size_t)y], P.len);
  set_body(P, body, 6);
  *out_len = P.stream_bytes;
  if (P.stream_bytes > cap) return kOutputFull;
  std::vector<uint32_t> words((size_t)((P.stream_bytes + 3) / 4), 0u);   // exactly the stream, as above
  write_frame(P, 1, kFlgFastest, adler32_serial(rows, n), words.data());
  int64_t at = 16 + P.hdr_bits;
  for (int y = 0; y < h; y++) {
    const uint32_t *tk = tok.data() + (int64_t)y * stride;
    write_segment(tk, ntok[(size_t)y], P.code, P.len, words.data(), at);
    at += segment_bits(tk, ntok[(size_t)y], P.len);
  }
  memcpy(dst, words.data(), (size_t)P.stream_bytes);
  return kOk;
}

}  // namespace deflate
}  // namespace gsky

#endif
