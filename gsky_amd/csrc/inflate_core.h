// inflate_core.h -- an RFC 1950 / RFC 1951 decoder written from the two RFCs,
// compiled for both sides: plain C++17 for the host (tools/inflate_check.cpp,
// gskyhip_inflate_blocks_host) and __host__ __device__ under hipcc for the
// wave-per-block kernel of inflate.hip.  No HIP header is needed.
//
// Shape.  The decoder is a token *producer*: one thread walks the bit stream
// and emits literal / match / stored-run tokens; whoever calls it *resolves*
// the tokens into bytes (the host serially, a wave with all 64 lanes).  The
// producer tracks the output position itself, so every check is made where
// the stream is read:
//   * every input read is checked against the block's input length,
//   * every token's output range against the block's capacity,
//   * every match distance against the bytes produced so far,
// before the token is handed over.  A violation ends the block with a status
// (GSKYHIP_INFLATE_* of include/gskyhip.h, restated below) -- never an
// out-of-range access.  Every loop consumes input or produces output, so it is
// bounded by the input length plus the output capacity.  No recursion, no
// allocation: the tables live in memory the caller supplies (LDS on the GPU).
//
// A batch of tokens is closed before a match that would read bytes produced
// by the same batch, so the tokens of one batch are independent of each other
// and can be resolved in any order (a match with distance < length repeats
// bytes that lie before it with period `distance`).
//
// What is accepted follows zlib's inflate() as shipped (windowBits 15, no
// INFLATE_STRICT) -- the host ingest decodes with it, and the two paths must
// agree: HLIT <= 286, HDIST <= 30; code-length code complete; literal/length
// and distance codes complete, or a single code of one bit, or (distance) none
// at all; an end-of-block code must exist; symbols 286/287 and distance symbols
// 30/31 are invalid when met.  Like that zlib, and unlike a strict reading of
// RFC 1950, the window size the header declares (CINFO <= 7 is required) does
// not bound the distances -- old writers declared 256 bytes and used 512 --
// only the bytes produced so far and the format's 32768 do; bytes after the
// Adler-32 (or after the last block of a raw stream) are ignored.
// tools/inflate_check.cpp holds the core to this against zlib: no stream that
// zlib refuses there decodes here.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifndef GSKY_HD
#if defined(__HIPCC__)
#define GSKY_HD __host__ __device__
#else
#define GSKY_HD
#endif
#endif

namespace gsky {
namespace inflate {

enum Status : int32_t {
  kOk = 0,
  kInputTruncated = 1,   // the stream ends before its last block / checksum
  kBadBlock = 2,         // zlib header, block type 3, stored LEN / NLEN
  kBadCodes = 3,         // code-length set over-subscribed / incomplete / bad repeat / invalid code met
  kBadDistance = 4,      // a match reaches before the start of the output
  kOutputFull = 5,       // more output than the capacity
  kBadChecksum = 6,      // Adler-32 mismatch
  kOutputShort = 7,      // stream fine, but fewer bytes than required
};

constexpr int kLitBits = 10;    // primary table: codes up to 10 bits in one lookup
constexpr int kDistBits = 8;
constexpr int kMaxBatch = 64;   // tokens per batch (one per lane)

// Huffman tables of the current block.  An entry of lit[] / dist[] is
// (symbol << 4) | length for a code of <= k*Bits bits (indexed by the next
// bits of the stream, LSB first), 0 for a longer or unused code: then the
// canonical walk over count / sym decides.
struct Tables {
  uint16_t lit[1 << kLitBits];
  uint16_t dist[1 << kDistBits];
  uint16_t lit_sym[288], dist_sym[32];       // symbols in canonical order
  uint16_t lit_count[16], dist_count[16];    // codes per length
  uint16_t clen[1 << 7];                     // code-length code, 7 bits at most
  uint8_t lens[288 + 32];                    // code lengths while a header is read
};

enum TokenKind : uint32_t { kLiteral = 0, kMatch = 1, kStored = 2 };

// kind_len = kind << 24 | length; arg: the byte / the distance / the input
// offset of a stored run; rel: output offset from the batch's first byte.
struct Token {
  uint32_t kind_len, arg, rel;
};

struct State {
  const uint8_t *in = nullptr;
  uint64_t n_in = 0, ip = 0;        // next input byte
  uint64_t hold = 0;                // bit buffer, LSB first
  int nbits = 0;
  uint64_t pos = 0, cap = 0;        // output bytes produced / capacity
  int phase = 0;                    // 0 stream header, 1 block header, 2 codes, 3 stored run, 4 trailer, 5 done
  int last = 0;                     // BFINAL of the current block
  int zlib = 0;
  uint32_t stored_left = 0;         // bytes of the stored block not yet handed over
  uint32_t adler_want = 0;
  int have_pending = 0;             // a match decoded but deferred to the next batch
  uint32_t pend_len = 0, pend_dist = 0;
};

GSKY_HD inline void init(State &s, const uint8_t *in, uint64_t n_in, uint64_t cap, int zlib_wrapper) {
  s = State();
  s.in = in;
  s.n_in = n_in;
  s.cap = cap;
  s.zlib = zlib_wrapper ? 1 : 0;
  s.phase = zlib_wrapper ? 0 : 1;
}

// ---- bits ---------------------------------------------------------------
GSKY_HD inline void refill(State &s) {
  if (s.nbits <= 32 && s.ip + 4 <= s.n_in) {
    const uint8_t *p = s.in + s.ip;
    const uint32_t w = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
    s.hold |= (uint64_t)w << s.nbits;
    s.nbits += 32;
    s.ip += 4;
  }
  while (s.nbits <= 56 && s.ip < s.n_in) {
    s.hold |= (uint64_t)s.in[s.ip++] << s.nbits;
    s.nbits += 8;
  }
}

// k <= 16 bits into v; false when the input ends first.
GSKY_HD inline bool take(State &s, int k, uint32_t &v) {
  if (s.nbits < k) {
    refill(s);
    if (s.nbits < k) return false;
  }
  v = (uint32_t)(s.hold & ((1u << k) - 1u));
  s.hold >>= k;
  s.nbits -= k;
  return true;
}

// Drop the bits up to the next byte boundary and hand the buffered whole
// bytes back to the input cursor.
GSKY_HD inline void byte_align(State &s) {
  const int drop = s.nbits & 7;
  s.hold >>= drop;
  s.nbits -= drop;
  s.ip -= (uint64_t)(s.nbits >> 3);
  s.hold = 0;
  s.nbits = 0;
}

// ---- code tables ----------------------------------------------------------
GSKY_HD inline uint32_t reverse_bits(uint32_t code, int len) {
  uint32_t r = 0;
  for (int i = 0; i < len; i++) {
    r = (r << 1) | (code & 1u);
    code >>= 1;
  }
  return r;
}

// Canonical code of `n` symbols with lengths `lens` (0: unused) into a lookup
// table of `tbits` bits, the per-length counts and the canonical symbol order.
// allow_short: a single code of one bit (or, allow_none, no code at all) is a
// legal incomplete set.  False: over-subscribed or incomplete.
GSKY_HD inline bool build_table(const uint8_t *lens, int n, uint16_t *table, int tbits, uint16_t *count,
                                uint16_t *sym, bool allow_short, bool allow_none) {
  for (int l = 0; l < 16; l++) count[l] = 0;
  for (int i = 0; i < n; i++) count[lens[i]]++;
  const int used = n - count[0];
  int left = 1, max_len = 0;
  for (int l = 1; l < 16; l++) {
    left <<= 1;
    left -= count[l];
    if (left < 0) return false;   // over-subscribed
    if (count[l]) max_len = l;
  }
  if (left > 0) {   // incomplete
    const bool single = used == 1 && max_len == 1;
    const bool none = used == 0;
    if (!((allow_short && single) || (allow_none && none))) return false;
  }
  // canonical order: by length, then by symbol
  uint16_t offs[16];
  offs[0] = 0;
  offs[1] = 0;
  for (int l = 1; l < 15; l++) offs[l + 1] = (uint16_t)(offs[l] + count[l]);
  for (int i = 0; i < n; i++)
    if (lens[i]) sym[offs[lens[i]]++] = (uint16_t)i;
  for (int i = 0; i < (1 << tbits); i++) table[i] = 0;
  uint32_t code = 0;
  int idx = 0;
  for (int l = 1; l <= 15; l++) {
    for (int k = 0; k < count[l]; k++, idx++, code++) {
      if (l > tbits) continue;
      const uint32_t r = reverse_bits(code, l);
      const uint16_t e = (uint16_t)((sym[idx] << 4) | l);
      for (uint32_t at = r; at < (1u << tbits); at += (1u << l)) table[at] = e;
    }
    code <<= 1;
  }
  count[0] = 0;
  return true;
}

// One symbol.  0 ok; kInputTruncated; kBadCodes (an unused code).
GSKY_HD inline int decode_symbol(State &s, const uint16_t *table, int tbits, const uint16_t *count,
                                 const uint16_t *sym, uint32_t &out) {
  if (s.nbits < 15) refill(s);
  const uint16_t e = table[s.hold & ((1u << tbits) - 1u)];
  if (e) {
    const int l = e & 15;
    if (l > s.nbits) return kInputTruncated;
    s.hold >>= l;
    s.nbits -= l;
    out = (uint32_t)(e >> 4);
    return kOk;
  }
  // a longer code, or none: walk the canonical code one bit at a time
  int code = 0, first = 0, index = 0;
  uint64_t bits = s.hold;
  for (int l = 1; l <= 15; l++) {
    code |= (int)(bits & 1u);
    bits >>= 1;
    const int c = count[l];
    if (code - c < first) {
      if (l > s.nbits) return kInputTruncated;
      s.hold >>= l;
      s.nbits -= l;
      out = sym[index + (code - first)];
      return kOk;
    }
    index += c;
    first += c;
    first <<= 1;
    code <<= 1;
  }
  // no code matches the next 15 bits: with fewer than 15 left the stream may
  // simply have ended inside a code
  return s.nbits < 15 ? kInputTruncated : kBadCodes;
}

GSKY_HD inline void fixed_lengths(uint8_t *lens) {
  int i = 0;
  for (; i < 144; i++) lens[i] = 8;
  for (; i < 256; i++) lens[i] = 9;
  for (; i < 280; i++) lens[i] = 7;
  for (; i < 288; i++) lens[i] = 8;
  for (; i < 320; i++) lens[i] = 5;
}

// The dynamic block header (RFC 1951 3.2.7) into t.  0 or a status.
GSKY_HD inline int read_dynamic(State &s, Tables &t) {
  uint32_t v;
  if (!take(s, 14, v)) return kInputTruncated;
  const int nlen = (int)(v & 31u) + 257, ndist = (int)((v >> 5) & 31u) + 1, ncode = (int)((v >> 10) & 15u) + 4;
  if (nlen > 286 || ndist > 30) return kBadBlock;
  const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  uint8_t cl[19];
  for (int i = 0; i < 19; i++) cl[i] = 0;
  for (int i = 0; i < ncode; i++) {
    if (!take(s, 3, v)) return kInputTruncated;
    cl[order[i]] = (uint8_t)v;
  }
  uint16_t cl_count[16], cl_sym[19];
  if (!build_table(cl, 19, t.clen, 7, cl_count, cl_sym, false, false)) return kBadCodes;
  int have = 0;
  const int total = nlen + ndist;
  while (have < total) {
    uint32_t symv;
    const int rc = decode_symbol(s, t.clen, 7, cl_count, cl_sym, symv);
    if (rc) return rc;
    if (symv < 16) {
      t.lens[have++] = (uint8_t)symv;
      continue;
    }
    uint8_t fill = 0;
    uint32_t rep;
    if (symv == 16) {
      if (have == 0) return kBadCodes;
      fill = t.lens[have - 1];
      if (!take(s, 2, rep)) return kInputTruncated;
      rep += 3;
    } else if (symv == 17) {
      if (!take(s, 3, rep)) return kInputTruncated;
      rep += 3;
    } else {
      if (!take(s, 7, rep)) return kInputTruncated;
      rep += 11;
    }
    if (have + (int)rep > total) return kBadCodes;   // a repeat may cross from literals into distances, not past the end
    for (uint32_t k = 0; k < rep; k++) t.lens[have++] = fill;
  }
  if (t.lens[256] == 0) return kBadCodes;   // no end-of-block code
  if (!build_table(t.lens, nlen, t.lit, kLitBits, t.lit_count, t.lit_sym, true, false)) return kBadCodes;
  if (!build_table(t.lens + nlen, ndist, t.dist, kDistBits, t.dist_count, t.dist_sym, true, true)) return kBadCodes;
  return kOk;
}

GSKY_HD inline uint32_t length_base(int i) {   // i = symbol - 257, 0..28
  const uint16_t b[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115,
                          131, 163, 195, 227, 258};
  return b[i];
}
GSKY_HD inline int length_extra(int i) { return (i < 8 || i == 28) ? 0 : (i - 4) >> 2; }
GSKY_HD inline uint32_t dist_base(int i) {   // i = 0..29
  const uint16_t b[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537,
                          2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
  return b[i];
}
GSKY_HD inline int dist_extra(int i) { return i < 4 ? 0 : (i - 2) >> 1; }

// ---- the producer -----------------------------------------------------------
// Decode up to `max_tok` (<= kMaxBatch) tokens into tok[]; *n_tok tokens were
// made, covering output bytes [start, s.pos) with start = s.pos on entry.
// Returns kOk with s.phase == 5 once the stream has ended, kOk with
// s.phase < 5 when the batch is closed (full, or the next match depends on
// it), or the status that ends the block.
GSKY_HD inline int produce(State &s, Tables &t, Token *tok, int max_tok, int *n_tok) {
  int &n = *n_tok;   // kept current, so that the tokens made before a status are still resolved
  n = 0;
  const uint64_t start = s.pos;
  if (s.have_pending) {   // the match that closed the batch before
    tok[n].kind_len = (kMatch << 24) | s.pend_len;
    tok[n].arg = s.pend_dist;
    tok[n].rel = 0;
    n++;
    s.pos += s.pend_len;
    s.have_pending = 0;
  }
  while (n < max_tok && s.phase != 5) {
    uint32_t v;
    if (s.phase == 0) {   // RFC 1950: CMF, FLG
      uint32_t cmf, flg;
      if (!take(s, 8, cmf) || !take(s, 8, flg)) return kInputTruncated;
      if ((cmf & 15u) != 8 || (cmf >> 4) > 7 || ((cmf << 8) | flg) % 31u != 0 || (flg & 0x20u)) return kBadBlock;
      s.phase = 1;
    } else if (s.phase == 1) {   // block header
      if (!take(s, 3, v)) return kInputTruncated;
      s.last = (int)(v & 1u);
      const uint32_t type = v >> 1;
      if (type == 0) {
        byte_align(s);
        if (s.n_in - s.ip < 4) return kInputTruncated;
        const uint32_t len = (uint32_t)s.in[s.ip] | ((uint32_t)s.in[s.ip + 1] << 8);
        const uint32_t nlen = (uint32_t)s.in[s.ip + 2] | ((uint32_t)s.in[s.ip + 3] << 8);
        if ((len ^ 0xFFFFu) != nlen) return kBadBlock;
        s.ip += 4;
        s.stored_left = len;
        s.phase = 3;
      } else if (type == 1) {
        fixed_lengths(t.lens);
        // the fixed codes are complete: the builds cannot fail
        build_table(t.lens, 288, t.lit, kLitBits, t.lit_count, t.lit_sym, false, false);
        build_table(t.lens + 288, 32, t.dist, kDistBits, t.dist_count, t.dist_sym, false, false);
        s.phase = 2;
      } else if (type == 2) {
        const int rc = read_dynamic(s, t);
        if (rc) return rc;
        s.phase = 2;
      } else {
        return kBadBlock;
      }
    } else if (s.phase == 3) {   // a stored run: one token
      if (s.stored_left) {
        const uint32_t len = s.stored_left;
        if (s.n_in - s.ip < len) return kInputTruncated;
        if (s.cap - s.pos < len) return kOutputFull;
        if (s.ip > 0xFFFFFFFFull) return kInputTruncated;   // offsets are 32 bits (the ABI refuses such inputs)
        tok[n].kind_len = (kStored << 24) | len;
        tok[n].arg = (uint32_t)s.ip;
        tok[n].rel = (uint32_t)(s.pos - start);
        n++;
        s.ip += len;
        s.pos += len;
        s.stored_left = 0;
      }
      s.phase = s.last ? 4 : 1;
    } else if (s.phase == 2) {   // literal / length
      int rc = decode_symbol(s, t.lit, kLitBits, t.lit_count, t.lit_sym, v);
      if (rc) return rc;
      if (v < 256) {
        if (s.pos >= s.cap) return kOutputFull;
        tok[n].kind_len = (kLiteral << 24) | 1u;
        tok[n].arg = v;
        tok[n].rel = (uint32_t)(s.pos - start);
        n++;
        s.pos++;
      } else if (v == 256) {
        s.phase = s.last ? 4 : 1;
      } else {
        if (v > 285) return kBadCodes;
        const int li = (int)v - 257;
        uint32_t len = length_base(li), extra = 0;
        if (length_extra(li) && !take(s, length_extra(li), extra)) return kInputTruncated;
        len += extra;
        uint32_t ds;
        rc = decode_symbol(s, t.dist, kDistBits, t.dist_count, t.dist_sym, ds);
        if (rc) return rc;
        if (ds > 29) return kBadCodes;
        uint32_t dist = dist_base((int)ds);
        extra = 0;
        if (dist_extra((int)ds) && !take(s, dist_extra((int)ds), extra)) return kInputTruncated;
        dist += extra;
        if ((uint64_t)dist > s.pos) return kBadDistance;
        if (s.cap - s.pos < len) return kOutputFull;
        // source bytes [pos - dist, pos - dist + min(len, dist)) must lie before this batch
        const uint64_t src_end = s.pos - dist + (len < dist ? len : dist);
        if (src_end > start && n > 0) {
          s.have_pending = 1;
          s.pend_len = len;
          s.pend_dist = dist;
          break;
        }
        tok[n].kind_len = (kMatch << 24) | len;
        tok[n].arg = dist;
        tok[n].rel = (uint32_t)(s.pos - start);
        n++;
        s.pos += len;
      }
    } else {   // phase 4: the end of the stream
      if (s.zlib) {
        byte_align(s);
        if (s.n_in - s.ip < 4) return kInputTruncated;
        s.adler_want = ((uint32_t)s.in[s.ip] << 24) | ((uint32_t)s.in[s.ip + 1] << 16) |
                       ((uint32_t)s.in[s.ip + 2] << 8) | (uint32_t)s.in[s.ip + 3];
        s.ip += 4;
      }
      s.phase = 5;
    }
  }
  return kOk;
}

// Output byte k of token tk, whose first byte is out[at]: the one rule both
// resolvers share.  `out` holds every byte before the batch.
GSKY_HD inline uint8_t token_byte(const Token &tk, uint32_t k, const uint8_t *in, const uint8_t *out, uint64_t at) {
  const uint32_t kind = tk.kind_len >> 24;
  if (kind == kLiteral) return (uint8_t)tk.arg;
  if (kind == kStored) return in[(uint64_t)tk.arg + k];
  const uint32_t d = tk.arg;
  return out[at - d + (k < d ? k : k % d)];
}

constexpr uint32_t kAdlerMod = 65521u;

// Adler-32 (RFC 1950 8.2) continued over n bytes; a starts at 1, b at 0.
GSKY_HD inline void adler_update(uint32_t &a, uint32_t &b, const uint8_t *p, uint64_t n) {
  while (n) {
    const uint64_t run = n < 5552 ? n : 5552;   // the sums stay below 2^32 over such a run
    for (uint64_t i = 0; i < run; i++) {
      a += p[i];
      b += a;
    }
    a %= kAdlerMod;
    b %= kAdlerMod;
    p += run;
    n -= run;
  }
}

// The status once the stream has ended and the output is complete.
GSKY_HD inline int finish(const State &s, uint32_t adler, uint64_t need) {
  if (s.zlib && adler != s.adler_want) return kBadChecksum;
  if (s.pos < need) return kOutputShort;
  return kOk;
}

// The whole block on one thread (the host side, and the reference the kernel
// is compared with).  Returns the status; *out_len = bytes produced.
inline int inflate_serial(const uint8_t *in, uint64_t n_in, uint8_t *out, uint64_t cap, uint64_t need,
                          int zlib_wrapper, uint64_t *out_len) {
  State s;
  Tables t;
  Token tok[kMaxBatch];
  init(s, in, n_in, cap, zlib_wrapper);
  int rc = kOk;
  while (s.phase != 5) {
    const uint64_t start = s.pos;
    int n = 0;
    rc = produce(s, t, tok, kMaxBatch, &n);
    // tokens made before an error are within bounds: resolve them, so that
    // out_len bytes are defined on both sides
    for (int i = 0; i < n; i++) {
      const uint32_t len = tok[i].kind_len & 0xFFFFFFu;
      const uint64_t at = start + tok[i].rel;
      for (uint32_t k = 0; k < len; k++) out[at + k] = token_byte(tok[i], k, in, out, at);
    }
    if (rc) break;
  }
  if (out_len) *out_len = s.pos;
  if (rc) return rc;
  uint32_t a = 1, b = 0;
  if (s.zlib) adler_update(a, b, out, s.pos);
  return finish(s, (b << 16) | a, need);
}

}  // namespace inflate
}  // namespace gsky
