// inflate_check.cpp -- the host build of gsky_amd/csrc/inflate_core.h against
// zlib, as a stand-alone program meant to be built with
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       -I gsky_amd/csrc tools/inflate_check.cpp -lz
// (tests/test_inflate_check.py does that).  A dozen buffers are deflated at
// several levels and strategies, as zlib and as raw streams; each stream is
// decoded intact, cut at every byte length, and with each bit of its first 64
// bytes flipped.  Required: the decoder returns; zlib failing implies a
// non-zero status; status 0 where zlib succeeds implies zlib's bytes.  The
// output buffer is allocated at exactly the capacity handed to the decoder, so
// the sanitizer sees any write past it; the input likewise.
#include <zlib.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "inflate_core.h"

namespace gi = gsky::inflate;
typedef std::vector<uint8_t> Bytes;

static uint32_t rng_state = 12345u;
static uint32_t rnd() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return rng_state >> 8;
}

static Bytes deflate_with(const Bytes &src, int level, int strategy, bool raw) {
  z_stream z;
  std::memset(&z, 0, sizeof(z));
  if (deflateInit2(&z, level, Z_DEFLATED, raw ? -15 : 15, 8, strategy) != Z_OK) std::abort();
  Bytes out(2 * src.size() + 1024);   // Z_FIXED can expand past deflateBound
  z.next_in = const_cast<Bytef *>(src.data());
  z.avail_in = (uInt)src.size();
  z.next_out = out.data();
  z.avail_out = (uInt)out.size();
  if (deflate(&z, Z_FINISH) != Z_STREAM_END) std::abort();
  out.resize(z.total_out);
  deflateEnd(&z);
  return out;
}

// zlib's verdict: true and the bytes when the stream decodes within `cap`.
static bool zlib_decode(const uint8_t *in, size_t n, size_t cap, bool raw, Bytes &out) {
  z_stream z;
  std::memset(&z, 0, sizeof(z));
  if (inflateInit2(&z, raw ? -15 : 15) != Z_OK) std::abort();
  out.assign(cap + 1, 0);
  z.next_in = const_cast<Bytef *>(in);
  z.avail_in = (uInt)n;
  z.next_out = out.data();
  z.avail_out = (uInt)out.size();
  const int rc = inflate(&z, Z_FINISH);
  const size_t got = z.total_out;
  inflateEnd(&z);
  if (rc != Z_STREAM_END || got > cap) return false;
  out.resize(got);
  return true;
}

static long n_runs = 0, n_ok = 0, n_fail = 0, n_stricter = 0;

// One decode of `stream` with the core; compared with zlib.
static bool check(const Bytes &stream, size_t cap, bool raw, const char *what) {
  // exact-size heap copies: the sanitizer guards both ends
  uint8_t *in = (uint8_t *)std::malloc(stream.size() ? stream.size() : 1);
  uint8_t *out = (uint8_t *)std::malloc(cap ? cap : 1);
  if (!stream.empty()) std::memcpy(in, stream.data(), stream.size());
  std::memset(out, 0xA5, cap ? cap : 1);
  uint64_t got = 0;
  const int st = gi::inflate_serial(in, stream.size(), out, cap, 0, raw ? 0 : 1, &got);
  Bytes ref;
  const bool zok = zlib_decode(stream.data(), stream.size(), cap, raw, ref);
  bool good = true;
  if (!zok && st == 0) {
    std::fprintf(stderr, "%s: zlib refuses the stream, the core returns ok\n", what);
    good = false;
  }
  if (zok && st == 0 && (got != ref.size() || (got && std::memcmp(out, ref.data(), ref.size()) != 0))) {
    std::fprintf(stderr, "%s: status ok but the bytes differ from zlib's\n", what);
    good = false;
  }
  if (got > cap) {
    std::fprintf(stderr, "%s: out_len beyond the capacity\n", what);
    good = false;
  }
  n_runs++;
  if (zok && st != 0) n_stricter++;   // allowed, reported
  if (st == 0) n_ok++; else n_fail++;
  std::free(in);
  std::free(out);
  return good;
}

int main() {
  std::vector<Bytes> bufs;
  bufs.push_back(Bytes());                                  // empty
  bufs.push_back(Bytes(1, 7));                              // one byte
  bufs.push_back(Bytes(3000, 0));                           // zeros: distance 1, overlapping copies
  { Bytes b(2500); for (auto &x : b) x = (uint8_t)rnd(); bufs.push_back(b); }          // incompressible
  { Bytes b; const char *s = "hello hello hello world"; for (int i = 0; i < 40; i++) b.insert(b.end(), s, s + 23); bufs.push_back(b); }
  { Bytes b; for (int i = 0; i < 120; i++) b.insert(b.end(), 1 + rnd() % 40, (uint8_t)rnd()); bufs.push_back(b); }   // runs
  { Bytes b(4000); for (auto &x : b) x = (uint8_t)(rnd() & 1); bufs.push_back(b); }    // two symbols
  { Bytes b; uint32_t a = 1, c = 1; for (int s = 0; s < 14; s++) { b.insert(b.end(), a, (uint8_t)s); uint32_t n = a + c; a = c; c = n; }
    for (size_t i = b.size() - 1; i > 0; i--) std::swap(b[i], b[rnd() % (i + 1)]);
    bufs.push_back(b); }   // skewed counts: long codes
  { Bytes b(3000); for (auto &x : b) x = (uint8_t)(rnd() & 3); Bytes c = b; c.insert(c.end(), b.begin(), b.end()); bufs.push_back(c); }   // far matches
  { Bytes b(2048); int16_t v = 0; for (size_t i = 0; i < b.size(); i += 2) { v = (int16_t)(v + (int)(rnd() % 7) - 3); std::memcpy(&b[i], &v, 2); } bufs.push_back(b); }
  { Bytes b(1500); for (auto &x : b) x = (uint8_t)rnd(); b.insert(b.end(), 1500, 0); const char *s = "abcabcabd"; for (int i = 0; i < 100; i++) b.insert(b.end(), s, s + 9); bufs.push_back(b); }
  { Bytes b(4096); for (size_t i = 0; i < b.size(); i++) b[i] = (uint8_t)((i * 7) ^ (i >> 5)); bufs.push_back(b); }

  struct Mode { int level, strategy; bool raw; };
  const Mode modes[] = {{0, Z_DEFAULT_STRATEGY, false}, {1, Z_DEFAULT_STRATEGY, false}, {6, Z_DEFAULT_STRATEGY, false},
                        {9, Z_DEFAULT_STRATEGY, false}, {6, Z_FIXED, false},           {6, Z_RLE, false},
                        {6, Z_HUFFMAN_ONLY, false},     {6, Z_FILTERED, true},         {9, Z_DEFAULT_STRATEGY, true}};
  bool good = true;
  for (size_t bi = 0; bi < bufs.size(); bi++) {
    for (const Mode &m : modes) {
      const Bytes &src = bufs[bi];
      const Bytes z = deflate_with(src, m.level, m.strategy, m.raw);
      char what[96];
      std::snprintf(what, sizeof(what), "buffer %zu level %d strategy %d %s", bi, m.level, m.strategy, m.raw ? "raw" : "zlib");
      // intact, at the exact capacity and one byte short of it
      good &= check(z, src.size(), m.raw, what);
      if (!src.empty()) good &= check(z, src.size() - 1, m.raw, what);
      good &= check(z, src.size() + 100, m.raw, what);
      // cut at every byte length
      for (size_t n = 0; n < z.size(); n++) good &= check(Bytes(z.begin(), z.begin() + n), src.size(), m.raw, what);
      // each bit of the first 64 bytes flipped
      for (size_t bit = 0; bit < 8 * std::min<size_t>(64, z.size()); bit++) {
        Bytes f = z;
        f[bit >> 3] ^= (uint8_t)(1u << (bit & 7));
        good &= check(f, src.size() + 300, m.raw, what);
      }
      // the last four bytes (the Adler-32 of a zlib stream) flipped, one at a time
      for (size_t k = 0; k < 4 && k < z.size(); k++) {
        Bytes f = z;
        f[z.size() - 1 - k] ^= 0x10;
        good &= check(f, src.size(), m.raw, what);
      }
      if (!good) {
        std::fprintf(stderr, "FAILED at %s\n", what);
        return 1;
      }
    }
  }
  // streams no bit flip above is sure to make: block type 3; a fixed block that
  // opens with a match (distance before the start of the output); an
  // over-subscribed code-length code
  {
    const Bytes type3 = {0x78, 0x9c, 0x07, 0, 0, 0, 0, 0};
    const Bytes early = {0x03, 0x02, 0x00};                    // raw: BFINAL, fixed, <3, 1>, end of block
    const Bytes over = {0x78, 0x9c, 0x05, 0x00, 0x92, 0x00, 0, 0, 0, 0, 0, 0};   // dynamic, code lengths 1, 1, 1
    good &= check(type3, 64, false, "block type 3");
    good &= check(early, 64, true, "match at the start");
    good &= check(over, 64, false, "over-subscribed code lengths");
    uint8_t out[64];
    uint64_t got = 0;
    if (gi::inflate_serial(type3.data(), type3.size(), out, 64, 0, 1, &got) != gi::kBadBlock ||
        gi::inflate_serial(early.data(), early.size(), out, 64, 0, 0, &got) != gi::kBadDistance ||
        gi::inflate_serial(over.data(), over.size(), out, 64, 0, 1, &got) != gi::kBadCodes) {
      std::fprintf(stderr, "a hand-made malformed stream got another status than expected\n");
      good = false;
    }
    if (!good) return 1;
  }
  // what zlib as shipped accepts beyond a strict reading of RFC 1950, and the
  // core with it (the host ingest decodes with zlib: the two must agree): a
  // header that declares a 256-byte window over distances of 3000, and bytes
  // after the checksum
  {
    Bytes unit(3000);
    for (auto &x : unit) x = (uint8_t)(rnd() & 3);
    Bytes src = unit;
    src.insert(src.end(), unit.begin(), unit.end());
    Bytes z = deflate_with(src, 9, Z_DEFAULT_STRATEGY, false);
    z[0] = 0x08;   // CM = 8, CINFO = 0
    z[1] = 0;
    while ((((unsigned)z[0] << 8) | z[1]) % 31 != 0) z[1]++;   // FCHECK; FDICT stays clear (z[1] < 31)
    Bytes ref, tail = deflate_with(src, 6, Z_DEFAULT_STRATEGY, false);
    tail.insert(tail.end(), {'j', 'u', 'n', 'k'});
    Bytes raw_tail = deflate_with(src, 6, Z_DEFAULT_STRATEGY, true);
    raw_tail.push_back(0xFF);
    uint64_t got = 0;
    Bytes out(src.size());
    const struct { const Bytes *s; bool raw; const char *what; } cases[] = {
        {&z, false, "small declared window"}, {&tail, false, "bytes after the checksum"},
        {&raw_tail, true, "bytes after a raw stream"}};
    for (const auto &c : cases) {
      good &= check(*c.s, src.size(), c.raw, c.what);
      if (!zlib_decode(c.s->data(), c.s->size(), src.size(), c.raw, ref) ||
          gi::inflate_serial(c.s->data(), c.s->size(), out.data(), out.size(), src.size(), c.raw ? 0 : 1, &got) != gi::kOk ||
          out != src) {
        std::fprintf(stderr, "%s: zlib and the core must both decode it\n", c.what);
        good = false;
      }
    }
    if (!good) return 1;
  }
  std::printf("inflate_check ok: %ld decodes, %ld accepted, %ld refused (%ld of them accepted by zlib)\n", n_runs, n_ok,
              n_fail, n_stricter);
  return 0;
}
