// deflate_check.cpp -- the host build of gsky_amd/csrc/deflate_core.h against
// zlib, as a stand-alone program meant to be built with
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       -I gsky_amd/csrc tools/deflate_check.cpp -lz
// (tests/test_deflate_check.py does that).  The block corpus of the encoder
// tests, rebuilt here, is encoded as zlib and as raw streams at levels 0 and
// 6.  Required: zlib inflates every stream to the input; the length is within
// the bound; a capacity one byte short is refused with nothing written.  The
// input is allocated at exactly its length and the output at exactly the
// capacity handed to the encoder, so the sanitizer sees any access past them.
// The Fibonacci-weighted block must have driven the code-length limiter.
// The PNG encoder's row path (encode_rows_host) runs over a constant, a noise
// and an upsampled buffer, rows of one byte and one row of three bytes, with 3
// and 4 bytes a pixel, under the same requirements.
#include <zlib.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "deflate_core.h"

namespace gd = gsky::deflate;
typedef std::vector<uint8_t> Bytes;

static uint32_t rng_state = 12345u;
static uint32_t rnd() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return rng_state >> 8;
}

static Bytes random_bytes(size_t n) {
  Bytes b(n);
  for (auto &v : b) v = (uint8_t)rnd();
  return b;
}

template <typename T> static Bytes shuffle(const std::vector<T> &a) {
  Bytes out(a.size() * sizeof(T));
  for (size_t e = 0; e < a.size(); e++) {
    uint8_t raw[sizeof(T)];
    std::memcpy(raw, &a[e], sizeof(T));
    for (size_t b = 0; b < sizeof(T); b++) out[b * a.size() + e] = raw[b];
  }
  return out;
}

static Bytes zlib_inflate(const uint8_t *z, size_t zn, size_t n, bool raw, bool *ok) {
  z_stream s;
  std::memset(&s, 0, sizeof(s));
  Bytes out(n + 1);
  *ok = false;
  if (inflateInit2(&s, raw ? -15 : 15) != Z_OK) return out;
  s.next_in = const_cast<Bytef *>(z);
  s.avail_in = (uInt)zn;
  s.next_out = out.data();
  s.avail_out = (uInt)out.size();
  const int rc = inflate(&s, Z_FINISH);
  *ok = rc == Z_STREAM_END && s.total_out == n && s.avail_in == 0;
  inflateEnd(&s);
  out.resize(n);
  return out;
}

static int fails = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      std::printf("FAIL %s: ", name.c_str());             \
      std::printf(__VA_ARGS__);                           \
      std::printf("\n");                                  \
      fails++;                                            \
    }                                                     \
  } while (0)

static int check_block(const std::string &name, const Bytes &src, int wrapper, int level) {
  // the input at exactly its length (a fresh heap block, never empty for malloc's sake)
  uint8_t *in = (uint8_t *)std::malloc(src.size() ? src.size() : 1);
  if (!src.empty()) std::memcpy(in, src.data(), src.size());
  const int64_t n = (int64_t)src.size(), bound = gd::bound(n);
  int32_t status = -1;
  int64_t len = -1;
  int limited = 0;
  uint8_t *out = (uint8_t *)std::malloc((size_t)bound);
  gd::encode_block_host(in, n, out, bound, wrapper, level, &status, &len, &limited);
  CHECK(status == gd::kOk, "status %d", (int)status);
  CHECK(len > 0 && len <= bound, "length %lld past the bound %lld", (long long)len, (long long)bound);
  bool ok = false;
  const Bytes back = zlib_inflate(out, (size_t)len, src.size(), !wrapper, &ok);
  CHECK(ok && back == src, "zlib does not give the input back (wrapper %d level %d)", wrapper, level);
  // exactly the stream's length: the same bytes
  uint8_t *exact = (uint8_t *)std::malloc((size_t)len);
  int64_t len2 = -1;
  gd::encode_block_host(in, n, exact, len, wrapper, level, &status, &len2, nullptr);
  CHECK(status == gd::kOk && len2 == len && std::memcmp(exact, out, (size_t)len) == 0, "not deterministic");
  // one byte short: refused, nothing written
  Bytes small((size_t)(len - 1), 0xA5);
  gd::encode_block_host(in, n, small.data(), len - 1, wrapper, level, &status, &len2, nullptr);
  CHECK(status == gd::kOutputFull && len2 == len, "capacity %lld accepted", (long long)(len - 1));
  for (uint8_t v : small) CHECK(v == 0xA5, "a refused block was written");
  std::free(exact);
  std::free(out);
  std::free(in);
  return limited;
}

// The PNG encoder's row path (encode_rows_host) over h rows of `stride` bytes,
// with 3 and 4 bytes a pixel, default and fixed codes only: the same checks,
// the output at exactly the 9 bits a byte no stream of that path exceeds.
static void check_rows(const std::string &name, const Bytes &src, int h, int stride) {
  uint8_t *in = (uint8_t *)std::malloc(src.size());
  std::memcpy(in, src.data(), src.size());
  const int64_t n = (int64_t)src.size(), cap = 2 + (3 + 9 * n + 7 + 7) / 8 + 4;
  for (int bpp : {3, 4})
    for (int fixed : {0, 1}) {
      uint8_t *out = (uint8_t *)std::malloc((size_t)cap);
      int64_t len = -1, len2 = -1;
      int32_t status = gd::encode_rows_host(in, h, stride, bpp, fixed, out, cap, &len);
      CHECK(status == gd::kOk && len > 0 && len <= cap, "status %d length %lld (bpp %d fixed %d)", (int)status,
            (long long)len, bpp, fixed);
      bool ok = false;
      const Bytes back = zlib_inflate(out, (size_t)len, src.size(), false, &ok);
      CHECK(ok && back == src, "zlib does not give the rows back (bpp %d fixed %d)", bpp, fixed);
      const int btype = (out[2] >> 1) & 3;   // never stored; fixed where asked for
      CHECK(out[0] == 0x78 && out[1] == 0x01 && (out[2] & 1) == 1 && (btype == 1 || (btype == 2 && !fixed)),
            "not one final Huffman-coded block (BTYPE %d, bpp %d fixed %d)", btype, bpp, fixed);
      uint8_t *exact = (uint8_t *)std::malloc((size_t)len);
      status = gd::encode_rows_host(in, h, stride, bpp, fixed, exact, len, &len2);
      CHECK(status == gd::kOk && len2 == len && std::memcmp(exact, out, (size_t)len) == 0, "not deterministic");
      Bytes small((size_t)(len - 1), 0xA5);
      status = gd::encode_rows_host(in, h, stride, bpp, fixed, small.data(), len - 1, &len2);
      CHECK(status == gd::kOutputFull && len2 == len, "capacity %lld accepted", (long long)(len - 1));
      for (uint8_t v : small) CHECK(v == 0xA5, "a refused stream was written");
      std::free(exact);
      std::free(out);
    }
  std::free(in);
}

static int check_png_rows() {
  const int h = 16, stride = 121;   // 1 + 3 * 40 = 1 + 4 * 30
  check_rows("rows_constant", Bytes((size_t)(h * stride), 7), h, stride);
  check_rows("rows_noise", random_bytes((size_t)(h * stride)), h, stride);
  for (int bpp : {3, 4}) {   // pixels and rows repeated four times, behind a filter byte
    const int w = 40, s = 1 + bpp * w;
    Bytes b((size_t)(h * s), 0);
    const Bytes px = random_bytes((size_t)((h / 4) * (w / 4) * bpp));
    for (int y = 0; y < h; y++)
      for (int x = 0; x < w; x++)
        for (int c = 0; c < bpp; c++) b[(size_t)(y * s + 1 + x * bpp + c)] = px[(size_t)(((y / 4) * (w / 4) + x / 4) * bpp + c)];
    check_rows("rows_upsampled" + std::to_string(bpp), b, h, s);
  }
  Bytes one(50);
  for (auto &v : one) v = (uint8_t)(rnd() % 5);
  check_rows("rows_of_one_byte", one, 50, 1);
  check_rows("one_row_of_three", Bytes{1, 2, 3}, 1, 3);
  return 6;
}

int main() {
  const int n_rows = check_png_rows();
  std::vector<std::pair<std::string, Bytes>> corpus;
  for (int n = 0; n <= 4; n++) {
    Bytes b;
    for (int i = 0; i < n; i++) b.push_back((uint8_t)(65 + i));
    corpus.push_back({"len" + std::to_string(n), b});
  }
  for (int n : {257, 258, 259, 516, 70000}) corpus.push_back({"run" + std::to_string(n), Bytes((size_t)n, 7)});
  corpus.push_back({"random8192", random_bytes(8192)});
  corpus.push_back({"random65535", random_bytes(65535)});
  corpus.push_back({"random65536", random_bytes(65536)});
  corpus.push_back({"one_value", Bytes(1000, 0xEE)});
  {
    Bytes b(256);
    for (int i = 0; i < 256; i++) b[i] = (uint8_t)i;
    corpus.push_back({"all256", b});
  }
  {
    const Bytes period = random_bytes(40000);
    Bytes b(100000);
    for (size_t i = 0; i < b.size(); i++) b[i] = period[i % 40000];
    corpus.push_back({"period40000", b});
  }
  {
    // Fibonacci-weighted byte counts, shuffled: a Huffman tree more than 15 deep even after the matches thin the counts
    Bytes b;
    uint32_t f0 = 1, f1 = 1;
    for (int k = 0; k < 25; k++) {
      b.insert(b.end(), f0, (uint8_t)(k * 11 + 3));
      const uint32_t f2 = f0 + f1;
      f0 = f1;
      f1 = f2;
    }
    for (size_t i = b.size() - 1; i > 0; i--) std::swap(b[i], b[rnd() % (i + 1)]);
    corpus.push_back({"fibonacci", b});
  }
  {
    std::vector<int8_t> a(53);
    for (auto &v : a) v = (int8_t)((int)(rnd() % 11) - 5);
    corpus.push_back({"row_i8_53", shuffle(a)});
    std::vector<float> f(257);
    for (size_t i = 0; i < f.size(); i++) f[i] = 280.0f + 0.03f * (float)i + 0.01f * (float)(rnd() % 100);
    corpus.push_back({"row_f32_257", shuffle(f)});
    std::vector<int16_t> h(2048);
    for (size_t i = 0; i < h.size(); i++) h[i] = (int16_t)(1000 + (int)(i / 40) + (int)(rnd() % 5));
    corpus.push_back({"row_i16_2048", shuffle(h)});
    std::vector<float> g(300);
    for (size_t i = 0; i < g.size(); i++) {
      g[i] = (float)(rnd() % 1000) / 7.0f;
      if (i % 7 == 0) g[i] = -0.0f;
      if (i % 11 == 3) {
        const uint32_t bits = 0x7FC00000u | (rnd() & 0xFFFFFu) | 1u;   // a NaN payload
        std::memcpy(&g[i], &bits, 4);
      }
    }
    corpus.push_back({"row_f32_nan", shuffle(g)});
    corpus.push_back({"const_f32_row", shuffle(std::vector<float>(2048, 273.15f))});
    corpus.push_back({"const_i16_67", shuffle(std::vector<int16_t>(67, (int16_t)-999))});
    std::vector<int16_t> hc(2048);
    for (auto &v : hc) v = (int16_t)(256 + rnd() % 256);
    corpus.push_back({"half_compressible", shuffle(hc)});
  }
  int fib_limited = 0;
  for (const auto &c : corpus)
    for (int wrapper = 0; wrapper < 2; wrapper++)
      for (int level : {0, 6}) {
        const int limited = check_block(c.first, c.second, wrapper, level);
        if (c.first == "fibonacci" && level == 6) fib_limited |= limited;
      }
  std::printf("fibonacci block: code-length limiter %s\n", fib_limited ? "ran" : "did not run");
  if (!fib_limited) fails++;
  if (fails) {
    std::printf("deflate_check: %d failures\n", fails);
    return 1;
  }
  std::printf("deflate_check ok: %zu blocks, %d row buffers\n", corpus.size(), n_rows);
  return 0;
}
