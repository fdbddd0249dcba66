// geotiff_check.cpp -- the host side of the WCS GeoTIFF writer
// (gsky_amd/csrc/tiffwrite.cpp: band rules, predictors, PackBits, BigTIFF
// framing, on the Deflate encoder's host twin of deflate_core.h) as a
// stand-alone program meant to be built with
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       -I include -I gsky_amd/csrc tools/geotiff_check.cpp gsky_amd/csrc/tiffwrite.cpp -lz -pthread
// (tests/test_geotiff_check.py does that).  The shapes of
// tests/test_geotiff_deflate.py -- every dtype with its predictors on 33 x 40
// with 16 x 16 tiles, two bands, a 1024 x 256 tile larger than the image on
// one and on both axes, an EmptyTile band between two real ones, a constant
// and a random band, zlevel 0 and 6, and PackBits -- are written through
// gskyhip_encode_geotiff_host.  Every band is allocated at exactly its size
// and the output at exactly gskyhip_geotiff_bound_opts, so the sanitizer sees
// any access past them.  Required: the IFD parses, tag 259 / 317 are what was
// asked for, zlib inflates every tile to exactly the tile's size (PackBits:
// every tile row decodes to its length), and the tile, un-predicted, is the
// input inside the image and the pad value outside it; a capacity one byte
// short is refused.
#include <zlib.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "gskyhip.h"

typedef std::vector<uint8_t> Bytes;

static uint32_t rng_state = 2468u;
static uint32_t rnd() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return rng_state >> 8;
}

static int fails = 0;
#define CHECK(cond, ...)                      \
  do {                                        \
    if (!(cond)) {                            \
      std::printf("FAIL %s: ", name.c_str()); \
      std::printf(__VA_ARGS__);               \
      std::printf("\n");                      \
      fails++;                                \
    }                                         \
  } while (0)

static int size_of(int dtype) { return dtype == GSKYHIP_FLOAT32 ? 4 : (dtype == GSKYHIP_INT16 || dtype == GSKYHIP_UINT16) ? 2 : 1; }

static uint64_t le(const uint8_t *p, int n) {
  uint64_t v = 0;
  for (int k = 0; k < n; k++) v |= (uint64_t)p[k] << (8 * k);
  return v;
}

// tag -> values (SHORT, LONG, LONG8 only; others are skipped), bounds-checked against the file
static bool read_ifd(const Bytes &f, std::map<int, std::vector<uint64_t>> &tags) {
  if (f.size() < 16 || f[0] != 'I' || f[1] != 'I' || le(&f[2], 2) != 43 || le(&f[4], 2) != 8) return false;
  const uint64_t ifd = le(&f[8], 8);
  if (ifd + 8 > f.size()) return false;
  const uint64_t n = le(&f[ifd], 8);
  if (n > 1000 || ifd + 8 + 20 * n + 8 > f.size()) return false;
  for (uint64_t i = 0; i < n; i++) {
    const uint8_t *e = &f[ifd + 8 + 20 * i];
    const int tag = (int)le(e, 2), type = (int)le(e + 2, 2);
    const uint64_t count = le(e + 4, 8);
    const int ts = type == 3 ? 2 : type == 4 ? 4 : type == 16 ? 8 : 0;
    if (!ts) continue;
    const uint8_t *v = e + 12;
    if (count * ts > 8) {
      const uint64_t at = le(e + 12, 8);
      if (at + count * ts > f.size()) return false;
      v = &f[at];
    }
    for (uint64_t k = 0; k < count; k++) tags[tag].push_back(le(v + k * ts, ts));
  }
  return true;
}

static bool zlib_inflate(const uint8_t *z, size_t zn, Bytes &out) {
  z_stream s;
  std::memset(&s, 0, sizeof(s));
  if (inflateInit2(&s, 15) != Z_OK) return false;
  Bytes buf(out.size() + 1);
  s.next_in = const_cast<Bytef *>(z);
  s.avail_in = (uInt)zn;
  s.next_out = buf.data();
  s.avail_out = (uInt)buf.size();
  const int rc = inflate(&s, Z_FINISH);
  const bool ok = rc == Z_STREAM_END && s.total_out == out.size() && s.avail_in == 0;
  inflateEnd(&s);
  std::memcpy(out.data(), buf.data(), out.size());
  return ok;
}

// rows of `rb` bytes each from tiled PackBits (row by row); false if the data does not end with the last row
static bool unpackbits(const uint8_t *d, size_t n, int rows, int rb, Bytes &out) {
  size_t i = 0, o = 0;
  for (int r = 0; r < rows; r++) {
    const size_t end = o + (size_t)rb;
    while (o < end) {
      if (i >= n) return false;
      const int c = d[i++];
      if (c < 128) {
        if (i + c + 1 > n || o + c + 1 > end) return false;
        std::memcpy(&out[o], d + i, (size_t)c + 1);
        i += (size_t)c + 1;
        o += (size_t)c + 1;
      } else if (c > 128) {
        if (i >= n || o + (size_t)(257 - c) > end) return false;
        std::memset(&out[o], d[i++], (size_t)(257 - c));
        o += (size_t)(257 - c);
      }
    }
  }
  return i == n;
}

static void unpredict(Bytes &t, int ts, int bx, int by, int predictor) {
  const size_t rb = (size_t)bx * ts;
  for (int r = 0; r < by; r++) {
    uint8_t *row = t.data() + r * rb;
    if (predictor == 2) {
      uint32_t acc = 0;
      for (int x = 0; x < bx; x++) {
        acc += (uint32_t)le(row + (size_t)x * ts, ts);
        for (int k = 0; k < ts; k++) row[(size_t)x * ts + k] = (uint8_t)(acc >> (8 * k));
      }
    } else if (predictor == 3) {
      for (size_t i = 1; i < rb; i++) row[i] = (uint8_t)(row[i] + row[i - 1]);
      const Bytes planes(row, row + rb);
      for (int x = 0; x < bx; x++)
        for (int p = 0; p < 4; p++) row[(size_t)x * 4 + 3 - p] = planes[(size_t)p * bx + x];
    }
  }
}

struct Case {
  std::string name;
  int dtype, width, height, n_bands, bx, by, compression, predictor, zlevel;
  int empty_band;   // -1: none
  int fill;         // 0: ramp + noise, 1: constant, 2: random
  bool nodata;
};

static void pad_sample(const Case &c, double v, uint8_t *p) {
  if (c.dtype == GSKYHIP_FLOAT32) { const float f = (float)v; std::memcpy(p, &f, 4); }
  else if (size_of(c.dtype) == 2) { const int16_t h = (int16_t)(int32_t)v; std::memcpy(p, &h, 2); }
  else p[0] = (uint8_t)(int)v;
}

static void run(const Case &c) {
  const std::string &name = c.name;
  const int ts = size_of(c.dtype);
  const size_t band_bytes = (size_t)c.width * c.height * ts;
  std::vector<uint8_t *> bands((size_t)c.n_bands, nullptr);
  std::vector<std::string> name_store;
  std::vector<const char *> names;
  std::vector<double> nodata;
  for (int b = 0; b < c.n_bands; b++) {
    name_store.push_back(b == c.empty_band ? "EmptyTile_" + std::to_string(b) : "band<" + std::to_string(b) + ">");
    nodata.push_back(3.0 + b);
  }
  for (int b = 0; b < c.n_bands; b++) names.push_back(name_store[(size_t)b].c_str());
  for (int b = 0; b < c.n_bands; b++) {
    if (b == c.empty_band) continue;   // skipped by the writer: no samples at all
    bands[(size_t)b] = (uint8_t *)std::malloc(band_bytes);   // exactly the band
    for (int y = 0; y < c.height; y++)
      for (int x = 0; x < c.width; x++) {
        uint8_t *p = bands[(size_t)b] + ((size_t)y * c.width + x) * ts;
        if (c.dtype == GSKYHIP_FLOAT32) {
          float f = c.fill == 1 ? 273.15f : c.fill == 2 ? (float)rnd() : 280.0f + 0.05f * x + 0.03f * y + 0.001f * (float)(rnd() % 1000);
          if (c.fill == 0 && x == 5 && y == 7) { const uint32_t bits = 0x7FC00001u; std::memcpy(&f, &bits, 4); }
          std::memcpy(p, &f, 4);
        } else {
          const uint32_t v = c.fill == 1 ? 1234u : c.fill == 2 ? rnd() : (uint32_t)(3 * x + 2 * y + 100 * b) + rnd() % 9;
          for (int k = 0; k < ts; k++) p[k] = (uint8_t)(v >> (8 * k));
        }
      }
  }
  const double geot[6] = {1500000.0, 25.0, 0.0, -3900000.0, 0.0, -25.0};
  const int64_t bound = gskyhip_geotiff_bound_opts(c.width, c.height, c.n_bands, c.dtype, c.bx, c.by, c.compression);
  CHECK(bound > 0, "bound %lld", (long long)bound);
  if (bound <= 0) return;
  uint8_t *out = (uint8_t *)std::malloc((size_t)bound);   // exactly the bound
  int64_t size = -1;
  int rc = gskyhip_encode_geotiff_host((const void *const *)bands.data(), c.n_bands, c.dtype, c.width, c.height, geot,
                                       3577, c.nodata ? nodata.data() : nullptr, names.data(), c.bx, c.by,
                                       c.compression, c.predictor, c.zlevel, 3, out, bound, &size);
  CHECK(rc == 0 && size > 16 && size <= bound, "rc %d size %lld bound %lld", rc, (long long)size, (long long)bound);
  int64_t size2 = -1;
  uint8_t *small = (uint8_t *)std::malloc((size_t)bound - 1);
  rc = gskyhip_encode_geotiff_host((const void *const *)bands.data(), c.n_bands, c.dtype, c.width, c.height, geot, 3577,
                                   c.nodata ? nodata.data() : nullptr, names.data(), c.bx, c.by, c.compression,
                                   c.predictor, c.zlevel, 3, small, bound - 1, &size2);
  CHECK(rc == GSKYHIP_E_ARG && size2 == -1, "a capacity below the bound was accepted (rc %d)", rc);
  std::free(small);
  if (size > 16 && size <= bound) {
    const Bytes file(out, out + size);
    std::map<int, std::vector<uint64_t>> tags;
    const bool parsed = read_ifd(file, tags);
    CHECK(parsed, "the IFD does not parse");
    const int ntx = (c.width + c.bx - 1) / c.bx, nty = (c.height + c.by - 1) / c.by;
    const size_t n_tiles = (size_t)c.n_bands * ntx * nty;
    CHECK(tags[259] == std::vector<uint64_t>{(uint64_t)c.compression}, "tag 259");
    CHECK(c.predictor == 1 ? tags.count(317) == 0 : tags[317] == std::vector<uint64_t>{(uint64_t)c.predictor}, "tag 317");
    CHECK(tags[324].size() == n_tiles && tags[325].size() == n_tiles, "%zu tile offsets", tags[324].size());
    int last_nd = -1;
    for (int b = 0; b < c.n_bands; b++)
      if (b != c.empty_band && c.nodata) last_nd = b;
    if (parsed && tags[324].size() == n_tiles && tags[325].size() == n_tiles)
      for (size_t t = 0; t < n_tiles; t++) {
        const uint64_t off = tags[324][t], cnt = tags[325][t];
        CHECK(off >= 16 && off + cnt <= file.size(), "tile %zu lies outside the file", t);
        if (off < 16 || off + cnt > file.size()) break;
        Bytes tile((size_t)c.bx * c.by * ts);
        const bool ok = c.compression == GSKYHIP_TIFF_DEFLATE ? zlib_inflate(&file[off], (size_t)cnt, tile)
                                                              : unpackbits(&file[off], (size_t)cnt, c.by, c.bx * ts, tile);
        CHECK(ok, "tile %zu does not decode to its size", t);
        if (!ok) break;
        if (c.zlevel == 0 && c.compression == GSKYHIP_TIFF_DEFLATE)
          CHECK(((file[off + 2] >> 1) & 3) == 0, "tile %zu at zlevel 0 is not stored", t);
        unpredict(tile, ts, c.bx, c.by, c.predictor);
        const int b = (int)(t / ((size_t)ntx * nty)), tx = (int)(t % (size_t)ntx), ty = (int)(t / (size_t)ntx % (size_t)nty);
        uint8_t pad[4] = {0, 0, 0, 0};
        pad_sample(c, b == c.empty_band ? (last_nd >= 0 ? nodata[(size_t)last_nd] : 0.0) : c.nodata ? nodata[(size_t)b] : 0.0, pad);
        size_t bad = 0;
        for (int r = 0; r < c.by; r++)
          for (int x = 0; x < c.bx; x++) {
            const int gx = tx * c.bx + x, gy = ty * c.by + r;
            const uint8_t *want = (bands[(size_t)b] && gx < c.width && gy < c.height)
                                      ? bands[(size_t)b] + ((size_t)gy * c.width + gx) * ts : pad;
            bad += std::memcmp(&tile[((size_t)r * c.bx + x) * ts], want, (size_t)ts) != 0;
          }
        CHECK(bad == 0, "tile %zu: %zu samples differ from the input", t, bad);
      }
  }
  std::free(out);
  for (uint8_t *b : bands) std::free(b);
}

int main() {
  std::vector<Case> cases;
  const int D = GSKYHIP_TIFF_DEFLATE, P = GSKYHIP_TIFF_PACKBITS;
  struct { const char *n; int dtype; } types[] = {{"u8", GSKYHIP_BYTE}, {"i8", GSKYHIP_SIGNEDBYTE}, {"i16", GSKYHIP_INT16},
                                                  {"u16", GSKYHIP_UINT16}, {"f32", GSKYHIP_FLOAT32}};
  for (auto &t : types)
    for (int p = 1; p <= (t.dtype == GSKYHIP_FLOAT32 ? 3 : 2); p++)
      cases.push_back({std::string(t.n) + "_p" + std::to_string(p), t.dtype, 33, 40, 1, 16, 16, D, p, 6, -1, 0, true});
  cases.push_back({"two_bands", GSKYHIP_INT16, 33, 40, 2, 16, 16, D, 2, 6, -1, 0, true});
  cases.push_back({"tile_over_image_i16", GSKYHIP_INT16, 300, 40, 1, 1024, 256, D, 2, 6, -1, 0, false});
  cases.push_back({"tile_over_image_f32", GSKYHIP_FLOAT32, 300, 40, 1, 1024, 256, D, 3, 6, -1, 0, true});
  cases.push_back({"tall_f32", GSKYHIP_FLOAT32, 40, 300, 1, 1024, 256, D, 3, 6, -1, 0, false});
  cases.push_back({"empty_between", GSKYHIP_INT16, 33, 40, 3, 16, 16, D, 2, 6, 1, 0, true});
  cases.push_back({"empty_no_nodata", GSKYHIP_FLOAT32, 33, 40, 2, 16, 16, D, 3, 6, 0, 0, false});
  cases.push_back({"constant_i16", GSKYHIP_INT16, 33, 40, 1, 16, 16, D, 2, 6, -1, 1, false});
  cases.push_back({"constant_f32", GSKYHIP_FLOAT32, 33, 40, 1, 16, 16, D, 3, 6, -1, 1, false});
  cases.push_back({"random_u8", GSKYHIP_BYTE, 33, 40, 1, 16, 16, D, 1, 6, -1, 2, false});
  cases.push_back({"random_f32", GSKYHIP_FLOAT32, 33, 40, 1, 16, 16, D, 3, 6, -1, 2, false});
  cases.push_back({"stored_i16", GSKYHIP_INT16, 33, 40, 1, 16, 16, D, 2, 0, -1, 0, true});
  cases.push_back({"packbits_i16", GSKYHIP_INT16, 33, 40, 2, 16, 16, P, 1, 6, -1, 0, true});
  cases.push_back({"packbits_constant", GSKYHIP_FLOAT32, 33, 40, 1, 16, 16, P, 1, 6, -1, 1, true});
  cases.push_back({"packbits_empty", GSKYHIP_BYTE, 300, 40, 3, 1024, 256, P, 1, 6, 1, 2, true});
  for (const Case &c : cases) run(c);
  if (fails) {
    std::printf("geotiff_check: %d failures\n", fails);
    return 1;
  }
  std::printf("geotiff_check ok: %zu files\n", cases.size());
  return 0;
}
