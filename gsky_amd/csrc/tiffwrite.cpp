// tiffwrite.cpp -- the host side of the WCS GeoTIFF writer (tiffwrite.h):
// plain C++17 without a HIP call (and without a HIP header under a host
// compiler), so that it also builds on its own (tools/geotiff_check.cpp).
//
// The opt-in Deflate file (compression 8) holds every tile as one zlib stream
// of the tile's block_y x block_x samples after the TIFF predictor:
//   1  none;
//   2  horizontal differencing: the differences of the samples' bit patterns
//      along a tile row, wrapping in the sample width, the first sample kept
//      (float32: of the 32-bit patterns);
//   3  floating point (TIFF Technical Note 3, float32 only): per tile row the
//      four byte planes, most significant first, then byte differences one
//      apart over the whole row of 4 * block_x bytes.
// The streams are the project's encoder's (deflate_core.h), not zlib's: here
// its host twin, on the device gskyhip_deflate_blocks' kernels -- the same
// bytes.  This option is beyond the reference, whose EncodeGdalOpen always
// writes PackBits.
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>   // the library builds every unit as HIP: deflate_core.h's device half needs it
#endif

#include "tiffwrite.h"

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>

#include "../../include/gskyhip.h"
#include "deflate_core.h"

namespace gsky {
namespace tiff {

int sample(int dtype, int &ts, uint16_t &fmt) {
  switch (dtype) {
    case GSKYHIP_BYTE: ts = 1; fmt = 1; return 0;
    case GSKYHIP_SIGNEDBYTE: ts = 1; fmt = 2; return 0;
    case GSKYHIP_INT16: ts = 2; fmt = 2; return 0;
    case GSKYHIP_UINT16: ts = 2; fmt = 1; return 0;
    case GSKYHIP_FLOAT32: ts = 4; fmt = 3; return 0;
    default: return GSKYHIP_E_TYPE;
  }
}

int Spec::check() {
  if (!geot || n_bands <= 0 || n_bands > 4096) return GSKYHIP_E_ARG;
  if (sample(dtype, ts, fmt)) return GSKYHIP_E_TYPE;
  if (width <= 0 || height <= 0 || block_x <= 0 || block_y <= 0 || block_x % 16 || block_y % 16) return GSKYHIP_E_ARG;
  if (compression == kPackBits) {
    if (predictor != 1) return GSKYHIP_E_ARG;
  } else if (compression == kDeflate) {
    if (predictor < 1 || predictor > 3 || (predictor == 3 && dtype != GSKYHIP_FLOAT32)) return GSKYHIP_E_ARG;
  } else {
    return GSKYHIP_E_ARG;
  }
  ntx = (width + block_x - 1) / block_x;
  nty = (height + block_y - 1) / block_y;
  tile_bytes = (int64_t)block_x * block_y * ts;
  if (compression == kDeflate && tile_bytes > kMaxTileBytes) return GSKYHIP_E_ARG;
  // EncodeGdal (ogc_encoders.go:357-436) skips EmptyTile bands: no nodata, no
  // long_name, no pixels -- GTiff fills their blocks at close with the
  // dataset nodata, the last value SetNoDataValue stored (one per GeoTIFF).
  empty.assign((size_t)n_bands, 0);
  last_nd = -1;
  for (int b = 0; b < n_bands; b++) {
    empty[b] = names && names[b] && std::strncmp(names[b], "EmptyTile", 9) == 0;
    if (!empty[b] && nodata) last_nd = b;
  }
  // edge-tile padding: the band's nodata in the band type (0 without one);
  // an EmptyTile band is all the dataset nodata
  pad.assign((size_t)n_bands * 8, 0);
  for (int b = 0; b < n_bands; b++) {
    uint8_t *pb = pad.data() + 8 * (size_t)b;
    const double v = empty[b] ? (last_nd >= 0 ? nodata[last_nd] : 0.0) : nodata ? nodata[b] : 0.0;
    if (dtype == GSKYHIP_FLOAT32) { const float f = (float)v; std::memcpy(pb, &f, 4); }
    else if (ts == 2) { const int16_t h = (int16_t)(dtype == GSKYHIP_UINT16 ? (int32_t)(uint16_t)v : (int32_t)v); std::memcpy(pb, &h, 2); }
    else pb[0] = (uint8_t)(int)v;
  }
  return 0;
}

namespace {

// BigTIFF writer state: IFD entries (sorted by tag on output) + out-of-line data.
struct TiffEntry {
  uint16_t tag, type;
  uint64_t count;
  std::vector<uint8_t> data;   // little-endian values
};

template <typename T> void put_le(std::vector<uint8_t> &o, T v) {
  for (size_t k = 0; k < sizeof(T); k++) o.push_back((uint8_t)((uint64_t)v >> (8 * k)));
}

TiffEntry tiff_shorts(uint16_t tag, const std::vector<uint16_t> &v) {
  TiffEntry e{tag, 3, v.size(), {}};
  for (uint16_t x : v) put_le(e.data, x);
  return e;
}
TiffEntry tiff_long(uint16_t tag, uint32_t v) {
  TiffEntry e{tag, 4, 1, {}};
  put_le(e.data, v);
  return e;
}
TiffEntry tiff_long8s(uint16_t tag, const std::vector<uint64_t> &v) {
  TiffEntry e{tag, 16, v.size(), {}};
  for (uint64_t x : v) put_le(e.data, x);
  return e;
}
TiffEntry tiff_doubles(uint16_t tag, const std::vector<double> &v) {
  TiffEntry e{tag, 12, v.size(), {}};
  for (double x : v) {
    uint64_t u;
    std::memcpy(&u, &x, 8);
    put_le(e.data, u);
  }
  return e;
}
TiffEntry tiff_ascii(uint16_t tag, const std::string &s) {
  TiffEntry e{tag, 2, s.size() + 1, {}};
  e.data.assign(s.begin(), s.end());
  e.data.push_back(0);
  return e;
}

bool epsg_geographic(int epsg) {
  return epsg == 4326 || epsg == 4283 || epsg == 4269 || epsg == 4258 || epsg == 4167 || epsg == 4674 ||
         epsg == 7844;
}

std::string xml_escape(const char *s) {
  std::string o;
  for (; s && *s; s++) {
    switch (*s) {
      case '&': o += "&amp;"; break;
      case '<': o += "&lt;"; break;
      case '>': o += "&gt;"; break;
      case '"': o += "&quot;"; break;
      default: o += *s;
    }
  }
  return o;
}

template <typename T> void diff_row(uint8_t *row, int n) {   // row[x] -= row[x - 1], wrapping in T
  for (int x = n - 1; x > 0; x--) {
    T a, b;
    std::memcpy(&a, row + (size_t)x * sizeof(T), sizeof(T));
    std::memcpy(&b, row + (size_t)(x - 1) * sizeof(T), sizeof(T));
    a = (T)(a - b);
    std::memcpy(row + (size_t)x * sizeof(T), &a, sizeof(T));
  }
}

}  // namespace

Writer::Writer(uint8_t *out, int64_t capacity, int64_t n_tiles) : out_(out), cap_(capacity) {
  toff_.reserve((size_t)n_tiles);
  tcnt_.reserve((size_t)n_tiles);
  std::vector<uint8_t> h;
  h.push_back('I'); h.push_back('I');
  put_le<uint16_t>(h, 43); put_le<uint16_t>(h, 8); put_le<uint16_t>(h, 0);
  put_le<uint64_t>(h, 0);   // first IFD offset, patched by finish()
  if ((int64_t)h.size() > cap_) { ok_ = false; return; }
  std::memcpy(out_, h.data(), h.size());
  at_ = (int64_t)h.size();
}

void Writer::begin_tile() { tile_at_ = at_; }

uint8_t *Writer::room(int64_t n) {
  if (!ok_ || n < 0 || n > cap_ - at_) { ok_ = false; return nullptr; }
  uint8_t *p = out_ + at_;
  at_ += n;
  return p;
}

void Writer::append(const uint8_t *p, int64_t n) {
  uint8_t *dst = room(n);
  if (dst && n) std::memcpy(dst, p, (size_t)n);
}

void Writer::end_tile() {
  toff_.push_back((uint64_t)tile_at_);
  tcnt_.push_back((uint64_t)(at_ - tile_at_));
}

int Writer::finish(const Spec &s, int64_t *size) {
  if (!ok_ || (int64_t)toff_.size() != s.n_tiles()) return GSKYHIP_E_ARG;
  const int n_bands = s.n_bands;
  const double *geot = s.geot;
  std::vector<uint8_t> o;   // from the IFD on
  if (at_ & 1) o.push_back(0);
  std::vector<TiffEntry> ents;
  ents.push_back(tiff_long(256, (uint32_t)s.width));
  ents.push_back(tiff_long(257, (uint32_t)s.height));
  ents.push_back(tiff_shorts(258, std::vector<uint16_t>((size_t)n_bands, (uint16_t)(8 * s.ts))));
  ents.push_back(tiff_shorts(259, {(uint16_t)s.compression}));   // PackBits, or Adobe Deflate
  // GTiff Create's default photometric: RGB for 3 or 4 Byte bands (the 4th
  // an associated alpha extra sample), MinIsBlack otherwise
  const bool byte = s.dtype == GSKYHIP_BYTE || s.dtype == GSKYHIP_SIGNEDBYTE;
  const bool rgb = byte && (n_bands == 3 || n_bands == 4);
  ents.push_back(tiff_shorts(262, {(uint16_t)(rgb ? 2 : 1)}));
  ents.push_back(tiff_shorts(277, {(uint16_t)n_bands}));
  ents.push_back(tiff_shorts(284, {(uint16_t)(n_bands > 1 ? 2 : 1)}));   // INTERLEAVE=BAND
  if (s.predictor != 1) ents.push_back(tiff_shorts(317, {(uint16_t)s.predictor}));
  ents.push_back(tiff_long(322, (uint32_t)s.block_x));
  ents.push_back(tiff_long(323, (uint32_t)s.block_y));
  ents.push_back(tiff_long8s(324, toff_));
  ents.push_back(tiff_long8s(325, tcnt_));
  if (rgb && n_bands == 4) ents.push_back(tiff_shorts(338, {1}));
  else if (!rgb && n_bands > 1) ents.push_back(tiff_shorts(338, std::vector<uint16_t>((size_t)n_bands - 1, 0)));
  ents.push_back(tiff_shorts(339, std::vector<uint16_t>((size_t)n_bands, s.fmt)));
  if (geot[2] == 0.0 && geot[4] == 0.0) {
    ents.push_back(tiff_doubles(33550, {geot[1], -geot[5], 0.0}));
    ents.push_back(tiff_doubles(33922, {0.0, 0.0, 0.0, geot[0], geot[3], 0.0}));
  } else {   // ModelTransformationTag for rotated grids
    ents.push_back(tiff_doubles(34264, {geot[1], geot[2], 0.0, geot[0], geot[4], geot[5], 0.0, geot[3],
                                        0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0}));
  }
  if (s.epsg > 0) {
    const bool geo = epsg_geographic(s.epsg);
    ents.push_back(tiff_shorts(34735, {1, 1, 0, 3, 1024, 0, 1, (uint16_t)(geo ? 2 : 1), 1025, 0, 1, 1,
                                       (uint16_t)(geo ? 2048 : 3072), 0, 1, (uint16_t)s.epsg}));
  }
  if (s.names) {   // GDALSetMetadataItem("long_name", NameSpace) per band
    std::string md = "<GDALMetadata>\n";
    for (int b = 0; b < n_bands; b++)
      if (s.names[b] && !s.empty[b])
        md += "  <Item name=\"long_name\" sample=\"" + std::to_string(b) + "\">" + xml_escape(s.names[b]) + "</Item>\n";
    md += "</GDALMetadata>";
    ents.push_back(tiff_ascii(42112, md));
  }
  if (s.last_nd >= 0) {   // GDAL_NODATA: a single dataset value, the last band's that set one
    char buf[64];
    std::snprintf(buf, sizeof(buf), "%.18g", s.nodata[s.last_nd]);
    ents.push_back(tiff_ascii(42113, buf));
  }
  std::sort(ents.begin(), ents.end(), [](const TiffEntry &a, const TiffEntry &b) { return a.tag < b.tag; });
  const uint64_t ifd = (uint64_t)at_ + o.size();
  const uint64_t ifd_bytes = 8 + 20 * ents.size() + 8;
  const uint64_t extra = ifd + ifd_bytes;
  std::vector<uint8_t> tail;
  put_le<uint64_t>(o, ents.size());
  for (auto &e : ents) {
    put_le<uint16_t>(o, e.tag);
    put_le<uint16_t>(o, e.type);
    put_le<uint64_t>(o, e.count);
    if (e.data.size() <= 8) {
      std::vector<uint8_t> v = e.data;
      v.resize(8, 0);
      o.insert(o.end(), v.begin(), v.end());
    } else {
      put_le<uint64_t>(o, extra + tail.size());
      tail.insert(tail.end(), e.data.begin(), e.data.end());
      if (tail.size() & 1) tail.push_back(0);
    }
  }
  put_le<uint64_t>(o, 0);   // no next IFD
  o.insert(o.end(), tail.begin(), tail.end());
  if ((int64_t)o.size() > cap_ - at_) return GSKYHIP_E_ARG;
  std::memcpy(out_ + at_, o.data(), o.size());
  at_ += (int64_t)o.size();
  for (int k = 0; k < 8; k++) out_[8 + k] = (uint8_t)(ifd >> (8 * k));
  *size = at_;
  return 0;
}

void predict_tile(const Spec &s, const uint8_t *band, int b, int tx, int ty, uint8_t *dst) {
  const int ts = s.ts, bx = s.block_x, by = s.block_y;
  const int64_t rb = (int64_t)bx * ts;
  const uint8_t *pad = s.pad.data() + 8 * (size_t)b;
  const int64_t x0 = (int64_t)tx * bx;
  const int nx = band ? (int)std::max<int64_t>(0, std::min<int64_t>(bx, s.width - x0)) : 0;
  std::vector<uint8_t> planes(s.predictor == 3 ? (size_t)rb : 0);
  for (int r = 0; r < by; r++) {
    uint8_t *row = dst + (int64_t)r * rb;
    const int64_t y = (int64_t)ty * by + r;
    const int n = y < s.height ? nx : 0;
    if (n) std::memcpy(row, band + (y * s.width + x0) * ts, (size_t)n * ts);
    for (int x = n; x < bx; x++) std::memcpy(row + (size_t)x * ts, pad, (size_t)ts);
    if (s.predictor == 2) {
      if (ts == 1) diff_row<uint8_t>(row, bx);
      else if (ts == 2) diff_row<uint16_t>(row, bx);
      else diff_row<uint32_t>(row, bx);
    } else if (s.predictor == 3) {   // ts == 4
      for (int x = 0; x < bx; x++)
        for (int p = 0; p < 4; p++) planes[(size_t)p * bx + x] = row[(size_t)x * 4 + 3 - p];
      row[0] = planes[0];
      for (int64_t i = 1; i < rb; i++) row[i] = (uint8_t)(planes[(size_t)i] - planes[(size_t)i - 1]);
    }
  }
}

int deflate_tile(const Spec &s, const uint8_t *band, int b, int tx, int ty, int zlevel, std::vector<uint8_t> &z) {
  std::vector<uint8_t> raw((size_t)s.tile_bytes);
  predict_tile(s, band, b, tx, ty, raw.data());
  const int64_t cap = deflate::bound(s.tile_bytes);
  z.resize((size_t)cap);
  int32_t status = -1;
  int64_t len = 0;
  deflate::encode_block_host(raw.data(), s.tile_bytes, z.data(), cap, 1, zlevel, &status, &len, nullptr);
  if (status != deflate::kOk || len <= 0 || len > cap) return GSKYHIP_E_ARG;
  z.resize((size_t)len);
  return 0;
}

int encode_host(const Spec &s, const void *const *bands, int zlevel, int n_threads, uint8_t *out, int64_t capacity,
                int64_t *size) {
  Writer W(out, capacity, s.n_tiles());
  const int64_t tpb = s.tiles_per_band();
  if (s.compression == kPackBits) {
    const int rb = (int)((int64_t)s.block_x * s.ts);
    std::vector<uint8_t> raw((size_t)s.tile_bytes), enc((size_t)(rb + rb / 128 + 2));
    for (int b = 0; b < s.n_bands; b++) {
      const uint8_t *band = s.empty[b] ? nullptr : (const uint8_t *)bands[b];
      for (int64_t t = 0; t < tpb; t++) {
        predict_tile(s, band, b, (int)(t % s.ntx), (int)(t / s.ntx), raw.data());
        W.begin_tile();
        for (int r = 0; r < s.block_y; r++)
          W.append(enc.data(), packbits_row(raw.data() + (int64_t)r * rb, rb, enc.data()));
        W.end_tile();
      }
    }
    return W.finish(s, size);
  }
  std::vector<uint8_t> empty_z;   // a tile that is all one pad value, compressed once
  uint32_t empty_pad = 0;
  for (int b = 0; b < s.n_bands; b++) {
    const uint8_t *band = s.empty[b] ? nullptr : (const uint8_t *)bands[b];
    if (!band) {
      if (empty_z.empty() || empty_pad != s.pad_bits(b)) {
        const int rc = deflate_tile(s, nullptr, b, 0, 0, zlevel, empty_z);
        if (rc) return rc;
        empty_pad = s.pad_bits(b);
      }
      for (int64_t t = 0; t < tpb; t++) {
        W.begin_tile();
        W.append(empty_z.data(), (int64_t)empty_z.size());
        W.end_tile();
      }
      continue;
    }
    std::vector<std::vector<uint8_t>> z((size_t)tpb);
    std::atomic<int64_t> next(0);
    std::atomic<int> err(0);
    auto work = [&]() {
      for (int64_t t = next++; t < tpb; t = next++) {
        const int rc = deflate_tile(s, band, b, (int)(t % s.ntx), (int)(t / s.ntx), zlevel, z[(size_t)t]);
        if (rc) err = rc;
      }
    };
    const int nth = (int)std::max<int64_t>(1, std::min<int64_t>(std::min(n_threads, 64), tpb));
    std::vector<std::thread> pool;
    for (int i = 1; i < nth; i++) pool.emplace_back(work);
    work();
    for (auto &th : pool) th.join();
    if (err.load()) return err.load();
    for (int64_t t = 0; t < tpb; t++) {
      W.begin_tile();
      W.append(z[(size_t)t].data(), (int64_t)z[(size_t)t].size());
      W.end_tile();
    }
  }
  return W.finish(s, size);
}

}  // namespace tiff
}  // namespace gsky

using namespace gsky;

extern "C" int64_t gskyhip_geotiff_bound(int width, int height, int n_bands, int dtype, int block_x, int block_y) {
  int ts;
  uint16_t fmt;
  if (width <= 0 || height <= 0 || n_bands <= 0 || block_x <= 0 || block_y <= 0 || tiff::sample(dtype, ts, fmt))
    return 0;
  const int64_t ntx = (width + block_x - 1) / block_x, nty = (height + block_y - 1) / block_y;
  const int64_t rows = (int64_t)n_bands * ntx * nty * block_y;
  const int64_t rb = (int64_t)block_x * ts;
  return rows * (rb + rb / 128 + 2) + (int64_t)n_bands * ntx * nty * 16 + 65536 + 512 * (int64_t)n_bands;
}

extern "C" int64_t gskyhip_geotiff_bound_opts(int width, int height, int n_bands, int dtype, int block_x, int block_y,
                                              int compression) {
  if (compression == GSKYHIP_TIFF_PACKBITS)
    return gskyhip_geotiff_bound(width, height, n_bands, dtype, block_x, block_y);
  int ts;
  uint16_t fmt;
  if (compression != GSKYHIP_TIFF_DEFLATE || width <= 0 || height <= 0 || n_bands <= 0 || block_x <= 0 ||
      block_y <= 0 || tiff::sample(dtype, ts, fmt))
    return 0;
  const int64_t ntx = (width + block_x - 1) / block_x, nty = (height + block_y - 1) / block_y;
  const int64_t tiles = (int64_t)n_bands * ntx * nty;
  return tiles * deflate::bound((int64_t)block_x * block_y * ts) + tiles * 16 + 65536 + 512 * (int64_t)n_bands;
}

extern "C" int gskyhip_encode_geotiff_host(const void *const *bands, int n_bands, int dtype, int width, int height,
                                           const double *geot, int epsg, const double *nodata,
                                           const char *const *names, int block_x, int block_y, int compression,
                                           int predictor, int zlevel, int n_threads, uint8_t *out, int64_t capacity,
                                           int64_t *size) {
  if (!bands || !out || !size) return GSKYHIP_E_ARG;
  try {
    tiff::Spec s;
    s.n_bands = n_bands; s.dtype = dtype; s.width = width; s.height = height;
    s.geot = geot; s.epsg = epsg; s.nodata = nodata; s.names = names;
    s.block_x = block_x; s.block_y = block_y; s.compression = compression; s.predictor = predictor;
    const int rc = s.check();
    if (rc) return rc;
    if (zlevel < 0 || zlevel > 9) return GSKYHIP_E_ARG;
    if (capacity < gskyhip_geotiff_bound_opts(width, height, n_bands, dtype, block_x, block_y, compression))
      return GSKYHIP_E_ARG;
    return tiff::encode_host(s, bands, zlevel, n_threads, out, capacity, size);
  } catch (...) {
    return GSKYHIP_E_ARG;
  }
}
