// tiffwrite.h -- the host side of the WCS GeoTIFF writer, plain C++17 (no
// HIP): the band rules of EncodeGdal (EmptyTile bands, the dataset nodata,
// the pad value of edge tiles), the BigTIFF framing (header, tile data, IFD,
// out-of-line tag data), PackBits of a tile row, the TIFF predictors 2 and 3
// of a tile, and the whole writer over host bands.  encode.hip's two device
// entry points frame their files with the same Writer; tools/geotiff_check.cpp
// builds tiffwrite.cpp on its own.
#ifndef GSKY_TIFFWRITE_H
#define GSKY_TIFFWRITE_H

#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define GSKY_TW_HD __host__ __device__ inline
#else
#define GSKY_TW_HD inline
#endif

namespace gsky {
namespace tiff {

constexpr int kPackBits = 32773, kDeflate = 8;
constexpr int64_t kMaxTileBytes = 1ll << 30;       // a tile is one Deflate block
constexpr int64_t kSlabRawBytes = 16ll << 20;      // raw tile bytes of a slab of the library's choice
constexpr int kSlabMaxTiles = 32768;

// PackBits (TIFF 6.0 section 9) of one tile row (libtiff encodes tiled
// PackBits row by row): runs of 3+ equal bytes as replicate runs, the rest
// as literal runs, at most 128 bytes each.  Returns the encoded length (at
// most n + n / 128 + 2).
GSKY_TW_HD int packbits_row(const uint8_t *in, int n, uint8_t *out) {
  int i = 0, o = 0;
  while (i < n) {
    int run = 1;
    while (i + run < n && run < 128 && in[i + run] == in[i]) run++;
    if (run >= 3) {
      out[o++] = (uint8_t)(257 - run);   // -(run - 1)
      out[o++] = in[i];
      i += run;
      continue;
    }
    // literal: up to the next run of 3 (or 128 bytes)
    int j = i, lit = 0;
    while (j < n && lit < 128) {
      if (j + 2 < n && in[j] == in[j + 1] && in[j] == in[j + 2]) break;
      j++;
      lit++;
    }
    out[o++] = (uint8_t)(lit - 1);
    for (int k = 0; k < lit; k++) out[o++] = in[i + k];
    i += lit;
  }
  return o;
}

// sample size and SampleFormat of a GSKYHIP_* type; GSKYHIP_E_TYPE otherwise
int sample(int dtype, int &ts, uint16_t &fmt);

// One coverage as the entry points receive it, checked (check()) and with
// the band rules resolved.
struct Spec {
  int n_bands = 0, dtype = 0, width = 0, height = 0;
  const double *geot = nullptr;
  int epsg = 0;
  const double *nodata = nullptr;
  const char *const *names = nullptr;
  int block_x = 0, block_y = 0;
  int compression = kPackBits, predictor = 1;
  // derived by check()
  int ts = 0;
  uint16_t fmt = 0;
  int ntx = 0, nty = 0;
  int64_t tile_bytes = 0;
  std::vector<char> empty;    // EncodeGdal skips the band (its name starts with "EmptyTile")
  int last_nd = -1;           // the band whose nodata the file keeps
  std::vector<uint8_t> pad;   // 8 bytes a band: the sample edge tiles (and empty bands) are filled with

  int64_t tiles_per_band() const { return (int64_t)ntx * nty; }
  int64_t n_tiles() const { return (int64_t)n_bands * ntx * nty; }
  uint32_t pad_bits(int b) const {
    return (uint32_t)pad[8 * (size_t)b] | (uint32_t)pad[8 * (size_t)b + 1] << 8 | (uint32_t)pad[8 * (size_t)b + 2] << 16 |
           (uint32_t)pad[8 * (size_t)b + 3] << 24;
  }
  // what gskyhip_encode_geotiff checks of these, then compression (PackBits
  // with predictor 1; Deflate with 1, 2, or 3 for float32) and the tile size;
  // fills the derived members.  GSKYHIP_E_ARG / GSKYHIP_E_TYPE.
  int check();
};

// The file: header | tile data (band-major, tiles row-major) | IFD |
// out-of-line tag data, written straight into `out`.
class Writer {
 public:
  Writer(uint8_t *out, int64_t capacity, int64_t n_tiles);
  void begin_tile();
  void append(const uint8_t *p, int64_t n);   // bytes of the open tile
  uint8_t *room(int64_t n);                   // n bytes of the open tile to be filled by the caller (NULL: full)
  void end_tile();
  uint8_t *cursor() const { return out_ + at_; }
  int64_t left() const { return cap_ - at_; }
  bool ok() const { return ok_; }
  // the IFD for `s`; *size = the file's length.  GSKYHIP_E_ARG when the file did not fit.
  int finish(const Spec &s, int64_t *size);

 private:
  uint8_t *out_;
  int64_t cap_, at_ = 0, tile_at_ = 0;
  bool ok_ = true;
  std::vector<uint64_t> toff_, tcnt_;
};

// Tile (tx, ty) of a host band (NULL: all pad) as the compressor receives it:
// block_y rows of block_x samples, edge tiles padded, the predictor applied.
// dst: tile_bytes.
void predict_tile(const Spec &s, const uint8_t *band, int b, int tx, int ty, uint8_t *dst);

// The zlib stream of one predicted tile of band b by the encoder's host twin.
int deflate_tile(const Spec &s, const uint8_t *band, int b, int tx, int ty, int zlevel, std::vector<uint8_t> &z);

// The whole file from host bands.
int encode_host(const Spec &s, const void *const *bands, int zlevel, int n_threads, uint8_t *out, int64_t capacity,
                int64_t *size);

}  // namespace tiff
}  // namespace gsky

#endif
