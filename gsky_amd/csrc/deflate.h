// deflate.h -- what the coverage writers use of deflate.hip: the chunks of a
// slab of coverage rows shuffled and deflated on the device (nc4write.cpp),
// and the tiles of a slab of GeoTIFF tiles predicted and deflated there
// (encode.hip).
#ifndef GSKY_DEFLATE_H
#define GSKY_DEFLATE_H

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

namespace gsky {

constexpr int64_t kNcSlabRawBytes = 16ll << 20;   // raw chunk bytes of a slab of the library's choice
constexpr int kNcSlabMaxRows = 65536;

// rows of a slab for rows of row_bytes: slab_rows if positive, else the
// library's choice (kNcSlabRawBytes of raw chunks, at least one row)
int nc_slab_rows(int64_t row_bytes, int height, int slab_rows);

// device bytes nc_deflate_slab needs for slabs of `rows` rows
int64_t nc_deflate_workspace(int64_t row_bytes, int rows);

// File rows [j0, j0 + rows) of a band (height x width of src_size-byte
// elements in HBM; file row j = image row height - 1 - j) widened to
// elem_size bytes (UInt16 -> int32), shuffled and deflated (zlib streams) on
// the device: z[j0 + i] receives chunk i's bytes.  copied += the compressed
// bytes brought to the host.  Returns a GSKYHIP_* code.
int nc_deflate_slab(const void *dev_band, int src_size, int elem_size, int width, int height, int j0, int rows,
                    int level, uint8_t *ws, int64_t ws_bytes, std::vector<std::vector<uint8_t>> &z, int64_t *copied,
                    hipStream_t s);

// tiles of a GeoTIFF slab for tiles of tile_bytes: slab_tiles if positive,
// else the library's choice (tiff::kSlabRawBytes of raw tiles, at least one)
int tiff_slab_tiles(int64_t tile_bytes, int64_t tiles_per_band, int slab_tiles);

// device bytes tiff_deflate_slab needs for slabs of `tiles` tiles
int64_t tiff_deflate_workspace(int64_t tile_bytes, int tiles);

// Tiles [tile0, tile0 + tiles) of a band (row-major over the band's ntx
// columns of tiles; height x width samples of ts bytes in HBM, NULL: all
// pad) gathered with edge padding (`pad`: the sample's bits), the TIFF
// predictor applied, and each deflated into one zlib stream on the device;
// the streams, packed end to end, are copied to dst (dst_cap bytes;
// GSKYHIP_E_ARG when they do not fit) and lens[k] receives the length of
// tile tile0 + k's.  copied += the compressed bytes brought to the host.
int tiff_deflate_slab(const void *dev_band, int ts, int predictor, int width, int height, int block_x, int block_y,
                      int ntx, int64_t tile0, int tiles, uint32_t pad, int level, uint8_t *ws, int64_t ws_bytes,
                      uint8_t *dst, int64_t dst_cap, int64_t *lens, int64_t *copied, hipStream_t s);

}  // namespace gsky

#endif
