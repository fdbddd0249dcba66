// deflate.h -- what nc4write.cpp uses of deflate.hip: the chunks of a slab of
// coverage rows shuffled and deflated on the device.
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

}  // namespace gsky

#endif
