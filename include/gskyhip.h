/*
 * gskyhip.h -- C-ABI of the MI355X-native GSKY raster hot path.
 *
 * libgskyhip.so (gsky_amd/libgskyhip.so) implements GSKY's per-request
 * raster hot path on gfx950 with hand-written HIP kernels:
 *   warp (reprojection + nearest/bilinear resampling)
 *   -> nodata-aware time-ordered mosaic (merge, masks)
 *   -> byte scaling -> palette / RGBA fill
 * and the drill (zonal) reduction.
 *
 * Every entry point names the reference interface it replaces
 * (chuc92man/gsky file:line).  Signatures use plain C types and pointers only.
 * "dev" pointers are HIP device pointers (hipMalloc / torch CUDA tensors);
 * `stream` is a hipStream_t passed as void* (NULL = default stream).
 * Batch entry points are asynchronous on `stream` and never allocate,
 * synchronise or copy to the host, so they can be captured in a hipGraph.
 *
 * Error codes: 0 OK; >0 follow the reference where one exists
 * (warp.go:103-140: 1 open failed, 2 band failed, 3 transformer failed);
 * negative values are GSKYHIP_E_* below.
 */
#ifndef GSKYHIP_H
#define GSKYHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- error codes -------------------------------------------------------- */
#define GSKYHIP_OK 0
#define GSKYHIP_E_ARG (-1)         /* bad argument / size                     */
#define GSKYHIP_E_TYPE (-2)        /* raster type not implemented             */
#define GSKYHIP_E_HIP (-3)         /* HIP runtime error                       */
#define GSKYHIP_E_CRS (-4)         /* unsupported CRS                          */
#define GSKYHIP_E_MASK (-5)        /* bad mask spec (tile_merger.go:315-323)   */
#define GSKYHIP_E_NOGPU (-6)       /* no HIP device                            */
#define GSKYHIP_E_RANGE (-7)       /* index out of range (Go would panic)      */
#define GSKYHIP_E_XFORM (-8)       /* GDALSuggestedWarpOutput() failed         */
#define GSKYHIP_E_SERVICE (-9)     /* per-node service unreachable / protocol  */

/* ---- raster data types: GDALDataType codes (warp.go:428-431) + 100 ------- */
#define GSKYHIP_BYTE 1
#define GSKYHIP_UINT16 2
#define GSKYHIP_INT16 3
#define GSKYHIP_UINT32 4
#define GSKYHIP_INT32 5
#define GSKYHIP_FLOAT32 6
#define GSKYHIP_FLOAT64 7
#define GSKYHIP_SIGNEDBYTE 100     /* warp.go:354-359 */

/* ---- coordinate reference systems --------------------------------------- */
#define GSKYHIP_CRS_LONGLAT 0      /* EPSG:4326, traditional GIS order, deg   */
#define GSKYHIP_CRS_WEBMERC 1      /* EPSG:3857                                 */
#define GSKYHIP_CRS_AEA 2          /* EPSG:3577 (GDA94 / Australian Albers)    */
#define GSKYHIP_CRS_SINU 3         /* MODIS sinusoidal, sphere R=6371007.181    */
#define GSKYHIP_CRS_TMERC 4        /* Transverse Mercator, ellipsoidal: UTM     *
                                    * (EPSG:326zz / 327zz), GDA94 / GDA2020 MGA *
                                    * (EPSG:283zz / 78zz), +proj=tmerc / utm    */
#define GSKYHIP_CRS_LCC 5          /* Lambert Conformal Conic, ellipsoidal, 1SP *
                                    * or 2SP: GDA94 / GDA2020 GA Lambert        *
                                    * (EPSG:3112 / 7845), +proj=lcc; constants   *
                                    * in n, c, rho0                              */
#define GSKYHIP_CRS_STERE_POLAR 6  /* polar stereographic, ellipsoidal: EPSG:3031 *
                                    * / 3413 / 3976, UPS 32661 / 32761,          *
                                    * +proj=stere +lat_0=+-90 / +proj=ups; akm1  *
                                    * in c, |lat_ts| in phi1                     */
#define GSKYHIP_CRS_GEOS 7         /* geostationary satellite view, ellipsoid or *
                                    * sphere: +proj=geos +h +lon_0 +sweep (y:    *
                                    * Himawari / Meteosat, x: GOES-R), WKT1       *
                                    * Geostationary_Satellite, CF geostationary; *
                                    * no EPSG code.  In units of a: h / a in     *
                                    * phi1, sweep flag (1: x) in phi2, radius_g  *
                                    * = 1 + h / a in n, radius_g^2 - 1 in c,     *
                                    * radius_p = sqrt(1 - es) in dd, 1 - es in   *
                                    * rho0, 1 / (1 - es) in ec.  The first kind  *
                                    * whose transform fails over whole regions:  *
                                    * forward beyond the limb, inverse off the   *
                                    * disc (ok = 0 in gskyhip_crs_transform)     */
#define GSKYHIP_CRS_LAEA 8         /* Lambert azimuthal equal area, ellipsoid or *
                                    * sphere, all four aspects: EASE-Grid 2.0    *
                                    * North / South (EPSG:6931 / 6932), ETRS89-   *
                                    * extended LAEA Europe (EPSG:3035), the       *
                                    * spherical EASE grids (EPSG:3408 / 3409),    *
                                    * +proj=laea, WKT1 Lambert_Azimuthal_Equal_   *
                                    * Area, CF lambert_azimuthal_equal_area.      *
                                    * lat_0 in phi0; aspect in phi2 (0 north      *
                                    * polar, 1 south polar, 2 equatorial, 3       *
                                    * oblique); qp in n, rq in c, dd in dd, xmf   *
                                    * in rho0, ymf in ec; and in the slots no     *
                                    * non-tmerc kind uses: sinb1 in tm_qn, cosb1  *
                                    * in tm_zb, the authalic series apa[0..2] in  *
                                    * tm_cgb[0..2].  All derive from a, es and    *
                                    * phi0.  The forward fails at the antipode of *
                                    * the centre, the inverse outside the disc    */
#define GSKYHIP_CRS_CEA 9          /* cylindrical equal area, ellipsoid or sphere: *
                                    * EASE-Grid 2.0 Global (EPSG:6933), the       *
                                    * spherical global EASE grid (EPSG:3410),     *
                                    * +proj=cea +lat_ts | +k_0, WKT1 Cylindrical_ *
                                    * Equal_Area, CF lambert_cylindrical_equal_   *
                                    * area.  k0 (from lat_ts, else given) in k0,  *
                                    * lat_ts in phi1, qp in n, apa[0..2] in       *
                                    * tm_cgb[0..2].  The inverse fails beyond the *
                                    * pole line                                   */
#define GSKYHIP_CRS_MERC 10        /* Mercator on an ellipsoid (1SP / 2SP), or on *
                                    * a sphere with lat_ts != 0 or k_0 != 1:      *
                                    * World Mercator (EPSG:3395), PDC Mercator    *
                                    * (EPSG:3832), +proj=merc, WKT1 Mercator_1SP  *
                                    * / Mercator_2SP, CF mercator.  k0 (from      *
                                    * lat_ts, else given) in k0, |lat_ts| in phi1. *
                                    * The forward fails at the poles.  The        *
                                    * spherical k0 = 1 case stays WEBMERC         */

typedef struct {
    int32_t kind;
    int32_t _pad;
    double a, ra, es, e, one_es;
    double lam0, phi0, phi1, phi2, x0, y0, k0;
    double n, c, dd, rho0, ec;      /* aea constants                           */
    /* tmerc (Poder / Engsager, 6th order): normalised meridian quadrant,
     * northing of the origin latitude, and the trigonometric series
     * Gaussian <-> geodetic latitude (cgb, cbg) and ellipsoidal <->
     * spherical northing / easting (utg, gtu)                                */
    double tm_qn, tm_zb;
    double tm_cgb[6], tm_cbg[6], tm_utg[6], tm_gtu[6];
} gskyhip_crs;

/* Parse an SRS as handed over by gsky-ows (tile_grpc.go:127-136 exports the
 * request CRS as WKT): WKT with a top-level AUTHORITY["EPSG",...], "EPSG:n",
 * a proj4 string, or "MODIS".  Returns 0 or GSKYHIP_E_CRS. */
int gskyhip_crs_from_srs(const char *srs, gskyhip_crs *out);

/* The coordinate transformation of the warp's GenImgProj transformer between
 * two parsed CRSs (PROJ pj_inv of src, then pj_fwd of dst; the
 * OGRCoordinateTransformation step of warp.go:130), on the host with the same
 * functions the kernels run: x[i], y[i] in place, ok[i] = 1 or 0 (the
 * transform failed; x / y then undefined).  Returns 0 or GSKYHIP_E_ARG. */
int gskyhip_crs_transform(const gskyhip_crs *src, const gskyhip_crs *dst, int n, double *x, double *y,
                          int32_t *ok);

/* ---- granules (the HBM-resident stand-in for an opened GDAL dataset) ----- */
#define GSKYHIP_MAX_OVR 12
typedef struct {
    const void *data;            /* dev: ysize x xsize of dtype, row-major   */
    int32_t dtype;               /* GSKYHIP_* (Byte for SignedByte data)       */
    int32_t xsize, ysize;
    int32_t signed_byte;         /* PIXELTYPE=SIGNEDBYTE                        */
    double geot[6];              /* GDALGetGeoTransform                          */
    double nodata;               /* GDALGetRasterNoDataValue (-1e10 if unset)   */
    int32_t has_nodata;
    int32_t crs;                 /* index into the CRS table of the call        */
    int32_t n_ovr;
    int32_t ns;                  /* namespace slot of this granule (merge)      */
    const void *ovr_data[GSKYHIP_MAX_OVR];  /* dev, finest first (GDALGetOverview) */
    int32_t ovr_xsize[GSKYHIP_MAX_OVR];
    int32_t ovr_ysize[GSKYHIP_MAX_OVR];
    double timestamp;            /* GeoTileGranule.TimeStamp                     */
    uint32_t polygon_hash;       /* fnv32a(GeoTileGranule.Polygon)               */
    int32_t block_x, block_y;    /* GDALGetBlockSize of the band (0: xsize x 1);  *
                                  * only bytesRead (warp.go:347) depends on it    */
    int32_t geoloc;              /* 0; k > 0: the k-th geolocation transformer of *
                                  * the call (the drop-in's GeoLocOpts requests) */
} gskyhip_granule;

/* One output tile of a GetMap batch.  Granules of the tile are
 * pair_granule[pair_begin..pair_end) in indexer / gRPC fan-out order
 * (tile_grpc.go:200-289). */
typedef struct {
    double dst_geot[6];          /* BBox2Geot (tile_grpc.go:380-382)             */
    int32_t width, height;
    int32_t pair_begin, pair_end;
} gskyhip_tile;

/* Scale parameters, utils.ScaleParams (raster_scaler.go:8-13). */
typedef struct {
    double offset, scale, clip;
    int32_t colour_scale;
    int32_t _pad;
} gskyhip_scale_params;

/* Mask layer, utils.Mask (utils/config.go:73-80).  `ns` is the namespace slot
 * whose rasters are the mask (Mask.ID == NameSpace); -1 = no mask.  value is
 * the base-2 Mask.Value string (may be NULL); bit_tests pairs. */
#define GSKYHIP_MAX_BIT_TESTS 8
typedef struct {
    int32_t ns;
    int32_t inclusive;
    int32_t n_bit_tests;         /* number of strings in bit_tests (even)        */
    int32_t _pad;
    const char *value;
    const char *bit_tests[GSKYHIP_MAX_BIT_TESTS];
} gskyhip_mask;

/* ---- native granule ingest ------------------------- */
/* What GDALOpenEx + GDALGetGeoTransform / GetRasterNoDataValue / GetOverview
 * report for a GeoTIFF (warp.go:89-101, 156-198, 246): classic TIFF and
 * BigTIFF, striped or tiled, chunky or planar, none / LZW / Deflate /
 * PackBits, predictors 1-3, 8-64 bit samples.  epsg: ProjectedCSTypeGeoKey
 * or GeographicTypeGeoKey, -1 for a user-defined sinusoidal on the MODIS
 * sphere, 0 when unknown.  nodata -1e10 when GDAL_NODATA is absent (the
 * value GDALGetRasterNoDataValue returns, warp.go:246). */
typedef struct {
    int32_t xsize, ysize, n_bands, dtype;
    int32_t signed_byte, block_x, block_y;
    int32_t compression, predictor, planar;
    int32_t epsg, has_nodata, n_ovr, _pad;
    double geot[6];
    double nodata;
    int32_t ovr_xsize[GSKYHIP_MAX_OVR], ovr_ysize[GSKYHIP_MAX_OVR];
} gskyhip_raster_info;

int gskyhip_geotiff_info(const char *path, gskyhip_raster_info *info);
/* Band `band` (1-based) of level `level` (0 = full resolution, k = overview
 * k) row-major into HOST memory (no device work; out_bytes >= x*y*size). */
int gskyhip_geotiff_read_host(const char *path, int band, int level, void *out, int64_t out_bytes);
/* The same into device memory: blocks decompressed by host threads into
 * pinned staging, one H2D copy, placed row-major on the GPU; returns after
 * the copy (the staging buffer is freed). */
int gskyhip_geotiff_read(const char *path, int band, int level, void *dev_out, int64_t out_bytes, void *stream);
/* Decode every level of (path, band) into HBM owned by the library and
 * register it for warp_operation_fast (freed by gskyhip_unregister_all).
 * warp_operation_fast does this itself for an unregistered *.tif / *.tiff
 * path, as GDALOpenEx would open it.  Returns 0, 1 (open failed), 2 (no such
 * band) or GSKYHIP_E_*. */
int gskyhip_register_geotiff(const char *path, int band);
/* netCDF classic (CDF-1/2/5) the way the GSKY_netCDF driver presents it
 * (libs/gdal/frmts/gsky_netcdf/netcdfdataset.cpp): path "NETCDF:file:var"
 * or a file holding one data variable; band = index along the leading
 * dimension of a 3-D variable (band_query, netcdfdataset.cpp:6994-7021);
 * geotransform from the coordinate variables (3504-3655, y increasing ->
 * rows returned north first); nodata from _FillValue / missing_value. */
int gskyhip_netcdf_info(const char *path, gskyhip_raster_info *info);
int gskyhip_netcdf_read_host(const char *path, int band, void *out, int64_t out_bytes);
/* The dataset SRS GSKY_netCDF reports for the srs_cf open option
 * (warp.go:95, netcdfdataset.cpp:7023-7025, 3661-3720): srs_cf = 0 -- the
 * grid mapping's GDAL WKT (spatial_ref / crs_wkt) when it names an EPSG
 * code, else the CF grid-mapping attributes; srs_cf = 1 -- the CF attributes
 * only.  out: "EPSG:<n>", a PROJ string, "" (none: the warp takes WGS84) or
 * "?" (a CF mapping outside the supported projections). */
int gskyhip_netcdf_srs(const char *path, int srs_cf, char *out, int cap);
int gskyhip_netcdf_read(const char *path, int band, void *dev_out, int64_t out_bytes, void *stream);
/* Decode (path, band) into library-owned HBM and register it; what
 * warp_operation_fast does itself for an unregistered netCDF path. */
int gskyhip_register_netcdf(const char *path, int band);

/* ---- overview pyramids built on the GPU ---------------------------------- */
/* For granules that come without overviews (netCDF, plain GeoTIFF, bands
 * registered from HBM), so that the overview pick of the warp (warp.go:
 * 156-198) has levels to choose from; what gdaladdo does offline.
 * Level k is ceil(n / 2^k) per axis (GDAL's (n + f - 1) / f); levels are
 * produced while max(xsize, ysize) of the level before exceeds min_size
 * (<= 0: 256), at most GSKYHIP_MAX_OVR.
 * NEAREST: level k (i, j) = level k-1 (2i, 2j) (QA / bit-mask bands).
 * AVERAGE, cascaded: level k (i, j) = mean of the valid pixels among level
 * k-1 (2i..2i+1, 2j..2j+1) clipped to the extent, from the stored (rounded)
 * values of level k-1.  Invalid: has_nodata and equal to the typed nodata
 * (GDALCopyWords of `nodata`, the warp's window fill, warp.go:247), or a
 * float32 NaN.  No valid pixel: the typed nodata, or without a nodata value
 * (an all-NaN float box) the quiet NaN 0x7fc00000.  Byte, SignedByte, Int16,
 * UInt16: exact int32 sum, sum / count rounded half away from zero in integer
 * arithmetic; Float32: fp32 sum from +0 in row-major box order, one fp32
 * division by the count.  A result is stored as computed, even if it happens
 * to equal the nodata value.  UInt32, Int32 and Float64: GSKYHIP_E_TYPE.
 * Parity with GDAL's overviews is unpinned. */
#define GSKYHIP_OVR_NEAREST 0
#define GSKYHIP_OVR_AVERAGE 1
/* level sizes, finest first (either array may be NULL); returns the level
 * count (0..12) or GSKYHIP_E_ARG */
int gskyhip_overview_levels(int xsize, int ysize, int min_size, int32_t *ovr_xsize, int32_t *ovr_ysize);
/* src and ovr_out[k] are device pointers (ovr_out, ovr_xsize, ovr_ysize:
 * host arrays of n_levels <= 12 entries, the first n_levels sizes that
 * gskyhip_overview_levels gives); dtype GSKYHIP_BYTE with signed_byte, or
 * GSKYHIP_SIGNEDBYTE, for int8.  Asynchronous on `stream`, no allocation:
 * one launch per three levels.  Arguments are checked before any HIP call. */
int gskyhip_build_overviews(const void *src, int dtype, int signed_byte, int xsize, int ysize,
                            int has_nodata, double nodata, int method, int n_levels,
                            void *const *ovr_out, const int32_t *ovr_xsize, const int32_t *ovr_ysize, void *stream);
/* gskyhip_register_geotiff / _netcdf, and when the band came without
 * overviews a pyramid of `method` down to `min_size` built into HBM the
 * library owns (freed with the granule).  A file's own overviews always win:
 * nothing is built over them.  GSKYHIP_E_TYPE (nothing registered) for a
 * band type the pyramid does not cover.  The request is remembered: when the
 * drop-in reads the file again (changed on disk, or evicted from the ingest
 * cache) it builds the same pyramid, until the plain register call or
 * gskyhip_unregister_all.
 * warp_operation_fast's own ingest of an unregistered path does the same
 * when GSKYHIP_BUILD_OVERVIEWS=nearest|average is in the environment (read
 * once; GSKYHIP_OVERVIEW_MIN_SIZE optional; unset or empty: no pyramid; band
 * types the pyramid does not cover are ingested without one). */
int gskyhip_register_geotiff_ovr(const char *path, int band, int method, int min_size);
int gskyhip_register_netcdf_ovr(const char *path, int band, int method, int min_size);

/* ---- Deflate decoded on the GPU; ingest with device-side block decode ----- */
/* Per-block status of gskyhip_inflate_blocks (RFC 1950 / 1951 streams). */
#define GSKYHIP_INFLATE_OK 0
#define GSKYHIP_INFLATE_E_INPUT 1     /* input truncated                          */
#define GSKYHIP_INFLATE_E_BLOCK 2     /* bad block type or header                 */
#define GSKYHIP_INFLATE_E_CODES 3     /* bad code lengths / invalid code          */
#define GSKYHIP_INFLATE_E_DIST 4      /* distance before the start of the output  */
#define GSKYHIP_INFLATE_E_CAP 5       /* output capacity exceeded                 */
#define GSKYHIP_INFLATE_E_CHECKSUM 6  /* Adler-32 mismatch                        */
#define GSKYHIP_INFLATE_E_SHORT 7     /* output shorter than required             */
/* n_blocks independent streams, one wave64 each: block k reads
 * dev_in[in_off[k] .. + in_len[k]) and writes dev_out[out_off[k] .. ) with at
 * most out_cap[k] bytes; fewer than out_need[k] (<= out_cap[k]) bytes is
 * GSKYHIP_INFLATE_E_SHORT.  zlib_wrapper: 1 -- RFC 1950 header and Adler-32
 * (verified); 0 -- a raw RFC 1951 stream.  The five offset / length arrays and
 * status / out_len (n_blocks each) are HOST memory; in_len[k] < 2^32.  No byte
 * outside a block's ranges is read or written whatever the stream holds; out
 * bytes past out_len[k], and all of them when status[k] != 0, are unspecified.
 * Returns GSKYHIP_OK once the launch has completed (the call waits for
 * `stream`); per-block results are in status[].  The _host twin runs the same
 * decoder (csrc/inflate_core.h) on up to 16 host threads over host pointers. */
int gskyhip_inflate_blocks(const uint8_t *dev_in, const int64_t *in_off, const int64_t *in_len, int n_blocks,
                           uint8_t *dev_out, const int64_t *out_off, const int64_t *out_cap,
                           const int64_t *out_need, int zlib_wrapper, int32_t *status, int64_t *out_len,
                           void *stream);
int gskyhip_inflate_blocks_host(const uint8_t *in, const int64_t *in_off, const int64_t *in_len, int n_blocks,
                                uint8_t *out, const int64_t *out_off, const int64_t *out_cap,
                                const int64_t *out_need, int zlib_wrapper, int32_t *status, int64_t *out_len);
/* ---- Deflate encoded on the GPU: the mirror of gskyhip_inflate_blocks ------ */
/* n_blocks independent blocks: block k, dev_in[in_off[k] .. + in_len[k]), is
 * compressed on its own into a complete RFC 1950 stream (zlib_wrapper 1:
 * header 78 9C, Adler-32) or a raw RFC 1951 stream (zlib_wrapper 0) at
 * dev_out[out_off[k] .. ).  level 0: stored blocks only; levels 1-9: the one
 * device encoding (csrc/deflate_core.h) -- of a dynamic-Huffman block, a
 * fixed-Huffman block and stored blocks the one whose stream is the shortest,
 * so out_len[k] <= gskyhip_deflate_bound(in_len[k]) for every input.  The
 * stream length is known before a byte is written: when it exceeds out_cap[k]
 * the block gets GSKYHIP_INFLATE_E_CAP, none of its bytes is written and
 * out_len[k] is the length it needs.  The offset / length arrays and status /
 * out_len (n_blocks each) are HOST memory; in_len[k] <= 2^30.  No byte outside
 * a block's ranges is read or written.  The bytes depend only on the block's
 * bytes, zlib_wrapper and level.  workspace: device memory of at least
 * gskyhip_deflate_workspace_size(n_blocks, sum of in_len) bytes (about 5.3
 * times the input).  Returns GSKYHIP_OK once the launch has completed (the
 * call waits for `stream`).  The _host twin gives the same bytes from the same
 * encoder on up to 16 host threads over host pointers, without a workspace. */
int64_t gskyhip_deflate_bound(int64_t in_len);   /* in_len + 5 * (in_len / 65535 + 1) + 6 */
int64_t gskyhip_deflate_workspace_size(int n_blocks, int64_t total_in_len);
int gskyhip_deflate_blocks(const uint8_t *dev_in, const int64_t *in_off, const int64_t *in_len, int n_blocks,
                           uint8_t *dev_out, const int64_t *out_off, const int64_t *out_cap, int zlib_wrapper,
                           int level, void *workspace, int64_t workspace_bytes, int32_t *status, int64_t *out_len,
                           void *stream);
int gskyhip_deflate_blocks_host(const uint8_t *in, const int64_t *in_off, const int64_t *in_len, int n_blocks,
                                uint8_t *out, const int64_t *out_off, const int64_t *out_cap, int zlib_wrapper,
                                int level, int32_t *status, int64_t *out_len);
/* gskyhip_geotiff_read / gskyhip_netcdf_read with the block decode on the
 * device.  decode = GSKYHIP_DECODE_HOST is exactly the call without _decode.
 * GSKYHIP_DECODE_DEVICE: the band's *compressed* blocks go to HBM in one copy,
 * are inflated there (gskyhip_inflate_blocks), un-predicted / un-shuffled /
 * byte-swapped and placed row-major by kernels.  GeoTIFF: compression 1, 8 and
 * 32946, every layout and predictor the host path reads; LZW and PackBits
 * files take the host path inside the same call.  netCDF-4: chunked variables
 * whose filters are a subset of {shuffle, deflate} in that order; anything
 * else (fletcher32, contiguous, compact, netCDF classic) takes the host path.
 * stats (HOST int64[4], or NULL) = {blocks decoded on the device, blocks
 * decoded on the host, compressed bytes copied to the device, decoded bytes
 * produced}.  The result is bit-identical to the host decode; a block whose
 * stream does not decode gives the host path's error (GSKYHIP_E_TYPE for a
 * GeoTIFF, GSKYHIP_E_ARG for netCDF), dev_out then unspecified. */
#define GSKYHIP_DECODE_HOST 0
#define GSKYHIP_DECODE_DEVICE 1
int gskyhip_geotiff_read_decode(const char *path, int band, int level, void *dev_out, int64_t out_bytes, int decode,
                                int64_t *stats, void *stream);
int gskyhip_netcdf_read_decode(const char *path, int band, void *dev_out, int64_t out_bytes, int decode,
                               int64_t *stats, void *stream);
/* gskyhip_register_geotiff[_ovr] / _netcdf[_ovr] with every level read
 * through the _decode call above; ovr_method -1: no pyramid is built.  The
 * decode mode is remembered like the pyramid request: the drop-in uses it
 * when it reads the file again (changed on disk, or evicted), until the file
 * is registered through another call. */
int gskyhip_register_geotiff_decode(const char *path, int band, int ovr_method, int min_size, int decode);
int gskyhip_register_netcdf_decode(const char *path, int band, int ovr_method, int min_size, int decode);

/* ---- drop-in for the cgo entry point of the worker ----------------------- */
/* Registers an HBM-resident granule under (path, band) so that the drop-in
 * below can find it (it replaces GDALOpenEx in warp.go:89-101; GeoTIFF files
 * the library decodes itself: gskyhip_register_geotiff above).  `g->data`
 * etc. must stay valid until unregistered. */
int gskyhip_register_granule(const char *path, int band, const gskyhip_granule *g,
                             const char *srs);
int gskyhip_unregister_all(void);

/* Same signature, ownership and return codes as
 *   int warp_operation_fast(const char *srcFilePath, char *srcProjRef,
 *       double *srcGeot, const char **geoLocOpts, const char *dstProjRef,
 *       double *dstGeot, int dstXImageSize, int dstYImageSize, int band,
 *       int srsCf, void **dstBuf, int *dstBufSize, int *dstBbox,
 *       double *noData, GDALDataType *dType, int *bytesRead)
 * (worker/gdalprocess/warp.go:82).  *dstBuf is host memory from malloc(); the
 * caller frees it with free() (warp.go:573-574).  srcGeot, when given, may be
 * overwritten by the overview pick (warp.go:186-189).  geoLocOpts (a
 * NULL-terminated GDAL geolocation option list, warp.go:128-141) selects the
 * geolocation-array transformer; 3 only when the options are incomplete or
 * their X / Y datasets cannot be read (createGeoLocTransformer fails,
 * warp.go:134-140).  Nearest-neighbour, like the reference.
 * Lookup (warp.go:89-118): "NETCDF:..." / "*.nc" paths are opened per band
 * (band_query) and read as band 1, i.e. (path, band) is looked up; other
 * paths: unregistered path -> 1, registered path without that band -> 2.
 * *bytesRead = block bytes x blocks read, with the reference's block-cache
 * heuristic (warp.go:278-347) over the granule's block_x x block_y. */
int warp_operation_fast(const char *srcFilePath, char *srcProjRef, double *srcGeot,
                        const char **geoLocOpts, const char *dstProjRef, double *dstGeot,
                        int dstXImageSize, int dstYImageSize, int band, int srsCf,
                        void **dstBuf, int *dstBufSize, int *dstBbox, double *noData,
                        int *dType, int *bytesRead);

/* ---- batched GetMap path (the MI355X hot path) --------------------------- */
/* Workspace bytes needed by gskyhip_render_tiles / gskyhip_warp_windows for
 * n_tiles tiles with n_pairs pairs whose tiles are at most max_tile_height
 * rows. */
int64_t gskyhip_render_workspace_size(int n_tiles, int n_pairs, int max_tile_height);

#define GSKYHIP_RESAMPLE_NEAREST 0
#define GSKYHIP_RESAMPLE_BILINEAR 1
/* Cubic convolution, GDAL 3.0.1 GWKCubicResample4Sample: with (sx, sy) the
 * source coordinate (pixel centres at +0.5), iX = floor(sx - 0.5), iY =
 * floor(sy - 0.5), tx = sx - 0.5 - iX, ty = sy - 0.5 - iY and
 *   CC(t, f0, f1, f2, f3) = f1 + 0.5 * (t * (f2 - f0) + t^2 * (2 f0 - 5 f1 +
 *                           4 f2 - f3) + t^3 * (3 (f1 - f2) + f3 - f0)),
 * the sample is CC(ty, h(-1), h(0), h(1), h(2)), h(j) = CC(tx, f(iX - 1, iY +
 * j), ..., f(iX + 2, iY + j)); Float32 results are cast, integer results go
 * through floor(r + 0.5) and saturate.  Where one of the 16 taps lies outside
 * the band or equals the band's nodata the pixel takes the bilinear rule's
 * value.  Accepted by gskyhip_render_tiles / _phase / _typed,
 * gskyhip_render_coverage and gskyhip_warp_windows. */
#define GSKYHIP_RESAMPLE_CUBIC 2
/* Area resampling, for destination pixels that cover more than one source
 * pixel; modelled on GDAL's GWKAverageOrMode (-r average, -r mode) and, like
 * bilinear and cubic, not pinned against it.  S(i, row) = (sx, sy) is the
 * source coordinate of window pixel (i, row) of a pair (pixel centres at
 * +0.5), whatever kind of row yields it.
 *  1. Footprint.  u = S(i + 1, row) - S(i, row); where i + 1 is outside the
 *     window [0, w) x [0, h) or that transform fails, u = S(i, row) - S(i - 1,
 *     row); where neither neighbour exists or succeeds, u = (0, 0).  v is the
 *     same along rows.  hx = max(0.5, 0.5 (|u.x| + |v.x|)), hy = max(0.5,
 *     0.5 (|u.y| + |v.y|)); the footprint is [sx - hx, sx + hx] x [sy - hy,
 *     sy + hy], the bounding box of the linearised pixel and never less than
 *     one source pixel wide.  A failed centre transform gives the window fill.
 *  2. Taps along an axis of n source pixels, for [x0, x1] = [s - h, s + h]: a
 *     non-finite bound means none; lo = max(floor(x0), 0), hi = min(ceil(x1),
 *     n), compared as doubles; hi <= lo means none; else stride = (hi - lo +
 *     7) / 8 (integers) and the taps are lo, lo + stride, ... < hi: at most 8
 *     per axis, 64 per pixel.  With stride 1 a tap xx weighs its covered
 *     length min(xx + 1, x1) - max(xx, x0), with a larger stride every tap
 *     weighs 1.
 *  3. A pixel's taps are the outer product of the two axes in scan order, rows
 *     outer, w = wx * wy; a tap equal to the band's nodata (a NaN nodata
 *     matches NaN) or with w <= 0 is dropped.  A signed-byte band enters as
 *     0..255, like bilinear.
 *  4. AVERAGE: accW += w, accR += d * w in scan order (fp64); accW < 0.00001
 *     gives the window fill, else r = accR / accW.
 *  5. MODE: taps of equal value form a class, a NaN tap that is not nodata a
 *     class of its own; a class weighs the sum of its taps' w in scan order;
 *     r is the value of the heaviest class, ties going to the class whose
 *     first tap comes first.  No surviving tap gives the window fill.
 *  6. Float32 results are cast, integer results go through floor(r + 0.5) and
 *     saturate.
 *  7. Rasters of the mask layer warp by nearest neighbour under both rules:
 *     bit fields can be neither averaged nor voted.
 * Differences from GDAL: the footprint is linearised from the pixel centre's
 * neighbours (GDAL transforms the pixel's corners), weights are fractional
 * coverages along each axis, and the taps are capped at 8 x 8 by striding.
 * With hx = hy = 0.5 AVERAGE takes the bilinear rule's taps and weights; an
 * aligned 2:1 footprint gives the 2 x 2 block mean.  Accepted wherever
 * GSKYHIP_RESAMPLE_CUBIC is. */
#define GSKYHIP_RESAMPLE_AVERAGE 3
#define GSKYHIP_RESAMPLE_MODE 4
/* Cubic B-spline (-r cubicspline: smooth, no overshoot) and Lanczos (-r
 * lanczos, a = 3: sharp), the two point kernels; modelled on GDAL 3.0.1's
 * general GWKResample at scale 1 with GWKBSpline / GWKLanczosSinc as the
 * weights and, like bilinear, cubic and the area rules, not pinned against
 * GDAL (parity unpinned).  (sx, sy) is the source coordinate, pixel centres
 * at +0.5; R = 2 for the spline (4 x 4 taps), R = 3 for Lanczos (6 x 6).
 *  1. Position.  fx = floor(sx - 0.5), fy = floor(sy - 0.5), tx = sx - 0.5 -
 *     fx, ty = sy - 0.5 - fy.  The centre 2 x 2, the taps (fx + i, fy + j),
 *     i, j in {0, 1}, must lie inside the nx x ny band (fx >= 0, fx + 1 < nx,
 *     fy >= 0, fy + 1 < ny, compared as doubles) and none of its four taps may
 *     equal the band's nodata (a NaN nodata matches NaN); otherwise the pixel
 *     takes the bilinear rule's value, edge cases included -- the hand-over
 *     that cubic makes.
 *  2. Weights along an axis, i = 1 - R .. R: w[i] = K(i - t).
 *     Spline, a = |x|: a < 1: ((4 - 6 a^2) + 3 a^3) / 6; a < 2: (2 - a)^3 / 6;
 *     else 0.  Lanczos: x == 0: 1; |x| >= 3: 0; else p = pi x, q = p / 3,
 *     sin(p) sin(q) / (p q).
 *  3. Sum, rows outer and columns inner over j, i = 1 - R .. R: a tap outside
 *     the band or equal to the nodata is dropped; for the others w = wx[i] *
 *     wy[j], accW += w, accR += d * w (fp64, in that order); r = accR / accW,
 *     always divided.  A signed-byte band enters as 0..255.  Float32 results
 *     are cast, integer results go through floor(r + 0.5) and saturate.
 *  4. Rasters of the mask layer warp by nearest neighbour under both rules:
 *     bit fields cannot be convolved.
 * Difference from GDAL: GDAL drops taps and renormalises with no condition,
 * except that a summed weight below 1e-6 gives no sample.  With Lanczos'
 * negative lobes the surviving weight can then fall to almost nothing (at
 * 15 % nodata 2.2 % of pixels fall below 1e-5 and sum|w| / sum w reaches
 * 5000).  The centre condition of step 1 prevents that: whichever outer taps
 * are dropped, Lanczos keeps accW >= 0.795 and sum|w| / accW <= 2.72 (both at
 * phase (0.5, 0.5)), the spline (all weights >= 0) accW >= 0.694 = (2/3 +
 * 1/6)^2.  Accepted wherever GSKYHIP_RESAMPLE_CUBIC is. */
#define GSKYHIP_RESAMPLE_CUBICSPLINE 5
#define GSKYHIP_RESAMPLE_LANCZOS 6

/* Warp + merge + scale + palette for a batch of tiles, replacing per tile:
 * gRPC warp fan-out (tile_grpc.go:200-289 -> warp.go:82-382), RasterMerger
 * (tile_merger.go:447-738), utils.Scale (raster_scaler.go:334) and the
 * EncodePNG pixel loop (ogc_encoders.go:82-134).
 *   granules, crs_table, tiles, pair_granule: dev arrays.
 *   out_ns[0..n_out_ns): HOST array of namespace slots rendered
 *     (ConfigPayLoad.NameSpaces order; 1 = palette/grey, 3 = RGB).
 *   mask, sp: HOST structs.
 *   ramp: dev 256x4 RGBA (GradientRGBAPalette) or NULL for grey.
 *   rgba_out: dev n_tiles x height x width x 4.
 *   canvas_out: optional dev buffer n_tiles x n_out_ns x height x width x 4
 *     bytes receiving the typed merged canvases (tile_merger.go:562-652), or NULL.
 *   auto_scale (Offset = Scale = Clip = 0) needs canvas_out.
 *   workspace: dev, gskyhip_render_workspace_size bytes. */
int gskyhip_render_tiles(const gskyhip_granule *granules, int n_granules,
                         const gskyhip_crs *crs_table, int n_crs, int dst_crs,
                         const gskyhip_tile *tiles, int n_tiles,
                         const int32_t *pair_granule, int n_pairs,
                         int max_tile_width, int max_tile_height,
                         const int32_t *out_ns, int n_out_ns,
                         const gskyhip_mask *mask, int resample,
                         const gskyhip_scale_params *sp, const uint8_t *ramp,
                         uint8_t *rgba_out, void *canvas_out,
                         void *workspace, int64_t workspace_bytes, void *stream);

/* The same call split in phases: 1 = planning kernels only (windows,
 * merge order, row plans into `workspace`), 2 = render kernels only (needs
 * a phase-1 call with identical arguments before it on the stream),
 * 0 = both (= gskyhip_render_tiles).  rgba_out may be NULL: typed canvases
 * only (WCS GetCoverage, FusionUnscale: ows.go:728), canvas_out required. */
int gskyhip_render_tiles_phase(int phase, const gskyhip_granule *granules, int n_granules,
                               const gskyhip_crs *crs_table, int n_crs, int dst_crs,
                               const gskyhip_tile *tiles, int n_tiles,
                               const int32_t *pair_granule, int n_pairs,
                               int max_tile_width, int max_tile_height,
                               const int32_t *out_ns, int n_out_ns,
                               const gskyhip_mask *mask, int resample,
                               const gskyhip_scale_params *sp, const uint8_t *ramp,
                               uint8_t *rgba_out, void *canvas_out,
                               void *workspace, int64_t workspace_bytes, void *stream);

/* The same with a hint: value_types = OR of GSKYHIP_VT_* over the value types
 * the batch's stack granules warp to (Byte/SignedByte/Int16/UInt16/Float32;
 * granules of a non-inclusive mask layer excluded), 0 = unknown.  With exactly
 * one type, one NN palette/grey namespace, RGBA output and no auto-scale the
 * batch runs the typed LDS-staged band kernel (the MI355X fast path); every
 * other combination runs the generic kernels.  Results are identical. */
#define GSKYHIP_VT_BYTE 1u
#define GSKYHIP_VT_SIGNEDBYTE 2u
#define GSKYHIP_VT_INT16 4u
#define GSKYHIP_VT_UINT16 8u
#define GSKYHIP_VT_FLOAT32 16u
int gskyhip_render_tiles_typed(int phase, uint32_t value_types, const gskyhip_granule *granules,
                               int n_granules, const gskyhip_crs *crs_table, int n_crs, int dst_crs,
                               const gskyhip_tile *tiles, int n_tiles,
                               const int32_t *pair_granule, int n_pairs,
                               int max_tile_width, int max_tile_height,
                               const int32_t *out_ns, int n_out_ns,
                               const gskyhip_mask *mask, int resample,
                               const gskyhip_scale_params *sp, const uint8_t *ramp,
                               uint8_t *rgba_out, void *canvas_out,
                               void *workspace, int64_t workspace_bytes, void *stream);

/* WCS GetCoverage (ows.go:815-1150): the chunk tiles rendered as typed
 * canvases (FusionUnscale, ows.go:728: no Scale / RGBA) of the first
 * namespace, each written straight into ONE coverage image at its chunk
 * offset -- tile t's row r lands at coverage_out + (tile_offsets[t] + r *
 * row_stride) elements -- instead of per-tile slots, so no assembly copy
 * follows.  tile_offsets: dev int64 per tile; the coverage's value type is
 * the canvas type (value_types hint as gskyhip_render_tiles_typed). */
int gskyhip_render_coverage(int phase, uint32_t value_types, const gskyhip_granule *granules,
                            int n_granules, const gskyhip_crs *crs_table, int n_crs, int dst_crs,
                            const gskyhip_tile *tiles, int n_tiles, const int32_t *pair_granule,
                            int n_pairs, int max_tile_width, int max_tile_height, int resample,
                            const gskyhip_scale_params *sp, const int64_t *tile_offsets,
                            int64_t row_stride, void *coverage_out, void *workspace,
                            int64_t workspace_bytes, void *stream);

/* Warped windows only (the FlexRasters of tile_grpc.go:228-241): for pair p
 * (tile t, granule g) writes window bbox[4*p..] = {xoff,yoff,w,h} and the
 * window data (dtype of warp.go:232-243) into win_out + p*win_stride bytes. */
int gskyhip_warp_windows(const gskyhip_granule *granules, int n_granules,
                         const gskyhip_crs *crs_table, int n_crs, int dst_crs,
                         const gskyhip_tile *tiles, int n_tiles,
                         const int32_t *pair_granule, int n_pairs,
                         int max_tile_width, int max_tile_height, int resample,
                         int32_t *bbox_out, int32_t *dtype_out, double *nodata_out,
                         void *win_out, int64_t win_stride,
                         void *workspace, int64_t workspace_bytes, void *stream);

/* ComputeReprojectExtent (worker/gdalprocess/warp.go:433-487, the worker's
 * "extent" operation), batched over n granules: for granule i,
 * GDALSuggestedWarpOutput of its GenImgProj transformer to crs_table[dst_crs]
 * (no destination dataset: destination georeferenced coordinates; dst_crs
 * -1 = the granule's own CRS), then its request's pixel counts
 *   out[2i]   = nPixels = int((bbox[2] - bbox[0] + xRes/2) / xRes)
 *   out[2i+1] = nLines  = int((bbox[3] - bbox[1] + yRes/2) / yRes)
 * with bbox = dst_bbox[4i..4i+3] (the request's DstGeot[0..3]) and xRes /
 * yRes the suggested geotransform's gt[1] / |gt[5]|.  status[i] = 0, or
 * GSKYHIP_E_XFORM where the reference returns "GDALSuggestedWarpOutput()
 * failed".  granules, crs_table, dst_bbox, out and status are device
 * pointers; asynchronous on `stream`. */
int gskyhip_compute_reproject_extent(const gskyhip_granule *granules, int n, const gskyhip_crs *crs_table,
                                     int n_crs, int dst_crs, const double *dst_bbox, int32_t *out,
                                     int32_t *status, void *stream);

/* ---- per-node warp service (SURVEY 8b threading contract, 8f row 1) ------
 * The reference runs N = NumCPU single-threaded gsky-gdal-process workers per
 * node (grpc-server/main.go:58, gdal-process/main.go:115-123; pool.go:19-74
 * and process.go:108-160 spawn, feed and kill them).  One daemon per GPU
 * (gskyhipd = gskyhip_service_run) owns the HIP context and the HBM-resident
 * granules; a worker whose environment has GSKYHIP_SERVICE=<socket> sends
 * each warp_operation_fast call there over a Unix socket and never touches
 * the GPU, so N workers share one context and a SIGKILLed worker leaves no
 * device state.  The daemon keeps two batches in flight: whenever requests
 * are queued and a batch slot is free it plans and warps up to `max_batch`
 * of them in one launch set (while the other batch is still on the GPU it may
 * first wait up to `window_us` for the batch to grow; with the GPU idle it
 * dispatches at once).  Each worker thread passes a sealed memfd reply arena
 * with its first request; the daemon registers it with HIP and the warp
 * kernel writes the window straight into it (GSKYHIP_SVC_DIRECT=0 in the
 * daemon's environment: staged in HBM and copied instead).  All pointers are
 * host. */
int gskyhip_service_run(const char *socket_path, int max_batch, int window_us);   /* blocks until shutdown */
int gskyhip_service_register_granule(const char *socket_path, const char *path, int band,
                                     const gskyhip_granule *g, const void *data, const void *const *ovr_data,
                                     const char *srs);   /* data / ovr_data: host arrays, uploaded by the daemon */
/* The same without overviews from the caller (g->n_ovr is ignored): the
 * daemon builds the pyramid (gskyhip_build_overviews: method, min_size) in
 * its own HBM after the upload.  A message kind of its own; the others are
 * unchanged. */
int gskyhip_service_register_granule_ovr(const char *socket_path, const char *path, int band,
                                         const gskyhip_granule *g, const void *data, const char *srs,
                                         int method, int min_size);
int gskyhip_service_unregister_all(const char *socket_path);
/* stats[4]: warp requests served, batches run, largest batch, registered granules */
int gskyhip_service_stats(const char *socket_path, int64_t *stats);
/* the same and, at [4], nanoseconds the dispatcher spent preparing and
 * launching batches, at [5] the summed residence of requests (enqueued ->
 * answer ready), at [6..8] the warp batches' launch, wait for the GPU and
 * staged window read-back (ns), at [9] replies whose window the GPU wrote into
 * the worker's arena, at [10] replies whose window was copied; the first
 * n_stats values are written (0 past what the daemon reports) */
int gskyhip_service_stats_n(const char *socket_path, int64_t *stats, int n_stats);
int gskyhip_service_shutdown(const char *socket_path);

/* Band-math on merged canvases (processor/tile_merger.go:523-731): evaluate
 * `expr` (govaluate subset: ?: || && == != < <= > >= + - * / % ** unary - ! +,
 * numbers, the variable names, parentheses; float32 per element) over the
 * canvases of one axis -- var_names[k] names canvases[k] (dev, n_px values
 * of dtypes[k], nodata nodatas[k]) -- into out (dev float32 n_px).  A pixel
 * where any variable equals its nodata, or whose result is not finite,
 * becomes out_nodata (the first namespace's nodata); an expression without
 * variables fills every valid pixel with its value unfiltered, finite or not
 * ("1e39" writes inf, "0 / 0" NaN), as the reference does with a scalar
 * result (tile_merger.go:698-708).  Every variable of the axis masks,
 * referenced or not; the comparison is float64(float32(v)) == nodata, so a
 * NaN nodata, or one that is no float32 value, masks nothing.
 * Grammar, loosest first: ?: (right-associative), ||, &&, == !=, < <= > >=,
 * + -, * / %, ** (right-associative), unary - ! +; all other binary
 * operators associate to the left.  == and != bind looser than the four
 * relations: "a == b < c" is a == (b < c).  Unary operators bind tighter
 * than **: "-a ** 2" is (-a) ** 2, and "2 ** -1" is 0.5.  Comparisons, !, &&
 * and || yield 1.0 / 0.0; everything but 0.0 and -0.0 is true, NaN included.
 * % is C fmod (sign of the dividend).  Numbers are decimal: digits [. digits]
 * or . digits, then an optional e|E [+|-] digits, rounded to float32; hex
 * forms, "inf" and "nan" are not numbers.  Names are [A-Za-z_][A-Za-z0-9_.]*,
 * case-sensitive.
 * ?: evaluates the condition and both arms, then selects.  An expression may
 * need at most 16 stack slots (operands pending at once) and compile to at
 * most 96 program words (one per number, variable reference and operator;
 * parentheses and unary + cost none).  So "a+(a+(..." nests 16 operands deep,
 * a chain "a+a+...+a" holds 48 terms, and since each pending arm of a chained
 * ternary keeps two slots, "c1 ? v1 : c2 ? v2 : ... : last" holds 7
 * conditions at most.
 * GSKYHIP_E_ARG: parse error, unknown variable (govaluate's errors), an
 * expression above either limit, n_vars outside 0..8 or a NULL pointer (the
 * canvases and out may be NULL when n_px is 0); out is then untouched.
 * GSKYHIP_E_TYPE: canvas type. */
#define GSKYHIP_BANDMATH_MAX_VARS 8
int gskyhip_band_math(const char *expr, const char *const *var_names, const void *const *canvases,
                      const int32_t *dtypes, const double *nodatas, int n_vars, int64_t n_px, double out_nodata,
                      float *out, void *stream);

/* ---- standalone stages (the reference's own operator boundaries) -------- */
/* FlexRaster (tile_types.go:95-106) as flat fields; data is dev. */
typedef struct {
    const void *data;
    int32_t data_w, data_h, width, height, off_x, off_y;
    int32_t dtype, ns;
    double nodata, timestamp;
    uint32_t polygon_hash;
    int32_t _pad;
} gskyhip_flex_raster;

/* RasterMerger.Run for one batch (tile_merger.go:447-503 ->
 * ProcessRasterStack 281-312 -> MergeMaskedRaster 38-225 / ComputeMask
 * 314-445).  rasters: HOST array (ordering metadata); their data: dev.
 * canvases: n_ns dev buffers of width*height*4 bytes (typed by the first
 * raster of each namespace); created/dtype/nodata: host outputs per ns. */
int gskyhip_merge_rasters(const gskyhip_flex_raster *rasters, int n,
                          const gskyhip_mask *mask, void *const *canvases, int n_ns,
                          int32_t *created, int32_t *dtype, double *nodata, void *stream);

/* utils.Scale for one raster (raster_scaler.go:30-332): data dev (n values),
 * out dev (n bytes).  Byte input is scaled in place like the reference. */
int gskyhip_scale(void *data, int dtype, int64_t n, double nodata,
                  const gskyhip_scale_params *sp, uint8_t *out, void *stream);

/* processor.RasterScaler.Run (tile_scaler.go:17-112, dead in the reference). */
int gskyhip_scale_legacy(void *data, int dtype, int64_t n, double nodata,
                         const gskyhip_scale_params *sp, uint8_t *out, void *stream);

/* GradientRGBAPalette (utils/palette.go:27-69): colours host n x RGBA,
 * ramp host 256 x RGBA. */
int gskyhip_gradient_palette(const uint8_t *colours, int n, int interpolate, uint8_t *ramp);

/* EncodePNG pixel loop (ogc_encoders.go:86-133): bands dev (1 or 3), ramp
 * dev or NULL, rgba dev w*h*4. */
int gskyhip_encode_rgba(const uint8_t *const *bands, int nbands, int w, int h,
                        const uint8_t *ramp, uint8_t *rgba, void *stream);

/* ComputeMask (tile_merger.go:314-445): data dev, out dev (n bytes 0/1). */
int gskyhip_compute_mask(const void *data, int dtype, int64_t n, const gskyhip_mask *mask,
                         uint8_t *out, void *stream);

/* ---- layer fusion (input_layers) ---------------------------------------- */
/* TilePipeline.processDeps (processor/tile_pipeline.go:196-324): a layer with
 * input_layers renders each dependent layer, scales it with that layer's own
 * ScaleParams, names the results fuse<j> (getFlexRaster, 482-632: polygon
 * "dummy_polygon", timestamps t, t-1 s, t-2 s, ... in layer order) and lets
 * RasterMerger fold them: layer 0 wins, every later layer only fills what is
 * still nodata.  Here the dependent layers are already rendered: layer l is
 * the typed canvases of gskyhip_render_tiles' canvas_out layout -- tile t,
 * namespace slot s at byte (t * n_ns + s) * max_w * max_h * 4, rows max_w
 * elements apart -- with one value type T_l, one nodata n_l, its ScaleParams
 * and an optional per-tile `present` flag (the reference's EmptyTile result
 * and its effective-date `continue`, 216-240, 264-269).
 *
 * The rule, per tile, namespace slot and pixel.  T(x) is Go's conversion of
 * the float64 x to the value type.
 *   Per-layer stage.  A layer is scaled when fusion_unscale == 0 and its
 *   (offset, scale, clip) are not all zero (251-253).
 *     scaled: the pixel is utils.Scale of it (raster_scaler.go:30-332) with
 *       colour_scale 0 -- the inner ScaleParams are built without it
 *       (254-257) -- the type becomes Byte and the nodata 0xFF (272).  The
 *       inner scale is never an auto-scale.
 *     unscaled: the pixel keeps its type.  Where layer 0 is unscaled and
 *       present on the tile it is the normalisation reference (283-286): if
 *       T(n_0) != T(n_l), pixels equal to T(n_l) become T(n_0) and the
 *       layer's nodata becomes n_0 (getFlexRaster's `normalise`).  With a NaN
 *       nodata the comparisons fall out as in Go: always "different", never
 *       "equal".
 *     The input canvases are never written (the reference's in-place Byte
 *     scale is not observable here).
 *   Fold.  p0 is the first present layer.  The fused canvas has p0's
 *     post-stage type, its nodata C is p0's post-stage nodata, and it starts
 *     as T(C).  p0 writes where v != T(n'); every later present layer writes
 *     where v != T(n') && canvas == T(n'), n' its OWN post-stage nodata
 *     (MergeMaskedRaster, tile_merger.go:38-225, fill mode: the timestamps
 *     decrease strictly).
 *   Type check.  Every layer's post-stage type must be the same, else
 *     GSKYHIP_E_TYPE (the reference would reinterpret the canvas bytes and
 *     panic).
 * Deviations from the reference:
 *   - its allFilled early stop (252, 300-305) is dead code: allFilled starts
 *     false and is only ever assigned false.  The kernels skip a layer's reads
 *     for a wave whose pixels that layer cannot fill, which changes no value;
 *   - a tile with no present layer gets a canvas of layer 0's post-stage
 *     nodata (C = n_0 for an unscaled layer 0) and transparent RGBA; the
 *     reference pushes a zero Byte "EmptyTile_dummy" raster (314-320): the
 *     same RGBA, another canvas;
 *   - where layer 0 is absent nothing is normalised; the reference can still
 *     normalise Byte layers against the EmptyTile raster. */
#define GSKYHIP_FUSE_MAX_LAYERS 8
typedef struct {
    const void *canvases;        /* dev: n_tiles x n_ns slots, see above         */
    int32_t dtype;               /* Byte, SignedByte, Int16, UInt16 or Float32   */
    int32_t _pad;
    double nodata;
    gskyhip_scale_params sp;     /* the layer's own ScaleParams                   */
    const uint8_t *present;      /* dev uint8[n_tiles], or NULL: all present      */
} gskyhip_fuse_layer;

/* The fused typed canvases.  layers: HOST array in input_layers order, 1 ..
 * GSKYHIP_FUSE_MAX_LAYERS; n_ns: 1 or 3; tiles: dev (width, height used);
 * canvas_out: dev, the layout of the inputs (pixels outside a tile's width x
 * height are left alone); nodata_out: dev double per tile, C; dtype_out: HOST,
 * the fused type.  One kernel on `stream`: no allocation, no copy, no
 * synchronisation, so the call can be captured in a graph.  Every argument
 * error (GSKYHIP_E_ARG: NULL pointer, n_layers, n_ns, sizes; GSKYHIP_E_TYPE:
 * a layer's value type, mixed post-stage types) returns before any HIP call. */
int gskyhip_fuse_layers(const gskyhip_fuse_layer *layers, int n_layers, int n_ns,
                        const gskyhip_tile *tiles, int n_tiles, int max_w, int max_h,
                        int fusion_unscale, void *canvas_out, double *nodata_out,
                        int32_t *dtype_out, void *stream);

/* The same, then the OUTER utils.Scale (outer_sp, colour_scale honoured,
 * nodata C) and the EncodePNG pixel rule (ogc_encoders.go:86-133; ramp: dev
 * 256 x RGBA or NULL for grey, ignored for n_ns = 3) in the same pass:
 * rgba_out dev n_tiles x max_h x max_w x 4.  canvas_out and nodata_out may be
 * NULL.  An outer auto-scale (offset = scale = clip = 0) needs a reduction
 * over the fused canvas and returns GSKYHIP_E_ARG: call gskyhip_fuse_layers,
 * then gskyhip_scale. */
int gskyhip_fuse_render(const gskyhip_fuse_layer *layers, int n_layers, int n_ns,
                        const gskyhip_tile *tiles, int n_tiles, int max_w, int max_h,
                        int fusion_unscale, const gskyhip_scale_params *outer_sp,
                        const uint8_t *ramp, uint8_t *rgba_out, void *canvas_out,
                        double *nodata_out, void *stream);

/* ---- output codecs ------------------------------------------------------ */
/* png.Encode of EncodePNG (utils/ogc_encoders.go:139; Go 1.12 image/png) for
 * a batch of RGBA tiles in HBM, e.g. the rgba_out of gskyhip_render_tiles:
 *   rgba: dev, tile t row y at rgba + t*tile_stride + y*row_stride (bytes);
 *   sizes: HOST int32 2 per tile {width, height} (<= max_w, max_h);
 *   png_out: HOST, png_capacity bytes per tile (>= gskyhip_png_bound(w, h));
 *   png_sizes: HOST int64 per tile, the PNG's length.
 * Colour type RGB when every alpha is 0xff else RGBA (NRGBA bytes), Go's
 * per-row filter choice, 32 KiB IDAT chunks (see encode.hip: the filtered
 * rows are Go's bytes; the zlib stream is deflated on the GPU -- LZ77 at run
 * / pixel / row / diagonal distances, per-tile Huffman codes -- so its bytes
 * are neither zlib's nor Go's compress/flate, parity unpinned).
 * n_threads host threads frame the PNGs; `stream` runs the GPU passes. */
int64_t gskyhip_png_workspace_size(int n_tiles, int max_w, int max_h);
int64_t gskyhip_png_bound(int width, int height);
int gskyhip_encode_png(const uint8_t *rgba, int n_tiles, int max_w, int max_h, int64_t tile_stride,
                       int64_t row_stride, const int32_t *sizes, void *workspace, int64_t workspace_bytes,
                       uint8_t *png_out, int64_t png_capacity, int64_t *png_sizes, int n_threads, void *stream);
/* The host twin of gskyhip_encode_png's GPU deflate, for tests and tools (no
 * product path calls it): the zlib stream of h rows of `stride` filtered bytes
 * (HOST; the filter byte included, bpp 3 or 4 bytes a pixel) from the functions
 * the kernels run, so the same bytes.  fixed_only: as GSKYHIP_PNG_FIXED=1.
 * *out_len is the stream's length; GSKYHIP_INFLATE_E_CAP (nothing written)
 * when it exceeds cap. */
int gskyhip_png_deflate_rows_host(const uint8_t *rows, int h, int stride, int bpp, int fixed_only, uint8_t *out,
                                  int64_t cap, int64_t *out_len);

/* Indexed-colour PNG (colour type 3) of a batch of one-band tiles in HBM: the
 * ByteRaster of utils.Scale, one index byte a pixel with 0xFF = nodata, and
 * the 256 x RGBA ramp of GradientRGBAPalette (gskyhip_gradient_palette) or
 * NULL for a grey layer.  Beyond the reference, and opt-in: EncodePNG
 * (ogc_encoders.go:82-142) always expands such a raster to an image.RGBA and
 * gskyhip_encode_png follows it; this encoder writes the index bytes
 * themselves, a quarter of the bytes through Deflate, and every decoder gives
 * the RGBA of the truecolour PNG of the same tile, pixel for pixel.  Go's
 * png.Encode never sees an image.Paletted here, so byte parity with it is
 * unpinned; the format is this library's:
 *   signature, IHDR (w, h, bit depth 8, colour type 3, 0, 0, 0), PLTE, tRNS,
 *   IDAT chunks of 32768 bytes (the last one shorter), IEND, each with its
 *   CRC-32;
 *   PLTE, 256 entries: entry i < 255 is the non-premultiplied RGB of ramp[i]
 *     (color.NRGBAModel, as gskyhip_encode_png converts a canvas: a = 255 the
 *     bytes, a = 0 (0, 0, 0), else per channel
 *     (((c * 0x101) * 0xFFFF) / (a * 0x101) >> 8) & 0xFF), or (i, i, i) for
 *     grey; entry 255 is (0, 0, 0);
 *   tRNS, 256 bytes: the alpha of ramp[i], or 255 for grey; entry 255 is 0
 *     (a nodata pixel is transparent black, ogc_encoders.go:96, 105);
 *   image data: every row is the filter byte 0 (None; no filter selection)
 *     and the row's w index bytes;
 *   zlib stream: gskyhip_encode_png's GPU deflate over those rows with one
 *     byte a pixel -- one final block, per-tile dynamic Huffman codes where
 *     they are shorter, else fixed codes, Adler-32 -- GSKYHIP_PNG_FIXED=1 and
 *     GSKYHIP_PNG_ZLIB=1 honoured alike; tiles of more than 4096 rows go to
 *     host zlib.
 * Arguments as gskyhip_encode_png:
 *   index: dev, tile t row y at index + t*tile_stride + y*row_stride (bytes,
 *     row_stride >= max_w, tile_stride >= row_stride * max_h);
 *   sizes: HOST int32 2 per tile {width, height} (<= max_w, max_h);
 *   ramp: HOST 256 x 4 bytes or NULL; PLTE and tRNS are framed once per call;
 *   workspace: dev, 8-byte aligned, >= gskyhip_png_indexed_workspace_size;
 *   png_out: HOST, png_capacity bytes per tile (>= gskyhip_png_indexed_bound
 *     (w, h)); png_sizes: HOST int64 per tile, the PNG's length.
 * GSKYHIP_E_ARG before any HIP call for a NULL pointer, a size outside
 * max_w x max_h, a short stride, capacity or workspace; n_tiles <= 0: 0.
 * Three-band tiles have no index: they stay with gskyhip_encode_png. */
int64_t gskyhip_png_indexed_workspace_size(int n_tiles, int max_w, int max_h);
int64_t gskyhip_png_indexed_bound(int width, int height);
int gskyhip_encode_png_indexed(const uint8_t *index, int n_tiles, int max_w, int max_h, int64_t tile_stride,
                               int64_t row_stride, const int32_t *sizes, const uint8_t *ramp, void *workspace,
                               int64_t workspace_bytes, uint8_t *png_out, int64_t png_capacity,
                               int64_t *png_sizes, int n_threads, void *stream);
/* The host twin of gskyhip_encode_png_indexed for one tile (index: HOST,
 * w * h bytes, rows w apart): the same functions in a loop, no HIP call, so
 * the PNG the device path writes, byte for byte.  fixed_only: as
 * GSKYHIP_PNG_FIXED=1.  *out_len is the PNG's length.  GSKYHIP_E_ARG for a
 * NULL index, out or out_len, w or h <= 0, more than 2^30 bytes of image
 * data, or a PNG longer than cap (nothing is written to out; *out_len is
 * still the length needed when the other arguments are good). */
int gskyhip_encode_png_indexed_host(const uint8_t *index, int w, int h, const uint8_t *ramp, int fixed_only,
                                    uint8_t *out, int64_t cap, int64_t *out_len);

/* What the last render left in every tile's typed canvases (the canvas_out
 * of gskyhip_render_tiles, same workspace and sizes): info_out HOST int32 8
 * per tile = created[4], dtype[4] by namespace slot (a slot no raster reached
 * is not created and its canvas was never written); nodata_out HOST double 4
 * per tile, the canvas NoData of each slot.  Synchronises `stream`. */
int gskyhip_render_canvas_info(void *workspace, int n_tiles, int n_pairs, int max_tile_height,
                               int32_t *info_out, double *nodata_out, void *stream);

/* EncodeGdalOpen + EncodeGdal for format "geotiff" (utils/ogc_encoders.go:
 * 277-450) of one WCS coverage held in HBM: a BigTIFF with the reference's
 * creation options COMPRESS=PACKBITS, TILED=YES, BIGTIFF=YES,
 * INTERLEAVE=BAND, BLOCKXSIZE / BLOCKYSIZE (ows.go passes 1024 x 256),
 * PIXELTYPE=SIGNEDBYTE for int8; the geotransform (ModelPixelScale +
 * ModelTiepoint, ModelTransformation when rotated), EPSG code as GeoKeys,
 * per-band long_name (GDAL_METADATA) and nodata (GDAL_NODATA: GeoTIFF holds
 * one, the last band's value), Photometric RGB for 3 or 4 Byte bands (the 4th
 * an associated alpha), MinIsBlack otherwise.  A band whose name starts with
 * "EmptyTile" is skipped as EncodeGdal skips it (ogc_encoders.go:364): no
 * nodata, no long_name, its pointer may be NULL and its samples are the
 * dataset nodata (0 without one).
 *   bands: HOST array of n_bands dev pointers, each height x width samples of
 *     dtype (GSKYHIP_BYTE / SIGNEDBYTE / INT16 / UINT16 / FLOAT32), row-major;
 *   geot: HOST 6 doubles (GDAL order); epsg <= 0 writes no GeoKeys;
 *   nodata, names: HOST n_bands each, or NULL;
 *   block_x, block_y: multiples of 16;
 *   workspace: dev, gskyhip_geotiff_workspace_size bytes;
 *   out: HOST, capacity >= gskyhip_geotiff_bound bytes; *size = file length.
 * PackBits runs on the GPU (one thread per tile row, libtiff encodes tiled
 * PackBits row by row); the framing on the host.  The bytes are a valid
 * GeoTIFF of the same samples, tags and keys GDAL writes, not GDAL's file
 * byte for byte (tag set and tile order differ: parity on decoded content). */
int64_t gskyhip_geotiff_workspace_size(int width, int height, int n_bands, int dtype, int block_x, int block_y);
int64_t gskyhip_geotiff_bound(int width, int height, int n_bands, int dtype, int block_x, int block_y);
int gskyhip_encode_geotiff(const void *const *bands, int n_bands, int dtype, int width, int height,
                           const double *geot, int epsg, const double *nodata, const char *const *names,
                           int block_x, int block_y, void *workspace, int64_t workspace_bytes, uint8_t *out,
                           int64_t capacity, int64_t *size, void *stream);
/* gskyhip_encode_geotiff with a choice of compression, beyond the reference
 * (EncodeGdalOpen always writes COMPRESS=PACKBITS, which removes nothing from
 * int16 reflectances or float32 fields).
 * compression = GSKYHIP_TIFF_PACKBITS (predictor must be 1): the file of
 * gskyhip_encode_geotiff, byte for byte.
 * compression = GSKYHIP_TIFF_DEFLATE: tag 259 = 8 (Adobe Deflate); every tile
 * is one complete zlib stream of its block_y x block_x samples (edge tiles
 * padded as the PackBits writer pads them) after the TIFF predictor, tag 317,
 * written only when it is not 1:
 *   1  none;
 *   2  horizontal differencing, any dtype: the differences of the samples' bit
 *      patterns along a tile row, wrapping in the sample width, the first
 *      sample of each tile row kept (float32: of the 32-bit patterns);
 *   3  floating point (TIFF Technical Note 3), GSKYHIP_FLOAT32 only: per tile
 *      row the four byte planes, most significant first, then byte differences
 *      one apart over the row of 4 * block_x bytes.
 * Every other tag, the layout and the EmptyTile rules are those of
 * gskyhip_encode_geotiff.  The streams are this library's encoder's
 * (gskyhip_deflate_blocks; zlevel 0: stored blocks, 1-9: the one encoding),
 * neither zlib's nor GDAL's bytes: parity is on decoded content, and
 * gskyhip_geotiff_read[_decode] reads the file back.
 * deflate = GSKYHIP_DEFLATE_DEVICE: per band and slab of slab_tiles tiles
 * (0: the library's choice, 16 MiB of raw tile bytes, at least one tile,
 * at most 32768) a kernel gathers the tiles from the band in HBM and applies
 * the predictor, gskyhip_deflate_blocks' kernels turn each tile into its
 * stream, the streams are packed on the device, and the host receives the
 * lengths and statuses and then one copy of exactly the compressed bytes,
 * straight to their place in `out`.  The device workspace (about 8.4 times the
 * slab's raw bytes) is allocated inside the call and freed before return.  The
 * file does not depend on slab_tiles.  A band without samples (EmptyTile, or a
 * NULL pointer) is one tile compressed once on the host and repeated.
 * deflate = GSKYHIP_DEFLATE_HOST: the bands are copied to the host once and
 * the same predictor and encoder run on up to n_threads host threads: the same
 * file, byte for byte.
 * stats (HOST int64[4], or NULL) = {tiles deflated on the device, raw bytes
 * read from HBM, compressed bytes copied to the host, device workspace bytes};
 * all zero in the host mode and after a failed call.
 * GSKYHIP_E_ARG / GSKYHIP_E_TYPE, before any device work, for what
 * gskyhip_encode_geotiff refuses and for an unknown compression, a predictor
 * outside 1-3 (or 3 on another type than float32, or not 1 with PackBits),
 * zlevel outside 0-9, deflate outside {0, 1}, slab_tiles < 0, a tile above
 * 1 GiB, or capacity < gskyhip_geotiff_bound_opts.  A tile whose stream fails
 * fails the call. */
#define GSKYHIP_TIFF_PACKBITS 32773
#define GSKYHIP_TIFF_DEFLATE 8
int64_t gskyhip_geotiff_bound_opts(int width, int height, int n_bands, int dtype, int block_x, int block_y,
                                   int compression);
int gskyhip_encode_geotiff_opts(const void *const *bands, int n_bands, int dtype, int width, int height,
                                const double *geot, int epsg, const double *nodata, const char *const *names,
                                int block_x, int block_y, int compression, int predictor, int zlevel, int deflate,
                                int slab_tiles, int n_threads, uint8_t *out, int64_t capacity, int64_t *size,
                                int64_t *stats, void *stream);
/* The same file from HOST band pointers: no device involved, no HIP call. */
int gskyhip_encode_geotiff_host(const void *const *bands, int n_bands, int dtype, int width, int height,
                                const double *geot, int epsg, const double *nodata, const char *const *names,
                                int block_x, int block_y, int compression, int predictor, int zlevel, int n_threads,
                                uint8_t *out, int64_t capacity, int64_t *size);

/* EncodeGdalOpen + EncodeGdal for format "netcdf" (utils/ogc_encoders.go:
 * 263-301, creation options COMPRESS=DEFLATE, ZLEVEL=6; ows.go:1172) of one
 * WCS coverage held in HBM: the netCDF-4 classic-model file GDAL 3.0.1's
 * netCDF driver creates for those options -- one variable per band
 * ("Band1", ...) with long_name = names[k] and _FillValue = nodata[k] (an
 * "EmptyTile" band skipped as EncodeGdal skips it), chunks of one row,
 * shuffle + deflate at zlevel, rows bottom-up with increasing y (GDAL's
 * WRITE_BOTTOMUP default), x / y (lon / lat) coordinate variables at pixel
 * centres, the "crs" grid mapping (CF attributes of `epsg`, spatial_ref
 * naming the EPSG code, GeoTransform).  Byte is NC_BYTE + _Unsigned "true",
 * UInt16 widens to NC_INT (the classic model has no unsigned types).
 *   bands: HOST array of n_bands dev pointers, height x width of dtype;
 *   out: HOST, capacity >= gskyhip_netcdf_bound bytes; *size = file length.
 * The rows are deflated by n_threads host threads after one copy of each
 * band to the host.  Parity with GDAL's bytes unpinned (no netCDF / HDF5
 * library here): checked by reading the file back (gskyhip_netcdf_read_host). */
int64_t gskyhip_netcdf_bound(int width, int height, int n_bands, int dtype);
int gskyhip_encode_netcdf(const void *const *bands, int n_bands, int dtype, int width, int height,
                          const double *geot, int epsg, const double *nodata, const char *const *names, int zlevel,
                          int n_threads, uint8_t *out, int64_t capacity, int64_t *size, void *stream);
/* gskyhip_encode_netcdf with a choice of where the chunks are compressed.
 * deflate = GSKYHIP_DEFLATE_HOST is exactly gskyhip_encode_netcdf.
 * GSKYHIP_DEFLATE_DEVICE: a kernel reads the band in HBM and writes the file's
 * chunks in file order (file row j = image row height - 1 - j; UInt16 widened
 * to int32; the HDF5 shuffle applied), gskyhip_deflate_blocks' kernels turn
 * each chunk into a zlib stream, the streams are packed on the device and come
 * back with their lengths -- two small copies (lengths, statuses) and one copy
 * of exactly the compressed bytes per slab.  The host allocates them into the
 * image and writes the B-tree and headers.  Everything but the chunk payloads
 * (and what follows from their sizes: addresses, B-tree keys) is what the host
 * path writes for the same arguments; the filter message records zlevel (0:
 * stored blocks; 1-9: the one device encoding).  Work proceeds in slabs of
 * slab_rows rows; <= 0: the library's choice, 16 MiB of raw chunk bytes (at
 * least one row, at most 65536 rows), which caps the device workspace --
 * allocated once per call and freed before return -- at about 8.4 times that,
 * 135 MiB, whatever the height (rows above 16 MiB: 8.4 times one row).  The
 * file does not depend on slab_rows.  n_threads is used by the host mode only.
 * stats (HOST int64[4], or NULL) = {chunks deflated on the device, raw bytes
 * read from HBM, compressed bytes copied to the host, device workspace bytes};
 * all zero in the host mode. */
#define GSKYHIP_DEFLATE_HOST 0
#define GSKYHIP_DEFLATE_DEVICE 1
int gskyhip_encode_netcdf_deflate(const void *const *bands, int n_bands, int dtype, int width, int height,
                                  const double *geot, int epsg, const double *nodata, const char *const *names,
                                  int zlevel, int n_threads, int deflate, int slab_rows, uint8_t *out,
                                  int64_t capacity, int64_t *size, int64_t *stats, void *stream);
/* The same from HOST bands (EncodeGdal's rasters are host memory in the
 * reference): no device involved. */
int gskyhip_encode_netcdf_host(const void *const *bands, int n_bands, int dtype, int width, int height,
                               const double *geot, int epsg, const double *nodata, const char *const *names,
                               int zlevel, int n_threads, uint8_t *out, int64_t capacity, int64_t *size);
/* The same for an SRS given as gskyhip_crs_from_srs takes it, for the
 * families without an EPSG code (geostationary: the CF `geostationary`
 * mapping with sweep_angle_axis always written, and the WKT1
 * Geostationary_Satellite node as spatial_ref).  GSKYHIP_E_CRS for an SRS
 * outside the supported families. */
int gskyhip_encode_netcdf_srs_host(const void *const *bands, int n_bands, int dtype, int width, int height,
                                   const double *geot, const char *srs, const double *nodata,
                                   const char *const *names, int zlevel, int n_threads, uint8_t *out,
                                   int64_t capacity, int64_t *size);

/* ---- drill (WPS zonal statistics) --------------------------------------- */
/* readData (worker/gdalprocess/drill.go:90-227), mean / pixel-count mode,
 * decileCount = 0, for a batch of polygons over one time stack.
 *   stack: dev float32, time-innermost layout [y][x][t] of an
 *     xsize x ysize x n_bands stack, t fastest, t padded to t_stride >= n_bands
 *     (xsize * ysize < 2^31).
 *   win: dev int32 4 per polygon {off_x, off_y, count_x, count_y}
 *     (DrillFileDescriptor, drill.go:25-29); pixels of a window outside the
 *     stack count as outside the mask.
 *   mask_off: dev int64 per polygon, byte offset into masks (dev uint8,
 *     255 = in, row-major count_x*count_y); the polygons' mask regions must
 *     not overlap and every region must lie inside [0, mask_bytes).
 *   bands: HOST int32 list of 1-based band numbers (the reference's
 *     `bands []int32`), or NULL for 1..n_bands (n_list ignored).
 *   band_strides as drill.go:110-219.  Rows per polygon =
 *     gskyhip_drill_rows(n_list, band_strides).
 *   mode 0: reference summation order, means bit-exact; mode 1: wave-split
 *     reduction (float32 partials over 1024-pixel segments, combined in
 *     float64), within 1e-5 relative of mode 0, not bound by the largest polygon.
 *   out_value: dev f64, out_count: dev i32, n_polys x rows.
 *   workspace: dev, gskyhip_drill_workspace_size bytes. */
int gskyhip_drill_rows(int n_bands, int band_strides);
int64_t gskyhip_drill_workspace_size(int n_polys, int64_t mask_bytes, int n_list, int band_strides,
                                     int mode);
int gskyhip_drill_batch(const float *stack, int xsize, int ysize, int n_bands, int t_stride,
                        const int32_t *win, const int64_t *mask_off, const uint8_t *masks,
                        int n_polys, int64_t mask_bytes, const int32_t *bands, int n_list,
                        float nodata, float clip_lower, float clip_upper, int pixel_count,
                        int band_strides, int mode, double *out_value, int32_t *out_count,
                        void *workspace, int64_t workspace_bytes, void *stream);
/* computeDeciles (worker/gdalprocess/drill.go:229-273; decileCount > 0,
 * bandStrides 1) for the same batch as gskyhip_drill_batch: per polygon and
 * selected band the in-mask, non-nodata values (no clipping) and the
 * reference's decile_count picks of their ascending order, found by radix
 * selection (no sort).
 *   totals: dev int32 n_polys x n_list, the out_count of the mean pass
 *     (gskyhip_drill_batch, same bands, band_strides 1): deciles only where
 *     total > 0, zeros elsewhere (drill.go:179-191);
 *   out: dev float32 n_polys x n_list x decile_count (decile_count <= 16);
 *   status: dev int32 n_polys x n_list -- 0, 1 (total 0: the reference's
 *     Count-0 zeros), GSKYHIP_E_RANGE (the reference indexes past the values
 *     and panics: len % (dc+1) == 0 with len == dc+1);
 *   band_chunk: bands per pass (workspace scales with mask_bytes x band_chunk). */
int64_t gskyhip_drill_deciles_workspace_size(int n_polys, int64_t mask_bytes, int band_chunk);
int gskyhip_drill_deciles(const float *stack, int xsize, int ysize, int n_bands, int t_stride,
                          const int32_t *win, const int64_t *mask_off, const uint8_t *masks, int n_polys,
                          int64_t mask_bytes, const int32_t *bands, int n_list, float nodata, int decile_count,
                          int band_chunk, const int32_t *totals, float *out, int32_t *status, void *workspace,
                          int64_t workspace_bytes, void *stream);

/* readData complete (worker/gdalprocess/drill.go:90-227), one call per
 * batch of polygons over one time stack -- what DrillDataset (drill.go:33-88)
 * calls after getDrillFileDescriptor: readData(ds, bands, geom, bandStrides,
 * decileCount, pixelCount, clipUpper, clipLower).  Mean / pixel-count
 * (pixel_count), decile_count >= 0 (<= 16), band_strides >= 1 with the
 * reference's bound-band reads and interpolated rows (every column, counts
 * math.Round of the two bounds' mean).  Arguments as gskyhip_drill_batch;
 * out_value (dev f64) / out_count (dev i32): n_polys x rows x (1 +
 * decile_count) = Result.TimeSeries (Value, Count) row-major with Shape
 * [rows, 1 + decile_count], rows = gskyhip_drill_rows(n_list, band_strides);
 * status: dev int32 per polygon, 0 or GSKYHIP_E_RANGE where computeDeciles
 * would panic (the reference's gsky-gdal-process dies; the request fails). */
int64_t gskyhip_drill_read_data_workspace_size(int n_polys, int64_t mask_bytes, int n_list, int band_strides,
                                               int decile_count, int mode);
int gskyhip_drill_read_data(const float *stack, int xsize, int ysize, int n_bands, int t_stride,
                            const int32_t *win, const int64_t *mask_off, const uint8_t *masks, int n_polys,
                            int64_t mask_bytes, const int32_t *bands, int n_list, float nodata,
                            float clip_lower, float clip_upper, int pixel_count, int band_strides,
                            int decile_count, int mode, double *out_value, int32_t *out_count,
                            int32_t *status, void *workspace, int64_t workspace_bytes, void *stream);

/* Round-1 form (bands 1..n_bands, mode 0): sizes and allocates its workspace
 * itself (one synchronous read-back of win / mask_off). */
int gskyhip_drill(const float *stack, int xsize, int ysize, int n_bands, int t_stride,
                  const int32_t *win, const int64_t *mask_off, const uint8_t *masks,
                  int n_polys, float nodata, float clip_lower, float clip_upper,
                  int pixel_count, int band_strides, double *out_value,
                  int32_t *out_count, void *stream);

/* getDrillFileDescriptor + createMask (drill.go:363-423, 275-327) for n
 * request geometries against one dataset (HOST function, no device work):
 *   geometries: GeoJSON (a Feature or a bare Polygon / MultiPolygon) in
 *     WGS84 lon/lat, as GeoRPCGranule.Geometry; first repaired as
 *     OGR_G_Buffer(g, 0, 30) does it (drill.go:364-367, GEOS 3.7.2's
 *     zero-distance buffer: self-intersecting / overlapping rings become the
 *     region of depth >= 1; an empty buffer keeps the rings as drawn);
 *   dataset_srs: the dataset's SRS (NULL / "" = no projection: no transform);
 *   geot, xsize, ysize: the dataset's geotransform and size.
 * Per polygon: win_out[4*i..] = {off_x, off_y, count_x, count_y} with the
 * reference's int32 truncations, status_out[i] = 0, GSKYHIP_E_ARG (geometry
 * not parsable), GSKYHIP_E_CRS (transform failed) or GSKYHIP_E_RANGE (the
 * polygon misses the file; window 0).  mask_off_out[i] = byte offset of its
 * mask (16-byte aligned, polygon order), *mask_bytes_out = total bytes.
 * masks_out: NULL sizes only; else a HOST buffer of *mask_bytes_out bytes
 * that receives the ALL_TOUCHED masks (255 = burnt) -- the layout
 * gskyhip_drill_batch takes (copy it to the device). */
int gskyhip_drill_descriptors(const char *const *geometries, int n, const char *dataset_srs,
                              const double *geot, int xsize, int ysize, int32_t *win_out,
                              int64_t *mask_off_out, int64_t *mask_bytes_out, uint8_t *masks_out,
                              int32_t *status_out);

/* DrillMerger weighted mean (drill_merger.go:79-93): values/counts dev
 * n_files x n_dates, out dev n_dates (NaN where no count). */
/* The same descriptors with the ALL_TOUCHED masks rasterized on the GPU
 * straight into masks_dev (dev, mask_bytes: call once with masks_dev NULL to
 * size it), one workgroup per polygon (edges, then scanlines) -- the
 * expressions of the host rasterizer, bit-identical masks.  win_out,
 * mask_off_out, mask_bytes_out, status_out are host arrays as above. */
int gskyhip_drill_descriptors_device(const char *const *geometries, int n, const char *dataset_srs,
                                     const double *geot, int xsize, int ysize, int32_t *win_out,
                                     int64_t *mask_off_out, int64_t *mask_bytes_out, uint8_t *masks_dev,
                                     int32_t *status_out, void *stream);

/* Device memory supplier of gskyhip_drill_masks_device: returns at least
 * `bytes` of device memory (or NULL), owned by the caller (cgo: a hipMalloc
 * wrapper; Python: a torch tensor kept alive by the caller). */
typedef void *(*gskyhip_alloc_fn)(void *ctx, int64_t bytes);

/* gskyhip_drill_descriptors_device in one pass (getDrillFileDescriptor +
 * createMask, drill.go:363-423 / 275-327, for a whole WPS request): every
 * polygon described once on up to 16 host threads, then alloc(alloc_ctx,
 * *mask_bytes_out) supplies the mask buffer (returned in *masks_dev_out) and
 * the masks are rasterized into it on `stream`.  GSKYHIP_E_HIP if alloc
 * returns NULL. */
int gskyhip_drill_masks_device(const char *const *geometries, int n, const char *dataset_srs, const double *geot,
                               int xsize, int ysize, int32_t *win_out, int64_t *mask_off_out,
                               int64_t *mask_bytes_out, gskyhip_alloc_fn alloc, void *alloc_ctx,
                               uint8_t **masks_dev_out, int32_t *status_out, void *stream);
/* The same with the n geometries packed NUL-separated in one buffer of
 * packed_bytes (every string NUL-terminated inside it). */
int gskyhip_drill_masks_device_packed(const char *packed, int64_t packed_bytes, int n, const char *dataset_srs,
                                      const double *geot, int xsize, int ysize, int32_t *win_out,
                                      int64_t *mask_off_out, int64_t *mask_bytes_out, gskyhip_alloc_fn alloc,
                                      void *alloc_ctx, uint8_t **masks_dev_out, int32_t *status_out, void *stream);
/* Test hook: the GeoJSON number parser of the drill descriptors on n
 * NUL-separated strings packed in `text`; out[i] the value, consumed[i] the
 * characters parsed (strtod semantics). */
int gskyhip_parse_numbers(const char *text, int n, double *out, int32_t *consumed);
int gskyhip_drill_merge(const double *values, const int32_t *counts, int n_files,
                        int n_dates, double *out, void *stream);

/* ---- misc ---------------------------------------------------------------- */
uint32_t gskyhip_fnv32a(const char *s, int64_t n);
const char *gskyhip_version(void);
int gskyhip_device_count(void);
/* Status of the last render call (TilePlan status of every tile, read back
 * synchronously): 0 OK or the first error code; n_tiles of the last call. */
int gskyhip_render_status(void *workspace, int n_tiles, int n_pairs, int max_tile_height, void *stream);

/* Diagnostics of the last plan in `workspace` (synchronous): per tile
 * {status, complex (1: some row needs exact per-pixel transforms or the value
 * types are mixed -> general kernel), common value type (GSKYHIP_* or 0),
 * merged entries}; counters_out (3 ints, may be NULL): leaf-pool entries used,
 * rows split by the approximation recursion, complex tiles.  No reference counterpart (an observability hook). */
int gskyhip_render_tile_info(void *workspace, int n_tiles, int n_pairs, int max_tile_height, int32_t *info_out,
                             int32_t *counters_out, void *stream);

/* Source footprint of every pair of a planned batch: info_out (n_pairs x 8
 * int32) = {granule, picked level width, height, element bytes, x0, y0, x1,
 * y1}: the bounding box [x0, x1) x [y0, y1) at that level of the source
 * pixels the pair's linear rows sample.  For the algorithmic bytes of a
 * batch (bench.py C5).  No reference counterpart (an observability hook). */
int gskyhip_render_pair_info(void *workspace, int n_tiles, int n_pairs, int max_tile_height, int32_t *info_out,
                             void *stream);

/* Algorithmic source bytes of a planned batch (unique
 * source bytes touched at the chosen overview level): bytes_out[0] = the
 * distinct source elements x element bytes that the window pixels of every
 * pair (data and mask rasters) pick by the nearest-neighbour rule of
 * warp.go:271-300; bytes_out[1] = the distinct 128-byte lines holding them
 * x 128.  Counted over each picked level once, however many pairs share it
 * (bench.py C5).  No reference counterpart (an observability hook). */
int gskyhip_render_touched(void *workspace, int n_tiles, int n_pairs, int max_tile_height, int64_t *bytes_out,
                           void *stream);

#ifdef __cplusplus
}
#endif
#endif
