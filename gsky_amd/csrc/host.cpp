// host.cpp -- C-ABI of libgskyhip.so (include/gskyhip.h).
//
// Host side of the MI355X path: Go strconv mask parsing, the (path, band) ->
// HBM granule registry behind the warp_operation_fast drop-in, and the launch
// sequences (SRS parsing is crs.cpp's).  All pixel work runs in the HIP kernels
// of plan.hip / render.hip / windows.hip / stages.hip / drill.hip; nothing here falls back to the CPU.
#include <hip/hip_runtime.h>
#include <sys/stat.h>

#include <atomic>
#include <chrono>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/gskyhip.h"
#include "crs.h"
#include "drill.h"
#include "gsky_device.h"
#include "ingest.h"
#include "render.h"
#include "stages.h"
#include "service.h"
#include "warp_batch.h"

using namespace gsky;

namespace {

// ---------------------------------------------------------------- Go strconv (base 2)
uint64_t go_parse_uint2(const char *s, int bits, bool *syntax = nullptr) {
  const uint64_t maxVal = (bits >= 64) ? UINT64_MAX : ((1ull << bits) - 1);
  if (syntax) *syntax = false;
  if (!s || !*s) { if (syntax) *syntax = true; return 0; }
  uint64_t n = 0;
  for (const char *p = s; *p; p++) {
    const char c = *p;
    int d;
    if (c >= '0' && c <= '9') d = c - '0';
    else if ((c | 0x20) >= 'a' && (c | 0x20) <= 'z') d = (c | 0x20) - 'a' + 10;
    else { if (syntax) *syntax = true; return 0; }
    if (d >= 2) { if (syntax) *syntax = true; return 0; }
    if (n >= UINT64_MAX / 2 + 1) return maxVal;
    n *= 2;
    const uint64_t n1 = n + (uint64_t)d;
    if (n1 < n || n1 > maxVal) return maxVal;
    n = n1;
  }
  return n;
}
int64_t go_parse_int2(const char *s, int bits) {
  if (!s || !*s) return 0;
  bool neg = false;
  if (*s == '+') s++;
  else if (*s == '-') { neg = true; s++; }
  bool syntax = false;
  const uint64_t un = go_parse_uint2(s, bits, &syntax);
  if (syntax) return 0;
  const uint64_t cutoff = 1ull << (bits - 1);
  if (!neg && un >= cutoff) return (int64_t)(cutoff - 1);
  if (neg && un > cutoff) return -(int64_t)cutoff;
  return neg ? -(int64_t)un : (int64_t)un;
}

// Mask specs for the four mask-raster types (tile_merger.go:328-439).
int build_mask_specs(const gskyhip_mask *m, MaskSpecS out[4]) {
  std::memset(out, 0, sizeof(MaskSpecS) * 4);
  if (!m || m->ns < 0) return 0;
  const bool has_value = m->value && *m->value;
  if (!has_value) {
    if (m->n_bit_tests == 0 || m->n_bit_tests % 2 != 0) return GSKYHIP_E_MASK;
  }
  if (m->n_bit_tests > GSKYHIP_MAX_BIT_TESTS) return GSKYHIP_E_ARG;
  const int dts[4] = {GSKYHIP_SIGNEDBYTE, GSKYHIP_BYTE, GSKYHIP_INT16, GSKYHIP_UINT16};
  for (int k = 0; k < 4; k++) {
    MaskSpecS &o = out[k];
    const int dt = dts[k];
    const int bits = (dt == GSKYHIP_INT16 || dt == GSKYHIP_UINT16) ? 16 : 8;
    o.has_value = has_value ? 1 : 0;
    if (has_value) {
      switch (dt) {
        case GSKYHIP_SIGNEDBYTE: o.value = (int8_t)go_parse_uint2(m->value, 8); break;
        case GSKYHIP_BYTE: o.value = (uint8_t)go_parse_uint2(m->value, 8); break;
        case GSKYHIP_INT16: o.value = (int16_t)go_parse_int2(m->value, 16); break;
        default: o.value = (uint16_t)go_parse_uint2(m->value, 16); break;
      }
    } else {
      o.n_tests = m->n_bit_tests / 2;
      for (int j = 0; j < o.n_tests; j++) {
        const int64_t f = go_parse_int2(m->bit_tests[2 * j], bits);
        const int64_t v = go_parse_int2(m->bit_tests[2 * j + 1], bits);
        switch (dt) {
          case GSKYHIP_SIGNEDBYTE: o.filt[j] = (int8_t)f; o.want[j] = (int8_t)v; break;
          case GSKYHIP_BYTE: o.filt[j] = (uint8_t)f; o.want[j] = (uint8_t)v; break;
          case GSKYHIP_INT16: o.filt[j] = (int16_t)f; o.want[j] = (int16_t)v; break;
          default: o.filt[j] = (uint16_t)f; o.want[j] = (uint16_t)v; break;
        }
      }
    }
  }
  return 0;
}

int mask_slot_h(int dtype) {
  switch (dtype) {
    case GSKYHIP_SIGNEDBYTE: return 0;
    case GSKYHIP_BYTE: return 1;
    case GSKYHIP_INT16: return 2;
    case GSKYHIP_UINT16: return 3;
    default: return -1;
  }
}

// ---------------------------------------------------------------- drop-in state
struct Registered {
  gskyhip_granule g;
  gskyhip_crs crs;
  bool has_crs;
  // netCDF: the SRS under srs_cf=yes (netcdfdataset.cpp:3666), and whether
  // either SRS is a projection the warp cannot represent (-> GSKYHIP_E_CRS)
  gskyhip_crs crs_cf;
  bool has_crs_cf = false, bad_crs = false, bad_crs_cf = false;
  std::vector<void *> owned;   // HBM the library allocated for it (ingested files)
  int64_t bytes = 0;           // ... and its size
  uint64_t last_use = 0;       // DropIn::tick of the last batch that used it
  int64_t mtime_ns = 0, fsize = -1;   // the file as ingested (fsize < 0: registered by the caller)
  bool stamped = false;                // the stamp could be taken: re-read the file when it changes
  Registered() { std::memset(&g, 0, sizeof(g)); }
  Registered(const Registered &) = delete;
  Registered &operator=(const Registered &) = delete;
  // The registry and every warp batch in flight that reads the granule hold
  // it (shared_ptr): its HBM is freed when the last of them lets go, so a
  // re-ingest, an eviction or unregister_all never frees what a launched
  // batch still reads.
  ~Registered() {
    for (void *p : owned) (void)hipFree(p);
  }
};
using RegPtr = std::shared_ptr<Registered>;

struct DropIn {
  std::mutex mu;
  std::map<std::pair<std::string, int>, RegPtr> reg;
  uint64_t tick = 0;     // one per warp batch (LRU order of the ingest cache)
  // (path, band) ingested by the _ovr calls -> (method, min_size): a re-read of the
  // file (changed on disk, or evicted and requested again) builds the same pyramid
  std::map<std::pair<std::string, int>, std::pair<int, int>> ovr_asked;
  // where a registered file's blocks are decoded when it is read again
  // (gskyhip_register_*_decode; absent: the host)
  std::map<std::pair<std::string, int>, int> decode_asked;
  std::map<std::string, std::shared_ptr<struct GeoLocEntry>> geolocs;   // by GeoLocOpts (geoloc_entry)
};
DropIn &dropin() {
  static DropIn *d = new DropIn();   // never destroyed: its entries would call HIP at process exit
  return *d;
}

// HBM the ingested (library-owned) granules may hold before the least
// recently used ones are released: GSKYHIP_INGEST_CACHE_MB, default 32 GiB
// (of 288 GB per MI355X).  Caller-registered granules are never evicted.
int64_t ingest_cache_cap() {
  static const int64_t cap = [] {
    const char *e = std::getenv("GSKYHIP_INGEST_CACHE_MB");
    const long long mb = e ? std::atoll(e) : 32768;
    return (int64_t)(mb > 0 ? mb : 32768) << 20;
  }();
  return cap;
}

// Make room for `need` more bytes of ingested granules: drop the least
// recently used ones that no batch holds (in flight, or being assembled:
// last_use == d.tick).
void evict_for(DropIn &d, int64_t need) {
  const int64_t cap = ingest_cache_cap();
  for (;;) {
    int64_t held = 0;
    auto victim = d.reg.end();
    for (auto it = d.reg.begin(); it != d.reg.end(); ++it) {
      const Registered &R = *it->second;
      held += R.bytes;
      if (R.bytes > 0 && R.last_use < d.tick && it->second.use_count() == 1 &&
          (victim == d.reg.end() || R.last_use < victim->second->last_use))
        victim = it;
    }
    if (held + need <= cap || victim == d.reg.end()) return;   // fits, or nothing evictable: exceed the cap
    d.reg.erase(victim);
  }
}

// mtime (ns) and size of a file; false if it cannot be stat'ed
bool file_stamp(const std::string &path, int64_t &mtime_ns, int64_t &size) {
  std::string f = path;
  if (f.compare(0, 7, "NETCDF:") == 0) {   // NETCDF:file:var / NETCDF:"file":var
    f = f.substr(7);
    if (!f.empty() && f[0] == '"') {
      const size_t q = f.find('"', 1);
      f = q == std::string::npos ? f.substr(1) : f.substr(1, q - 1);
    } else {
      const size_t c = f.rfind(':');
      if (c != std::string::npos) f = f.substr(0, c);
    }
  }
  struct stat st;
  if (stat(f.c_str(), &st) != 0) return false;
  mtime_ns = (int64_t)st.st_mtim.tv_sec * 1000000000 + st.st_mtim.tv_nsec;
  size = (int64_t)st.st_size;
  return true;
}

bool have_gpu() {
  int n = 0;
  return hipGetDeviceCount(&n) == hipSuccess && n > 0;
}

// The pyramid an ingest builds for a band that came without overviews
// (overview.hip): method GSKYHIP_OVR_* or -1 (none), min_size as
// gskyhip_overview_levels takes it.  strict: a band type the pyramid does
// not cover fails the ingest (the _ovr calls); else it is ingested without.
struct OvrBuild {
  int method = -1, min_size = 0;
  bool strict = false;
  int decode = GSKYHIP_DECODE_HOST;   // where the file's blocks are decoded (gskyhip_register_*_decode)
};

bool ovr_type_ok(int dtype) {
  return dtype == GSKYHIP_BYTE || dtype == GSKYHIP_INT16 || dtype == GSKYHIP_UINT16 || dtype == GSKYHIP_FLOAT32;
}

// Level sizes of the pyramid `ob` asks for into info (n_ovr 0 on entry), or
// GSKYHIP_E_TYPE; *bytes grows by the levels' size.
int ovr_plan(const OvrBuild &ob, gskyhip_raster_info &info, int64_t *bytes) {
  if (ob.method < 0 || info.n_ovr > 0) return 0;   // a file's own overviews always win
  if (ob.method != GSKYHIP_OVR_NEAREST && ob.method != GSKYHIP_OVR_AVERAGE) return GSKYHIP_E_ARG;
  if (!ovr_type_ok(info.dtype)) return ob.strict ? GSKYHIP_E_TYPE : 0;
  const int n = gskyhip_overview_levels(info.xsize, info.ysize, ob.min_size, info.ovr_xsize, info.ovr_ysize);
  if (n < 0) return n;
  info.n_ovr = n;
  for (int k = 0; k < n; k++) *bytes += (int64_t)info.ovr_xsize[k] * info.ovr_ysize[k] * type_size(info.dtype);
  return 0;
}

// Allocate (into r.owned, after level 0) and build the levels ovr_plan sized;
// returns once they are complete, so any stream may read them.
int ovr_build(const gskyhip_raster_info &info, int method, Registered &r) {
  if (info.n_ovr <= 0) return 0;   // nothing planned (a small band, or a type ingested without)
  void *lv[GSKYHIP_MAX_OVR];
  const int ts = type_size(info.dtype);
  for (int k = 0; k < info.n_ovr; k++) {
    void *p = nullptr;
    if (hipMalloc(&p, (size_t)((int64_t)info.ovr_xsize[k] * info.ovr_ysize[k] * ts)) != hipSuccess) return GSKYHIP_E_HIP;
    r.owned.push_back(p);
    lv[k] = p;
  }
  const int rc = gskyhip_build_overviews(r.owned[0], info.dtype, info.signed_byte, info.xsize, info.ysize,
                                         info.has_nodata, info.nodata, method, info.n_ovr, lv, info.ovr_xsize,
                                         info.ovr_ysize, nullptr);
  if (rc) return rc;
  return hipStreamSynchronize(nullptr) == hipSuccess ? 0 : GSKYHIP_E_HIP;
}

// GDALOpenEx + GDALGetRasterBand of a GeoTIFF (warp.go:89-118) for the
// registry: every level of band `band` decoded into HBM the library owns
// (ingest.hip), registered under (path, band) with the file's SRS; a
// band without overviews gets the pyramid `ob` asks for.  Returns
// 0, 1 (open failed), 2 (no such band) or GSKYHIP_E_*.  d.mu held.
int ingest_geotiff_locked(DropIn &d, const std::string &path, int band, const OvrBuild &ob) {
  gskyhip_raster_info info;
  int rc = gskyhip_geotiff_info(path.c_str(), &info);
  if (rc) return rc;
  if (band < 1 || band > info.n_bands) return 2;
  if (!have_gpu()) return GSKYHIP_E_NOGPU;
  RegPtr rp = std::make_shared<Registered>();
  Registered &r = *rp;
  const int ts = type_size(info.dtype);
  if (ts <= 0) return GSKYHIP_E_TYPE;
  int64_t total = 0;
  for (int lv = 0; lv <= info.n_ovr; lv++)
    total += (int64_t)(lv ? info.ovr_xsize[lv - 1] : info.xsize) * (lv ? info.ovr_ysize[lv - 1] : info.ysize) * ts;
  const bool build = ob.method >= 0 && info.n_ovr == 0;
  if (build && (rc = ovr_plan(ob, info, &total))) return rc;
  d.reg.erase({path, band});   // a batch still holding the old entry keeps it alive
  evict_for(d, total);
  r.bytes = total;
  r.last_use = d.tick;
  r.stamped = file_stamp(path, r.mtime_ns, r.fsize);
  if (!r.stamped) r.fsize = 0;
  for (int lv = 0; lv <= info.n_ovr; lv++) {
    const int64_t xs = lv ? info.ovr_xsize[lv - 1] : info.xsize, ys = lv ? info.ovr_ysize[lv - 1] : info.ysize;
    void *p = nullptr;
    if (hipMalloc(&p, (size_t)(xs * ys * ts)) != hipSuccess) return GSKYHIP_E_HIP;
    r.owned.push_back(p);
    rc = ob.decode == GSKYHIP_DECODE_HOST
             ? gskyhip_geotiff_read(path.c_str(), band, lv, p, xs * ys * ts, nullptr)
             : gskyhip_geotiff_read_decode(path.c_str(), band, lv, p, xs * ys * ts, ob.decode, nullptr, nullptr);
    if (rc) return rc;
    if (build) break;   // the planned levels are built, not read
  }
  if (build && (rc = ovr_build(info, ob.method, r))) return rc;
  gskyhip_granule &g = r.g;
  g.data = r.owned[0];
  g.dtype = info.dtype; g.xsize = info.xsize; g.ysize = info.ysize; g.signed_byte = info.signed_byte;
  for (int k = 0; k < 6; k++) g.geot[k] = info.geot[k];
  g.nodata = info.nodata; g.has_nodata = info.has_nodata;
  g.n_ovr = info.n_ovr;
  for (int k = 0; k < info.n_ovr; k++) {
    g.ovr_data[k] = r.owned[k + 1]; g.ovr_xsize[k] = info.ovr_xsize[k]; g.ovr_ysize[k] = info.ovr_ysize[k];
  }
  g.block_x = info.block_x; g.block_y = info.block_y;
  r.has_crs = false;
  char srs[32] = {0};
  if (info.epsg > 0) std::snprintf(srs, sizeof(srs), "EPSG:%d", info.epsg);
  else if (info.epsg == -1) std::snprintf(srs, sizeof(srs), "MODIS");
  if (srs[0] && parse_srs(srs, &r.crs) == 0) r.has_crs = true;
  d.reg[{path, band}] = std::move(rp);
  return 0;
}

// The same for a netCDF classic variable band (band_query semantics,
// warp.go:89-101: the band is registered under (path, band)).
int ingest_netcdf_locked(DropIn &d, const std::string &path, int band, const OvrBuild &ob) {
  gskyhip_raster_info info;
  std::string srs_no, srs_cf;
  int rc = netcdf_info_srs(path.c_str(), &info, &srs_no, &srs_cf);
  if (rc) return rc;
  if (band < 1 || band > info.n_bands) return 1;   // band_query past the variable: the open fails
  if (!have_gpu()) return GSKYHIP_E_NOGPU;
  const int ts = type_size(info.dtype);
  if (ts <= 0) return GSKYHIP_E_TYPE;
  RegPtr rp = std::make_shared<Registered>();
  Registered &r = *rp;
  void *p = nullptr;
  const int64_t bytes0 = (int64_t)info.xsize * info.ysize * ts;
  int64_t bytes = bytes0;
  if ((rc = ovr_plan(ob, info, &bytes))) return rc;
  d.reg.erase({path, band});   // a batch still holding the old entry keeps it alive
  evict_for(d, bytes);
  r.bytes = bytes;
  r.last_use = d.tick;
  r.stamped = file_stamp(path, r.mtime_ns, r.fsize);
  if (!r.stamped) r.fsize = 0;
  if (hipMalloc(&p, (size_t)bytes0) != hipSuccess) return GSKYHIP_E_HIP;
  r.owned.push_back(p);
  rc = ob.decode == GSKYHIP_DECODE_HOST
           ? gskyhip_netcdf_read(path.c_str(), band, p, bytes0, nullptr)
           : gskyhip_netcdf_read_decode(path.c_str(), band, p, bytes0, ob.decode, nullptr, nullptr);
  if (rc) return rc;
  if ((rc = ovr_build(info, ob.method, r))) return rc;
  gskyhip_granule &g = r.g;
  g.data = p;
  g.dtype = info.dtype; g.xsize = info.xsize; g.ysize = info.ysize; g.signed_byte = info.signed_byte;
  for (int k = 0; k < 6; k++) g.geot[k] = info.geot[k];
  g.nodata = info.nodata; g.has_nodata = info.has_nodata;
  g.n_ovr = info.n_ovr;
  for (int k = 0; k < info.n_ovr; k++) {
    g.ovr_data[k] = r.owned[k + 1]; g.ovr_xsize[k] = info.ovr_xsize[k]; g.ovr_ysize[k] = info.ovr_ysize[k];
  }
  g.block_x = info.block_x; g.block_y = info.block_y;
  // "" -> no SRS (the warp takes WGS84, warp.go:107-112); "?" or one the
  // warp cannot parse -> the request fails with GSKYHIP_E_CRS
  auto set_crs = [](const std::string &srs, gskyhip_crs &c, bool &has, bool &bad) {
    has = false;
    bad = false;
    if (srs.empty()) return;
    if (srs != "?" && parse_srs(srs.c_str(), &c) == 0) has = true;
    else bad = true;
  };
  set_crs(srs_no, r.crs, r.has_crs, r.bad_crs);
  set_crs(srs_cf, r.crs_cf, r.has_crs_cf, r.bad_crs_cf);
  d.reg[{path, band}] = std::move(rp);
  return 0;
}

// ---------------------------------------------------------------- geolocation arrays
// GDALCreateGeoLocTransformer (GDAL 3.0.1 alg/gdalgeoloc.cpp [ext], called by
// createGeoLocTransformer, warp.go:52-67) for the drop-in: the X / Y bands
// named by GeoLocOpts (registered, or opened like any source file), read as
// double (GeoLocLoadFullData: a 1-row X and a 1-row Y band form a regular
// grid), then the backmap (GeoLocGenerateBackMap), kept in HBM and cached by
// the option strings.  Parity unpinned (GDAL is absent; oracle/ restates the
// same algorithm independently).
struct GeoLocEntry {
  GeoLocD d;
  std::vector<void *> owned;
  RegPtr x_src, y_src;   // the X / Y datasets it was built from: rebuilt when either is re-read
  GeoLocEntry() { std::memset(&d, 0, sizeof(d)); }
  GeoLocEntry(const GeoLocEntry &) = delete;
  GeoLocEntry &operator=(const GeoLocEntry &) = delete;
  ~GeoLocEntry() {
    for (void *p : owned) (void)hipFree(p);
  }
};
using GeoLocPtr = std::shared_ptr<GeoLocEntry>;

int ingest_geotiff_locked(DropIn &d, const std::string &path, int band, const OvrBuild &ob);
int ingest_netcdf_locked(DropIn &d, const std::string &path, int band, const OvrBuild &ob);

// The pyramid of the drop-in's own ingest (an unregistered path handed to
// warp_operation_fast, here or in the daemon): GSKYHIP_BUILD_OVERVIEWS =
// nearest | average, GSKYHIP_OVERVIEW_MIN_SIZE optional; read once.  Unset,
// empty or anything else: none.
const OvrBuild &auto_ovr() {
  static const OvrBuild ob = [] {
    OvrBuild o;
    const char *m = std::getenv("GSKYHIP_BUILD_OVERVIEWS");
    if (m && !std::strcmp(m, "nearest")) o.method = GSKYHIP_OVR_NEAREST;
    else if (m && !std::strcmp(m, "average")) o.method = GSKYHIP_OVR_AVERAGE;
    const char *ms = std::getenv("GSKYHIP_OVERVIEW_MIN_SIZE");
    if (ms) o.min_size = std::atoi(ms);
    return o;
  }();
  return ob;
}
bool is_geotiff_path(const std::string &p);

bool is_netcdf_path(const std::string &p) {
  return p.compare(0, 7, "NETCDF:") == 0 || (p.size() >= 3 && p.compare(p.size() - 3, 3, ".nc") == 0);
}

// The registry entry of (path, band) as GDALOpenEx would see it now: an
// ingested file that changed on disk is dropped and read again (never an
// entry this batch already uses: last_use == d.tick); an unregistered
// GeoTIFF / netCDF path is opened and ingested.  *irc: the ingest's code (0,
// 1 no such file, 2 no such band, GSKYHIP_E_*), or 0 when nothing was read.
RegPtr lookup_dataset(DropIn &d, const std::string &path, int band, int *irc) {
  *irc = 0;
  auto it = d.reg.find({path, band});
  if (it != d.reg.end() && it->second->fsize >= 0 && it->second->stamped && it->second->last_use != d.tick) {
    int64_t mt = 0, sz = 0;
    if (!file_stamp(path, mt, sz) || mt != it->second->mtime_ns || sz != it->second->fsize) {
      d.reg.erase(it);   // batches in flight keep their reference
      it = d.reg.end();
    }
  }
  const bool nc = is_netcdf_path(path);
  if (it == d.reg.end() && (nc || is_geotiff_path(path))) {
    OvrBuild ob = auto_ovr();
    const auto asked = d.ovr_asked.find({path, band});
    if (asked != d.ovr_asked.end()) {
      ob.method = asked->second.first;
      ob.min_size = asked->second.second;
    }
    const auto how = d.decode_asked.find({path, band});
    if (how != d.decode_asked.end()) ob.decode = how->second;
    *irc = nc ? ingest_netcdf_locked(d, path, band, ob) : ingest_geotiff_locked(d, path, band, ob);
    if (*irc == 0) it = d.reg.find({path, band});
  }
  if (it == d.reg.end()) return RegPtr();
  it->second->last_use = d.tick;
  return it->second;
}

bool band_as_double(const Registered &R, std::vector<double> &out) {
  const gskyhip_granule &g = R.g;
  const int ts = type_size(g.dtype);
  if (ts <= 0 || !g.data) return false;
  const size_t n = (size_t)g.xsize * g.ysize;
  std::vector<uint8_t> raw(n * ts);
  if (hipMemcpy(raw.data(), g.data, raw.size(), hipMemcpyDeviceToHost) != hipSuccess) return false;
  out.resize(n);
  for (size_t i = 0; i < n; i++) {
    const uint8_t *p = raw.data() + i * ts;
    switch (g.dtype) {
      case GSKYHIP_BYTE: out[i] = g.signed_byte ? (double)(int8_t)p[0] : (double)p[0]; break;
      case GSKYHIP_INT16: { int16_t v; std::memcpy(&v, p, 2); out[i] = v; break; }
      case GSKYHIP_UINT16: { uint16_t v; std::memcpy(&v, p, 2); out[i] = v; break; }
      case GSKYHIP_INT32: { int32_t v; std::memcpy(&v, p, 4); out[i] = v; break; }
      case GSKYHIP_UINT32: { uint32_t v; std::memcpy(&v, p, 4); out[i] = v; break; }
      case GSKYHIP_FLOAT32: { float v; std::memcpy(&v, p, 4); out[i] = v; break; }
      default: { double v; std::memcpy(&v, p, 8); out[i] = v; break; }
    }
  }
  return true;
}

// GeoLocGenerateBackMap: extent of the valid geolocation points, a grid of
// ~1.3 cells per point, every point splatted bilinearly into its 4 cells
// (source pixel / line weighted), cells with weight > 0.25 averaged (the
// others -1), then 3 passes filling holes from their set 4-neighbours (a cell
// filled in pass k is used from pass k+1 on).
bool geoloc_backmap(const std::vector<double> &gx, const std::vector<double> &gy, int nx, int ny, bool has_nd,
                    double nd, double pix_off, double line_off, double pix_step, double line_step,
                    std::vector<float> &bmx, std::vector<float> &bmy, int &bw, int &bh, double gt[6]) {
  const int nMaxIter = 3;
  double minX = 0, maxX = 0, minY = 0, maxY = 0;
  bool init = false;
  for (int64_t i = (int64_t)nx * ny - 1; i >= 0; i--) {
    if (has_nd && gx[i] == nd) continue;
    if (init) {
      minX = std::min(minX, gx[i]); maxX = std::max(maxX, gx[i]);
      minY = std::min(minY, gy[i]); maxY = std::max(maxY, gy[i]);
    } else {
      init = true;
      minX = maxX = gx[i];
      minY = maxY = gy[i];
    }
  }
  const double target = (double)nx * ny * 1.3;
  const double ps = std::sqrt((maxX - minX) * (maxY - minY) / target);
  if (!(ps > 0.0) || !std::isfinite(ps)) return false;
  const double fw = std::ceil((maxX - minX) / ps) + 1, fh = std::ceil((maxY - minY) / ps) + 1;
  if (!(fw > 0 && fw < 65536.0 * 64) || !(fh > 0 && fh < 65536.0 * 64) || fw * fh > 4.0e9) return false;
  bw = (int)fw;
  bh = (int)fh;
  minX -= ps / 2.0;
  maxY += ps / 2.0;
  gt[0] = minX; gt[1] = ps; gt[2] = 0.0; gt[3] = maxY; gt[4] = 0.0; gt[5] = -ps;
  const size_t nbm = (size_t)bw * bh;
  bmx.assign(nbm, 0.0f);
  bmy.assign(nbm, 0.0f);
  std::vector<float> wgt(nbm, 0.0f);
  for (int iY = 0; iY < ny; iY++)
    for (int iX = 0; iX < nx; iX++) {
      const size_t o = (size_t)iX + (size_t)iY * nx;
      if (has_nd && gx[o] == nd) continue;
      const double dBMX = (gx[o] - minX) / ps - 0.5;
      const double dBMY = (maxY - gy[o]) / ps - 0.5;
      const int iBMX = (int)std::floor(dBMX), iBMY = (int)std::floor(dBMY);
      const double fx = dBMX - iBMX, fy = dBMY - iBMY;
      const double sp = iX * pix_step + pix_off, sl = iY * line_step + line_off;
      for (int k = 0; k < 4; k++) {
        const int cx = iBMX + (k & 1), cy = iBMY + (k >> 1);
        if (cx < 0 || cx >= bw || cy < 0 || cy >= bh) continue;
        const double w = ((k & 1) ? fx : 1.0 - fx) * ((k >> 1) ? fy : 1.0 - fy);
        const size_t c = (size_t)cx + (size_t)cy * bw;
        bmx[c] += (float)(sp * w);
        bmy[c] += (float)(sl * w);
        wgt[c] += (float)w;
      }
    }
  for (size_t i = 0; i < nbm; i++) {
    if (wgt[i] > 0.25f) {
      bmx[i] /= wgt[i];
      bmy[i] /= wgt[i];
      wgt[i] = (float)(nMaxIter + 1);
    } else {
      bmx[i] = -1.0f;
      bmy[i] = -1.0f;
      wgt[i] = 0.0f;
    }
  }
  for (int iter = 0; iter < nMaxIter; iter++) {
    size_t valid = 0;
    const int mark = nMaxIter - iter;
    for (int y = 0; y < bh; y++)
      for (int x = 0; x < bw; x++) {
        const size_t c = (size_t)x + (size_t)y * bw;
        if (bmx[c] >= 0) { valid++; continue; }
        int n = 0;
        double sx = 0.0, sy = 0.0;
        auto take = [&](size_t j) { if (wgt[j] > mark) { sx += bmx[j]; sy += bmy[j]; n++; } };
        if (x > 0) take(c - 1);
        if (x + 1 < bw) take(c + 1);
        if (y > 0) take(c - bw);
        if (y + 1 < bh) take(c + bw);
        if (n > 0) {
          bmx[c] = (float)(sx / n);
          bmy[c] = (float)(sy / n);
          wgt[c] = (float)mark;
        }
      }
    if (valid == nbm) break;
  }
  return true;
}

// The transformer of one GeoLocOpts list (cached while its X / Y datasets
// are unchanged), or NULL (the reference's GDALCreateGeoLocTransformer
// failure: warp_operation_fast returns 3).
GeoLocPtr geoloc_entry(DropIn &d, const std::vector<std::string> &opts) {
  std::string key;
  for (const std::string &o : opts) key += o + '\n';
  std::map<std::string, std::string> kv;
  for (const std::string &o : opts) {
    const size_t e = o.find('=');
    if (e != std::string::npos) kv[o.substr(0, e)] = o.substr(e + 1);   // CSLFetchNameValue: KEY=VALUE
  }
  for (const char *k : {"PIXEL_OFFSET", "LINE_OFFSET", "PIXEL_STEP", "LINE_STEP", "X_BAND", "Y_BAND",
                        "X_DATASET", "Y_DATASET"})
    if (!kv.count(k)) return nullptr;   // "Missing some geolocation fields"
  int irc = 0;
  const RegPtr X = lookup_dataset(d, kv["X_DATASET"], std::atoi(kv["X_BAND"].c_str()), &irc);
  const RegPtr Y = lookup_dataset(d, kv["Y_DATASET"], std::atoi(kv["Y_BAND"].c_str()), &irc);
  if (!X || !Y) return nullptr;
  auto hit = d.geolocs.find(key);
  if (hit != d.geolocs.end()) {
    if (hit->second->x_src == X && hit->second->y_src == Y) return hit->second;
    d.geolocs.erase(hit);   // a dataset was re-read: build the transformer again
  }
  std::vector<double> ax, ay;
  if (!band_as_double(*X, ax) || !band_as_double(*Y, ay)) return nullptr;
  // GeoLocLoadFullData: a regular grid when both bands are one row
  const bool regular = X->g.ysize == 1 && Y->g.ysize == 1;
  const int nx = X->g.xsize, ny = regular ? Y->g.xsize : X->g.ysize;
  if (!regular && (Y->g.xsize != nx || Y->g.ysize != ny)) return nullptr;
  std::vector<double> gx((size_t)nx * ny), gy((size_t)nx * ny);
  for (int j = 0; j < ny; j++)
    for (int i = 0; i < nx; i++) {
      const size_t o = (size_t)j * nx + i;
      gx[o] = regular ? ax[i] : ax[o];
      gy[o] = regular ? ay[j] : ay[o];
    }
  GeoLocPtr e = std::make_shared<GeoLocEntry>();
  e->x_src = X;
  e->y_src = Y;
  GeoLocD &g = e->d;
  g.nx = nx; g.ny = ny;
  g.has_nodata = X->g.has_nodata ? 1 : 0;
  g.nodata_x = X->g.nodata;
  g.pixel_offset = std::atof(kv["PIXEL_OFFSET"].c_str());   // CPLAtof
  g.line_offset = std::atof(kv["LINE_OFFSET"].c_str());
  g.pixel_step = std::atof(kv["PIXEL_STEP"].c_str());
  g.line_step = std::atof(kv["LINE_STEP"].c_str());
  std::vector<float> bmx, bmy;
  int bw = 0, bh = 0;
  if (!geoloc_backmap(gx, gy, nx, ny, g.has_nodata != 0, g.nodata_x, g.pixel_offset, g.line_offset, g.pixel_step,
                      g.line_step, bmx, bmy, bw, bh, g.bm_gt))
    return nullptr;
  g.bm_w = bw; g.bm_h = bh;
  auto up = [&](const void *src, size_t bytes) -> void * {
    void *p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
    e->owned.push_back(p);
    if (hipMemcpy(p, src, bytes, hipMemcpyHostToDevice) != hipSuccess) return nullptr;
    return p;
  };
  g.gx = (const double *)up(gx.data(), gx.size() * 8);
  g.gy = (const double *)up(gy.data(), gy.size() * 8);
  g.bmx = (const float *)up(bmx.data(), bmx.size() * 4);
  g.bmy = (const float *)up(bmy.data(), bmy.size() * 4);
  if (!g.gx || !g.gy || !g.bmx || !g.bmy) return nullptr;
  d.geolocs[key] = e;
  return e;
}

bool is_geotiff_path(const std::string &p) {
  auto ends = [&](const char *suf) {
    const size_t n = std::strlen(suf);
    if (p.size() < n) return false;
    for (size_t i = 0; i < n; i++)
      if (std::tolower((unsigned char)p[p.size() - n + i]) != suf[i]) return false;
    return true;
  };
  return ends(".tif") || ends(".tiff");
}

}  // namespace

// ======================================================================== C-ABI
extern "C" {

int gskyhip_crs_transform(const gskyhip_crs *src, const gskyhip_crs *dst, int n, double *x, double *y,
                          int32_t *ok) {
  if (!src || !dst || n < 0 || (n > 0 && (!x || !y || !ok))) return GSKYHIP_E_ARG;
  for (int i = 0; i < n; i++) {
    double lam, phi;
    ok[i] = crs_inverse(*src, x[i], y[i], lam, phi) && crs_forward(*dst, lam, phi, x[i], y[i]) ? 1 : 0;
  }
  return 0;
}

uint32_t gskyhip_fnv32a(const char *s, int64_t n) {
  uint32_t h = 2166136261u;  // Go hash/fnv New32a (tile_merger.go:473-475)
  for (int64_t i = 0; i < n; i++) {
    h ^= (uint8_t)s[i];
    h *= 16777619u;
  }
  return h;
}

const char *gskyhip_version(void) { return "gskyhip 0.1 gfx950"; }

int gskyhip_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int gskyhip_register_granule(const char *path, int band, const gskyhip_granule *g, const char *srs) {
  if (!path || !g || !g->data || g->xsize <= 0 || g->ysize <= 0 || type_size(g->dtype) <= 0) return GSKYHIP_E_ARG;
  if (g->n_ovr < 0 || g->n_ovr > GSKYHIP_MAX_OVR) return GSKYHIP_E_ARG;
  for (int k = 0; k < g->n_ovr; k++)
    if (!g->ovr_data[k] || g->ovr_xsize[k] <= 0 || g->ovr_ysize[k] <= 0) return GSKYHIP_E_ARG;
  RegPtr r = std::make_shared<Registered>();
  r->g = *g;
  r->has_crs = false;
  if (srs && *srs) {
    if (parse_srs(srs, &r->crs)) return GSKYHIP_E_CRS;
    r->has_crs = true;
  }
  DropIn &d = dropin();
  std::lock_guard<std::mutex> lk(d.mu);
  d.reg[{std::string(path), band}] = std::move(r);
  return 0;
}

int gskyhip_unregister_all(void) {
  DropIn &d = dropin();
  std::lock_guard<std::mutex> lk(d.mu);
  d.reg.clear();       // HBM of ingested granules is freed once no batch in flight holds it
  d.ovr_asked.clear();
  d.decode_asked.clear();
  d.geolocs.clear();
  return 0;
}

int gskyhip_register_geotiff(const char *path, int band) {
  if (!path) return GSKYHIP_E_ARG;
  DropIn &d = dropin();
  std::lock_guard<std::mutex> lk(d.mu);
  d.ovr_asked.erase({path, band});
  d.decode_asked.erase({path, band});
  return ingest_geotiff_locked(d, path, band, OvrBuild());
}

int gskyhip_register_netcdf(const char *path, int band) {
  if (!path) return GSKYHIP_E_ARG;
  DropIn &d = dropin();
  std::lock_guard<std::mutex> lk(d.mu);
  d.ovr_asked.erase({path, band});
  d.decode_asked.erase({path, band});
  return ingest_netcdf_locked(d, path, band, OvrBuild());
}

int gskyhip_register_geotiff_ovr(const char *path, int band, int method, int min_size) {
  if (!path || (method != GSKYHIP_OVR_NEAREST && method != GSKYHIP_OVR_AVERAGE)) return GSKYHIP_E_ARG;
  DropIn &d = dropin();
  std::lock_guard<std::mutex> lk(d.mu);
  d.decode_asked.erase({path, band});
  OvrBuild ob;
  ob.method = method; ob.min_size = min_size; ob.strict = true;
  const int rc = ingest_geotiff_locked(d, path, band, ob);
  if (rc == 0) d.ovr_asked[{path, band}] = {method, min_size};
  return rc;
}

int gskyhip_register_netcdf_ovr(const char *path, int band, int method, int min_size) {
  if (!path || (method != GSKYHIP_OVR_NEAREST && method != GSKYHIP_OVR_AVERAGE)) return GSKYHIP_E_ARG;
  DropIn &d = dropin();
  std::lock_guard<std::mutex> lk(d.mu);
  d.decode_asked.erase({path, band});
  OvrBuild ob;
  ob.method = method; ob.min_size = min_size; ob.strict = true;
  const int rc = ingest_netcdf_locked(d, path, band, ob);
  if (rc == 0) d.ovr_asked[{path, band}] = {method, min_size};
  return rc;
}

static int register_decode(const char *path, int band, int method, int min_size, int decode, bool nc) {
  if (!path || (method != -1 && method != GSKYHIP_OVR_NEAREST && method != GSKYHIP_OVR_AVERAGE) ||
      (decode != GSKYHIP_DECODE_HOST && decode != GSKYHIP_DECODE_DEVICE))
    return GSKYHIP_E_ARG;
  DropIn &d = dropin();
  std::lock_guard<std::mutex> lk(d.mu);
  OvrBuild ob;
  ob.decode = decode;
  if (method < 0) {
    d.ovr_asked.erase({path, band});
  } else {
    ob.method = method; ob.min_size = min_size; ob.strict = true;
  }
  const int rc = nc ? ingest_netcdf_locked(d, path, band, ob) : ingest_geotiff_locked(d, path, band, ob);
  if (rc == 0 && method >= 0) d.ovr_asked[{path, band}] = {method, min_size};
  if (rc == 0 && decode != GSKYHIP_DECODE_HOST) d.decode_asked[{path, band}] = decode;
  else d.decode_asked.erase({path, band});
  return rc;
}

int gskyhip_register_geotiff_decode(const char *path, int band, int ovr_method, int min_size, int decode) {
  return register_decode(path, band, ovr_method, min_size, decode, false);
}

int gskyhip_register_netcdf_decode(const char *path, int band, int ovr_method, int min_size, int decode) {
  return register_decode(path, band, ovr_method, min_size, decode, true);
}

}  // extern "C"

// ---------------------------------------------------------------- warp batches
namespace gsky {

// warp.go:82-382 for n requests at once: per request the registry lookup and
// the reference's early returns (open / band / transformer failures), then
// every request with the same destination SRS planned and warped in one set
// of launches (one tile + one pair each), the window and bytesRead of every
// request in one pass, one read-back of the reply records.  Split in
// launch / finish so the service keeps two batches in flight (service.cpp).
namespace {
std::atomic<int64_t> g_wb_ns[4];
int64_t now_ns() {
  return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch())
      .count();
}
int64_t a256(int64_t v) { return (v + 255) & ~(int64_t)255; }
}  // namespace

void warp_batch_timers(int64_t out[4]) {
  for (int k = 0; k < 4; k++) out[k] = g_wb_ns[k].load();
}

// One batch's device, upload and read-back buffers, stream and completion
// event.  A slot carries one batch at a time; the buffers grow and are kept.
struct WarpSlot {
  hipStream_t stream = nullptr;
  hipEvent_t ev = nullptr;
  char *dev = nullptr;   // per group: header | results | stats | workspace | staged windows | scratch
  size_t dev_bytes = 0;
  char *up = nullptr;    // pinned: the groups' headers
  size_t up_bytes = 0;
  char *pin = nullptr;   // pinned: reply records, then staged windows
  size_t pin_bytes = 0;
  struct Job {
    int req;
    int err;                       // a launch failure of its group (GSKYHIP_E_*), else 0
    int64_t res_pin;               // reply record in `pin`
    int64_t win_dev, win_pin;      // staged window: device / pinned offsets (-1: written in place)
    int64_t stride;
  };
  std::vector<Job> jobs;
  std::vector<RegPtr> hold;        // granules the batch reads (freed only after it finished)
  std::vector<GeoLocPtr> hold_gl;
  WarpResp *out = nullptr;
  bool inflight = false;
};

WarpSlot *warp_slot_create() { return new WarpSlot(); }

void warp_slot_destroy(WarpSlot *s) {
  if (!s) return;
  warp_batch_finish(*s);
  if (s->dev) (void)hipFree(s->dev);
  if (s->up) (void)hipHostFree(s->up);
  if (s->pin) (void)hipHostFree(s->pin);
  if (s->ev) (void)hipEventDestroy(s->ev);
  if (s->stream) (void)hipStreamDestroy(s->stream);
  delete s;
}

namespace {
template <typename T> bool grow_dev(T *&p, size_t &have, size_t need) {
  if (have >= need) return true;
  if (p) (void)hipFree(p);
  p = nullptr;
  have = 0;
  if (hipMalloc((void **)&p, need) != hipSuccess) return false;
  have = need;
  return true;
}
bool grow_pin(char *&p, size_t &have, size_t need) {
  if (have >= need) return true;
  if (p) (void)hipHostFree(p);
  p = nullptr;
  have = 0;
  if (hipHostMalloc((void **)&p, need, hipHostMallocDefault) != hipSuccess) return false;
  have = need;
  return true;
}
}  // namespace

void warp_batch_launch(WarpSlot &S, const WarpReq *reqs, int n, WarpResp *out, uint8_t *const *direct,
                       const int64_t *direct_cap) {
  const int64_t t0 = now_ns();
  g_wb_ns[3]++;
  S.jobs.clear();
  S.out = out;
  S.inflight = false;
  DropIn &d = dropin();
  std::lock_guard<std::mutex> lk(d.mu);
  d.tick++;
  struct Item { int req; gskyhip_granule g; gskyhip_crs src; int bx, by; const GeoLocEntry *gl; };
  std::map<std::pair<int, std::string>, std::vector<Item>> groups;   // (has dst, dst srs) -> items
  for (int i = 0; i < n; i++) {
    const WarpReq &q = reqs[i];
    WarpResp &r = out[i];
    r = WarpResp();
    // warp.go:89-101: "NETCDF:..." and "*.nc" are opened through GSKY_netCDF
    // with band_query=<band>, which exposes that band as band 1; any other
    // path is opened whole and GDALGetRasterBand(band) may fail (114-118).
    const bool netcdf = is_netcdf_path(q.path);
    int irc = 0;
    const RegPtr RP = lookup_dataset(d, q.path, q.band, &irc);
    if (irc == 2) { r.rc = 2; continue; }
    if (irc < 0) { r.rc = irc; continue; }   // HBM exhausted, unsupported encoding, ...: an error, not "open failed"
    if (!RP) {   // (irc 1: no such file) a path registered with other bands is an open dataset without this band
      bool path_known = false;
      for (const auto &kv : d.reg) if (kv.first.first == q.path) { path_known = true; break; }
      r.rc = (netcdf || !path_known) ? 1 : 2;                         // open failed / band failed
      continue;
    }
    const Registered &R = *RP;
    if (!R.g.data) { r.rc = 2; continue; }                             // band failed
    if (q.width <= 0 || q.height <= 0) { r.rc = GSKYHIP_E_ARG; continue; }
    Item it2;
    it2.req = i;
    it2.gl = nullptr;
    if (q.geoloc) {   // warp.go:134-140: createGeoLocTransformer, 3 when it fails
      GeoLocPtr gl = geoloc_entry(d, q.geoloc_opts);
      if (!gl) { r.rc = 3; continue; }
      it2.gl = gl.get();
      S.hold_gl.push_back(std::move(gl));
    }
    // the dataset SRS: GSKY_netCDF opened with srs_cf=yes takes the CF
    // grid mapping only (warp.go:95, netcdfdataset.cpp:3666)
    const bool cf = netcdf && q.srs_cf > 0 && R.fsize >= 0;
    const bool has_crs = cf ? R.has_crs_cf : R.has_crs, bad_crs = cf ? R.bad_crs_cf : R.bad_crs;
    if (q.has_src_srs) {
      if (parse_srs(q.src_srs.c_str(), &it2.src)) { r.rc = 3; continue; }
    } else if (bad_crs) {
      r.rc = GSKYHIP_E_CRS;                                            // a projection outside the four families
      continue;
    } else if (has_crs) {
      it2.src = cf ? R.crs_cf : R.crs;
    } else {
      parse_srs("EPSG:4326", &it2.src);                                // warp.go:107-112
    }
    if (q.has_dst_srs) {
      gskyhip_crs tmp;
      if (parse_srs(q.dst_srs.c_str(), &tmp)) { r.rc = 3; continue; }
    }
    it2.g = R.g;
    it2.g.ns = 0;
    if (q.has_src_gt) std::memcpy(it2.g.geot, q.src_gt, sizeof(it2.g.geot));
    it2.bx = R.g.block_x > 0 ? R.g.block_x : 0;                      // 0: one scanline of the chosen level
    it2.by = R.g.block_y > 0 ? R.g.block_y : 1;
    S.hold.push_back(RP);
    groups[{q.has_dst_srs, q.has_dst_srs ? q.dst_srs : std::string()}].push_back(it2);
  }
  if (groups.empty()) { g_wb_ns[0] += now_ns() - t0; return; }
  auto fail_all = [&](int code) {
    for (auto &kv : groups) for (const Item &it : kv.second) out[it.req].rc = code;
  };
  if (!have_gpu()) { fail_all(GSKYHIP_E_NOGPU); return; }
  if ((!S.stream && hipStreamCreateWithFlags(&S.stream, hipStreamNonBlocking) != hipSuccess) ||
      (!S.ev && hipEventCreateWithFlags(&S.ev, hipEventDisableTiming) != hipSuccess)) {
    fail_all(GSKYHIP_E_HIP);
    return;
  }
  // ---- layout of every group in the slot's three buffers
  // device group: granules | geolocation transformers | crs (m sources + dst) | tiles | pairs
  //               | block-stats jobs | window destinations (uploaded up to here) | reply records
  //               | stats | workspace | staged windows | block-stats scratch
  struct Lay {
    const std::vector<Item> *items;
    const std::string *dst;
    int has_dst, m, max_w, max_h, n_staged;
    int64_t o_gl, o_crs, o_tiles, o_pairs, o_jobs, o_outs, o_res, o_stats, o_ws, ws, stride, o_win, o_scr, max_px;
    int64_t dev_base, up_base, pin_res, pin_win;
    std::vector<BlockStatsJob> jobs;
    std::vector<char> staged;
  };
  std::vector<Lay> lays;
  int64_t dev_total = 0, up_total = 0, pin_total = 0;
  for (auto &kv : groups) {
    Lay L;
    L.items = &kv.second;
    L.has_dst = kv.first.first;
    L.dst = &kv.first.second;
    const std::vector<Item> &items = kv.second;
    const int m = L.m = (int)items.size();
    L.max_w = 1; L.max_h = 1; L.max_px = 0; L.n_staged = 0;
    int64_t st_bytes = 0;
    std::vector<int64_t> n_words(m);
    L.jobs.resize(m);
    L.staged.assign(m, 0);
    for (int k = 0; k < m; k++) {
      const WarpReq &q = reqs[items[k].req];
      L.max_w = std::max(L.max_w, q.width);
      L.max_h = std::max(L.max_h, q.height);
      const gskyhip_granule &g = items[k].g;
      const int bx0 = items[k].bx > 0 ? items[k].bx : g.xsize;
      const int64_t nblocks = ((int64_t)(g.xsize + bx0 - 1) / bx0) * ((g.ysize + items[k].by - 1) / items[k].by);
      n_words[k] = (nblocks + 31) / 32;
      const int64_t px = (int64_t)q.width * q.height;
      L.max_px = std::max(L.max_px, px);
      BlockStatsJob &J = L.jobs[k];
      J.bx = items[k].bx; J.by = items[k].by; J.n_words = (int32_t)n_words[k]; J._pad = 0;
      J.xsrc_off = st_bytes;                     // xsrc of every job, then every job's bitmap
      st_bytes += a256(px * 4);
      const int i = items[k].req;
      // a window is written in place when the caller gave a destination big
      // enough for any value type (8 bytes per pixel)
      const bool in_place = direct && direct[i] && direct_cap && direct_cap[i] >= px * 8;
      if (!in_place) { L.staged[k] = 1; L.n_staged++; }
    }
    for (int k = 0; k < m; k++) {
      L.jobs[k].bits_off = st_bytes;
      st_bytes += a256(n_words[k] * 4);
    }
    L.o_gl = a256((int64_t)m * sizeof(gskyhip_granule));
    L.o_crs = L.o_gl + a256((int64_t)m * sizeof(GeoLocD));
    L.o_tiles = L.o_crs + a256((int64_t)(m + 1) * sizeof(gskyhip_crs));
    L.o_pairs = L.o_tiles + a256((int64_t)m * sizeof(gskyhip_tile));
    L.o_jobs = L.o_pairs + a256((int64_t)m * 4);
    L.o_outs = L.o_jobs + a256((int64_t)m * sizeof(BlockStatsJob));
    L.o_res = L.o_outs + a256((int64_t)m * sizeof(void *));
    L.o_stats = L.o_res + a256((int64_t)m * sizeof(WarpResult));
    L.o_ws = L.o_stats + a256((int64_t)m * 16);
    L.ws = render_workspace_size(m, m, L.max_h);
    L.stride = a256((int64_t)L.max_w * L.max_h * 8);
    L.o_win = L.o_ws + a256(L.ws);
    L.o_scr = L.o_win + L.stride * L.n_staged;
    L.dev_base = dev_total;
    dev_total += a256(L.o_scr + st_bytes);
    L.up_base = up_total;
    up_total += a256(L.o_res);
    L.pin_res = pin_total;
    pin_total += a256((int64_t)m * sizeof(WarpResult));
    L.pin_win = pin_total;
    pin_total += L.stride * L.n_staged;
    lays.push_back(std::move(L));
  }
  if (!grow_dev(S.dev, S.dev_bytes, (size_t)dev_total) || !grow_pin(S.up, S.up_bytes, (size_t)up_total) ||
      !grow_pin(S.pin, S.pin_bytes, (size_t)pin_total)) {
    fail_all(GSKYHIP_E_HIP);
    return;
  }
  // ---- headers, launches, reply read-back
  for (Lay &L : lays) {
    const std::vector<Item> &items = *L.items;
    const int m = L.m;
    char *base = S.dev + L.dev_base;
    char *hdr = S.up + L.up_base;
    std::memset(hdr, 0, (size_t)L.o_res);
    gskyhip_granule *hg = (gskyhip_granule *)hdr;
    gskyhip_crs *hc = (gskyhip_crs *)(hdr + L.o_crs);
    gskyhip_tile *ht = (gskyhip_tile *)(hdr + L.o_tiles);
    int32_t *hp = (int32_t *)(hdr + L.o_pairs);
    uint8_t **houts = (uint8_t **)(hdr + L.o_outs);
    int dst_crs = -1;
    if (L.has_dst) {
      parse_srs(L.dst->c_str(), &hc[m]);
      dst_crs = m;
    }
    std::memcpy(hdr + L.o_jobs, L.jobs.data(), (size_t)m * sizeof(BlockStatsJob));
    GeoLocD *hgl = (GeoLocD *)(hdr + L.o_gl);
    bool any_gl = false;
    int si = 0;
    for (int k = 0; k < m; k++) {
      const WarpReq &q = reqs[items[k].req];
      hg[k] = items[k].g;
      hg[k].crs = k;
      hg[k].geoloc = 0;
      if (items[k].gl) {
        hgl[k] = items[k].gl->d;
        hg[k].geoloc = k + 1;
        any_gl = true;
      }
      hc[k] = items[k].src;
      std::memcpy(ht[k].dst_geot, q.dst_gt, sizeof(ht[k].dst_geot));
      ht[k].width = q.width;
      ht[k].height = q.height;
      ht[k].pair_begin = k;
      ht[k].pair_end = k + 1;
      hp[k] = k;
      WarpSlot::Job J;
      J.req = items[k].req;
      J.err = 0;
      J.res_pin = L.pin_res + (int64_t)k * sizeof(WarpResult);
      J.stride = L.stride;
      if (L.staged[k]) {
        J.win_dev = L.dev_base + L.o_win + L.stride * si;
        J.win_pin = L.pin_win + L.stride * si;
        si++;
        houts[k] = (uint8_t *)(S.dev + J.win_dev);
      } else {
        J.win_dev = J.win_pin = -1;
        houts[k] = direct[J.req];
      }
      S.jobs.push_back(J);
    }
    const size_t first_job = S.jobs.size() - (size_t)m;
    auto fail = [&](int code) { for (size_t j = first_job; j < S.jobs.size(); j++) S.jobs[j].err = code; };
    if (hipMemcpyAsync(base, hdr, (size_t)L.o_res, hipMemcpyHostToDevice, S.stream) != hipSuccess) {
      fail(GSKYHIP_E_HIP);
      continue;
    }
    MaskSpecS ms[4];
    std::memset(ms, 0, sizeof(ms));
    RenderCall rc;
    rc.granules = (const gskyhip_granule *)base; rc.n_granules = m;
    rc.crs = (const gskyhip_crs *)(base + L.o_crs); rc.n_crs = m + 1; rc.dst_crs = dst_crs;
    rc.tiles = (const gskyhip_tile *)(base + L.o_tiles); rc.n_tiles = m;
    rc.pair_granule = (const int32_t *)(base + L.o_pairs); rc.n_pairs = m;
    rc.max_w = L.max_w; rc.max_h = L.max_h;
    rc.mask_ns = -1; rc.mask_inclusive = 0; rc.mask_specs = ms;
    rc.resample = GSKYHIP_RESAMPLE_NEAREST;
    rc.value_types = 0;
    rc.cov_offsets = nullptr;
    rc.cov_stride = 0;
    rc.workspace = base + L.o_ws; rc.workspace_bytes = L.ws;
    rc.stream = S.stream;
    rc.geolocs = any_gl ? (const GeoLocD *)(base + L.o_gl) : nullptr;
    int code = launch_warp_jobs(rc, (const BlockStatsJob *)(base + L.o_jobs), L.max_px, base + L.o_scr,
                                (int32_t *)(base + L.o_stats), (uint8_t *const *)(base + L.o_outs),
                                (WarpResult *)(base + L.o_res));
    if (!code && hipMemcpyAsync(S.pin + L.pin_res, base + L.o_res, (size_t)m * sizeof(WarpResult),
                                hipMemcpyDeviceToHost, S.stream) != hipSuccess)
      code = GSKYHIP_E_HIP;
    if (code) fail(code);
  }
  if (hipEventRecord(S.ev, S.stream) != hipSuccess) {
    for (WarpSlot::Job &J : S.jobs) J.err = GSKYHIP_E_HIP;
    (void)hipStreamSynchronize(S.stream);
  }
  S.inflight = true;
  g_wb_ns[0] += now_ns() - t0;
}

void warp_batch_finish(WarpSlot &S) {
  if (!S.inflight) {
    if (!S.hold.empty() || !S.hold_gl.empty()) {
      std::lock_guard<std::mutex> lk(dropin().mu);
      S.hold.clear();
      S.hold_gl.clear();
    }
    return;
  }
  const int64_t t0 = now_ns();
  const bool ok = hipEventSynchronize(S.ev) == hipSuccess;
  const int64_t t1 = now_ns();
  g_wb_ns[1] += t1 - t0;
  bool copy_ok = true;
  std::vector<int64_t> staged(S.jobs.size(), 0);   // staged window bytes to take per job
  int n_copies = 0;
  for (size_t j = 0; j < S.jobs.size(); j++) {
    const WarpSlot::Job &J = S.jobs[j];
    WarpResp &r = S.out[J.req];
    if (J.err || !ok) { r.rc = J.err ? J.err : GSKYHIP_E_HIP; continue; }
    WarpResult w;
    std::memcpy(&w, S.pin + J.res_pin, sizeof(w));
    for (int k = 0; k < 4; k++) r.bbox[k] = w.bbox[k];
    r.dtype = w.dtype;
    r.nodata = w.nodata;
    r.bytes_read = w.bytes_read;
    std::memcpy(r.src_gt, w.src_gt, sizeof(r.src_gt));
    const int64_t bytes = std::min<int64_t>(std::max<int64_t>((int64_t)w.bbox[2] * w.bbox[3] * type_size(w.dtype), 0),
                                            J.stride);
    if (J.win_dev < 0) {
      r.in_place = bytes;   // already in the caller's destination
    } else if (bytes > 0) {
      if (hipMemcpyAsync(S.pin + J.win_pin, S.dev + J.win_dev, (size_t)bytes, hipMemcpyDeviceToHost, S.stream) !=
          hipSuccess)
        copy_ok = false;
      staged[j] = bytes;
      n_copies++;
    }
  }
  if (n_copies && (!copy_ok || hipStreamSynchronize(S.stream) != hipSuccess)) copy_ok = false;
  for (size_t j = 0; j < S.jobs.size(); j++) {
    if (!staged[j]) continue;
    const WarpSlot::Job &J = S.jobs[j];
    WarpResp &r = S.out[J.req];
    if (!copy_ok) { r.rc = GSKYHIP_E_HIP; continue; }
    r.data.assign(S.pin + J.win_pin, S.pin + J.win_pin + staged[j]);
  }
  {
    std::lock_guard<std::mutex> lk(dropin().mu);
    S.hold.clear();
    S.hold_gl.clear();
  }
  S.inflight = false;
  g_wb_ns[2] += now_ns() - t1;
}

void warp_batch(const WarpReq *reqs, int n, WarpResp *out) {
  static std::mutex mu;
  static WarpSlot *slot = new WarpSlot();   // never destroyed: no HIP calls at process exit
  std::lock_guard<std::mutex> lk(mu);
  warp_batch_launch(*slot, reqs, n, out, nullptr, nullptr);
  warp_batch_finish(*slot);
}

}  // namespace gsky

extern "C" {

// warp.go:82 drop-in: one request through warp_batch -- in this process, or
// forwarded to the per-node service when GSKYHIP_SERVICE names its socket
// (service.cpp; the worker process then never touches the GPU).  The window
// comes back in malloc'd host memory the caller frees (warp.go:573-574).
int warp_operation_fast(const char *srcFilePath, char *srcProjRef, double *srcGeot,
                        const char **geoLocOpts, const char *dstProjRef, double *dstGeot,
                        int dstXImageSize, int dstYImageSize, int band, int srsCf, void **dstBuf,
                        int *dstBufSize, int *dstBbox, double *noData, int *dType, int *bytesRead) {
  *bytesRead = 0;
  if (!srcFilePath) return 1;
  if (!dstGeot) return GSKYHIP_E_ARG;
  WarpReq q;
  q.path = srcFilePath;
  q.band = band;
  q.has_src_srs = srcProjRef ? 1 : 0;
  if (srcProjRef) q.src_srs = srcProjRef;
  q.has_src_gt = srcGeot ? 1 : 0;
  if (srcGeot) std::memcpy(q.src_gt, srcGeot, sizeof(q.src_gt));
  q.geoloc = geoLocOpts ? 1 : 0;
  if (geoLocOpts)   // NULL-terminated (warp.go:514-526)
    for (int k = 0; geoLocOpts[k] && k < 64; k++) q.geoloc_opts.push_back(geoLocOpts[k]);
  q.has_dst_srs = dstProjRef ? 1 : 0;
  if (dstProjRef) q.dst_srs = dstProjRef;
  std::memcpy(q.dst_gt, dstGeot, sizeof(q.dst_gt));
  q.width = dstXImageSize;
  q.height = dstYImageSize;
  q.srs_cf = srsCf;
  WarpResp r;
  const char *svc = std::getenv("GSKYHIP_SERVICE");
  if (svc && *svc) {   // the window arrives straight in the malloc'd buffer
    void *mb = nullptr;
    size_t ml = 0;
    const int e = service_warp(svc, q, r, &mb, &ml);
    if (e) return e;
    if (r.rc) { std::free(mb); return r.rc; }
    *dstBuf = mb;
    *dstBufSize = (int)ml;
  } else {
    warp_batch(&q, 1, &r);
    if (r.rc) return r.rc;
    *dstBufSize = (int)r.data.size();
    *dstBuf = std::malloc(r.data.empty() ? 1 : r.data.size());
    if (!*dstBuf) return GSKYHIP_E_ARG;
    if (!r.data.empty()) std::memcpy(*dstBuf, r.data.data(), r.data.size());
  }
  for (int k = 0; k < 4; k++) dstBbox[k] = r.bbox[k];
  *noData = r.nodata;
  *dType = r.dtype;
  *bytesRead = r.bytes_read;
  if (srcGeot) std::memcpy(srcGeot, r.src_gt, sizeof(r.src_gt));
  return 0;
}

int64_t gskyhip_render_workspace_size(int n_tiles, int n_pairs, int max_tile_height) {
  return render_workspace_size(n_tiles, n_pairs, max_tile_height);
}

int gskyhip_render_tiles_phase(int phase, const gskyhip_granule *granules, int n_granules,
                               const gskyhip_crs *crs_table, int n_crs, int dst_crs, const gskyhip_tile *tiles,
                               int n_tiles, const int32_t *pair_granule, int n_pairs, int max_tile_width,
                               int max_tile_height, const int32_t *out_ns, int n_out_ns, const gskyhip_mask *mask,
                               int resample, const gskyhip_scale_params *sp, const uint8_t *ramp,
                               uint8_t *rgba_out, void *canvas_out, void *workspace, int64_t workspace_bytes,
                               void *stream) {
  return gskyhip_render_tiles_typed(phase, 0u, granules, n_granules, crs_table, n_crs, dst_crs, tiles, n_tiles,
                                    pair_granule, n_pairs, max_tile_width, max_tile_height, out_ns, n_out_ns, mask,
                                    resample, sp, ramp, rgba_out, canvas_out, workspace, workspace_bytes, stream);
}

static int render_call(int phase, uint32_t value_types, const gskyhip_granule *granules, int n_granules,
                       const gskyhip_crs *crs_table, int n_crs, int dst_crs, const gskyhip_tile *tiles,
                       int n_tiles, const int32_t *pair_granule, int n_pairs, int max_tile_width,
                       int max_tile_height, const int32_t *out_ns, int n_out_ns, const gskyhip_mask *mask,
                       int resample, const gskyhip_scale_params *sp, const uint8_t *ramp, uint8_t *rgba_out,
                       void *canvas_out, const int64_t *cov_offsets, int64_t cov_stride, void *workspace,
                       int64_t workspace_bytes, void *stream);

int gskyhip_render_coverage(int phase, uint32_t value_types, const gskyhip_granule *granules, int n_granules,
                            const gskyhip_crs *crs_table, int n_crs, int dst_crs, const gskyhip_tile *tiles,
                            int n_tiles, const int32_t *pair_granule, int n_pairs, int max_tile_width,
                            int max_tile_height, int resample, const gskyhip_scale_params *sp,
                            const int64_t *tile_offsets, int64_t row_stride, void *coverage_out, void *workspace,
                            int64_t workspace_bytes, void *stream) {
  if (!tile_offsets || !coverage_out || row_stride < max_tile_width) return GSKYHIP_E_ARG;
  const int32_t out_ns[1] = {0};
  return render_call(phase, value_types, granules, n_granules, crs_table, n_crs, dst_crs, tiles, n_tiles,
                     pair_granule, n_pairs, max_tile_width, max_tile_height, out_ns, 1, nullptr, resample, sp,
                     nullptr, nullptr, coverage_out, tile_offsets, row_stride, workspace, workspace_bytes, stream);
}

int gskyhip_render_tiles_typed(int phase, uint32_t value_types, const gskyhip_granule *granules,
                               int n_granules, const gskyhip_crs *crs_table, int n_crs, int dst_crs,
                               const gskyhip_tile *tiles, int n_tiles, const int32_t *pair_granule, int n_pairs,
                               int max_tile_width, int max_tile_height, const int32_t *out_ns, int n_out_ns,
                               const gskyhip_mask *mask, int resample, const gskyhip_scale_params *sp,
                               const uint8_t *ramp, uint8_t *rgba_out, void *canvas_out, void *workspace,
                               int64_t workspace_bytes, void *stream) {
  return render_call(phase, value_types, granules, n_granules, crs_table, n_crs, dst_crs, tiles, n_tiles,
                     pair_granule, n_pairs, max_tile_width, max_tile_height, out_ns, n_out_ns, mask, resample, sp,
                     ramp, rgba_out, canvas_out, nullptr, 0, workspace, workspace_bytes, stream);
}

static int render_call(int phase, uint32_t value_types, const gskyhip_granule *granules, int n_granules,
                       const gskyhip_crs *crs_table, int n_crs, int dst_crs, const gskyhip_tile *tiles,
                       int n_tiles, const int32_t *pair_granule, int n_pairs, int max_tile_width,
                       int max_tile_height, const int32_t *out_ns, int n_out_ns, const gskyhip_mask *mask,
                       int resample, const gskyhip_scale_params *sp, const uint8_t *ramp, uint8_t *rgba_out,
                       void *canvas_out, const int64_t *cov_offsets, int64_t cov_stride, void *workspace,
                       int64_t workspace_bytes, void *stream) {
  if (!sp || !out_ns || n_tiles < 0 || n_pairs < 0 || phase < 0 || phase > 2) return GSKYHIP_E_ARG;
  MaskSpecS ms[4];
  int r = build_mask_specs(mask, ms);
  if (r) return r;
  RenderCall rc;
  rc.granules = granules; rc.n_granules = n_granules;
  rc.crs = crs_table; rc.n_crs = n_crs; rc.dst_crs = dst_crs;
  rc.tiles = tiles; rc.n_tiles = n_tiles;
  rc.pair_granule = pair_granule; rc.n_pairs = n_pairs;
  rc.max_w = max_tile_width; rc.max_h = max_tile_height;
  rc.mask_ns = mask ? mask->ns : -1;
  rc.mask_inclusive = mask ? mask->inclusive : 0;
  rc.mask_specs = ms;
  rc.resample = resample;
  rc.value_types = value_types;
  rc.cov_offsets = cov_offsets;
  rc.cov_stride = cov_stride;
  rc.workspace = workspace; rc.workspace_bytes = workspace_bytes;
  rc.stream = (hipStream_t)stream;
  return launch_render(rc, out_ns, n_out_ns, *sp, ramp, rgba_out, canvas_out, phase);
}

int gskyhip_render_tiles(const gskyhip_granule *granules, int n_granules, const gskyhip_crs *crs_table,
                         int n_crs, int dst_crs, const gskyhip_tile *tiles, int n_tiles,
                         const int32_t *pair_granule, int n_pairs, int max_tile_width, int max_tile_height,
                         const int32_t *out_ns, int n_out_ns, const gskyhip_mask *mask, int resample,
                         const gskyhip_scale_params *sp, const uint8_t *ramp, uint8_t *rgba_out,
                         void *canvas_out, void *workspace, int64_t workspace_bytes, void *stream) {
  return gskyhip_render_tiles_phase(0, granules, n_granules, crs_table, n_crs, dst_crs, tiles, n_tiles,
                                    pair_granule, n_pairs, max_tile_width, max_tile_height, out_ns, n_out_ns,
                                    mask, resample, sp, ramp, rgba_out, canvas_out, workspace, workspace_bytes,
                                    stream);
}

int gskyhip_render_status(void *workspace, int n_tiles, int n_pairs, int max_tile_height, void *stream) {
  if (n_tiles <= 0) return 0;
  const int64_t off = gsky::render_tile_plans_offset(n_tiles, n_pairs, max_tile_height);
  std::vector<TilePlan> tp((size_t)n_tiles);
  if (hipMemcpyAsync(tp.data(), (char *)workspace + off, sizeof(TilePlan) * n_tiles, hipMemcpyDeviceToHost,
                     (hipStream_t)stream) != hipSuccess)
    return GSKYHIP_E_HIP;
  if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return GSKYHIP_E_HIP;
  for (const auto &t : tp)
    if (t.status) return t.status;
  return 0;
}

int gskyhip_render_tile_info(void *workspace, int n_tiles, int n_pairs, int max_tile_height, int32_t *info_out,
                             int32_t *counters_out, void *stream) {
  if (n_tiles < 0 || n_pairs < 0 || (n_tiles > 0 && (!workspace || !info_out))) return GSKYHIP_E_ARG;
  if (n_tiles == 0) return 0;
  const int64_t off = gsky::render_tile_plans_offset(n_tiles, n_pairs, max_tile_height);
  if (counters_out) {
    const int64_t c_off = gsky::render_counters_offset(n_tiles, n_pairs, max_tile_height);
    if (hipMemcpyAsync(counters_out, (char *)workspace + c_off, 3 * sizeof(int32_t), hipMemcpyDeviceToHost,
                       (hipStream_t)stream) != hipSuccess)
      return GSKYHIP_E_HIP;
  }
  std::vector<TilePlan> tp((size_t)n_tiles);
  if (hipMemcpyAsync(tp.data(), (char *)workspace + off, sizeof(TilePlan) * n_tiles, hipMemcpyDeviceToHost,
                     (hipStream_t)stream) != hipSuccess)
    return GSKYHIP_E_HIP;
  if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return GSKYHIP_E_HIP;
  for (int t = 0; t < n_tiles; t++) {
    info_out[4 * t] = tp[t].status;
    info_out[4 * t + 1] = tp[t].complex;
    info_out[4 * t + 2] = tp[t].vt;
    info_out[4 * t + 3] = tp[t].n_entries;
  }
  return 0;
}

int gskyhip_render_canvas_info(void *workspace, int n_tiles, int n_pairs, int max_tile_height, int32_t *info_out,
                               double *nodata_out, void *stream) {
  if (n_tiles < 0 || n_pairs < 0 || (n_tiles > 0 && (!workspace || !info_out || !nodata_out))) return GSKYHIP_E_ARG;
  if (n_tiles == 0) return 0;
  const int64_t off = gsky::render_tile_plans_offset(n_tiles, n_pairs, max_tile_height);
  std::vector<TilePlan> tp((size_t)n_tiles);
  if (hipMemcpyAsync(tp.data(), (char *)workspace + off, sizeof(TilePlan) * n_tiles, hipMemcpyDeviceToHost,
                     (hipStream_t)stream) != hipSuccess ||
      hipStreamSynchronize((hipStream_t)stream) != hipSuccess)
    return GSKYHIP_E_HIP;
  for (int t = 0; t < n_tiles; t++)
    for (int k = 0; k < 4; k++) {
      info_out[8 * t + k] = tp[t].created[k];
      info_out[8 * t + 4 + k] = tp[t].dtype[k];
      nodata_out[4 * t + k] = tp[t].nodata[k];
    }
  return 0;
}

int gskyhip_render_touched(void *workspace, int n_tiles, int n_pairs, int max_tile_height, int64_t *bytes_out,
                           void *stream) {
  if (n_tiles < 0 || n_pairs < 0 || !bytes_out || (n_pairs > 0 && !workspace)) return GSKYHIP_E_ARG;
  return launch_pair_touched(workspace, n_tiles, n_pairs, max_tile_height, bytes_out, (hipStream_t)stream);
}

int gskyhip_render_pair_info(void *workspace, int n_tiles, int n_pairs, int max_tile_height, int32_t *info_out,
                             void *stream) {
  if (n_tiles < 0 || n_pairs < 0 || (n_pairs > 0 && (!workspace || !info_out))) return GSKYHIP_E_ARG;
  if (n_pairs == 0) return 0;
  int32_t *dev = nullptr;
  if (hipMalloc((void **)&dev, (size_t)n_pairs * 8 * sizeof(int32_t)) != hipSuccess) return GSKYHIP_E_HIP;
  hipStream_t s = (hipStream_t)stream;
  int rc = launch_pair_footprint(workspace, n_tiles, n_pairs, max_tile_height, dev, s);
  if (!rc && (hipMemcpyAsync(info_out, dev, (size_t)n_pairs * 8 * sizeof(int32_t), hipMemcpyDeviceToHost, s) !=
                  hipSuccess ||
              hipStreamSynchronize(s) != hipSuccess))
    rc = GSKYHIP_E_HIP;
  (void)hipFree(dev);
  return rc;
}

int gskyhip_warp_windows(const gskyhip_granule *granules, int n_granules, const gskyhip_crs *crs_table,
                         int n_crs, int dst_crs, const gskyhip_tile *tiles, int n_tiles,
                         const int32_t *pair_granule, int n_pairs, int max_tile_width, int max_tile_height,
                         int resample, int32_t *bbox_out, int32_t *dtype_out, double *nodata_out,
                         void *win_out, int64_t win_stride, void *workspace, int64_t workspace_bytes,
                         void *stream) {
  MaskSpecS ms[4];
  std::memset(ms, 0, sizeof(ms));
  RenderCall rc;
  rc.granules = granules; rc.n_granules = n_granules;
  rc.crs = crs_table; rc.n_crs = n_crs; rc.dst_crs = dst_crs;
  rc.tiles = tiles; rc.n_tiles = n_tiles;
  rc.pair_granule = pair_granule; rc.n_pairs = n_pairs;
  rc.max_w = max_tile_width; rc.max_h = max_tile_height;
  rc.mask_ns = -1; rc.mask_inclusive = 0; rc.mask_specs = ms;
  rc.resample = resample;
  rc.value_types = 0;
  rc.cov_offsets = nullptr;
  rc.cov_stride = 0;
  rc.workspace = workspace; rc.workspace_bytes = workspace_bytes;
  rc.stream = (hipStream_t)stream;
  if (win_stride < (int64_t)max_tile_width * max_tile_height * 4) return GSKYHIP_E_ARG;
  return launch_warp_windows(rc, bbox_out, dtype_out, nodata_out, win_out, win_stride);
}

// ComputeReprojectExtent (warp.go:433-487), batched: one wavefront per granule.
int gskyhip_compute_reproject_extent(const gskyhip_granule *granules, int n, const gskyhip_crs *crs_table,
                                     int n_crs, int dst_crs, const double *dst_bbox, int32_t *out,
                                     int32_t *status, void *stream) {
  if (n < 0 || n_crs <= 0 || dst_crs >= n_crs || (n > 0 && (!granules || !crs_table || !dst_bbox || !out || !status)))
    return GSKYHIP_E_ARG;
  return launch_extent(granules, n, crs_table, dst_crs, dst_bbox, out, status, (hipStream_t)stream);
}

int64_t gskyhip_drill_deciles_workspace_size(int n_polys, int64_t mask_bytes, int band_chunk) {
  return drill_deciles_workspace_size(n_polys, mask_bytes, band_chunk);
}

// computeDeciles (drill.go:229-273) for a polygon batch: segmented GPU sort.
int gskyhip_drill_deciles(const float *stack, int xsize, int ysize, int n_bands, int t_stride, const int32_t *win,
                          const int64_t *mask_off, const uint8_t *masks, int n_polys, int64_t mask_bytes,
                          const int32_t *bands, int n_list, float nodata, int decile_count, int band_chunk,
                          const int32_t *totals, float *out, int32_t *status, void *workspace,
                          int64_t workspace_bytes, void *stream) {
  if (!stack || !win || !mask_off || !masks || !totals || !out || !status) return GSKYHIP_E_ARG;
  DecileCall c;
  c.stack = stack; c.xsize = xsize; c.ysize = ysize; c.n_bands = n_bands; c.t_stride = t_stride;
  c.win = win; c.mask_off = mask_off; c.masks = masks; c.n_polys = n_polys; c.mask_bytes = mask_bytes;
  c.bands = bands; c.n_list = n_list; c.nodata = nodata; c.decile_count = decile_count;
  c.band_chunk = band_chunk; c.totals = totals; c.out = out; c.status = status;
  c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.stream = (hipStream_t)stream;
  return launch_drill_deciles(c);
}

int64_t gskyhip_drill_read_data_workspace_size(int n_polys, int64_t mask_bytes, int n_list, int band_strides,
                                               int decile_count, int mode) {
  return drill_read_data_workspace_size(n_polys, mask_bytes, n_list, band_strides, decile_count, mode);
}

int gskyhip_drill_read_data(const float *stack, int xsize, int ysize, int n_bands, int t_stride, const int32_t *win,
                            const int64_t *mask_off, const uint8_t *masks, int n_polys, int64_t mask_bytes,
                            const int32_t *bands, int n_list, float nodata, float clip_lower, float clip_upper,
                            int pixel_count, int band_strides, int decile_count, int mode, double *out_value,
                            int32_t *out_count, int32_t *status, void *workspace, int64_t workspace_bytes,
                            void *stream) {
  if (!stack || !win || !mask_off || !masks || !out_value || !out_count || !status) return GSKYHIP_E_ARG;
  if (mode != 0 && mode != 1) return GSKYHIP_E_ARG;
  ReadDataCall c;
  c.stack = stack; c.xsize = xsize; c.ysize = ysize; c.n_bands = n_bands; c.t_stride = t_stride;
  c.win = win; c.mask_off = mask_off; c.masks = masks; c.n_polys = n_polys; c.mask_bytes = mask_bytes;
  c.bands = bands; c.n_list = n_list; c.nodata = nodata; c.lo = clip_lower; c.hi = clip_upper;
  c.pixel_count = pixel_count; c.band_strides = band_strides; c.decile_count = decile_count; c.mode = mode;
  c.out_value = out_value; c.out_count = out_count; c.status = status;
  c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.stream = (hipStream_t)stream;
  return launch_drill_read_data(c);
}

// RasterMerger.Run for one batch over warped FlexRasters (tile_merger.go:447-503).
int gskyhip_merge_rasters(const gskyhip_flex_raster *rasters, int n, const gskyhip_mask *mask,
                          void *const *canvases, int n_ns, int32_t *created, int32_t *dtype, double *nodata,
                          void *stream) {
  MaskSpecS ms[4];
  int r = build_mask_specs(mask, ms);
  if (r) return r;
  const int mask_ns = mask ? mask->ns : -1;
  const bool inclusive = mask && mask->inclusive;
  hipStream_t s = (hipStream_t)stream;
  std::vector<double> stamp(n);
  std::vector<int> keys;
  std::vector<char> in_stack(n, 0);
  for (int i = 0; i < n; i++) {
    stamp[i] = rasters[i].timestamp + (double)rasters[i].polygon_hash;   // 473-475
    if (mask_ns >= 0 && rasters[i].ns == mask_ns) {
      if (mask_slot_h(rasters[i].dtype) < 0) return GSKYHIP_E_MASK;      // 440-442
      if (!inclusive) continue;                                          // 485-487
    }
    in_stack[i] = 1;
  }
  // stable order: geoStamp descending, arrival order within a key (281-290)
  std::vector<int> order;
  for (int i = 0; i < n; i++) if (in_stack[i]) order.push_back(i);
  for (size_t a = 1; a < order.size(); a++) {
    const int v = order[a];
    size_t j = a;
    while (j > 0 && stamp[order[j - 1]] < stamp[v]) { order[j] = order[j - 1]; j--; }
    order[j] = v;
  }
  for (int k = 0; k < n_ns; k++) { created[k] = 0; dtype[k] = 0; nodata[k] = 0; }
  std::vector<std::vector<FlexEntry>> per_ns(n_ns);
  std::vector<double> canvas_ts(n_ns, 0.0);
  int width = 0, height = 0;
  for (int idx : order) {
    const gskyhip_flex_raster &fr = rasters[idx];
    if (fr.ns < 0 || fr.ns >= n_ns) return GSKYHIP_E_RANGE;
    width = fr.width; height = fr.height;
    if (!created[fr.ns]) {                                               // 291-297
      created[fr.ns] = 1;
      dtype[fr.ns] = fr.dtype;
      nodata[fr.ns] = fr.nodata;
      canvas_ts[fr.ns] = 0;
    } else if (dtype[fr.ns] != fr.dtype) {
      return GSKYHIP_E_TYPE;
    }
    FlexEntry e;
    std::memset(&e, 0, sizeof(e));
    e.data = fr.data;
    e.data_w = fr.data_w; e.data_h = fr.data_h; e.off_x = fr.off_x; e.off_y = fr.off_y;
    e.dtype = fr.dtype;
    e.nodata = fr.nodata;
    e.fill_mode = fr.timestamp < canvas_ts[fr.ns] ? 1 : 0;              // 47
    if (!e.fill_mode) canvas_ts[fr.ns] = fr.timestamp;
    for (int q = 0; q < n; q++) {                                        // maskMap[geoStamp]
      if (mask_ns >= 0 && rasters[q].ns == mask_ns && stamp[q] == stamp[idx]) {
        e.mask_data = rasters[q].data;
        e.mask_dtype = rasters[q].dtype;
        e.mask_len = (int64_t)rasters[q].data_w * rasters[q].data_h;
      }
    }
    if (e.mask_data && (int64_t)e.data_w * e.data_h > e.mask_len) return GSKYHIP_E_RANGE;
    per_ns[fr.ns].push_back(e);
  }
  for (int k = 0; k < n_ns; k++) {
    if (!created[k]) continue;
    const int slot = mask_slot_h(per_ns[k].empty() ? 0 : per_ns[k][0].mask_dtype);
    const MaskSpecS &m = ms[slot < 0 ? 0 : slot];
    // all mask rasters of one layer share a dtype; pick its spec
    MaskSpecS mm = m;
    for (const auto &e : per_ns[k]) {
      if (e.mask_data) { int sl = mask_slot_h(e.mask_dtype); if (sl >= 0) mm = ms[sl]; break; }
    }
    r = launch_merge_fold(per_ns[k].data(), (int)per_ns[k].size(), width, height, dtype[k], nodata[k], mm,
                          canvases[k], s);
    if (r) return r;
  }
  if (hipStreamSynchronize(s) != hipSuccess) return GSKYHIP_E_HIP;
  return 0;
}

int gskyhip_scale(void *data, int dtype, int64_t n, double nodata, const gskyhip_scale_params *sp,
                  uint8_t *out, void *stream) {
  if (!sp) return GSKYHIP_E_ARG;
  return launch_scale(data, dtype, n, nodata, *sp, out, (hipStream_t)stream);
}

int gskyhip_scale_legacy(void *data, int dtype, int64_t n, double nodata, const gskyhip_scale_params *sp,
                         uint8_t *out, void *stream) {
  if (!sp) return GSKYHIP_E_ARG;
  return launch_scale_legacy(data, dtype, n, nodata, *sp, out, (hipStream_t)stream);
}

// GradientRGBAPalette (utils/palette.go:27-69); 256 entries, host only.
int gskyhip_gradient_palette(const uint8_t *colours, int n, int interpolate, uint8_t *ramp) {
  auto interp = [](uint8_t a, uint8_t b, long i, long section) {
    const long q = (i * ((long)b - (long)a)) / section;   // Go int, truncating division
    return (uint8_t)(a + (uint8_t)q);                      // uint8 wrap
  };
  if (interpolate) {
    if (n < 2) return GSKYHIP_E_ARG;
    const int bins = n - 1, section = 256 / bins, bonus = 256 - section * bins;
    if (section == 0) return GSKYHIP_E_ARG;  // Go: integer divide by zero panic (palette.go:12)
    int index = 0;
    for (int s = 0; s < bins; s++) {
      const uint8_t *a = colours + 4 * s, *b = colours + 4 * (s + 1);
      const int cnt = section + (s < bonus ? 1 : 0);
      for (int i = 0; i < cnt; i++, index++) {
        uint8_t *o = ramp + 4 * index;
        o[0] = interp(a[0], b[0], i, section);
        o[1] = interp(a[1], b[1], i, section);
        o[2] = interp(a[2], b[2], i, section);
        o[3] = a[3];
      }
    }
  } else {
    if (n < 1) return GSKYHIP_E_ARG;
    const int bins = n, section = 256 / bins, bonus = 256 - section * bins;
    int index = 0;
    for (int s = 0; s < bins; s++) {
      const int cnt = section + (s < bonus ? 1 : 0);
      for (int i = 0; i < cnt; i++, index++) std::memcpy(ramp + 4 * index, colours + 4 * s, 4);
    }
  }
  return 0;
}

int gskyhip_encode_rgba(const uint8_t *const *bands, int nbands, int w, int h, const uint8_t *ramp,
                        uint8_t *rgba, void *stream) {
  if (nbands != 1 && nbands != 3) return GSKYHIP_E_ARG;
  return launch_encode_rgba(bands[0], nbands == 3 ? bands[1] : nullptr, nbands == 3 ? bands[2] : nullptr,
                            nbands, (int64_t)w * h, ramp, rgba, (hipStream_t)stream);
}

int gskyhip_compute_mask(const void *data, int dtype, int64_t n, const gskyhip_mask *mask, uint8_t *out,
                         void *stream) {
  gskyhip_mask m = mask ? *mask : gskyhip_mask{};
  m.ns = 0;
  MaskSpecS ms[4];
  int r = build_mask_specs(&m, ms);
  if (r) return r;
  const int slot = mask_slot_h(dtype);
  if (slot < 0) return GSKYHIP_E_MASK;
  return launch_compute_mask(data, dtype, n, ms[slot], out, (hipStream_t)stream);
}

int gskyhip_drill_rows(int n_bands, int band_strides) { return drill_rows_per_poly(n_bands, band_strides); }

int64_t gskyhip_drill_workspace_size(int n_polys, int64_t mask_bytes, int n_list, int band_strides, int mode) {
  return drill_workspace_size(n_polys, mask_bytes, n_list, band_strides, mode);
}

int gskyhip_drill_batch(const float *stack, int xsize, int ysize, int n_bands, int t_stride, const int32_t *win,
                        const int64_t *mask_off, const uint8_t *masks, int n_polys, int64_t mask_bytes,
                        const int32_t *bands, int n_list, float nodata, float clip_lower, float clip_upper,
                        int pixel_count, int band_strides, int mode, double *out_value, int32_t *out_count,
                        void *workspace, int64_t workspace_bytes, void *stream) {
  DrillCall c;
  c.stack = stack; c.xsize = xsize; c.ysize = ysize; c.n_bands = n_bands; c.t_stride = t_stride;
  c.win = win; c.mask_off = mask_off; c.masks = masks; c.n_polys = n_polys; c.mask_bytes = mask_bytes;
  c.bands = bands; c.n_list = n_list; c.nodata = nodata; c.lo = clip_lower; c.hi = clip_upper;
  c.pixel_count = pixel_count; c.band_strides = band_strides; c.mode = mode;
  c.out_value = out_value; c.out_count = out_count;
  c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.stream = (hipStream_t)stream;
  return launch_drill_batch(c);
}

// Round-1 entry point: sizes the workspace from the windows (synchronous
// read-back) and runs the reference-order batch over bands 1..n_bands.
int gskyhip_drill(const float *stack, int xsize, int ysize, int n_bands, int t_stride, const int32_t *win,
                  const int64_t *mask_off, const uint8_t *masks, int n_polys, float nodata, float clip_lower,
                  float clip_upper, int pixel_count, int band_strides, double *out_value, int32_t *out_count,
                  void *stream) {
  if (n_polys <= 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  std::vector<int32_t> w(4 * (size_t)n_polys);
  std::vector<int64_t> off((size_t)n_polys);
  if (hipMemcpyAsync(w.data(), win, w.size() * 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipMemcpyAsync(off.data(), mask_off, off.size() * 8, hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return GSKYHIP_E_HIP;
  int64_t mask_bytes = 0;
  for (int p = 0; p < n_polys; p++)
    mask_bytes = std::max<int64_t>(mask_bytes, off[p] + (int64_t)std::max(0, w[4 * p + 2]) * std::max(0, w[4 * p + 3]));
  const int64_t ws = drill_workspace_size(n_polys, mask_bytes, n_bands, band_strides, 0);
  void *buf = nullptr;
  if (hipMallocAsync(&buf, (size_t)ws, s) != hipSuccess) return GSKYHIP_E_HIP;
  const int r = gskyhip_drill_batch(stack, xsize, ysize, n_bands, t_stride, win, mask_off, masks, n_polys,
                                    mask_bytes, nullptr, n_bands, nodata, clip_lower, clip_upper, pixel_count,
                                    band_strides, 0, out_value, out_count, buf, ws, stream);
  if (hipFreeAsync(buf, s) != hipSuccess) return GSKYHIP_E_HIP;
  return r;
}

int gskyhip_drill_merge(const double *values, const int32_t *counts, int n_files, int n_dates, double *out,
                        void *stream) {
  return launch_drill_merge(values, counts, n_files, n_dates, out, (hipStream_t)stream);
}

}  // extern "C"
