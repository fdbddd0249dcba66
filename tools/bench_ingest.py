#!/usr/bin/env python
"""Granule ingest: block decode on host threads (decode="host", the path every
release so far has) against block decode on the GPU (decode="device"), on the
same files in the same run.  One JSON line.

The files are written here with the test suite's writers:
  * `--files` GeoTIFFs of `--size`^2 int16, Deflate, 256 x 256 tiles, predictor 2;
  * one netCDF-4 file of `--nc-bands` x `--nc-size`^2 float32, shuffle + deflate,
    chunks of (1, `--nc-rows`, `--nc-size`) -- row bands.
Each timing is a host clock around ingest.read(), which returns after the
stream has been synchronised, so it covers the file read (page cache), the
decode, the copies and the kernels: what a cold granule cache pays per band.
Every (file, mode) is warmed once; the modes are then timed alternately,
`--runs` times, and the median is reported -- per file, and for all files of
a kind back to back.  The two modes' tensors are compared bit for bit first."""
import argparse
import datetime
import hashlib
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np   # noqa: E402
import torch         # noqa: E402

from gsky_amd import ingest                     # noqa: E402
from tests.h5write import Var, write_nc4        # noqa: E402
from tests.tiffwrite import write_tiff          # noqa: E402

MODES = ("host", "device")


def field(rng, n, dtype):
    """A smooth field plus noise: what a predictor and Deflate meet in a granule."""
    y, x = np.mgrid[0:n, 0:n].astype(np.float32)
    f = 3000.0 * np.sin(x / 97.0) * np.cos(y / 131.0) + 0.4 * x + rng.standard_normal((n, n)).astype(np.float32) * 12.0
    return f.astype(dtype)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def measure(jobs, runs):
    """jobs: list of (path, band).  Per-job and back-to-back medians, in ms."""
    stats = {}
    for path, band in jobs:
        outs = {}
        for mode in MODES:   # warm-up, statistics and the comparison
            t, st = ingest.read(path, band, decode=mode, return_stats=True)
            outs[mode] = t
            stats.setdefault(mode, []).append(st)
        if not torch.equal(outs["host"], outs["device"]):
            raise SystemExit("bench_ingest: the two decodes differ on %s band %d" % (path, band))
        del outs
    per = {m: [[] for _ in jobs] for m in MODES}
    batch = {m: [] for m in MODES}
    for _ in range(runs):
        for mode in MODES:
            for k, (path, band) in enumerate(jobs):
                per[mode][k].append(timed(lambda: ingest.read(path, band, decode=mode)))
        for mode in MODES:
            batch[mode].append(timed(lambda: [ingest.read(p, b, decode=mode) for p, b in jobs]))
    res = {}
    for mode in MODES:
        one = [statistics.median(v) for v in per[mode]]
        res[mode] = {"per_file_ms_median": statistics.median(one), "per_file_ms_min": min(one),
                     "per_file_ms_max": max(one), "all_files_ms_median": statistics.median(batch[mode]),
                     "all_files_ms_min": min(batch[mode]), "all_files_ms_max": max(batch[mode]),
                     "blocks_device": sum(s[0] for s in stats[mode]), "blocks_host": sum(s[1] for s in stats[mode])}
    dev = stats["device"]
    res["bytes_in"] = sum(s[2] for s in dev)       # compressed bytes copied to the device
    res["bytes_out"] = sum(s[3] for s in dev)      # decoded bytes produced
    res["device_to_host_ratio_one_file"] = res["device"]["per_file_ms_median"] / res["host"]["per_file_ms_median"]
    res["device_to_host_ratio_all_files"] = res["device"]["all_files_ms_median"] / res["host"]["all_files_ms_median"]
    return res


def lib_sha():
    h = hashlib.sha256()
    with open(os.path.join(ROOT, "gsky_amd", "libgskyhip.so"), "rb") as f:
        h.update(f.read())
    return h.hexdigest()[:16]


def write_files(d, args):
    """The GeoTIFFs as [(path, band)] and the netCDF-4 file's path."""
    rng = np.random.default_rng(7)
    tiffs = []
    base = field(rng, args.size, np.int16)
    for k in range(args.files):
        p = os.path.join(d, "g%02d.tif" % k)
        write_tiff(p, [np.roll(base, 37 * k, axis=1) + np.int16(k)], tile=(256, 256), compression=8, predictor=2)
        tiffs.append((p, 1))
    n = args.nc_size
    two = [field(rng, n, np.float32) for _ in range(2)]
    cube = np.stack([np.roll(two[k % 2], 11 * k, axis=0) for k in range(args.nc_bands)])
    nc = os.path.join(d, "cube.nc")
    write_nc4(nc, [("time", args.nc_bands), ("lat", n), ("lon", n)],
              [Var("lat", ("lat",), -10.0 - 0.01 * np.arange(n), filters=()),
               Var("lon", ("lon",), 110.0 + 0.01 * np.arange(n), filters=()),
               Var("time", ("time",), np.arange(args.nc_bands, dtype=np.float64), filters=()),
               Var("v", ("time", "lat", "lon"), cube, chunks=(1, args.nc_rows, n), filters=("shuffle", "deflate"))],
              {"Conventions": "CF-1.6"})
    return tiffs, nc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4000)
    ap.add_argument("--files", type=int, default=10)
    ap.add_argument("--nc-size", type=int, default=2048)
    ap.add_argument("--nc-bands", type=int, default=16)
    ap.add_argument("--nc-rows", type=int, default=128)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--dir", default=None, help="where the files are written (default: a temporary directory)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ingest: needs a HIP device")
    torch.cuda.set_device(0)
    with tempfile.TemporaryDirectory(dir=args.dir) as d:
        tiffs, nc = write_files(d, args)
        n = args.nc_size
        res = {"tool": "bench_ingest", "runs": args.runs, "lib_sha16": lib_sha(),
               "date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0),
               "geotiff": dict(measure(tiffs, args.runs), files=args.files, size=args.size, dtype="int16",
                               tile=256, predictor=2, file_bytes=sum(os.path.getsize(p) for p, _ in tiffs)),
               "netcdf4": dict(measure([(nc, b + 1) for b in range(args.nc_bands)], args.runs),
                               bands=args.nc_bands, size=n, dtype="float32", chunk_rows=args.nc_rows,
                               filters="shuffle+deflate", file_bytes=os.path.getsize(nc))}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
