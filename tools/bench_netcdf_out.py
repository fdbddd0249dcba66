#!/usr/bin/env python
"""WCS netCDF output: the chunks deflated on host threads (deflate="host", 16
zlib threads -- the path every release so far has, and the yardstick here)
against the chunks shuffled and deflated on the GPU (deflate="device"), on the
same bands in the same run.  One JSON line.

Inputs, one band each, already in HBM as a rendered coverage is:
  * the C3 field (float32, 200 + 50 sin(lon / 3) cos(lat / 2)
    plus uniform noise in [0, 1), 1% nodata -9999) at 1024^2 and at 4096^2;
  * a C2-style int16 band at 4000^2 (a smooth field plus noise, as
    tools/bench_ingest.py makes it).
Each timing is a host clock around the whole encode_netcdf call (copies,
kernels, host framing; the call returns the finished file).  Every (input,
mode) pair is warmed once; the modes are then timed alternately, `--runs`
times, and the median is reported with the file sizes and the device / host
ratio of both.  The device file is read back and compared with the band
first."""
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

from gsky_amd import encode, ingest   # noqa: E402

MODES = ("host", "device")
GT = [112.0, 0.01, 0.0, -10.0, 0.0, -0.01]


def c3_field(n, seed=1):
    rng = np.random.default_rng(seed)
    lon = 112.0 + 42.0 * (np.arange(n) + 0.5) / n
    lat = -10.0 - 34.0 * (np.arange(n) + 0.5) / n
    v = (200.0 + 50.0 * np.sin(lon[None, :] / 3.0) * np.cos(lat[:, None] / 2.0) + rng.random((n, n))).astype(np.float32)
    v[rng.random((n, n)) < 0.01] = -9999.0
    return v


def c2_field(n, seed=2):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:n, 0:n].astype(np.float32)
    f = 3000.0 * np.sin(x / 97.0) * np.cos(y / 131.0) + 0.4 * x + rng.standard_normal((n, n)).astype(np.float32) * 12.0
    return f.astype(np.int16)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def lib_sha():
    h = hashlib.sha256()
    with open(os.path.join(ROOT, "gsky_amd", "libgskyhip.so"), "rb") as f:
        h.update(f.read())
    return h.hexdigest()[:16]


def measure(name, band, nodata, runs, threads, tmp):
    dev = [torch.from_numpy(band).cuda()]
    enc = lambda mode: encode.encode_netcdf(dev, GT, 4326, nodata=[nodata], names=[name], deflate=mode,   # noqa: E731
                                            threads=threads)
    files = {m: enc(m) for m in MODES}   # warm-up, sizes and the check
    blob, stats = encode.encode_netcdf(dev, GT, 4326, nodata=[nodata], names=[name], deflate="device",
                                       return_stats=True)
    p = os.path.join(tmp, name + ".nc")
    with open(p, "wb") as f:
        f.write(blob)
    if not np.array_equal(ingest.read_host(p, 1).view(np.uint8), band.view(np.uint8)):
        raise SystemExit("bench_netcdf_out: the device file of %s does not read back" % name)
    os.remove(p)
    ms = {m: [] for m in MODES}
    for _ in range(runs):
        for m in MODES:
            ms[m].append(timed(lambda: enc(m)))
    res = {"shape": list(band.shape), "dtype": str(band.dtype), "raw_bytes": int(band.nbytes)}
    for m in MODES:
        res[m] = {"encode_ms_median": statistics.median(ms[m]), "encode_ms_min": min(ms[m]),
                  "encode_ms_max": max(ms[m]), "file_bytes": len(files[m])}
    res["device_to_host_time_ratio"] = res["device"]["encode_ms_median"] / res["host"]["encode_ms_median"]
    res["device_to_host_size_ratio"] = len(files["device"]) / len(files["host"])
    res["device_stats"] = {"chunks": stats[0], "raw_bytes_read": stats[1], "compressed_bytes_copied": stats[2],
                           "workspace_bytes": stats[3]}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16, help="host zlib threads of the yardstick")
    ap.add_argument("--sizes", default="1024,4096", help="C3 field sizes")
    ap.add_argument("--c2-size", type=int, default=4000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_netcdf_out: needs a HIP device")
    torch.cuda.set_device(0)
    res = {"tool": "bench_netcdf_out", "runs": args.runs, "host_threads": args.threads, "lib_sha16": lib_sha(),
           "date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0), "inputs": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for n in [int(s) for s in args.sizes.split(",") if s]:
            res["inputs"]["c3_f32_%d" % n] = measure("c3_%d" % n, c3_field(n), -9999.0, args.runs, args.threads, tmp)
        if args.c2_size > 0:
            res["inputs"]["c2_i16_%d" % args.c2_size] = measure("c2_%d" % args.c2_size, c2_field(args.c2_size), -999.0,
                                                                args.runs, args.threads, tmp)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
