#!/usr/bin/env python
"""WCS GeoTIFF output: the reference's PackBits file (the unchanged path and
the yardstick here) against the opt-in Deflate file with the tiles deflated on
host threads (deflate="host") and in HBM (deflate="device"), on the same bands
in the same run.  One JSON line.

Inputs, one band each, already in HBM as a rendered coverage is -- the three
of tools/bench_netcdf_out.py:
  * the C3 field (float32) at 1024^2 and at 4096^2, written with predictor 3;
  * a C2-style int16 band at 4000^2, written with predictor 2.
Block 1024 x 256, what ows.go passes.  Each timing is a host clock around the
whole encode_geotiff call (allocation of the output, copies, kernels, host
framing; the call returns the finished file).  Every (input, mode) pair is
warmed once; the modes are then timed alternately, `--runs` times, and the
median is reported with min and max, the file size and the compressed bytes
the device mode copied.  The device file is first compared with the host
mode's (the same bytes) and read back against the band."""
import argparse
import datetime
import json
import os
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np   # noqa: E402
import torch         # noqa: E402

from gsky_amd import encode, ingest   # noqa: E402
from tools.bench_netcdf_out import GT, c2_field, c3_field, lib_sha, timed   # noqa: E402

MODES = ("packbits", "deflate_host", "deflate_device")
BLOCK = (1024, 256)


def measure(name, band, nodata, predictor, runs, threads, tmp):
    dev = [torch.from_numpy(band).cuda()]
    kw = dict(nodata=[nodata], names=[name], block=BLOCK, threads=threads)
    enc = {"packbits": lambda: encode.encode_geotiff(dev, GT, 4326, **kw),
           "deflate_host": lambda: encode.encode_geotiff(dev, GT, 4326, compression="deflate", predictor=predictor,
                                                         deflate="host", **kw),
           "deflate_device": lambda: encode.encode_geotiff(dev, GT, 4326, compression="deflate", predictor=predictor,
                                                           deflate="device", **kw)}
    files = {m: enc[m]() for m in MODES}   # warm-up, sizes and the checks
    if files["deflate_device"] != files["deflate_host"]:
        raise SystemExit("bench_geotiff_out: the device and host files of %s differ" % name)
    blob, stats = encode.encode_geotiff(dev, GT, 4326, compression="deflate", predictor=predictor, deflate="device",
                                        return_stats=True, **kw)
    p = os.path.join(tmp, name + ".tif")
    with open(p, "wb") as f:
        f.write(blob)
    if not np.array_equal(ingest.read_host(p, 1).view(np.uint8), band.view(np.uint8)):
        raise SystemExit("bench_geotiff_out: the device file of %s does not read back" % name)
    os.remove(p)
    ms = {m: [] for m in MODES}
    for _ in range(runs):
        for m in MODES:
            ms[m].append(timed(enc[m]))
    res = {"shape": list(band.shape), "dtype": str(band.dtype), "raw_bytes": int(band.nbytes), "predictor": predictor}
    for m in MODES:
        res[m] = {"encode_ms_median": statistics.median(ms[m]), "encode_ms_min": min(ms[m]),
                  "encode_ms_max": max(ms[m]), "file_bytes": len(files[m])}
    for m in MODES[1:]:
        res[m]["time_ratio_to_packbits"] = res[m]["encode_ms_median"] / res["packbits"]["encode_ms_median"]
        res[m]["size_ratio_to_packbits"] = len(files[m]) / len(files["packbits"])
    res["device_stats"] = {"tiles": stats[0], "raw_bytes_read": stats[1], "compressed_bytes_copied": stats[2],
                           "workspace_bytes": stats[3]}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16, help="host threads of deflate=\"host\"")
    ap.add_argument("--sizes", default="1024,4096", help="C3 field sizes")
    ap.add_argument("--c2-size", type=int, default=4000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_geotiff_out: needs a HIP device")
    torch.cuda.set_device(0)
    res = {"tool": "bench_geotiff_out", "runs": args.runs, "host_threads": args.threads, "block": list(BLOCK),
           "lib_sha16": lib_sha(), "date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0),
           "inputs": {}}
    with tempfile.TemporaryDirectory() as tmp:
        for n in [int(s) for s in args.sizes.split(",") if s]:
            res["inputs"]["c3_f32_%d" % n] = measure("c3_%d" % n, c3_field(n), -9999.0, 3, args.runs, args.threads, tmp)
        if args.c2_size > 0:
            res["inputs"]["c2_i16_%d" % args.c2_size] = measure("c2_%d" % args.c2_size, c2_field(args.c2_size), -999.0,
                                                                2, args.runs, args.threads, tmp)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
