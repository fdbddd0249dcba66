#!/usr/bin/env python
"""Timing of gskyhip_build_overviews on the GPU (DESIGN.md "Overview
pyramids") and what a built pyramid buys a zoomed-out batch.  One JSON line.

Kernel time: HIP events around `--calls` back-to-back pyramids, each over
its own copy of a size x size granule (the copies together exceed the 256 MiB
Infinity Cache, so the source comes from HBM), median of `--runs` such
windows after a warm-up.  Algorithmic bytes = source once + every level
written; the fraction is of the 8 TB/s roofline DESIGN.md uses.
With GSKYHIP_LIB=ab the one-launch-per-level variant of the same kernel
(GSKYHIP_OVR_PASS_LEVELS=1) is timed alternately with the three-level pass.

Touched bytes: gskyhip_render_touched of one 16-tile zoomed-out batch over
the granule, with and without the built pyramid."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np   # noqa: E402
import torch         # noqa: E402

from gsky_amd import GranuleSet, ScaleParams, TileBatch, _lib, ingest   # noqa: E402
from gsky_amd.tiles import DTYPE_OF_TORCH                                # noqa: E402


def time_method(srcs, outs, sizes, method, calls, runs, warmup, nodata=-999.0):
    L = _lib.lib()
    n = len(sizes)
    xs = (C.c_int32 * n)(*[w for w, _ in sizes])
    ys = (C.c_int32 * n)(*[h for _, h in sizes])
    ptrs = [(C.c_void_p * n)(*[o.data_ptr() for o in lv]) for lv in outs]
    ysize, xsize = srcs[0].shape
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    dt = DTYPE_OF_TORCH[srcs[0].dtype]

    def window():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for k in range(calls):
            i = k % len(srcs)
            rc = L.gskyhip_build_overviews(C.c_void_p(srcs[i].data_ptr()), dt, 0, xsize, ysize, 1, nodata,
                                           _lib.OVR_METHODS[method], n, ptrs[i], xs, ys, stream)
            if rc:
                raise _lib.GskyError(rc, "build_overviews")
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e-3 / calls

    for _ in range(warmup):
        window()
    t = sorted(window() for _ in range(runs))
    return {"median_us": statistics.median(t) * 1e6, "min_us": t[0] * 1e6, "max_us": t[-1] * 1e6}


def touched(a, build):
    """(element bytes, 128-byte line bytes) one 4 x 4 batch of 128-pixel
    EPSG:3857 tiles over the whole granule touches."""
    n = a.shape[0]
    geot = [110.0, 40.0 / n, 0.0, -10.0, 0.0, -40.0 / n]
    r = 6378137.0
    mx = lambda lon: r * np.radians(lon)
    my = lambda lat: r * np.log(np.tan(np.pi / 4 + np.radians(lat) / 2))
    x0, x1, y0, y1 = mx(110.0), mx(150.0), my(-50.0), my(-10.0)
    tiles = []
    for j in range(4):
        for i in range(4):
            tiles.append(((x0 + (x1 - x0) * i / 4, y0 + (y1 - y0) * j / 4, x0 + (x1 - x0) * (i + 1) / 4,
                           y0 + (y1 - y0) * (j + 1) / 4), 128, 128))
    gs = GranuleSet("cuda:0")
    gs.add(a, geot, "EPSG:4326", -999.0, build_overviews=build)
    tb = TileBatch(gs, "EPSG:3857", tiles, [[0]] * len(tiles))
    tb.render(ScaleParams(0.0, 0.03, 8000.0), None)
    torch.cuda.synchronize()
    assert tb.status() == 0
    return tb.touched_bytes()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4000)
    ap.add_argument("--copies", type=int, default=10)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--runs", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_overviews: needs a HIP device")
    torch.cuda.set_device(0)
    n = args.size
    rng = np.random.default_rng(1)
    host = rng.integers(-2000, 20000, (n, n)).astype(np.int16)
    host[rng.random((n, n)) < 0.1] = -999
    t = torch.from_numpy(host)
    touched_bytes = {"plain": touched(t, None), "built_nearest": touched(t, "nearest")}
    srcs = [torch.from_numpy(host).cuda() for _ in range(args.copies)]
    sizes = ingest.overview_levels(n, n, 256)
    outs = [[torch.empty((h, w), dtype=torch.int16, device="cuda") for w, h in sizes] for _ in range(args.copies)]
    alg = 2 * (n * n + sum(w * h for w, h in sizes))
    res = {"size": n, "dtype": "int16", "levels": sizes, "algorithmic_bytes": alg, "copies": args.copies,
           "calls_per_window": args.calls, "runs": args.runs, "lib": os.environ.get("GSKYHIP_LIB", "") or "product"}
    ab = os.environ.get("GSKYHIP_LIB", "") == "ab"
    variants = [("3", "three_level_pass"), ("1", "one_level_per_launch")] if ab else [(None, "three_level_pass")]
    for method in ("average", "nearest"):
        for rep in range(2 if ab else 1):   # alternate the variants
            for knob, name in variants:
                if knob is not None:
                    os.environ["GSKYHIP_OVR_PASS_LEVELS"] = knob
                r = time_method(srcs, outs, sizes, method, args.calls, args.runs, args.warmup)
                r["roofline_fraction_8TBs"] = alg / (r["median_us"] * 1e-6) / 8e12
                res.setdefault(method, {}).setdefault(name, []).append(r)
    res["touched_bytes"] = touched_bytes
    print(json.dumps(res))


if __name__ == "__main__":
    main()
