#!/usr/bin/env python
"""GetMap PNG output: the truecolour encoder every WMS client gets today
(encode_png of render()'s RGBA; the unchanged path and the yardstick here)
against the opt-in indexed-colour encoder (encode_png_indexed of
render_bytes()'s ByteRasters), on the same tiles in the same run (DESIGN.md
4f).  One JSON line.

Input: `--tiles` covered tiles of the C2 batch (evenly spaced over the tiles
the index gives a granule, as bench.py's --png-tiles leg picks them), rendered
once and left in HBM as RGBA and as index bytes.  Each timing is a host clock
around the whole encode call (workspace and output allocation, kernels, the
copy of the compressed bytes, host framing; the call returns the finished
PNGs, so it ends synchronised).  Each mode is warmed once; the modes are then
timed alternately, `--runs` times, and the median is reported with min and
max, tiles/s and the mean PNG size.  render_bytes() -- the canvases and
gskyhip_scale, the extra step the indexed path needs in front -- is timed on
its own beside render().  Every indexed PNG is first decoded and compared with
the RGBA tile."""
import argparse
import datetime
import io
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np   # noqa: E402
import torch         # noqa: E402

from gsky_amd import GranuleSet, Palette, ScaleParams, TileBatch, synth   # noqa: E402
from gsky_amd.encode import encode_png, encode_png_indexed    # noqa: E402
from tools.bench_netcdf_out import lib_sha, timed             # noqa: E402

MODES = ("truecolour", "indexed")


def c2_batch(cfg, ids, dev):
    """The config's granules in HBM and tiles `ids` as one TileBatch."""
    gs = GranuleSet(dev)
    for g in cfg.granules:
        gs.add(torch.from_numpy(np.ascontiguousarray(g.data)), g.geot, g.srs, g.nodata,
               [torch.from_numpy(np.ascontiguousarray(o)) for o in g.overviews], g.timestamp, g.polygon, g.namespace)
    return TileBatch(gs, cfg.dst_srs, [cfg.tiles[i] for i in ids], [cfg.pairs[i] for i in ids], cfg.namespaces)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--tiles", type=int, default=256)
    ap.add_argument("--threads", type=int, default=0, help="host framing threads (0: the cores this process may use, 16 at most)")
    ap.add_argument("--scale", type=float, default=1.0, help="synth.config_c2 scale (1: the benchmark's batch)")
    ap.add_argument("--tiles-per-side", type=int, default=64)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_png: needs a HIP device")
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    threads = args.threads or max(1, min(16, len(os.sched_getaffinity(0))))
    cfg = synth.config_c2(scale=args.scale, tiles_per_side=args.tiles_per_side)
    covered = [i for i in range(len(cfg.tiles)) if cfg.pairs[i]]
    sample = [covered[k] for k in range(0, len(covered), max(1, len(covered) // args.tiles))][: args.tiles]
    batch = c2_batch(cfg, sample, dev)
    sp, pal = ScaleParams(*cfg.scale), Palette(cfg.palette, True)
    sizes = batch.tile_sizes
    rgba = batch.render(sp, pal).clone()
    index = batch.render_bytes(sp).clone()
    torch.cuda.synchronize()
    if batch.status() != 0:
        raise SystemExit("bench_png: render status %d" % batch.status())
    enc = {"truecolour": lambda: encode_png(rgba, sizes, n_threads=threads),
           "indexed": lambda: encode_png_indexed(index, pal, sizes, n_threads=threads)}
    pngs = {m: enc[m]() for m in MODES}   # warm-up, sizes and the check
    from PIL import Image
    host = rgba.cpu().numpy()
    for t, (w, h) in enumerate(sizes):
        im = np.asarray(Image.open(io.BytesIO(pngs["indexed"][t])).convert("RGBA"))
        if not np.array_equal(im, host[t, :h, :w]):
            raise SystemExit("bench_png: indexed tile %d does not decode to the rendered RGBA" % t)
    ms = {m: [] for m in MODES}
    for _ in range(args.runs):
        for m in MODES:
            ms[m].append(timed(enc[m]))
    prep = {"render_rgba": [], "render_bytes": []}
    for _ in range(args.runs):
        prep["render_rgba"].append(timed(lambda: batch.render(sp, pal)))
        prep["render_bytes"].append(timed(lambda: batch.render_bytes(sp)))
    n = len(sample)
    res = {"tool": "bench_png", "runs": args.runs, "tiles": n, "host_threads": threads, "lib_sha16": lib_sha(),
           "date": datetime.date.today().isoformat(), "device": torch.cuda.get_device_name(0),
           "tile_px": [batch.max_w, batch.max_h],
           "transparent_tiles": int(sum(bool((host[t, :h, :w, 3] == 0).any()) for t, (w, h) in enumerate(sizes)))}
    for m in MODES:
        med = statistics.median(ms[m])
        res[m] = {"encode_ms_median": med, "encode_ms_min": min(ms[m]), "encode_ms_max": max(ms[m]),
                  "tiles_per_s": n / (med / 1e3), "png_bytes_mean": float(np.mean([len(b) for b in pngs[m]])),
                  "png_bytes_total": int(sum(len(b) for b in pngs[m]))}
    res["indexed"]["time_ratio_to_truecolour"] = res["indexed"]["encode_ms_median"] / res["truecolour"]["encode_ms_median"]
    res["indexed"]["size_ratio_to_truecolour"] = res["indexed"]["png_bytes_total"] / res["truecolour"]["png_bytes_total"]
    for k, v in prep.items():
        res[k + "_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
