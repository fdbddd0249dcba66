#!/usr/bin/env python3
"""C3 (WCS 16384^2 float32 coverage, N=1) render time at resample 1, 2, 5 and
6 (render_bil_kernel, render_cub_kernel, render_kern_kernel for the cubic
B-spline and for Lanczos) of the same build, in one process: phase 2 (the
render kernels alone, after a phase-1 plan with the same arguments) between
HIP events on the launch stream, warmed up, the four resamplings interleaved
launch by launch so clock drift hits all alike.  Prints one JSON line: per
code the median and minimum ms, the ratios to cubic, the share of pixels on
the bilinear hand-over (valid pixels whose value equals the bilinear
coverage's bit for bit: both take bil4_renorm() / bilinear_rule() there), and
how many pixels differ from the cubic coverage and by how much.  --small: a
1/8 scale coverage (a functional check of the tool, not a measurement).
GSKYHIP_LIB=ab selects the A/B build."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gsky_amd import GranuleSet, ScaleParams, TileBatch, coverage, synth  # noqa: E402

CODES = (1, 2, 5, 6)
NAMES = {1: "bilinear", 2: "cubic", 5: "spline", 6: "lanczos"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg = synth.config_c3(scale=0.125, out_px=2048) if args.small else synth.config_c3()
    chunks = coverage.chunk_requests(cfg.bbox, cfg.out_w, cfg.out_h)
    pairs = [cfg.index_chunk(c.bbox) for c in chunks]
    gs = GranuleSet(dev)
    for g in cfg.granules:
        gs.add(torch.from_numpy(np.ascontiguousarray(g.data)), g.geot, g.srs, g.nodata, [], g.timestamp,
               g.polygon, g.namespace)
    tiles = [(c.bbox, c.width, c.height) for c in chunks]
    # one batch (and planning workspace) per resampling: phase 2 replays its own plan
    tbs = {r: TileBatch(gs, cfg.dst_srs, tiles, pairs, cfg.namespaces) for r in CODES}
    offs = torch.tensor(coverage.band_offsets(chunks, 0, cfg.out_w), dtype=torch.int64, device=dev)
    bands = {r: torch.empty((cfg.out_h, cfg.out_w), dtype=torch.float32, device=dev) for r in CODES}
    sp = ScaleParams(*cfg.scale)
    for r in CODES:
        tbs[r].render_coverage(sp, bands[r], offs, resample=r, phase=1)
        assert tbs[r].status() == 0
    s = torch.cuda.current_stream()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ts = {r: [] for r in CODES}
    for k in range(args.warmup + args.reps):
        for r in CODES:
            ev[0].record(s)
            tbs[r].render_coverage(sp, bands[r], offs, resample=r, phase=2)
            ev[1].record(s)
            torch.cuda.synchronize()
            if k >= args.warmup:
                ts[r].append(ev[0].elapsed_time(ev[1]))
    rec = {"label": args.label, "config": "c3_small" if args.small else "c3",
           "lib": os.environ.get("GSKYHIP_LIB", "default"), "reps": args.reps}
    for r in CODES:
        rec[NAMES[r] + "_ms_median"] = round(float(np.median(ts[r])), 4)
        rec[NAMES[r] + "_ms_min"] = round(float(np.min(ts[r])), 4)
    nd = -9999.0
    for r in (5, 6):
        n = NAMES[r]
        rec[n + "_over_cubic"] = round(rec[n + "_ms_median"] / rec["cubic_ms_median"], 3)
        rec[n + "_over_bilinear"] = round(rec[n + "_ms_median"] / rec["bilinear_ms_median"], 3)
        rec[n + "_nodata_mask_identical"] = bool(torch.equal(bands[r] == nd, bands[2] == nd))
        valid = (bands[r] != nd) & (bands[2] != nd) & (bands[1] != nd)
        rec[n + "_hand_over_frac"] = round(float((bands[r][valid] == bands[1][valid]).double().mean().item()), 4)
        d = (bands[r][valid].double() - bands[2][valid].double()).abs()
        rec[n + "_differing_from_cubic_frac"] = round(float((d > 0).double().mean().item()), 4)
        rec[n + "_max_abs_diff_from_cubic"] = float(d.max().item())
        rec[n + "_mean_abs_diff_from_cubic"] = float(d.mean().item())
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
