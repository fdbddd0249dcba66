#!/usr/bin/env python3
"""C3 (WCS 16384^2 float32 coverage, N=1) render time at resample = 0, 1, 2
and 3 (render_nn_kernel, render_bil_kernel, render_cub_kernel,
render_avg_kernel) of the same build, in one process, and a second leg over
the same granules at 3.5 source pixels per output pixel (a 4681^2 coverage:
the average footprint is about 4 x 4 taps), where the point samplers alias.
Each figure is phase 2 (the render kernels alone, after a phase-1 plan with
the same arguments) between HIP events on the launch stream, warmed up, the
resamplings interleaved rep by rep so clock drift hits all alike; the median
and the minimum of the repeated windows.  Prints one JSON line per leg, with
the average kernel's fraction of the HBM roofline over the leg's algorithmic
bytes (the output written once and the 64 source granules read once).
--small: 1/8 scale coverages (a functional check of the tool, not a
measurement).  GSKYHIP_LIB=ab selects the A/B build."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gsky_amd import GranuleSet, ScaleParams, TileBatch, coverage, synth  # noqa: E402

HBM_BPS = 8.0e12         # MI355X peak HBM bandwidth
NAMES = {0: "nearest", 1: "bilinear", 2: "cubic", 3: "average"}


def leg(gs, cfg, out_px, reps, warmup, dev):
    """Phase-2 times (ms) per resampling of one out_px^2 coverage of cfg's bbox."""
    chunks = coverage.chunk_requests(cfg.bbox, out_px, out_px)
    pairs = [cfg.index_chunk(c.bbox) for c in chunks]
    tiles = [(c.bbox, c.width, c.height) for c in chunks]
    # one batch (and planning workspace) per resampling: phase 2 replays its own plan
    tbs = {r: TileBatch(gs, cfg.dst_srs, tiles, pairs, cfg.namespaces) for r in NAMES}
    offs = torch.tensor(coverage.band_offsets(chunks, 0, out_px), dtype=torch.int64, device=dev)
    bands = {r: torch.empty((out_px, out_px), dtype=torch.float32, device=dev) for r in NAMES}
    sp = ScaleParams(*cfg.scale)
    for r in NAMES:
        tbs[r].render_coverage(sp, bands[r], offs, resample=r, phase=1)
        assert tbs[r].status() == 0
    s = torch.cuda.current_stream()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ts = {r: [] for r in NAMES}
    for k in range(warmup + reps):
        for r in NAMES:
            ev[0].record(s)
            tbs[r].render_coverage(sp, bands[r], offs, resample=r, phase=2)
            ev[1].record(s)
            torch.cuda.synchronize()
            if k >= warmup:
                ts[r].append(ev[0].elapsed_time(ev[1]))
    rec = {}
    for r, name in NAMES.items():
        rec[name + "_ms_median"] = round(float(np.median(ts[r])), 4)
        rec[name + "_ms_min"] = round(float(np.min(ts[r])), 4)
    rec["nodata_mask_identical_to_bilinear"] = bool(torch.equal(bands[1] == -9999.0, bands[3] == -9999.0))
    valid = (bands[1] != -9999.0) & (bands[3] != -9999.0)
    rec["max_abs_diff_to_bilinear"] = float((bands[1][valid].double() - bands[3][valid].double()).abs().max().item())
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg = synth.config_c3(scale=0.125, out_px=2048) if args.small else synth.config_c3()
    gs = GranuleSet(dev)
    for g in cfg.granules:
        gs.add(torch.from_numpy(np.ascontiguousarray(g.data)), g.geot, g.srs, g.nodata, [], g.timestamp,
               g.polygon, g.namespace)
    src_bytes = sum(g.data.nbytes for g in cfg.granules)
    for name, out_px in (("c3", cfg.out_w), ("c3_3.5to1", int(round(cfg.out_w / 3.5)))):
        rec = {"label": args.label, "config": name + ("_small" if args.small else ""),
               "lib": os.environ.get("GSKYHIP_LIB", "default"), "reps": args.reps, "out_px": out_px}
        rec.update(leg(gs, cfg, out_px, args.reps, args.warmup, dev))
        rec["average_over_bilinear"] = round(rec["average_ms_median"] / rec["bilinear_ms_median"], 3)
        if not args.small:
            nbytes = out_px * out_px * 4 + src_bytes
            rec["algorithmic_bytes"] = nbytes
            rec["average_hbm_roofline_frac"] = round(nbytes / (rec["average_ms_median"] * 1e-3) / HBM_BPS, 3)
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
