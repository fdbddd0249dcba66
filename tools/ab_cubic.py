#!/usr/bin/env python3
"""C3 (WCS 16384^2 float32 coverage, N=1) render time at resample=1
(render_bil_kernel) and resample=2 (render_cub_kernel) of the same build, in
one process: phase 2 (the render kernels alone, after a phase-1 plan with the
same arguments) between HIP events on the launch stream, warmed up, the two
resamplings interleaved rep by rep so clock drift hits both alike.  Prints
one JSON line: both medians and minima, their ratio and the cubic kernel's
fraction of the HBM roofline over C3's algorithmic bytes.  --small: a 1/8
scale coverage (a functional check of the tool, not a measurement).
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

C3_BYTES = 2.147e9       # algorithmic bytes of C3: 16384^2 x 4 B written + the 64 source granules read once
HBM_BPS = 8.0e12         # MI355X peak HBM bandwidth


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
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
    tbs = {r: TileBatch(gs, cfg.dst_srs, tiles, pairs, cfg.namespaces) for r in (1, 2)}
    offs = torch.tensor(coverage.band_offsets(chunks, 0, cfg.out_w), dtype=torch.int64, device=dev)
    bands = {r: torch.empty((cfg.out_h, cfg.out_w), dtype=torch.float32, device=dev) for r in (1, 2)}
    sp = ScaleParams(*cfg.scale)
    for r in (1, 2):
        tbs[r].render_coverage(sp, bands[r], offs, resample=r, phase=1)
        assert tbs[r].status() == 0
    s = torch.cuda.current_stream()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ts = {1: [], 2: []}
    for k in range(args.warmup + args.reps):
        for r in (1, 2):
            ev[0].record(s)
            tbs[r].render_coverage(sp, bands[r], offs, resample=r, phase=2)
            ev[1].record(s)
            torch.cuda.synchronize()
            if k >= args.warmup:
                ts[r].append(ev[0].elapsed_time(ev[1]))
    b1, b2 = bands[1], bands[2]
    valid = (b1 != -9999.0) & (b2 != -9999.0)
    rec = {"label": args.label, "config": "c3_small" if args.small else "c3",
           "lib": os.environ.get("GSKYHIP_LIB", "default"), "reps": args.reps,
           "bilinear_ms_median": round(float(np.median(ts[1])), 4), "bilinear_ms_min": round(float(np.min(ts[1])), 4),
           "cubic_ms_median": round(float(np.median(ts[2])), 4), "cubic_ms_min": round(float(np.min(ts[2])), 4)}
    rec["cubic_over_bilinear"] = round(rec["cubic_ms_median"] / rec["bilinear_ms_median"], 3)
    if not args.small:
        rec["cubic_hbm_roofline_frac"] = round(C3_BYTES / (rec["cubic_ms_median"] * 1e-3) / HBM_BPS, 3)
    rec["nodata_mask_identical"] = bool(torch.equal(b1 == -9999.0, b2 == -9999.0))
    rec["pixels_differing_frac"] = round(float((b1[valid] != b2[valid]).double().mean().item()), 4)
    rec["max_abs_diff"] = float((b1[valid].double() - b2[valid].double()).abs().max().item())
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
