"""gskyhip_fuse_render against the staged composition of the entry points
that exist without it (gskyhip_scale per layer, then per tile
gskyhip_merge_rasters, gskyhip_scale, gskyhip_encode_rgba), on the same
inputs: 64 tiles x 512^2, 3 Int16 scaled layers, one namespace, a palette.
Checks that both give the same bytes, alternates 5 rounds of 50 fused and 2
staged calls (host clock, ending in a synchronise), times the fused call
between device events, and prints one JSON line.

    python tools/bench_fusion.py [out.json]
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import gsky_amd  # noqa: E402
from gsky_amd import _lib, fusion  # noqa: E402
from gsky_amd.raster import fnv32a  # noqa: E402

NT, W, H, L = 64, 512, 512, 3
dev = torch.device("cuda:0")
lib = _lib.lib()
rng = np.random.default_rng(3)
sps = [(0.0, 0.0, 10000.0), (100.0, 0.02, 9000.0), (0.0, 0.025, 10000.0)]
outer = gsky_amd.ScaleParams(0.0, 1.0, 254.0, 0)
pal = gsky_amd.Palette([[0, 0, 255, 255], [0, 255, 0, 255], [255, 0, 0, 255]], True)
ramp = torch.from_numpy(gsky_amd.gradient_rgba_palette(pal)).to(dev)

layers, flat = [], []
for l in range(L):
    v = rng.integers(0, 10000, (NT, H, W)).astype(np.int16)
    holes = rng.random((NT, H // 32, W // 32)) < 0.3        # 30 % nodata in 32 x 32 blocks
    v[np.repeat(np.repeat(holes, 32, 1), 32, 2)] = -999
    buf = np.zeros((NT, 1, W * H * 4), np.uint8)
    buf[:, 0, : W * H * 2] = v.reshape(NT, -1).view(np.uint8)
    layers.append(fusion.LayerCanvases(torch.from_numpy(buf).to(dev), "Int16", -999.0, gsky_amd.ScaleParams(*sps[l])))
    flat.append(torch.from_numpy(v).to(dev))                  # the staged path's contiguous copy
tiles = fusion.tile_table([(W, H)] * NT, dev)
out_f = torch.zeros((NT, H, W, 4), dtype=torch.uint8, device=dev)
stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)


def fused():
    fusion.render_fused_canvases(layers, tiles, NT, W, H, outer, out=out_f, ramp=ramp)


# staged: gskyhip_scale per layer (whole batch at once), then per tile
# gskyhip_merge_rasters, gskyhip_scale and gskyhip_encode_rgba
scaled = [torch.empty((NT, H, W), dtype=torch.uint8, device=dev) for _ in range(L)]
canv = torch.empty((NT, W * H * 4), dtype=torch.uint8, device=dev)
bytes_o = torch.empty((NT, H, W), dtype=torch.uint8, device=dev)
out_s = torch.zeros((NT, H, W, 4), dtype=torch.uint8, device=dev)
ph = fnv32a("dummy_polygon")
sp_c = [gsky_amd.ScaleParams(*s).c() for s in sps]
outer_c = outer.c()
created, dts, nds = (C.c_int32 * 1)(), (C.c_int32 * 1)(), (C.c_double * 1)()


def staged():
    for l in range(L):
        _lib.check(lib.gskyhip_scale(C.c_void_p(flat[l].data_ptr()), _lib.INT16, NT * H * W, -999.0,
                                     C.byref(sp_c[l]), C.c_void_p(scaled[l].data_ptr()), stream))
    fr = (_lib.FlexRasterC * L)()
    for t in range(NT):
        for l in range(L):
            fr[l].data = scaled[l][t].data_ptr()
            fr[l].data_w, fr[l].data_h, fr[l].width, fr[l].height = W, H, W, H
            fr[l].dtype, fr[l].ns, fr[l].nodata = _lib.BYTE, 0, 255.0
            fr[l].timestamp, fr[l].polygon_hash = 1.6e9 - l, ph
        cp = (C.c_void_p * 1)(canv[t].data_ptr())
        _lib.check(lib.gskyhip_merge_rasters(fr, L, None, cp, 1, created, dts, nds, stream))
        _lib.check(lib.gskyhip_scale(C.c_void_p(canv[t].data_ptr()), _lib.BYTE, H * W, 255.0, C.byref(outer_c),
                                     C.c_void_p(bytes_o[t].data_ptr()), stream))
        bp = (C.c_void_p * 1)(bytes_o[t].data_ptr())
        _lib.check(lib.gskyhip_encode_rgba(bp, 1, W, H, C.c_void_p(ramp.data_ptr()),
                                           C.c_void_p(out_s[t].data_ptr()), stream))


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


fused(); staged()
torch.cuda.synchronize()
same = bool(torch.equal(out_f, out_s))
opaque = float((out_f[..., 3] > 0).float().mean().item())
tf, ts = [], []
for _ in range(5):                       # alternate the two, several rounds
    tf.append(timed(fused, 50))
    ts.append(timed(staged, 2))
# the kernel alone, by device events
ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
ev[0].record()
for _ in range(200):
    fused()
ev[1].record()
torch.cuda.synchronize()
t_kernel = ev[0].elapsed_time(ev[1]) / 200 / 1e3
px = NT * W * H
bytes_algo = px * (L * 2 * 1 + 4)
res = dict(shape=dict(tiles=NT, w=W, h=H, layers=L, dtype="Int16", n_ns=1, palette=True),
           same_bytes=same, opaque_fraction=opaque,
           fused_s=tf, staged_s=ts, fused_min_s=min(tf), staged_min_s=min(ts), ratio=min(ts) / min(tf),
           fused_event_s=t_kernel, bytes_algo=bytes_algo, achieved_GBps=bytes_algo / t_kernel / 1e9,
           hbm_peak_GBps=8000.0, roofline_fraction=bytes_algo / t_kernel / 8e12)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(res, f, indent=1)
print(json.dumps(res))
assert same
