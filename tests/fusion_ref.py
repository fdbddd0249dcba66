"""The reference of layer fusion, as a composition of the existing oracle.

TilePipeline.processDeps (processor/tile_pipeline.go:196-324) for one tile:
per layer oracle.scale (scaled layers) or a numpy restatement of
getFlexRaster's normalisation (482-632, unscaled layers), then
oracle.merge_batch over the fuse<j> rasters -- namespace slot j, timestamp
t0 - l, polygon "dummy_polygon" -- then oracle.scale and oracle.encode_rgba
for the RGBA.  Also the seeded inputs the fusion tests share.
"""
from __future__ import annotations

import numpy as np

T0 = 1.6e9   # the request's start time (any value: only the order matters)

TYPES = {"Byte": np.uint8, "SignedByte": np.int8, "Int16": np.int16, "UInt16": np.uint16, "Float32": np.float32}


def go_conv(x: float, dt):
    """Go's T(x) of a float64 on amd64: CVTTSD2SL (NaN / out of range ->
    0x80000000), then truncation to the integer width; float32(x)."""
    dt = np.dtype(dt)
    if dt == np.float32:
        with np.errstate(all="ignore"):
            return np.float32(x)
    i = int(np.trunc(x)) if (x == x and -2147483649.0 < x < 2147483648.0) else -(1 << 31)
    return np.array([i & ((1 << (8 * dt.itemsize)) - 1)], np.uint64).astype("u%d" % dt.itemsize).view(dt)[0]


def is_scaled(sp, fusion_unscale=0) -> bool:
    return fusion_unscale == 0 and not (sp[0] == 0 and sp[1] == 0 and sp[2] == 0)


def stage(O, layers, fusion_unscale=0):
    """Per present layer, in order: (l, [array per namespace], nodata') after
    the per-layer stage.  layers: dicts with data (list per namespace of 2-D
    arrays of one tile), nodata, sp (offset, scale, clip) and present."""
    out = []
    l0 = layers[0]
    norm_ref = l0["present"] and not is_scaled(l0["sp"], fusion_unscale)
    for l, ly in enumerate(layers):
        if not ly["present"]:
            continue
        if is_scaled(ly["sp"], fusion_unscale):
            out.append((l, [O.scale(a, ly["nodata"], ly["sp"][0], ly["sp"][1], ly["sp"][2], 0) for a in ly["data"]],
                        255.0))
            continue
        data = [np.array(a, copy=True) for a in ly["data"]]
        nodata = ly["nodata"]
        dt = data[0].dtype
        if norm_ref and l > 0 and dt == l0["data"][0].dtype:
            n0, nl = go_conv(l0["nodata"], dt), go_conv(ly["nodata"], dt)
            if n0 != nl:   # a NaN: always different
                for a in data:
                    a[a == nl] = n0   # a NaN: never equal
                nodata = l0["nodata"]
        out.append((l, data, nodata))
    return out


def post_types(layers, fusion_unscale=0):
    return {np.dtype(np.uint8) if is_scaled(ly["sp"], fusion_unscale) else ly["data"][0].dtype for ly in layers}


def fuse(O, layers, fusion_unscale=0):
    """([fused canvas per namespace], nodata C) of one tile."""
    staged = stage(O, layers, fusion_unscale)
    n_ns = len(layers[0]["data"])
    h, w = layers[0]["data"][0].shape
    if not staged:   # no present layer: layer 0's post-stage nodata everywhere
        l0 = layers[0]
        sc = is_scaled(l0["sp"], fusion_unscale)
        dt = np.uint8 if sc else l0["data"][0].dtype
        c = 255.0 if sc else l0["nodata"]
        return [np.full((h, w), go_conv(c, dt), dt) for _ in range(n_ns)], c
    ph = O.fnv32a("dummy_polygon")
    rasters = []
    for l, data, nodata in staged:
        for j, a in enumerate(data):
            rasters.append(dict(data=a, off_x=0, off_y=0, nodata=nodata, timestamp=T0 - l, polygon_hash=ph, ns=j))
    merged = O.merge_batch(rasters, n_ns, w, h)
    return [m[0] for m in merged], merged[0][1]


def closed_form(O, layers, fusion_unscale=0):
    """"The first layer whose post-stage value is not its nodata", else the
    first present layer's nodata: what the fold gives when every post-stage
    nodata converts to the same value."""
    staged = stage(O, layers, fusion_unscale)
    _, d0, c = staged[0]
    out = []
    for j in range(len(d0)):
        dt = d0[j].dtype
        cv = np.full(d0[j].shape, go_conv(c, dt), dt)
        done = np.zeros(d0[j].shape, bool)
        for _, data, nodata in staged:
            valid = data[j] != go_conv(nodata, dt)
            cv = np.where(valid & ~done, data[j], cv)
            done |= valid
        out.append(cv)
    return out, c


def render(O, layers, outer, ramp=None, fusion_unscale=0):
    """(RGBA (h, w, 4), [fused canvas per namespace], nodata C) of one tile;
    outer = (offset, scale, clip, colour_scale)."""
    canv, c = fuse(O, layers, fusion_unscale)
    h, w = canv[0].shape
    bands = [O.scale(a, c, outer[0], outer[1], outer[2], int(outer[3])) for a in canv]
    return O.encode_rgba(bands, w, h, ramp if len(bands) == 1 else None), canv, c


def contributions(O, layers, fusion_unscale=0):
    """Per namespace: (pixels each present layer contributed, pixels left
    nodata), by the closed form's rule."""
    staged = stage(O, layers, fusion_unscale)
    res = []
    for j in range(len(staged[0][1])):
        done = np.zeros(staged[0][1][j].shape, bool)
        counts = []
        for _, data, nodata in staged:
            valid = data[j] != go_conv(nodata, data[j].dtype)
            counts.append(int((valid & ~done).sum()))
            done |= valid
        res.append((counts, int((~done).sum())))
    return res


# ---------------------------------------------------------------- shared inputs
SLOT = (64, 64)                       # (max_w, max_h)
SIZES = [(64, 64), (37, 19)]          # (w, h) per tile: full rows, and a width % 4 tail in a wider slot


def random_values(rng, dt, shape):
    dt = np.dtype(dt)
    if dt == np.float32:
        return (rng.standard_normal(shape) * 900.0).astype(np.float32)
    lo, hi = {"uint8": (0, 256), "int8": (-128, 128), "int16": (-3000, 12000), "uint16": (0, 60000)}[dt.name]
    return rng.integers(lo, hi, shape).astype(dt)


SEED = 1   # chosen on the CPU: with it every layer of up to 4 contributes to every tile and slot


def random_layer(seed, l, dt, nodata, n_ns, frac=0.3, block=(2, 3), sizes=SIZES, slot=SLOT):
    """Layer l: (n_tiles, n_ns, max_h, max_w) values of dt with about `frac`
    of every tile nodata, in blocks of block = (rows, columns), plus one block
    that is nodata in every layer; valid pixels never hold the nodata value.
    The holes depend on (seed, l) only, not on the type."""
    mw, mh = slot
    a = random_values(np.random.default_rng([seed, l]), dt, (len(sizes), n_ns, mh, mw))
    nd = go_conv(nodata, dt)
    if nd == nd:
        bump = a == nd
        a[bump] = np.float32(1.5) if np.dtype(dt) == np.float32 else (a[bump] ^ 1)
    by, bx = block
    holes = np.random.default_rng([seed, 1000 + l]).random(
        (len(sizes), n_ns, (mh + by - 1) // by, (mw + bx - 1) // bx)) < frac
    holes = np.repeat(np.repeat(holes, by, axis=2), bx, axis=3)[:, :, :mh, :mw]
    holes[:, :, 2:5, 3:8] = True
    a[holes] = nd
    return a


def tile_layers(arrays, nodatas, sps, t, sizes=SIZES, present=None):
    """The layer dicts of tile t from per-layer (n_tiles, n_ns, H, W) arrays."""
    w, h = sizes[t]
    return [dict(data=[np.ascontiguousarray(a[t, j, :h, :w]) for j in range(a.shape[1])], nodata=nodatas[l],
                 sp=sps[l], present=bool(present[l][t]) if present is not None and present[l] is not None else True)
            for l, a in enumerate(arrays)]
