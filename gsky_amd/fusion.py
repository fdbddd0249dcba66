"""Layer fusion (input_layers) over the MI355X kernels.

The reference's TilePipeline.processDeps (processor/tile_pipeline.go:196-324)
renders every dependent layer of a layer with `input_layers`, scales each with
its own ScaleParams, and lets RasterMerger fold the results: layer 0 wins,
each later layer only fills what is still nodata.  Here each dependent layer
is a TileBatch rendered into its own typed canvases, and one kernel
(gskyhip_fuse_layers / gskyhip_fuse_render, csrc/fuse.hip) does the per-layer
scale, the nodata normalisation, the fold and -- for render_fused -- the outer
scale and the RGBA rule in a single pass.  The rule is written out in
include/gskyhip.h; nothing here computes pixels on the CPU.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import check, lib
from .raster import TORCH_OF, TYPE_CODES, TYPE_NAMES, Palette, ScaleParams, gradient_rgba_palette

_NBYTES = {"Byte": 1, "SignedByte": 1, "Int16": 2, "UInt16": 2, "Float32": 4}
_VT_NAME = {1: "Byte", 2: "SignedByte", 4: "Int16", 8: "UInt16", 16: "Float32"}


@dataclass
class LayerCanvases:
    """One rendered input layer: `canvases` is a uint8 HBM tensor (n_tiles,
    n_ns, max_h * max_w * 4) in the canvas layout of TileBatch.render() --
    rows max_w elements of `type_name` apart -- with one nodata, the layer's
    own ScaleParams and an optional per-tile present flag (uint8 HBM tensor;
    None: present everywhere)."""
    canvases: torch.Tensor
    type_name: str
    nodata: float
    params: ScaleParams
    present: Optional[torch.Tensor] = None


@dataclass
class FusionLayer:
    """One entry of `input_layers`: the layer's tiles as a TileBatch, its own
    ScaleParams and resampling.  present: per tile, False where the reference
    has no raster for the layer (EmptyTile, or the request outside the layer's
    effective dates); None: tiles without a granule are absent."""
    batch: "object"
    params: ScaleParams
    resample: int = 0                  # _lib.RESAMPLE_*, 0..6, as TileBatch.render()
    present: Optional[Sequence[bool]] = None

    def render(self) -> LayerCanvases:
        """The layer's typed canvases (TileBatch.render(rgba=False))."""
        b = self.batch
        tname = _VT_NAME.get(b.value_types)
        if tname is None:
            raise ValueError("a fusion layer needs granules of one value type")
        nds = {float(g.nodata) if g.nodata is not None else -1e10 for g in b.granules.items
               if g.namespace in b.namespaces}
        if len(nds) > 1 and not all(n != n for n in nds):
            raise ValueError("a fusion layer needs granules of one nodata")
        nodata = next(iter(nds)) if nds else 0.0
        pres = self.present
        if pres is None:
            pres = [t.pair_end > t.pair_begin for t in b._tarr[: b.n_tiles]]
        if len(pres) != b.n_tiles:
            raise ValueError("one present flag per tile")
        pt = None if all(pres) else torch.tensor([1 if p else 0 for p in pres], dtype=torch.uint8, device=b.device)
        cv = b.render(self.params, None, self.resample, rgba=False)
        return LayerCanvases(cv, tname, nodata, self.params, pt)


def tile_table(sizes: Sequence[Tuple[int, int]], device) -> torch.Tensor:
    """A device gskyhip_tile array carrying only (width, height) per tile, for
    fusing canvases that did not come from a TileBatch."""
    arr = (_lib.Tile * max(1, len(sizes)))()
    for i, (w, h) in enumerate(sizes):
        arr[i].width, arr[i].height = int(w), int(h)
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device)


def post_type(layers: Sequence[LayerCanvases], fusion_unscale: int = 0) -> str:
    """The fused canvas type: Byte for scaled layers, else the layers' type."""
    names = set()
    for ly in layers:
        p = ly.params
        scaled = fusion_unscale == 0 and not (p.offset == 0 and p.scale == 0 and p.clip == 0)
        names.add("Byte" if scaled else ly.type_name)
    if len(names) != 1:
        raise _lib.GskyError(-2, "fuse: layers of mixed post-stage types")
    return names.pop()


def _layer_array(layers: Sequence[LayerCanvases]):
    if not 1 <= len(layers) <= _lib.FUSE_MAX_LAYERS:
        raise ValueError("fusion takes 1..%d layers" % _lib.FUSE_MAX_LAYERS)
    shape = layers[0].canvases.shape
    arr = (_lib.FuseLayer * len(layers))()
    for i, ly in enumerate(layers):
        cv = ly.canvases
        if not cv.is_cuda or not cv.is_contiguous() or cv.dtype != torch.uint8 or cv.dim() != 3:
            raise ValueError("layer canvases: a contiguous uint8 HBM tensor (n_tiles, n_ns, bytes)")
        if cv.shape != shape:
            raise ValueError("layers must share tile count, namespaces and slot")
        if ly.type_name not in TYPE_CODES:
            raise ValueError("Raster type not implemented")
        if ly.present is not None and (ly.present.dtype != torch.uint8 or ly.present.numel() != shape[0]
                                       or not ly.present.is_cuda):
            raise ValueError("present: a uint8 HBM tensor, one flag per tile")
        arr[i].canvases = cv.data_ptr()
        arr[i].dtype = TYPE_CODES[ly.type_name]
        arr[i].nodata = float(ly.nodata)
        arr[i].sp = ly.params.c()
        arr[i].present = ly.present.data_ptr() if ly.present is not None else None
    return arr


def _check_slot(layers, n_tiles, max_w, max_h):
    n, n_ns, nbytes = layers[0].canvases.shape
    if n != n_tiles or nbytes != max_w * max_h * 4 or n_ns not in (1, 3):
        raise ValueError("layer canvases do not match (n_tiles, 1 or 3, max_h * max_w * 4)")
    return n_ns


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def fuse_canvases(layers: Sequence[LayerCanvases], tiles: torch.Tensor, n_tiles: int, max_w: int, max_h: int,
                  fusion_unscale: int = 0, out: Optional[torch.Tensor] = None):
    """gskyhip_fuse_layers: (fused canvases in the layout of the inputs, type
    name, per-tile nodata as a float64 HBM tensor).  tiles: a device
    gskyhip_tile array (TileBatch._tiles or tile_table())."""
    arr = _layer_array(layers)
    n_ns = _check_slot(layers, n_tiles, max_w, max_h)
    dev = layers[0].canvases.device
    if out is None:
        out = torch.empty_like(layers[0].canvases)
    nd = torch.empty(max(1, n_tiles), dtype=torch.float64, device=dev)
    dt = C.c_int32(0)
    check(lib().gskyhip_fuse_layers(arr, len(layers), n_ns, C.c_void_p(tiles.data_ptr()), n_tiles, max_w, max_h,
                                    int(fusion_unscale), C.c_void_p(out.data_ptr()), C.c_void_p(nd.data_ptr()),
                                    C.byref(dt), _stream()), "fuse_layers")
    return out, TYPE_NAMES[dt.value], nd[:n_tiles]


def render_fused_canvases(layers: Sequence[LayerCanvases], tiles: torch.Tensor, n_tiles: int, max_w: int,
                          max_h: int, outer_params: ScaleParams, palette: Optional[Palette] = None,
                          canvas: bool = False, fusion_unscale: int = 0, out: Optional[torch.Tensor] = None,
                          ramp: Optional[torch.Tensor] = None):
    """gskyhip_fuse_render: RGBA (n_tiles, max_h, max_w, 4); with canvas=True
    also (fused canvases, type name, per-tile nodata).  ramp: the palette's
    256 x RGBA already in HBM (a caller replaying the call keeps it alive)."""
    arr = _layer_array(layers)
    n_ns = _check_slot(layers, n_tiles, max_w, max_h)
    dev = layers[0].canvases.device
    if ramp is None and palette is not None and n_ns == 1:
        ramp = torch.from_numpy(gradient_rgba_palette(palette)).to(dev)
    if out is None:
        out = torch.empty((n_tiles, max_h, max_w, 4), dtype=torch.uint8, device=dev)
    cv = torch.empty_like(layers[0].canvases) if canvas else None
    nd = torch.empty(max(1, n_tiles), dtype=torch.float64, device=dev) if canvas else None
    sp = outer_params.c()
    check(lib().gskyhip_fuse_render(arr, len(layers), n_ns, C.c_void_p(tiles.data_ptr()), n_tiles, max_w, max_h,
                                    int(fusion_unscale), C.byref(sp),
                                    C.c_void_p(ramp.data_ptr()) if ramp is not None else None,
                                    C.c_void_p(out.data_ptr()),
                                    C.c_void_p(cv.data_ptr()) if cv is not None else None,
                                    C.c_void_p(nd.data_ptr()) if nd is not None else None, _stream()),
          "fuse_render")
    if canvas:
        return out, (cv, post_type(layers, fusion_unscale), nd[:n_tiles])
    return out


def canvas_views(canvases: torch.Tensor, type_name: str, max_w: int, max_h: int) -> List[torch.Tensor]:
    """Per namespace slot, the canvases as a typed (n_tiles, max_h, max_w) view."""
    n = max_w * max_h * _NBYTES[type_name]
    return [canvases[:, j, :n].view(TORCH_OF[type_name]).reshape(canvases.shape[0], max_h, max_w)
            for j in range(canvases.shape[1])]


def _rendered(layers: Sequence[FusionLayer]):
    if not layers:
        raise ValueError("fusion needs at least one layer")
    b0 = layers[0].batch
    for ly in layers[1:]:
        b = ly.batch
        if (b.n_tiles, b.max_w, b.max_h, b.tile_sizes, len(b.namespaces)) != \
                (b0.n_tiles, b0.max_w, b0.max_h, b0.tile_sizes, len(b0.namespaces)):
            raise ValueError("fusion layers must share tile count, tile sizes, slot and namespace count")
    return [ly.render() for ly in layers], b0


def fuse(layers: Sequence[FusionLayer], fusion_unscale: int = 0):
    """processDeps + RasterMerger for a batch of tiles: every layer renders
    into its own canvases, one kernel fuses them.  Returns (canvases, type
    name, nodata per tile); canvases in the layout of TileBatch.render()."""
    rendered, b0 = _rendered(layers)
    return fuse_canvases(rendered, b0._tiles, b0.n_tiles, b0.max_w, b0.max_h, fusion_unscale)


def render_fused(layers: Sequence[FusionLayer], outer_params: ScaleParams, palette: Optional[Palette] = None,
                 canvas: bool = False, fusion_unscale: int = 0):
    """The GetMap of a layer with input_layers: fuse(), the outer utils.Scale
    and the EncodePNG pixel rule in one kernel.  RGBA (n_tiles, H, W, 4); with
    canvas=True also (canvases, type name, nodata per tile).  An outer
    auto-scale raises GskyError(-1): use fuse() and raster.scale()."""
    rendered, b0 = _rendered(layers)
    return render_fused_canvases(rendered, b0._tiles, b0.n_tiles, b0.max_w, b0.max_h, outer_params, palette,
                                 canvas, fusion_unscale)


def fuse_weighted(layer_sets: Sequence[Sequence[FusionLayer]], fusion_unscale: int = 0) -> Dict[str, tuple]:
    """The `weighted_time` axis: one fuse() per time slice iw, its namespace
    slot j named fuse<j>_<iw>.  Returns {name: (typed canvases (n_tiles, H, W),
    nodata per tile)}; tile t's (name, canvases[t], nodata[t]) is a variable
    of raster.band_math."""
    out: Dict[str, tuple] = {}
    for iw, layers in enumerate(layer_sets):
        cv, tname, nd = fuse(layers, fusion_unscale)
        b0 = layers[0].batch
        for j, v in enumerate(canvas_views(cv, tname, b0.max_w, b0.max_h)):
            out["fuse%d_%d" % (j, iw)] = (v, nd)
    return out
