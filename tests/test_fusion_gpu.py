"""Layer fusion on the MI355X: gskyhip_fuse_layers / gskyhip_fuse_render
(csrc/fuse.hip) against the reference composition of tests/fusion_ref.py, bit
for bit.  Two tiles in a 64 x 64 slot -- 64 x 64, and 37 x 19 for the
width % 4 tail and the row stride -- with the layer canvases uploaded directly;
the last test renders two synthetic layers through TileBatch first."""
import copy
from dataclasses import dataclass, field
from typing import Callable, List, Optional

import numpy as np
import pytest

from tests import fusion_ref as R

pytestmark = pytest.mark.gpu

NOSP = (0.0, 0.0, 0.0)
ND = {"Byte": 255.0, "SignedByte": -128.0, "Int16": -999.0, "UInt16": 65535.0, "Float32": -999.0}
MW, MH = R.SLOT
PALETTE = [[0, 0, 255, 255], [0, 255, 0, 255], [255, 255, 0, 255], [255, 0, 0, 255]]
NAN = float("nan")


@dataclass
class Case:
    types: List[str]
    nodatas: List[float]
    sps: List[tuple]
    n_ns: int = 1
    present: Optional[list] = None        # per layer: None or a flag per tile
    unscale: int = 0
    outer: Optional[tuple] = None         # (offset, scale, clip, colour_scale): also fuse_render
    palette: bool = False
    contrib: bool = True                  # every layer contributes, a pixel stays nodata
    edit: Optional[Callable] = None       # changes the layer arrays in place
    _arrays: list = field(default=None, repr=False)

    def arrays(self):
        if self._arrays is None:
            self._arrays = [R.random_layer(R.SEED, l, R.TYPES[t], nd, self.n_ns)
                            for l, (t, nd) in enumerate(zip(self.types, self.nodatas))]
            if self.edit:
                self.edit(self._arrays)
        return self._arrays

    def tile(self, t):
        return R.tile_layers(self.arrays(), self.nodatas, self.sps, t, present=self.present)


def typed(tname, L, n_ns):
    return Case([tname] * L, [ND[tname]] * L, [NOSP] * L, n_ns)


def _all_nodata_middle(arrays):
    arrays[1][...] = -999


def _layer0_valid(arrays):
    a = arrays[0]
    a[a == -999] = 17


def _inject_ff(arrays):
    arrays[0][:, :, 10, 8:12] = 8160      # 8160 / 32 = 255: a valid value that scales to 0xFF


CASES = {
    # scaled layers, each with its own parameters: all become Byte / 0xFF.  The
    # Byte layer's clip 1000 wraps to uint8(1000) = 232 (raster_scaler.go's uint8(clip)).
    "scaled": Case(["Int16", "UInt16", "Float32", "Byte"], [-999.0, 0.0, -999.0, 7.0],
                   [(0.0, 0.03125, 8160.0), (100.0, 0.0, 60000.0), (2500.0, 0.05, 5000.0), (3.0, 0.9, 1000.0)],
                   outer=(0.0, 1.0, 254.0, 0), palette=True, edit=_inject_ff),
    "normalise": Case(["Int16"] * 3, [-999.0, -32768.0, -999.0], [NOSP] * 3, outer=(3000.0, 0.0, 15000.0, 0)),
    "nan_layer0": Case(["Float32"] * 3, [NAN, -999.0, NAN], [NOSP] * 3, outer=(2500.0, 0.05, 5000.0, 0),
                       contrib=False),
    "nan_layer1": Case(["Float32"] * 3, [-999.0, NAN, -999.0], [NOSP] * 3, outer=(2500.0, 0.05, 5000.0, 0),
                       contrib=False),
    "all_nodata_layer": Case(["Int16"] * 3, [-999.0] * 3, [NOSP] * 3, contrib=False, edit=_all_nodata_middle),
    "layer0_valid": Case(["Int16"] * 3, [-999.0] * 3, [NOSP] * 3, outer=(0.0, 0.0, 12000.0, 0), contrib=False,
                         edit=_layer0_valid),
    "absent_middle": Case(["Int16"] * 3, [-999.0, -32768.0, -999.0], [NOSP] * 3, present=[None, [0, 1], None],
                          outer=(0.0, 0.0, 12000.0, 0), contrib=False),
    "absent_layer0": Case(["Int16"] * 3, [-999.0, -32768.0, -999.0], [NOSP] * 3, present=[[0, 0], None, [1, 0]],
                          outer=(0.0, 0.0, 12000.0, 0), contrib=False),
    "absent_all": Case(["Int16"] * 2, [-999.0, -5.0], [NOSP] * 2, present=[[0, 0], [0, 1]],
                       outer=(0.0, 0.0, 12000.0, 0), palette=True, contrib=False),
    "absent_all_scaled": Case(["Int16"] * 2, [-999.0, -5.0], [(0.0, 0.02, 12000.0)] * 2, present=[[0, 0], [0, 0]],
                              outer=(0.0, 1.0, 254.0, 0), contrib=False),
    "render_grey": Case(["UInt16"] * 2, [0.0, 0.0], [NOSP] * 2, outer=(0.0, 0.0, 60000.0, 0)),
    "render_ramp": Case(["UInt16"] * 2, [0.0, 0.0], [NOSP] * 2, outer=(0.0, 0.0, 60000.0, 0), palette=True),
    "render_rgb": Case(["Byte"] * 3, [0.0, 255.0, 0.0], [NOSP] * 3, n_ns=3, outer=(0.0, 1.0, 254.0, 0)),
    "render_rgb_scaled": Case(["Int16", "Float32"], [-999.0, -999.0], [(0.0, 0.02, 12000.0), (2500.0, 0.05, 5000.0)],
                              n_ns=3, outer=(0.0, 1.0, 254.0, 0)),
    "unscale": Case(["Int16"] * 2, [-999.0, -999.0], [(0.0, 0.02, 12000.0)] * 2, unscale=1,
                    outer=(0.0, 0.02, 12000.0, 0)),
    # log10 of the fused Float32 canvas: negative values become nodata
    "colour_scale": Case(["Float32"] * 2, [-999.0, -999.0], [NOSP] * 2, outer=(1.0, 0.0, 4.0, 1), palette=True),
}
for _t in R.TYPES:
    for _L in (1, 2, 4):
        for _n in (1, 3):
            CASES["typed_%s_L%d_ns%d" % (_t, _L, _n)] = typed(_t, _L, _n)


# ---------------------------------------------------------------- device side
def _upload(a, dev):
    import torch
    n, n_ns = a.shape[:2]
    buf = np.zeros((n, n_ns, MW * MH * 4), np.uint8)
    buf[:, :, : MW * MH * a.dtype.itemsize] = np.ascontiguousarray(a).reshape(n, n_ns, -1).view(np.uint8)
    return torch.from_numpy(buf).to(dev)


def _device_layers(case, dev):
    import torch

    import gsky_amd
    from gsky_amd import fusion
    out = []
    for l, a in enumerate(case.arrays()):
        p = case.present[l] if case.present is not None else None
        pt = torch.tensor(p, dtype=torch.uint8, device=dev) if p is not None else None
        out.append(fusion.LayerCanvases(_upload(a, dev), case.types[l], case.nodatas[l],
                                        gsky_amd.ScaleParams(*case.sps[l]), pt))
    return out, fusion.tile_table(R.SIZES, dev)


def _same(a, b):
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype == np.float32:
        return bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())
    return np.array_equal(a, b)


def _check_canvases(cv, tname, nd, refs, n_ns, what):
    """cv: the (2, n_ns, bytes) result written over a 0x5A fill."""
    dt = R.TYPES[tname]
    raw = cv.cpu().numpy()
    nd = nd.cpu().numpy()
    n = MW * MH * np.dtype(dt).itemsize
    assert (raw[:, :, n:] == 0x5A).all(), what               # nothing past the typed slot
    full = raw[:, :, :n].copy().view(dt).reshape(len(R.SIZES), n_ns, MH, MW)
    for t, (w, h) in enumerate(R.SIZES):
        canv, c = refs[t]
        assert nd[t] == c or (nd[t] != nd[t] and c != c), (what, t, nd[t], c)
        for j in range(n_ns):
            assert _same(full[t, j, :h, :w], canv[j]), (what, t, j)
            outside = full[t, j].copy().view(np.uint8).reshape(MH, -1)
            outside[:h, : w * np.dtype(dt).itemsize] = 0x5A
            assert (outside == 0x5A).all(), (what, t, j)     # pixels outside the tile are left alone


def _check_rgba(rgba, refs, what):
    got = rgba.cpu().numpy()
    for t, (w, h) in enumerate(R.SIZES):
        assert np.array_equal(got[t, :h, :w], refs[t]), (what, t)
        outside = got[t].copy()
        outside[:h, :w] = 0x5A
        assert (outside == 0x5A).all(), (what, t)


@pytest.mark.parametrize("name", sorted(CASES))
def test_fusion(gpu, oracle, name):
    import torch

    import gsky_amd
    from gsky_amd import fusion
    case = CASES[name]
    n_tiles = len(R.SIZES)
    refs = [R.fuse(oracle, case.tile(t), case.unscale) for t in range(n_tiles)]
    if case.contrib:
        for t in range(n_tiles):
            for counts, left in R.contributions(oracle, case.tile(t), case.unscale):
                assert all(n > 0 for n in counts) and left > 0, (name, t, counts, left)
    if name == "scaled":   # a valid Int16 value whose scaled byte is the nodata 0xFF
        _, data, _ = R.stage(oracle, case.tile(1))[0]
        assert data[0][10, 8] == 0xFF and case.tile(1)[0]["data"][0][10, 8] == 8160
    if name == "layer0_valid":
        assert all(R.contributions(oracle, case.tile(t))[0][0][1:] == [0, 0] for t in range(n_tiles))
    layers, tiles = _device_layers(case, gpu)
    out = torch.full_like(layers[0].canvases, 0x5A)
    cv, tname, nd = fusion.fuse_canvases(layers, tiles, n_tiles, MW, MH, case.unscale, out=out)
    torch.cuda.synchronize()
    assert R.TYPES[tname] == refs[0][0][0].dtype
    _check_canvases(cv, tname, nd, refs, case.n_ns, name)
    for ly, a in zip(layers, case.arrays()):                  # the inputs are never written
        assert np.array_equal(ly.canvases.cpu().numpy(), _upload(a, "cpu").numpy())
    if case.outer is None:
        return
    pal = gsky_amd.Palette(PALETTE, True) if case.palette else None
    ramp = oracle.gradient_palette(PALETTE, True) if case.palette else None
    rrefs = [R.render(oracle, case.tile(t), case.outer, ramp, case.unscale)[0] for t in range(n_tiles)]
    assert any((r[..., 3] > 0).any() for r in rrefs) or name.startswith("absent_all")
    sp = gsky_amd.ScaleParams(*case.outer)
    rgba = fusion.render_fused_canvases(layers, tiles, n_tiles, MW, MH, sp, pal, fusion_unscale=case.unscale,
                                        out=torch.full((n_tiles, MH, MW, 4), 0x5A, dtype=torch.uint8, device=gpu))
    torch.cuda.synchronize()
    _check_rgba(rgba, rrefs, name)
    # with canvas_out: the same RGBA, and the canvases of gskyhip_fuse_layers
    rgba2, (cv2, tname2, nd2) = fusion.render_fused_canvases(
        layers, tiles, n_tiles, MW, MH, sp, pal, canvas=True, fusion_unscale=case.unscale,
        out=torch.full((n_tiles, MH, MW, 4), 0x5A, dtype=torch.uint8, device=gpu))
    torch.cuda.synchronize()
    _check_rgba(rgba2, rrefs, name)
    assert tname2 == tname
    n = MW * MH * np.dtype(R.TYPES[tname]).itemsize
    full = cv2.cpu().numpy()[:, :, :n].copy().view(R.TYPES[tname]).reshape(n_tiles, case.n_ns, MH, MW)
    for t, (w, h) in enumerate(R.SIZES):
        assert nd2[t].item() == refs[t][1] or refs[t][1] != refs[t][1]
        for j in range(case.n_ns):
            assert _same(full[t, j, :h, :w], refs[t][0][j]), (name, t, j)
    if name.startswith("absent_all"):                          # the empty tile: transparent
        assert not rgba.cpu().numpy()[0, : R.SIZES[0][1], : R.SIZES[0][0]].any()


@pytest.mark.parametrize("name", ["scaled", "render_rgb", "colour_scale"])
def test_fused_render_equals_staged_calls(gpu, name):
    """gskyhip_fuse_render against gskyhip_fuse_layers + gskyhip_scale +
    gskyhip_encode_rgba: the same bytes."""
    import torch

    import gsky_amd
    from gsky_amd import fusion
    case = CASES[name]
    n_tiles = len(R.SIZES)
    layers, tiles = _device_layers(case, gpu)
    pal = gsky_amd.Palette(PALETTE, True) if case.palette else None
    sp = gsky_amd.ScaleParams(*case.outer)
    rgba = fusion.render_fused_canvases(layers, tiles, n_tiles, MW, MH, sp, pal).cpu().numpy()
    cv, tname, nd = fusion.fuse_canvases(layers, tiles, n_tiles, MW, MH)
    nd = nd.cpu().numpy()
    views = fusion.canvas_views(cv, tname, MW, MH)
    for t, (w, h) in enumerate(R.SIZES):
        crops = [v[t, :h, :w].clone().contiguous() for v in views]
        bands = gsky_amd.scale(crops, [float(nd[t])] * len(crops), sp, [tname] * len(crops))
        exp = gsky_amd.encode_rgba(bands, pal).cpu().numpy()
        assert (exp[..., 3] > 0).any() and np.array_equal(rgba[t, :h, :w], exp), (name, t)


def test_fuse_render_graph_replay(gpu, oracle):
    """One linear stream, one kernel: the call is captured and replayed."""
    import torch

    import gsky_amd
    from gsky_amd import fusion
    case = CASES["scaled"]
    n_tiles = len(R.SIZES)
    layers, tiles = _device_layers(case, gpu)
    sp = gsky_amd.ScaleParams(*case.outer)
    ramp_h = oracle.gradient_palette(PALETTE, True)
    ramp = torch.from_numpy(ramp_h).to(gpu)
    out = torch.full((n_tiles, MH, MW, 4), 0x5A, dtype=torch.uint8, device=gpu)
    fusion.render_fused_canvases(layers, tiles, n_tiles, MW, MH, sp, out=out, ramp=ramp)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fusion.render_fused_canvases(layers, tiles, n_tiles, MW, MH, sp, out=out, ramp=ramp)
    torch.cuda.synchronize()
    out.fill_(0x5A)
    g.replay()
    torch.cuda.synchronize()
    rrefs = [R.render(oracle, case.tile(t), case.outer, ramp_h)[0] for t in range(n_tiles)]
    _check_rgba(out, rrefs, "graph")


def test_render_fused_end_to_end(gpu, oracle):
    """Two synthetic Int16 layers warped and merged by TileBatch, then fused:
    render_fused against oracle_render per layer + fusion_ref."""
    import torch

    import gsky_amd
    from gsky_amd import synth
    from tests.helpers import gpu_batch, oracle_render
    cfg_a = synth.config_c2(scale=0.02, tiles_per_side=2, tile_px=48, grid=2)
    for g in cfg_a.granules:
        g.data[8:30, 15:50] = -999                 # a hole for the second layer to fill
    cfg_b = copy.deepcopy(cfg_a)
    for g in cfg_b.granules:                       # other values, holes elsewhere
        g.data = np.ascontiguousarray(np.roll(g.data, 23, axis=1)[::-1])
    sps = [(0.0, 0.0, 10000.0), (500.0, 0.02, 9000.0)]
    outer = (0.0, 1.0, 254.0, 0)
    cvs = []
    for cfg in (cfg_a, cfg_b):
        _, cv, created = oracle_render(oracle, cfg, canvas=True)
        assert created[:, 0].all()
        cvs.append(cv)
    ramp = oracle.gradient_palette(synth.PALETTE_GSKY, True)
    batches = [gpu_batch(cfg, gpu) for cfg in (cfg_a, cfg_b)]
    layers = [gsky_amd.FusionLayer(b, gsky_amd.ScaleParams(*sp)) for b, sp in zip(batches, sps)]
    rgba, (cv, tname, nd) = gsky_amd.render_fused(layers, gsky_amd.ScaleParams(*outer),
                                                  gsky_amd.Palette(synth.PALETTE_GSKY, True), canvas=True)
    torch.cuda.synchronize()
    assert all(b.status() == 0 for b in batches) and tname == "Byte"
    got = rgba.cpu().numpy()
    filled_by_b = 0
    for t, (_, w, h) in enumerate(cfg_a.tiles):
        tl = [dict(data=[c[t, 0].view(np.int16)[: 48 * 48].reshape(48, 48)[:h, :w]], nodata=-999.0, sp=sp,
                   present=True)
              for c, sp in zip(cvs, sps)]
        exp, _, c = R.render(oracle, tl, outer, ramp)
        assert c == 255.0 and np.array_equal(got[t, :h, :w], exp), t
        filled_by_b += R.contributions(oracle, tl)[0][0][1]
    assert filled_by_b > 0 and (got[..., 3] > 0).any()
    # fuse() alone gives the same canvases as render_fused(canvas=True)
    cv2, tname2, _ = gsky_amd.fuse(layers)
    assert tname2 == "Byte" and torch.equal(cv2[:, :, : 48 * 48], cv[:, :, : 48 * 48])
