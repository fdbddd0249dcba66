"""Layer fusion, the rule (CPU): a hand-derived known answer through the
reference composition (tests/fusion_ref.py), the reference against the closed
form "first layer whose post-stage value is not its nodata", and every
argument error of gskyhip_fuse_layers / gskyhip_fuse_render, which return
before any HIP call.  No kernel is launched here."""
import ctypes as C

import numpy as np
import pytest

from tests import fusion_ref as R

E_ARG, E_TYPE = -1, -2


def _layer(rows, nodata, sp=(0.0, 0.0, 0.0), dt=np.int16, present=True):
    return dict(data=[np.array(rows, dt)], nodata=nodata, sp=sp, present=present)


def test_known_answer(oracle):
    # layer 0 wins (5 over 7 and 1); layer 1 fills a hole (8); layer 2 fills
    # one (3) although its nodata is -32768: it is normalised to layer 0's
    # -999, so its -32768 pixel stays a hole and its 3 passes "canvas == nodata"
    layers = [_layer([[5, -999], [-999, -999]], -999.0),
              _layer([[7, 8], [-999, -999]], -999.0),
              _layer([[1, 2], [3, -32768]], -32768.0)]
    canv, c = R.fuse(oracle, layers)
    assert c == -999.0 and canv[0].dtype == np.int16
    assert canv[0].tolist() == [[5, 8], [3, -999]]
    # without the normalisation (layer 0 absent) layer 2 keeps -32768, which
    # the canvas never equals once layer 1 made it: its 3 is not written
    absent0 = [dict(layers[0], present=False), layers[1], layers[2]]
    canv, c = R.fuse(oracle, absent0)
    assert c == -999.0 and canv[0].tolist() == [[7, 8], [-999, -999]]
    # outer Scale with clip 127 (scale 254 / 127 = 2) and the grey rule
    rgba, _, _ = R.render(oracle, layers, (0.0, 0.0, 127.0, 0))
    grey = lambda v: [v, v, v, 255]
    assert rgba.tolist() == [[grey(10), grey(16)], [grey(6), [0, 0, 0, 0]]]
    # scaled layers: Byte, nodata 0xFF; a valid value scaling to 0xFF reads as a hole
    sp = (0.0, 1.0, 300.0)
    layers = [_layer([[255, -999], [-999, 20]], -999.0, sp), _layer([[1, 2], [3, 4]], -5.0, sp)]
    canv, c = R.fuse(oracle, layers)
    assert c == 255.0 and canv[0].dtype == np.uint8 and canv[0].tolist() == [[1, 2], [3, 20]]


@pytest.mark.parametrize("case", ["int16_normalised", "float32_scaled", "byte_3ns"])
def test_reference_is_first_valid_layer(oracle, case):
    """The strictly decreasing timestamps put every later layer in
    MergeMaskedRaster's fill branch: the composition equals the closed form."""
    if case == "int16_normalised":
        dt, n_ns, nodatas = np.int16, 1, [-999.0, -999.0, -32768.0, 7.0]
        sps = [(0.0, 0.0, 0.0)] * 4
    elif case == "float32_scaled":
        dt, n_ns, nodatas = np.float32, 1, [-999.0, 1e20, -1.0]
        sps = [(100.0, 0.0, 3000.0), (0.0, 0.05, 2500.0), (500.0, 0.1, 2000.0)]
    else:
        dt, n_ns, nodatas = np.uint8, 3, [0.0, 255.0]
        sps = [(0.0, 0.0, 0.0)] * 2
    arrays = [R.random_layer(R.SEED, l, dt, nd, n_ns) for l, nd in enumerate(nodatas)]
    for t in range(len(R.SIZES)):
        layers = R.tile_layers(arrays, nodatas, sps, t)
        got, c = R.fuse(oracle, layers)
        exp, c2 = R.closed_form(oracle, layers)
        assert c == c2
        for g, e in zip(got, exp):
            assert g.dtype == e.dtype and np.array_equal(g, e)
        for counts, left in R.contributions(oracle, layers):
            assert all(n > 0 for n in counts) and left > 0


# ---------------------------------------------------------------- argument errors
@pytest.fixture(scope="module")
def L():
    from gsky_amd import _lib
    return _lib.lib()


def _layers(specs):
    """specs: (dtype code, (offset, scale, clip), canvases pointer)."""
    from gsky_amd import _lib
    arr = (_lib.FuseLayer * len(specs))()
    for i, (dt, sp, ptr) in enumerate(specs):
        arr[i].canvases = ptr
        arr[i].dtype = dt
        arr[i].nodata = -999.0
        arr[i].sp = _lib.ScaleParams(sp[0], sp[1], sp[2], 0, 0)
    return arr


PTR = 0x1000   # never dereferenced: every case below fails its checks first
NOSP, SP = (0.0, 0.0, 0.0), (0.0, 0.0, 100.0)
INT16, FLOAT32, UINT32, FLOAT64 = 3, 6, 4, 7


def _call_layers(L, layers, n_layers, n_ns=1, tiles=PTR, canvas=PTR, nodata=PTR, dtype=True, max_w=64, max_h=64,
                 unscale=0):
    dt = C.c_int32(0)
    return L.gskyhip_fuse_layers(layers, n_layers, n_ns, tiles, 2, max_w, max_h, unscale, canvas, nodata,
                                 C.byref(dt) if dtype else None, None)


def _call_render(L, layers, n_layers, n_ns=1, tiles=PTR, outer=(0.0, 0.0, 100.0), rgba=PTR, max_w=64, max_h=64,
                 unscale=0):
    from gsky_amd import _lib
    sp = _lib.ScaleParams(outer[0], outer[1], outer[2], 0, 0) if outer is not None else None
    return L.gskyhip_fuse_render(layers, n_layers, n_ns, tiles, 2, max_w, max_h, unscale,
                                 C.byref(sp) if sp is not None else None, None, rgba, None, None, None)


@pytest.mark.parametrize("call", [_call_layers, _call_render], ids=["fuse_layers", "fuse_render"])
def test_argument_errors(L, call):
    ok = _layers([(INT16, NOSP, PTR), (INT16, NOSP, PTR)])
    assert call(L, None, 2) == E_ARG                          # layers NULL
    assert call(L, ok, 2, tiles=None) == E_ARG                # tiles NULL
    assert call(L, _layers([(INT16, NOSP, PTR), (INT16, NOSP, None)]), 2) == E_ARG   # a layer without canvases
    assert call(L, ok, 0) == E_ARG and call(L, ok, -1) == E_ARG
    nine = _layers([(INT16, NOSP, PTR)] * 9)
    assert call(L, nine, 9) == E_ARG                          # > GSKYHIP_FUSE_MAX_LAYERS
    for n_ns in (0, 2, 4):
        assert call(L, ok, 2, n_ns=n_ns) == E_ARG
    assert call(L, ok, 2, max_w=0) == E_ARG and call(L, ok, 2, max_h=0) == E_ARG
    for bad in (UINT32, FLOAT64, 0):
        assert call(L, _layers([(INT16, NOSP, PTR), (bad, NOSP, PTR)]), 2) == E_TYPE


def test_argument_errors_outputs(L):
    ok = _layers([(INT16, NOSP, PTR)])
    assert _call_layers(L, ok, 1, canvas=None) == E_ARG
    assert _call_layers(L, ok, 1, nodata=None) == E_ARG
    assert _call_layers(L, ok, 1, dtype=False) == E_ARG
    assert _call_render(L, ok, 1, rgba=None) == E_ARG
    assert _call_render(L, ok, 1, outer=None) == E_ARG
    assert _call_render(L, ok, 1, outer=(0.0, 0.0, 0.0)) == E_ARG   # outer auto-scale: fuse_layers + gskyhip_scale


@pytest.mark.parametrize("call", [_call_layers, _call_render], ids=["fuse_layers", "fuse_render"])
def test_mixed_types(L, call):
    # two unscaled value types
    assert call(L, _layers([(INT16, NOSP, PTR), (FLOAT32, NOSP, PTR)]), 2) == E_TYPE
    # a scaled layer is Byte, an unscaled Int16 layer is not
    assert call(L, _layers([(INT16, SP, PTR), (INT16, NOSP, PTR)]), 2) == E_TYPE
    # FusionUnscale leaves both layers their types
    assert call(L, _layers([(INT16, SP, PTR), (FLOAT32, SP, PTR)]), 2, unscale=1) == E_TYPE


def test_python_mirror_rejects_mismatched_batches():
    import gsky_amd
    from gsky_amd import fusion

    class B:   # the attributes _rendered() compares
        def __init__(self, n_tiles, max_w, max_h, sizes):
            self.n_tiles, self.max_w, self.max_h, self.tile_sizes, self.namespaces = n_tiles, max_w, max_h, sizes, [""]

    sp = gsky_amd.ScaleParams()
    a = gsky_amd.FusionLayer(B(2, 64, 64, [(64, 64), (37, 19)]), sp)
    for other in (B(1, 64, 64, [(64, 64)]), B(2, 128, 64, [(64, 64), (37, 19)]), B(2, 64, 64, [(64, 64), (36, 19)])):
        with pytest.raises(ValueError):
            fusion.fuse([a, gsky_amd.FusionLayer(other, sp)])
    with pytest.raises(ValueError):
        fusion.fuse([])
