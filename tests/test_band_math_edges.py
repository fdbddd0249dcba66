"""Edge cases of gskyhip_band_math (csrc/bandmath.hip) on the GPU, against the
explicit numpy table of tests/band_math_cases.py -- not against the oracle's
parser, which has the device compiler's structure: the grammar, the
refusals, `**`, the five canvas types, non-finite and denormal pixels, the
shapes up to the first size at which the grid-stride loop strides, and the
stack / program limits of include/gskyhip.h.

Everything is compared bit for bit (NaNs equal to each other), except `**`,
compared within POW_BAR ulp of float64 np.power rounded to float32."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

from tests import band_math_cases as bm

pytestmark = pytest.mark.gpu

OUT_NODATA = -999.0
E_ARG, E_TYPE = -1, -2
SENTINEL = 12345.5

# Largest distance of the device's powf from float64 np.power rounded to
# float32 over the `**` cases of the table (special operands, small integers
# and 1792 pairs with the base in [0.01, 100) and the exponent in [-8, 8)),
# measured on an MI355X with the compiler and device libraries of ROCm
# POW_MEASURED_ON: 1 ulp (at `p ** q` and `p ** 0.5`; 0 at every case with an
# integer result).  The bar is one more, since another ROCm may ship another
# powf.
POW_MEASURED_ULP = 1
POW_MEASURED_ON = "7.2.0"
POW_BAR = POW_MEASURED_ULP + 1


@functools.lru_cache(maxsize=None)
def _device_vars(name, dev):
    import torch
    return [(n, torch.from_numpy(np.array(a)).to(dev), nd) for n, a, nd in bm.variables(name)]


def _run(case, gpu, out_nodata=OUT_NODATA):
    from gsky_amd import band_math
    return band_math(case.expr, _device_vars(case.vars, str(gpu)), out_nodata).cpu().numpy()


def _raw(expr, variables, n_px, out, out_nodata=OUT_NODATA, dtypes=None, null=None, n_vars=None):
    """gskyhip_band_math through lib(): variables = [(name, tensor, nodata)]
    -> the return code."""
    import torch

    from gsky_amd import _lib
    from gsky_amd.raster import TYPE_CODES, type_of_tensor
    k = len(variables)
    names = (C.c_char_p * max(k, 1))(*[v[0].encode() for v in variables])
    ptrs = (C.c_void_p * max(k, 1))(*[v[1].data_ptr() for v in variables])
    if null is not None:
        ptrs[null] = None
    dts = np.array(dtypes if dtypes is not None else [TYPE_CODES[type_of_tensor(v[1])] for v in variables] or [0],
                   np.int32)
    nds = np.array([float(v[2]) for v in variables] or [0.0], np.float64)
    rc = _lib.lib().gskyhip_band_math(expr.encode(), names, ptrs, dts.ctypes.data_as(C.c_void_p),
                                      nds.ctypes.data_as(C.c_void_p), k if n_vars is None else n_vars, n_px,
                                      float(out_nodata), C.c_void_p(out.data_ptr()) if out is not None else None,
                                      C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


def _ids(cases):
    return [repr(c.expr)[:60] for c in cases]


# ---------------------------------------------------------------- 2a grammar, 2c **
@pytest.mark.parametrize("case", bm.CASES, ids=_ids(bm.CASES))
def test_grammar(gpu, case):
    """Every entry of the table, bit for bit.  `**` cases: the device's powf
    was measured at most 1 ulp from float64 np.power rounded to float32 (MI355X,
    ROCm 7.2.0) and is held to that plus one, 2 ulp, with nodata at exactly
    the expected pixels; the distance of each case is printed."""
    exp, computed = bm.expected(case, bm.variables(case.vars), OUT_NODATA, return_computed=True)
    share = computed.mean()
    if case.share:
        assert 0.2 <= share <= 0.8, share
    else:
        assert share == 0.0
    got = _run(case, gpu)
    if case.pow:
        ok, worst = bm.pow_close(got, exp, computed, OUT_NODATA, POW_BAR)
        print("pow ulp %r: %d" % (case.expr, worst))
        assert ok, worst
    else:
        assert bm.same_bits(got, exp), np.flatnonzero(got.view(np.uint32) != exp.view(np.uint32))[:8]


# ---------------------------------------------------------------- 2b refusals
@pytest.mark.parametrize("expr", bm.REFUSED + bm.LIMIT_REFUSED, ids=lambda e: repr(e)[:60])
def test_refused(gpu, expr):
    import torch
    vs = _device_vars("default", str(gpu))
    n = vs[0][1].numel()
    out = torch.full((n,), SENTINEL, dtype=torch.float32, device=gpu)
    assert _raw(expr, vs, n, out) == E_ARG
    assert bool((out == SENTINEL).all())


def test_refused_raises_gsky_error(gpu):
    from gsky_amd import GskyError, band_math
    for expr in ("0x10", "a +", bm.LIMIT_REFUSED[0]):
        with pytest.raises(GskyError) as ei:
            band_math(expr, _device_vars("default", str(gpu)), OUT_NODATA)
        assert ei.value.code == E_ARG


# ---------------------------------------------------------------- 2d dtypes
DTYPE_VALUES = {
    np.int8: [-128, -1, 127, 0, 1, -127, 126, 5],
    np.uint8: [0, 128, 255, 1, 127, 254, 129, 5],
    np.int16: [-32768, -1, 32767, 0, 1, -32767, 255, -256],
    np.uint16: [0, 32768, 65535, 1, 32767, 65534, 256, 255],
    np.float32: [-9999.9, 0.5, -0.0, 3e38, 1e-40, -2.5, 16777216.0, 255.0],
}
# per dtype: (nodata, the values it masks)
DTYPE_NODATA = {
    np.int8: [(-128.0, [-128]), (127.0, [127]), (-129.0, []), (float("nan"), []), (0.5, [])],
    np.uint8: [(255.0, [255]), (0.0, [0]), (300.0, []), (-1.0, []), (float("nan"), [])],
    np.int16: [(-32768.0, [-32768]), (32767.0, [32767]), (-32769.0, []), (65535.0, []), (float("nan"), [])],
    np.uint16: [(65535.0, [65535]), (32768.0, [32768]), (65536.0, []), (-1.0, []), (float("nan"), [])],
    np.float32: [(-9999.9, []), (float(np.float32(-9999.9)), [np.float32(-9999.9)]), (float("nan"), []),
                 (0.0, [0.0]), (1e-40, []), (float(np.float32(1e-40)), [np.float32(1e-40)])],
}
IDENTITIES = [bm.case("v", lambda v: v["v"]), bm.case("v * 1", lambda v: v["v"] * bm.F(1)),
              bm.case("v - 0", lambda v: v["v"] - bm.F(0))]


@pytest.mark.parametrize("dt", list(DTYPE_VALUES), ids=lambda d: np.dtype(d).name)
def test_dtypes(gpu, dt):
    """Each canvas type on its own, extremes included: the value arrives as
    float32(v), and nodata masks exactly the pixels whose float32 value equals
    it as a float64 -- an extreme, a value outside the type (nothing), a
    float64 that is no float32 (nothing), NaN (nothing)."""
    import torch

    from gsky_amd import band_math
    v = np.array(DTYPE_VALUES[dt], dt)
    tv = torch.from_numpy(v).to(gpu)
    for nodata, masked in DTYPE_NODATA[dt]:
        for case in IDENTITIES:
            exp, computed = bm.expected(case, [("v", v, nodata)], OUT_NODATA, return_computed=True)
            assert sorted(v[~computed].tolist()) == sorted(np.array(masked, dt).tolist()), (nodata, masked)
            got = band_math(case.expr, [("v", tv, nodata)], OUT_NODATA).cpu().numpy()
            assert bm.same_bits(got, exp), (case.expr, nodata, got, exp)


def test_all_dtypes_together_and_unreferenced_mask(gpu):
    """One variable per type in one call; a variable the expression does not
    name still masks the pixel where it is its nodata."""
    import torch

    from gsky_amd import band_math
    names = {np.int8: "i8", np.uint8: "u8", np.int16: "i16", np.uint16: "u16", np.float32: "f32"}
    nod = {np.int8: -128.0, np.uint8: 255.0, np.int16: -32768.0, np.uint16: 65535.0, np.float32: 0.5}
    vs = [(names[dt], np.array(vals, dt), nod[dt]) for dt, vals in DTYPE_VALUES.items()]
    dv = [(n, torch.from_numpy(a).to(gpu), nd) for n, a, nd in vs]
    cases = [bm.case("i8 + u8 + i16 + u16", lambda v: ((v["i8"] + v["u8"]) + v["i16"]) + v["u16"]),
             bm.case("u16 - i16 * i8", lambda v: v["u16"] - (v["i16"] * v["i8"])),
             bm.case("u8", lambda v: v["u8"]),           # i8, i16, u16, f32 unreferenced: pixels 0, 1, 2 masked
             bm.case("7", lambda v: bm.F(7))]
    for case in cases:
        exp, computed = bm.expected(case, vs, OUT_NODATA, return_computed=True)
        assert computed.tolist() == [False, False, False, True, True, True, True, True]
        got = band_math(case.expr, dv, OUT_NODATA).cpu().numpy()
        assert bm.same_bits(got, exp), (case.expr, got, exp)


def test_abi_arguments(gpu):
    import torch

    from gsky_amd import _lib
    a = torch.arange(5, dtype=torch.int16, device=gpu)
    out = torch.full((5,), SENTINEL, dtype=torch.float32, device=gpu)
    for bad in (0, 4, 5, 7, 99, -1):                      # UInt32, Int32, Float64 and no type at all
        assert _raw("a", [("a", a, -1.0)], 5, out, dtypes=[bad]) == E_TYPE
    nine = [("v%d" % k, a, -1.0) for k in range(9)]
    assert _raw("v0", nine, 5, out) == E_ARG
    assert _raw("a", [("a", a, -1.0)], 5, out, n_vars=-1) == E_ARG
    assert _raw("a", [("a", a, -1.0)], 5, out, null=0) == E_ARG
    assert _raw("a", [("a", a, -1.0)], 5, None) == E_ARG
    assert _raw("a", [("a", a, -1.0)], -1, out) == E_ARG
    assert bool((out == SENTINEL).all())
    # n_vars = 0: every pixel is valid
    assert _raw("2.5", [], 5, out) == 0
    assert out.cpu().tolist() == [2.5] * 5
    assert _raw("1e39", [], 3, out) == 0
    assert out.cpu().tolist() == [np.inf] * 3 + [2.5] * 2
    assert _raw("a", [], 5, out) == E_ARG
    # n_px = 0: compiled, nothing launched, nothing written
    assert _raw("a + 1", [("a", a, -1.0)], 0, out) == 0
    assert _raw("a +", [("a", a, -1.0)], 0, out) == E_ARG
    assert out.cpu().tolist() == [np.inf] * 3 + [2.5] * 2
    assert _lib.FLOAT32 == 6 and _lib.SIGNEDBYTE == 100


# ---------------------------------------------------------------- 2e non-finite and tiny pixels
@pytest.mark.parametrize("case", bm.SPECIAL_CASES, ids=_ids(bm.SPECIAL_CASES))
def test_special_values(gpu, case):
    """NaN, the infinities, both zeros, denormals (kept, never flushed), the
    smallest normal and FLT_MAX through every kind of operator."""
    exp = bm.expected(case, bm.variables("special"), OUT_NODATA)
    got = _run(case, gpu)
    assert bm.same_bits(got, exp), [(s, g, e) for s, g, e in zip(bm.SPECIALS, got, exp)
                                    if not bm.same_bits(np.float32([g]), np.float32([e]))]


def test_special_values_by_hand(gpu):
    """What the table gives at the pixels the issue names, stated as numbers,
    and out_nodata: a finite result equal to it is kept, and it is stored as
    float32(out_nodata)."""
    s = bm.SPECIALS
    at = {"nan": 0, "inf": 1, "-inf": 2, "0": 3, "-0": 4, "1e-40": 5, "den": 7, "2.5": 17}
    by_expr = {c.expr: c for c in bm.SPECIAL_CASES}

    def run(expr, out_nodata=OUT_NODATA):
        return _run(by_expr[expr], gpu, out_nodata)

    nd = np.float32(OUT_NODATA)
    neg = run("-c")
    assert np.signbit(neg[at["0"]]) and neg[at["0"]] == 0 and not np.signbit(neg[at["-0"]])
    assert neg[at["nan"]] == nd and neg[at["inf"]] == nd and neg[at["-inf"]] == nd
    half = run("c * 0.5")
    assert half[at["1e-40"]] == np.float32(1e-40) * np.float32(0.5) and half[at["1e-40"]] != 0
    assert half[at["den"]] == 0                                   # 2**-150 ties to even
    assert run("c == c")[at["nan"]] == 0 and run("c != c")[at["nan"]] == 1
    n = run("!c")
    assert (n[at["nan"]], n[at["0"]], n[at["-0"]], n[at["den"]]) == (0, 1, 1, 0)
    t = run("c ? 1 : 2")
    assert (t[at["nan"]], t[at["-0"]], t[at["0"]], t[at["den"]]) == (1, 2, 2, 1)
    assert run("c && 1")[at["nan"]] == 1 and run("c || 0")[at["-0"]] == 0
    m = run("c % 2")
    assert m[at["inf"]] == nd and m[at["-inf"]] == nd and m[at["nan"]] == nd and m[at["2.5"]] == 0.5
    q = run("c / c")
    assert q[at["0"]] == nd and q[at["inf"]] == nd and q[at["1e-40"]] == 1 and q[at["den"]] == 1
    assert run("2.5")[at["nan"]] == 2.5 and run("2.5")[-1] == nd and run("2.5")[-2] == nd
    kept = run("c", 2.5)
    assert kept[at["2.5"]] == 2.5 and kept[at["nan"]] == 2.5 and kept[at["-0"]] == 0
    stored = run("c", -9999.9)
    assert stored[at["nan"]] == np.float32(-9999.9) and stored[-1] == np.float32(-9999.9)
    assert bm.same_bits(stored, bm.expected(by_expr["c"], bm.variables("special"), -9999.9))
    assert s[at["den"]] == bm.DENORM_MIN and s[at["2.5"]] == 2.5


# ---------------------------------------------------------------- 2f shapes
SHAPE_CASE = bm.case("a * b - 1", lambda v: (v["a"] * v["b"]) - bm.F(1))


def _shape_vars(n):
    rng = np.random.default_rng(100 + n)
    a = rng.integers(-100, 100, n).astype(np.int16)
    b = rng.normal(0, 3, n).astype(np.float32)
    a[rng.random(n) < 0.2] = -999
    return [("a", a, -999.0), ("b", b, -9999.0)]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1000])
def test_sizes(gpu, n):
    import torch

    from gsky_amd import band_math
    vs = _shape_vars(n)
    got = band_math(SHAPE_CASE.expr, [(nm, torch.from_numpy(a).to(gpu), nd) for nm, a, nd in vs], OUT_NODATA)
    assert got.shape == (n,) and got.dtype == torch.float32
    assert bm.same_bits(got.cpu().numpy(), bm.expected(SHAPE_CASE, vs, OUT_NODATA))


def test_shape_is_kept_and_must_agree(gpu):
    import torch

    from gsky_amd import band_math
    vs = [(nm, a.reshape(7, 13), nd) for nm, a, nd in _shape_vars(91)]
    dv = [(nm, torch.from_numpy(a).to(gpu), nd) for nm, a, nd in vs]
    got = band_math(SHAPE_CASE.expr, dv, OUT_NODATA)
    assert got.shape == (7, 13)
    assert bm.same_bits(got.cpu().numpy(), bm.expected(SHAPE_CASE, vs, OUT_NODATA))
    with pytest.raises(ValueError):
        band_math(SHAPE_CASE.expr, [dv[0], (dv[1][0], dv[1][1].reshape(13, 7), dv[1][2])], OUT_NODATA)
    with pytest.raises(ValueError):
        band_math(SHAPE_CASE.expr, [dv[0], (dv[1][0], dv[1][1][:6], dv[1][2])], OUT_NODATA)
    with pytest.raises(ValueError):
        band_math("1", [], OUT_NODATA)
    with pytest.raises(ValueError):
        band_math("1", [("v%d" % k, dv[0][1], -1.0) for k in range(9)], OUT_NODATA)


def test_grid_stride(gpu):
    """65536 blocks x 256 threads + 257 pixels: the smallest size at which
    the loop of band_math_kernel goes round a second time."""
    import torch

    from gsky_amd import band_math
    n = 65536 * 256 + 257
    a = (torch.arange(n, device=gpu, dtype=torch.int32) % 251).to(torch.uint8)
    got = band_math("a + 1", [("a", a, 255.0)], OUT_NODATA)
    assert torch.equal(got, a.float() + 1)


def test_views(gpu):
    """A stride-2 view, and a typed slice cut from a byte workspace the way
    fusion.canvas_views cuts canvases, give what their contiguous copies give."""
    import torch

    from gsky_amd import band_math
    vs = _shape_vars(600)
    exp = bm.expected(SHAPE_CASE, [(nm, a[::2], nd) for nm, a, nd in vs], OUT_NODATA)
    dv = [(nm, torch.from_numpy(a).to(gpu)[::2], nd) for nm, a, nd in vs]
    assert not dv[0][1].is_contiguous()
    assert bm.same_bits(band_math(SHAPE_CASE.expr, dv, OUT_NODATA).cpu().numpy(), exp)
    # (n_tiles, n_ns, bytes) workspace: namespace 1 of every tile as int16 (h, w), namespace 2 as float32
    w, h, tiles = 13, 7, 3
    rng = np.random.default_rng(3)
    ws = rng.integers(0, 256, (tiles, 3, w * h * 4), dtype=np.uint8)
    fl = rng.normal(0, 3, (tiles, w * h)).astype(np.float32)
    ws[:, 2, :] = fl.view(np.uint8)
    dws = torch.from_numpy(ws).to(gpu)
    a_np = ws[:, 1, :w * h * 2].copy().view(np.int16).reshape(tiles, h, w)
    a_dev = dws[:, 1, :w * h * 2].view(torch.int16).reshape(tiles, h, w)
    b_dev = dws[:, 2, :w * h * 4].view(torch.float32).reshape(tiles, h, w)
    nd = float(a_np.flat[5])
    got = band_math(SHAPE_CASE.expr, [("a", a_dev, nd), ("b", b_dev, -9999.0)], OUT_NODATA)
    assert got.shape == (tiles, h, w)
    exp = bm.expected(SHAPE_CASE, [("a", a_np, nd), ("b", fl.reshape(tiles, h, w), -9999.0)], OUT_NODATA)
    assert (exp == np.float32(OUT_NODATA)).any() and bm.same_bits(got.cpu().numpy(), exp)
    same = band_math(SHAPE_CASE.expr, [("a", a_dev.contiguous(), nd), ("b", b_dev.contiguous(), -9999.0)],
                     OUT_NODATA)
    assert torch.equal(got, same)


def test_side_stream(gpu):
    import torch

    from gsky_amd import band_math
    vs = _shape_vars(5000)
    dv = [(nm, torch.from_numpy(a).to(gpu), nd) for nm, a, nd in vs]
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=gpu)
    with torch.cuda.stream(side):
        got = band_math(SHAPE_CASE.expr, dv, OUT_NODATA)
    side.synchronize()
    assert bm.same_bits(got.cpu().numpy(), bm.expected(SHAPE_CASE, vs, OUT_NODATA))


# ---------------------------------------------------------------- 2g limits
@pytest.mark.parametrize("case", bm.LIMIT_ACCEPTED, ids=_ids(bm.LIMIT_ACCEPTED))
def test_limits_accepted(gpu, case):
    """16 stack slots, 95 of 96 program words, 7 chained conditions, 8
    variables: accepted and right, so slot 15 and the last words hold values.
    (One more of each is in test_refused.)"""
    exp, computed = bm.expected(case, bm.variables("default"), OUT_NODATA, return_computed=True)
    assert 0.2 <= computed.mean() <= 0.8 and np.unique(exp).size >= 3
    assert bm.same_bits(_run(case, gpu), exp)
