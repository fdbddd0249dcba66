"""The band-math grammar on the CPU: oracle.band_math against the explicit
numpy table of tests/band_math_cases.py (which goes through no parser), and
the host compiler of csrc/bandmath.hip -- which runs before any HIP call --
accepting and refusing what the table says.  No GPU is used: the compiler is
reached with n_px = 0, where gskyhip_band_math returns after compiling.

`**` cases: the table's reference is float64 np.power rounded to float32; the
oracle computes numpy's float32 power, which is the C library's powf.  glibc
documents powf as correctly rounded in all but rare cases and within 1 ulp
always, so the oracle is held to 1 ulp of the table."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from tests import band_math_cases as bm

ORACLE_POW_ULP = 1
ALL_CASES = bm.CASES + bm.SPECIAL_CASES + bm.LIMIT_ACCEPTED
OUT_NODATA = -999.0


def _ids(cases):
    return [repr(c.expr)[:60] for c in cases]


@pytest.mark.parametrize("case", ALL_CASES, ids=_ids(ALL_CASES))
def test_oracle_answers_to_the_table(oracle, case):
    vs = bm.variables(case.vars)
    exp, computed = bm.expected(case, vs, OUT_NODATA, return_computed=True)
    got = oracle.band_math(case.expr, vs, OUT_NODATA)
    if case.pow:
        ok, worst = bm.pow_close(got, exp, computed, OUT_NODATA, ORACLE_POW_ULP)
        assert ok, (case.expr, worst)
    else:
        assert bm.same_bits(got, exp), case.expr
    share = computed.mean()
    if case.share:
        assert 0.2 <= share <= 0.8, (case.expr, share)
    elif case.share is False:
        assert share == 0.0 and (exp.view(np.uint32) == np.float32(OUT_NODATA).view(np.uint32)).all()


@pytest.mark.parametrize("expr", bm.REFUSED, ids=repr)
def test_oracle_refuses(oracle, expr):
    with pytest.raises(ValueError):
        oracle.band_math(expr, bm.variables("default"), OUT_NODATA)


def test_table_known_answers():
    """The table itself, by hand: what the issue states in words."""
    px = [("a", np.array([3, 0, -2], np.int16), -999.0)]

    def val(expr):
        (c,) = [k for k in bm.CASES if k.expr == expr]
        return bm.expected(c, px, -1.0).tolist()

    assert val("2 ** 3 ** 2") == [512.0] * 3
    assert val("2 ** -1") == [0.5] * 3
    assert val("-a ** 2") == [9.0, 0.0, 4.0]
    assert val("-7 % 3") == [-1.0] * 3
    assert val("a % -3") == [0.0, 0.0, -2.0]
    assert val("16777217") == [16777216.0] * 3
    assert val("1e-46") == [0.0] * 3
    assert val("1e39") == [np.inf] * 3
    assert val("1e39 * a") == [-1.0] * 3
    assert val("a / 0") == [-1.0] * 3
    assert val("a > 0 ? 1/0 : 2") == [-1.0, 2.0, 2.0]
    assert val("0 ** 0") == [1.0] * 3
    assert all(np.isnan(val("0 / 0"))) and all(np.isnan(val("(0-8) ** (1/3)")))
    assert val("!a == 0") == [1.0, 0.0, 1.0]
    # == binds looser than <: a == (b < c), not (a == b) < c
    abc = [("a", np.array([2], np.int16), -999.0), ("b", np.array([2], np.int16), -999.0),
           ("c", np.array([5], np.int16), -999.0)]
    (c,) = [k for k in bm.CASES if k.expr == "a == b < c"]
    assert bm.expected(c, abc, -1.0).tolist() == [0.0]   # 2 == (2 < 5) is 0, while (2 == 2) < 5 would be 1


def test_masking_rule():
    """expected(): an unreferenced variable masks, the comparison is made on
    float64(float32(v)), a NaN nodata masks nothing."""
    c = bm.case("v", lambda v: v["v"])
    v = np.array([1.0, -9999.9, np.nan, np.inf], np.float32)
    w = np.array([0, 0, 0, 7], np.uint8)
    assert bm.expected(c, [("v", v, -9999.9), ("w", w, 9.0)], -1.0).tolist()[:2] == [1.0, float(np.float32(-9999.9))]
    got = bm.expected(c, [("v", v, float(np.float32(-9999.9))), ("w", w, 7.0)], -1.0)
    assert got.tolist() == [1.0, -1.0, -1.0, -1.0]
    got = bm.expected(c, [("v", v, float("nan")), ("w", w, 9.0)], -2.0)
    assert got.tolist() == [1.0, float(np.float32(-9999.9)), -2.0, -2.0]
    s = bm.case("2.5", lambda v: bm.F(2.5))
    assert bm.expected(s, [("v", v, 1.0)], -1.0).tolist() == [-1.0, 2.5, 2.5, 2.5]
    assert bm.expected(s, [], -1.0, shape=(3,)).tolist() == [2.5] * 3


def test_every_operation_rounds_on_its_own():
    """The `a * b + c` inputs tell a fused multiply-add from two roundings at
    no fewer than 200 of the 1000 pixels (the fused value: the exact float64
    product plus c, rounded)."""
    a, b, c = (np.asarray(x[1]) for x in bm.variables("round")[:3])
    two = (a * b) + c
    fused = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    differ = two.view(np.uint32) != fused.view(np.uint32)
    assert differ.sum() >= 200, differ.sum()
    (case,) = [k for k in bm.CASES if k.vars == "round"]
    exp, computed = bm.expected(case, bm.variables("round"), OUT_NODATA, return_computed=True)
    assert (differ & computed).sum() >= 100
    assert bm.same_bits(exp[computed], two[computed])


def test_variable_sets_hold_what_the_cases_need():
    d = {n: np.asarray(a) for n, a, _ in bm.variables("default")}
    assert {d["a"].dtype, d["b"].dtype, d["c"].dtype} == {np.dtype(np.int16), np.dtype(np.uint8), np.dtype(np.float32)}
    eq = d["a"].astype(np.float32) == d["b"].astype(np.float32)
    assert 0.05 < eq.mean() < 0.5                      # a == b at some pixels: < and <= differ there
    assert (d["a"] == 0).any() and (d["a"] < 0).any() and (d["c"] == 0).any()
    s = np.asarray(bm.variables("special")[0][1])
    assert np.isnan(s).any() and np.isinf(s).sum() == 2 and np.signbit(s[s == 0]).sum() == 1
    assert ((s != 0) & (np.abs(s) < bm.NORM_MIN)).sum() >= 4   # denormals


# ---------------------------------------------------------------- host compiler
def _compile(expr, names):
    """gskyhip_band_math with n_px = 0: the expression is compiled, nothing is
    launched and no canvas pointer is followed (they point at a host word)."""
    from gsky_amd import _lib
    L = _lib.lib()
    k = len(names)
    arr = (C.c_char_p * max(k, 1))(*[n.encode() for n in names])
    word = np.zeros(1, np.float32)
    ptrs = (C.c_void_p * max(k, 1))(*[word.ctypes.data] * k)
    dts = np.full(max(k, 1), _lib.FLOAT32, np.int32)
    nds = np.zeros(max(k, 1), np.float64)
    return L.gskyhip_band_math(expr.encode(), arr, ptrs, dts.ctypes.data_as(C.c_void_p),
                               nds.ctypes.data_as(C.c_void_p), k, 0, 0.0, None, None)


@pytest.mark.parametrize("case", ALL_CASES, ids=_ids(ALL_CASES))
def test_host_compiler_accepts(case):
    assert _compile(case.expr, [n for n, _, _ in bm.variables(case.vars)]) == 0


@pytest.mark.parametrize("expr", bm.REFUSED + bm.LIMIT_REFUSED, ids=lambda e: repr(e)[:60])
def test_host_compiler_refuses(expr):
    assert _compile(expr, [n for n, _, _ in bm.variables("default")]) == -1


def test_host_compiler_hex_is_no_number():
    """strtod reads "0x10" as 16 and "0x1p3" as 8; the grammar has decimal
    numbers only.  A variable named like the tail does not rescue it."""
    for expr in ("0x10", "0X10", "0x1p3", "a + 0x10", "0x10 + a", "1e", "1.5.2"):
        assert _compile(expr, ["a", "x10", "X10", "x1p3", "e"]) == -1, expr
    for expr in ("0 * x10", "08", "1e3", "1.e3", ".5e-1", "5.E+2"):
        assert _compile(expr, ["a", "x10"]) == 0, expr
