"""What the band-math grammar of include/gskyhip.h means, stated without a
parser: each entry of CASES pairs an expression with the same computation
written out in numpy on float32 arrays -- one numpy operation per operator,
fully parenthesised, float32 constants, np.where for ?:, float32 1 / 0 for
truth values.  expected() puts the masking rule of tile_merger.go:664-724
around it.  Both parsers (oracle.band_math and the host compiler of
csrc/bandmath.hip) answer to this table: tests/test_band_math_rule.py holds
the oracle to it on the CPU, tests/test_band_math_edges.py the kernel.

`**` is the one operator whose result is not pinned to the bit: its numpy
function is float64 np.power of the float32 operands rounded to float32, and
the tests compare within a stated ulp distance (`pow=True` on the case).
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

F = np.float32
ONE, ZERO = F(1), F(0)
FLT_MAX = np.finfo(np.float32).max
DENORM_MIN = np.frombuffer(np.uint32(1).tobytes(), np.float32)[0]   # 2**-149
NORM_MIN = np.finfo(np.float32).tiny                                   # 2**-126

# expr: the text; fn: {name: float32 array} -> float32 array, or a float32
# scalar for an expression without variables; vars: the variable set
# (VARSETS); pow: compared within an ulp distance; share: the 20-80 % share of
# computed pixels is asserted (False: the expression itself yields nodata
# everywhere; None: the set is a list of chosen values, nothing is sprinkled)
Case = namedtuple("Case", "expr fn vars pow share")


def case(expr, fn, vars="default", pow=False, share=True):
    return Case(expr, fn, vars, pow, share)


def T(x):
    """A truth value: float32 1 / 0."""
    return np.where(x, ONE, ZERO)


def sel(c, x, y):
    """c ? x : y"""
    return np.where(c != ZERO, x, y).astype(F)


def mod(x, y):
    """C fmod (sign of the dividend).  fmod of two float32 values is a float32
    value, so computing it in float64 and narrowing rounds nothing."""
    return np.fmod(np.asarray(x, np.float64), np.asarray(y, np.float64)).astype(F)


def pw(x, y):
    """The `**` reference: float64 np.power of the float32 operands, rounded
    to float32."""
    return np.power(np.asarray(x, np.float64), np.asarray(y, np.float64)).astype(F)


def land(x, y):
    return T((x != ZERO) & (y != ZERO))


def lor(x, y):
    return T((x != ZERO) | (y != ZERO))


def lnot(x):
    return T(x == ZERO)


# ---------------------------------------------------------------- variables
def _frozen(a):
    a.flags.writeable = False
    return a


def _sprinkle(rng, a, nodata, share):
    a[rng.random(a.shape[0]) < share] = nodata
    return _frozen(a)


@functools.lru_cache(maxsize=None)
def variables(name):
    """The variable set `name`: [(variable name, array, nodata)], read-only
    arrays, the same on every call."""
    return VARSETS[name]()


def _vars_default():
    """Eight variables (the limit) over int16 / uint8 / float32, small values
    so that equal operands, zeros and negative bases all occur; 5 % nodata in
    each, about two thirds of the pixels valid."""
    rng = np.random.default_rng(5)
    n = 2000
    half = np.arange(-4, 7, dtype=np.float32) * F(0.5)
    quarter = np.arange(-4, 9, dtype=np.float32) * F(0.25)
    return [
        ("a", _sprinkle(rng, rng.integers(-3, 5, n).astype(np.int16), -999, 0.05), -999.0),
        ("b", _sprinkle(rng, rng.integers(0, 5, n).astype(np.uint8), 255, 0.05), 255.0),
        ("c", _sprinkle(rng, rng.choice(half, n), -9999.0, 0.05), -9999.0),
        ("d", _sprinkle(rng, rng.integers(-2, 4, n).astype(np.int16), -32768, 0.05), -32768.0),
        ("e", _sprinkle(rng, rng.integers(0, 4, n).astype(np.uint8), 200, 0.05), 200.0),
        ("b1", _sprinkle(rng, rng.choice(quarter, n), F(-1e30), 0.05), float(F(-1e30))),
        ("b1.x", _sprinkle(rng, rng.integers(-5, 6, n).astype(np.int16), -999, 0.05), -999.0),
        ("_n.2_", _sprinkle(rng, rng.integers(0, 7, n).astype(np.uint8), 0, 0.05), 0.0),
    ]


def _vars_round():
    """a * b + c where a fused multiply-add rounds differently at about a
    quarter of the pixels.  The nodata sits in a fourth, unreferenced variable
    so that all 1000 triples stay."""
    rng = np.random.default_rng(11)
    a, b, c = (_frozen(rng.normal(0, 100, 1000).astype(np.float32)) for _ in range(3))
    q = _sprinkle(np.random.default_rng(12), np.ones(1000, np.uint8), 0, 0.3)
    return [("a", a, -9999.0), ("b", b, -9999.0), ("c", c, -9999.0), ("q", q, 0.0)]


POW_BASES = [np.inf, -np.inf, 0.0, -0.0, 1.0, -1.0, 2.0, -2.0, 0.5, np.nan, 1e-40, FLT_MAX, 10.5]
POW_EXPS = [0.0, -0.0, 1.0, -1.0, 2.0, -2.0, 3.0, -3.0, 0.5, -0.5, np.inf, -np.inf, np.nan, 1.0 / 3.0, 127.0, -149.0]


def _vars_pow():
    """p ** q: every pair of POW_BASES x POW_EXPS (inf, zero, negative and NaN
    operands: C99 F.9.4.4), then 1792 ordinary pairs, p in [0.01, 100), q in
    [-8, 8), about a quarter of them nodata; m, n: small integers (negative bases
    with integer exponents, 0 ** 0)."""
    rng = np.random.default_rng(13)
    g = len(POW_BASES) * len(POW_EXPS)
    n = g + 1792
    p = np.empty(n, np.float32)
    q = np.empty(n, np.float32)
    p[:g] = np.repeat(np.array(POW_BASES, np.float32), len(POW_EXPS))
    q[:g] = np.tile(np.array(POW_EXPS, np.float32), len(POW_BASES))
    p[g:] = np.exp(rng.uniform(np.log(0.01), np.log(100.0), n - g)).astype(np.float32)
    q[g:] = rng.uniform(-8, 8, n - g).astype(np.float32)
    hole = np.zeros(n, bool)
    hole[g:] = rng.random(n - g) < 0.1
    p[hole] = -9999.0
    hole[g:] = rng.random(n - g) < 0.1
    q[hole] = -9999.0
    m = rng.integers(-6, 7, n).astype(np.int16)
    hole[g:] = rng.random(n - g) < 0.05
    m[hole] = -999
    k = rng.integers(0, 6, n).astype(np.uint8)
    hole[g:] = rng.random(n - g) < 0.05
    k[hole] = 255
    return [("p", _frozen(p), -9999.0), ("q", _frozen(q), -9999.0), ("m", _frozen(m), -999.0),
            ("n", _frozen(k), 255.0)]


SPECIALS = [np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-40, -1e-40, DENORM_MIN, -DENORM_MIN, NORM_MIN, -NORM_MIN, 1e-20,
            FLT_MAX, -FLT_MAX, 1.0, -1.0, 2.0, 2.5, 3.0, -7.5, 0.1, 16777216.0, -9999.0, 5.0]


def _vars_special():
    """c: the float32 values where arithmetic has rules of its own (NaN, the
    infinities, both zeros, denormals, the smallest normal, FLT_MAX) among
    ordinary ones; one pixel is c's nodata, one is k's."""
    c = _frozen(np.array(SPECIALS, np.float32))
    k = np.full(c.shape[0], 7, np.uint8)
    k[-1] = 255
    return [("c", c, -9999.0), ("k", _frozen(k), 255.0)]


VARSETS = {"default": _vars_default, "round": _vars_round, "pow": _vars_pow, "special": _vars_special}


# ---------------------------------------------------------------- the rule
def expected(case, variables, out_nodata, shape=None, return_computed=False):
    """tile_merger.go:664-724 around case.fn: a pixel is nodata where
    float64(float32(v)) == nodata for any variable of the axis, referenced or
    not; non-finite array results become float32(out_nodata); an expression
    without a variable fills every valid pixel with its value, finite or not.
    `shape` stands in where there is no variable.  With return_computed also
    the mask of the pixels that carry a computed value."""
    env = {n: np.asarray(a).astype(np.float32) for n, a, _ in variables}
    if variables:
        shape = np.asarray(variables[0][1]).shape
    valid = np.ones(shape, bool)
    for n, _, nd in variables:
        valid &= env[n].astype(np.float64) != float(nd)
    with np.errstate(all="ignore"):
        res = case.fn(env)
        nd32 = F(out_nodata)
    assert np.asarray(res).dtype == np.float32, case.expr
    computed = valid
    if np.ndim(res) != 0:                      # an array: non-finite values are dropped
        assert np.shape(res) == tuple(shape), case.expr
        computed = valid & np.isfinite(res)
    out = np.where(computed, res, nd32).astype(np.float32)
    return (out, computed) if return_computed else out


def same_bits(got, exp):
    """Bit equality of two float32 arrays.  NaNs compare equal to each other
    whatever their sign and payload (IEEE 754 fixes neither for 0/0)."""
    got, exp = np.asarray(got), np.asarray(exp)
    if got.dtype != np.float32 or exp.dtype != np.float32 or got.shape != exp.shape:
        return False
    gn, en = np.isnan(got), np.isnan(exp)
    g = np.where(gn, np.uint32(0x7FC00000), np.ascontiguousarray(got).view(np.uint32))
    e = np.where(en, np.uint32(0x7FC00000), np.ascontiguousarray(exp).view(np.uint32))
    return bool(np.array_equal(g, e))


def ulp_distance(x, y):
    """Distance in float32 steps between finite values (both zeros at 0)."""
    def key(z):
        i = np.ascontiguousarray(z, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(x) - key(y))


def pow_close(got, exp, computed, out_nodata, max_ulp):
    """The `**` comparison: nodata at exactly the expected pixels, every
    other pixel finite (NaN only where a variable-free expression gives NaN)
    and within max_ulp of the reference, zeros with the reference's sign.
    Returns (ok, largest ulp distance)."""
    got, exp = np.asarray(got), np.asarray(exp)
    if not same_bits(got[~computed], exp[~computed]):
        return False, -1
    g, e = got[computed], exp[computed]
    if not np.array_equal(np.isfinite(g), np.isfinite(e)):
        return False, -1
    if not same_bits(g[~np.isfinite(e)], e[~np.isfinite(e)]):
        return False, -1
    fin = np.isfinite(e)
    if not fin.any():
        return True, 0
    dist = ulp_distance(g[fin], e[fin])
    zero = e[fin] == 0
    signs = np.array_equal(np.signbit(g[fin][zero]), np.signbit(e[fin][zero]))
    return bool(signs and dist.max() <= max_ulp), int(dist.max())


# ---------------------------------------------------------------- the table
def _v(*names):
    return lambda f: (lambda v: f(*[v[n] for n in names]))


abc = _v("a", "b", "c")
abcde = _v("a", "b", "c", "d", "e")
ab = _v("a", "b")
a_ = _v("a")
c_ = _v("c")

CASES = [
    # ---- binary operators associate to the left
    case("a - b - c", abc(lambda a, b, c: (a - b) - c)),
    case("a / b / c", abc(lambda a, b, c: (a / b) / c)),
    case("a % b % c", abc(lambda a, b, c: mod(mod(a, b), c))),
    case("a < b < c", abc(lambda a, b, c: T(T(a < b) < c))),
    case("a == b == 0", abc(lambda a, b, c: T(T(a == b) == F(0)))),
    case("a - b + c", abc(lambda a, b, c: (a - b) + c)),
    case("a / b * c", abc(lambda a, b, c: (a / b) * c)),
    case("a != b != c", abc(lambda a, b, c: T(T(a != b) != c))),
    # ---- ** and ?: associate to the right
    case("2 ** 3 ** 2", lambda v: pw(F(2), pw(F(3), F(2))), pow=True),
    case("a ? b : c ? d : e", abcde(lambda a, b, c, d, e: sel(a, b, sel(c, d, e)))),
    case("a ? b ? 1 : 2 : 3", abcde(lambda a, b, c, d, e: sel(a, sel(b, F(1), F(2)), F(3)))),
    case("(a ? b : c) ? d : e", abcde(lambda a, b, c, d, e: sel(sel(a, b, c), d, e))),
    # ---- precedence
    case("a + b * c", abc(lambda a, b, c: a + (b * c))),
    case("a * b + c", abc(lambda a, b, c: (a * b) + c)),
    case("a - b / c", abc(lambda a, b, c: a - (b / c))),
    case("a && b || c", abc(lambda a, b, c: lor(land(a, b), c))),
    case("a || b && c", abc(lambda a, b, c: lor(a, land(b, c)))),
    case("a < b == c", abc(lambda a, b, c: T(T(a < b) == c))),
    case("a == b < c", abc(lambda a, b, c: T(a == T(b < c)))),
    case("a != b >= c", abc(lambda a, b, c: T(a != T(b >= c)))),
    case("a + b < c * 2", abc(lambda a, b, c: T((a + b) < (c * F(2))))),
    case("a == b && c", abc(lambda a, b, c: land(T(a == b), c))),
    case("a || b ? c : d", abcde(lambda a, b, c, d, e: sel(lor(a, b), c, d))),
    case("!a == 0", a_(lambda a: T(lnot(a) == F(0)))),
    case("-a ** 2", a_(lambda a: pw(-a, F(2))), pow=True),
    case("2 ** -1", lambda v: pw(F(2), -F(1)), pow=True),
    case("a ** -b", ab(lambda a, b: pw(a, -b)), pow=True),
    case("a * b ** 2", ab(lambda a, b: a * pw(b, F(2))), pow=True),
    # ---- the six comparisons, on operands that are often equal
    case("a < b", ab(lambda a, b: T(a < b))),
    case("a <= b", ab(lambda a, b: T(a <= b))),
    case("a > b", ab(lambda a, b: T(a > b))),
    case("a >= b", ab(lambda a, b: T(a >= b))),
    case("a == b", ab(lambda a, b: T(a == b))),
    case("a != b", ab(lambda a, b: T(a != b))),
    # ---- sign runs and spacing
    case("a--b", ab(lambda a, b: a - (-b))),
    case("a - -b", ab(lambda a, b: a - (-b))),
    case("a+-b", ab(lambda a, b: a + (-b))),
    case("a*-b", ab(lambda a, b: a * (-b))),
    case("- - a", a_(lambda a: -(-a))),
    case("!-a", a_(lambda a: lnot(-a))),
    case("-!a", a_(lambda a: -lnot(a))),
    case("!!a", a_(lambda a: lnot(lnot(a)))),
    case("+a", a_(lambda a: a)),
    case("\ta\n+\rb ", ab(lambda a, b: a + b)),
    case("a<b", ab(lambda a, b: T(a < b))),
    case("( ( a ) )", a_(lambda a: a)),
    # ---- identifiers: '.', '_' and digits; one name a prefix of another
    case("b1.x", _v("b1.x")(lambda x: x)),
    case("b1 - b", _v("b1", "b")(lambda b1, b: b1 - b)),
    case("b1.x + b1 * b - _n.2_", _v("b1.x", "b1", "b", "_n.2_")(lambda x, b1, b, n: (x + (b1 * b)) - n)),
    case("b1.x / _n.2_", _v("b1.x", "_n.2_")(lambda x, n: x / n)),
    case("a + b + c + d + e + b1 + b1.x + _n.2_",
         _v("a", "b", "c", "d", "e", "b1", "b1.x", "_n.2_")(
             lambda a, b, c, d, e, b1, x, n: ((((((a + b) + c) + d) + e) + b1) + x) + n)),
    # ---- numbers
    case(".5", lambda v: F(0.5)),
    case("5.", lambda v: F(5.0)),
    case("1e3", lambda v: F(1000.0)),
    case("1.e3", lambda v: F(1000.0)),
    case("1E-2", lambda v: F(0.01)),
    case("1e+2", lambda v: F(100.0)),
    case("08", lambda v: F(8.0)),
    case("16777217", lambda v: F(16777216.0)),           # 2**24 + 1 rounds to even
    case("1e-46", lambda v: F(0.0)),                     # below half the smallest denormal
    case("1e39", lambda v: F(np.inf)),                   # a scalar: written to every valid pixel
    case("1e39 * a", a_(lambda a: F(np.inf) * a), share=False),   # an array: nodata (NaN at a == 0)
    case("a * .5 + 5.", a_(lambda a: (a * F(0.5)) + F(5.0))),
    case("a + 16777217", a_(lambda a: a + F(16777216.0))),
    case("a * 0.1", a_(lambda a: a * F(0.1))),
    case("a+1e-2", a_(lambda a: a + F(0.01))),
    # ---- every operation rounds on its own (no fused multiply-add)
    case("a * b + c", abc(lambda a, b, c: (a * b) + c), vars="round"),
    # ---- mod and division
    case("a % 3", a_(lambda a: mod(a, F(3)))),
    case("-7 % 3", lambda v: mod(-F(7), F(3))),          # -1: the sign of the dividend
    case("a % -3", a_(lambda a: mod(a, -F(3)))),
    case("c % 1.5", c_(lambda c: mod(c, F(1.5)))),
    case("a % 0", a_(lambda a: mod(a, F(0))), share=False),
    case("a / 0", a_(lambda a: a / F(0)), share=False),
    case("0 / 0", lambda v: F(0) / F(0)),                # a scalar: NaN, written as it is
    case("a * 0 / 0", a_(lambda a: (a * F(0)) / F(0)), share=False),
    case("a > 0 ? 1/0 : 2", a_(lambda a: sel(T(a > F(0)), F(1) / F(0), F(2)))),
    case("a / 3", a_(lambda a: a / F(3))),
    # ---- ** (test_band_math_edges.py 2c)
    case("m ** n", _v("m", "n")(lambda m, n: pw(m, n)), vars="pow", pow=True),
    case("p ** 0.5", _v("p")(lambda p: pw(p, F(0.5))), vars="pow", pow=True),
    case("p ** q", _v("p", "q")(lambda p, q: pw(p, q)), vars="pow", pow=True),
    case("0 ** 0", lambda v: pw(F(0), F(0)), vars="pow", pow=True),
    case("(0-8) ** (1/3)", lambda v: pw(F(0) - F(8), F(1) / F(3)), vars="pow", pow=True),   # a scalar: NaN
    case("(m*0-8) ** (1/3)", _v("m")(lambda m: pw((m * F(0)) - F(8), F(1) / F(3))), vars="pow", pow=True,
         share=False),
]

# ---- non-finite and tiny pixels (test_band_math_edges.py 2e): c from SPECIALS
SPECIAL_CASES = [
    case("c", c_(lambda c: c), vars="special", share=None),
    case("-c", c_(lambda c: -c), vars="special", share=None),                       # -(0.0) is -0.0
    case("c * 0.5", c_(lambda c: c * F(0.5)), vars="special", share=None),          # denormal results stay
    case("c * c", c_(lambda c: c * c), vars="special", share=None),                 # 1e-20 ** 2: a denormal from normals
    case("c / 3", c_(lambda c: c / F(3)), vars="special", share=None),
    case("c + 0", c_(lambda c: c + F(0)), vars="special", share=None),              # -0.0 + 0 is +0.0
    case("c == c", c_(lambda c: T(c == c)), vars="special", share=None),            # 0 at NaN
    case("c != c", c_(lambda c: T(c != c)), vars="special", share=None),            # 1 at NaN
    case("c < 1", c_(lambda c: T(c < F(1))), vars="special", share=None),
    case("c >= 0", c_(lambda c: T(c >= F(0))), vars="special", share=None),
    case("!c", c_(lambda c: lnot(c)), vars="special", share=None),                  # 0 at NaN, 1 at +-0
    case("c ? 1 : 2", c_(lambda c: sel(c, F(1), F(2))), vars="special", share=None),   # 1 at NaN, 2 at -0.0
    case("c && 1", c_(lambda c: land(c, F(1))), vars="special", share=None),
    case("c || 0", c_(lambda c: lor(c, F(0))), vars="special", share=None),
    case("c % 2", c_(lambda c: mod(c, F(2))), vars="special", share=None),          # nodata at +-inf
    case("2 % c", c_(lambda c: mod(F(2), c)), vars="special", share=None),
    case("c / c", c_(lambda c: c / c), vars="special", share=None),
    case("1 / c", c_(lambda c: F(1) / c), vars="special", share=None),
    case("c - c", c_(lambda c: c - c), vars="special", share=None),
    case("2.5", lambda v: F(2.5), vars="special", share=None),                      # a scalar: 2.5 at the NaN pixel too
]

REFUSED = [
    "", " ", "()", "(a", "a)",
    "a +", "a b", "1 2",
    "a = b", "a & b", "a | b", "~a",
    "a ? b", "a : b", "a ?: b",
    "1.5.2", "1e", "1_0",
    "a ! = b", "a***b", "a * *b", "a,b", "a;", "'a'",
    "A", "inf", "nan", "true",
    "0x10", "0X10", "0x1p3",
    # neighbours of the above
    "1e+", "1.e", ".", ".e3", "a ? b :", "a <", "!", "-", "a ** ", "0x", "1x", "a..b + 1", "$a", "a == = b",
]


# ---------------------------------------------------------------- the limits
# gskyhip.h: an expression may need 16 stack slots and 96 program words.
def _fold_right(names, ops):
    """n0 op0 (n1 op1 (n2 ... n_last)) and its numpy function."""
    expr = ""
    for k, n in enumerate(names[:-1]):
        expr += "%s%s(" % (n, ops[k % len(ops)])
    expr += names[-1] + ")" * (len(names) - 1)

    def fn(v):
        r = v[names[-1]]
        for k in range(len(names) - 2, -1, -1):
            op = ops[k % len(ops)]
            x = v[names[k]]
            r = x + r if op == "+" else (x - r if op == "-" else x * r)
        return r
    return expr, fn


def _fold_left(names):
    """n0 + n1 + n2 ... and its numpy function."""
    def fn(v):
        r = v[names[0]]
        for n in names[1:]:
            r = r + v[n]
        return r
    return "+".join(names), fn


def _chain_ternary(conds):
    """c0 ? 1 : c1 ? 2 : ... : 9 and its numpy function."""
    expr = " : ".join("%s ? %d" % (n, k + 1) for k, n in enumerate(conds)) + " : 9"

    def fn(v):
        r = np.full(v[conds[0]].shape, F(9))
        for k in range(len(conds) - 1, -1, -1):
            r = sel(v[conds[k]], F(k + 1), r)
        return r
    return expr, fn


_NAMES = ["a", "b", "c", "d", "e", "b1", "b1.x", "_n.2_"]


def _cycle(n):
    return [_NAMES[k % len(_NAMES)] for k in range(n)]


LIMIT_ACCEPTED = [
    case(*_fold_right(["a"] * 16, ["+"])),                  # a+(a+(...: 16 stack slots
    case(*_fold_right(_cycle(16), ["+", "-", "*"])),        # the same depth, every slot another value
    case(*_fold_left(["a"] * 48)),                          # 95 program words
    case(*_fold_left(_cycle(48))),
    case(*_chain_ternary(["a"] * 7)),                       # 7 conditions: 15 slots
    case(*_chain_ternary(_NAMES[:7])),
]
LIMIT_REFUSED = [
    _fold_right(["a"] * 17, ["+"])[0],                      # 17 slots
    _fold_left(["a"] * 49)[0],                              # 97 words
    _chain_ternary(["a"] * 8)[0],                           # 8 conditions: 17 slots
]
