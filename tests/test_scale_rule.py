"""The scale rule (utils.Scale, utils/raster_scaler.go:30-332, and the legacy
RasterScaler, processor/tile_scaler.go:17-112) in numpy, written from the Go
text, the table of cases every implementation is held to, and checks of the
rule.  tests/test_scale_edges.py drives the five device implementations with
the same table; this module needs no GPU.

The rule, in the order of the Go text:
  conversions   float64 -> int8 / uint8 / int16 / uint16 is CVTTSD2SL to int32
                (NaN or out of range -> 0x80000000) and truncation to the low
                bits; uint8(float32) is CVTTSS2SL, the same rule.  Restated
                here (`go_cvtt32`, `go_conv`, `go_u8_f32`), not imported.
  constant      scale = float32(Scale); scale <= 0: 1 if Clip <= 0, else
                float32(float32(254) / float32(Clip))  (raster_scaler.go:31-38)
  integers      noData, offset, clip = T(NoData), T(Offset), T(Clip); nodata ->
                0xFF; value += offset wraps in T; clip first, then 0; the byte
                is uint8(float32(value) * scale)  (41-45, 80-93 and siblings)
  float32       value == float32(NoData) first; ColourScale > 0: normalise()
                in float64 against the float64 NoData (15-28) -- with a NaN
                NoData `v == NoData` is false and a NaN goes on through the
                arithmetic; then add, clamp, multiply in float32  (305-326)
  auto          Scale == Clip == Offset == 0: the sequential loop (48-67,
                268-293) as a Python loop: min and max start at 0 and only a
                valid element 0 sets them, so a NaN anywhere else loses every
                comparison and a NaN at element 0 makes everything NaN;
                maxVal += 0.1 in float32; scale = 254 / (max - min); the
                integer offset and clip re-derived from float32 through T()
  Log10         Go's portable math/log.go and log10.go step by step in float64
                with np.frexp: the algorithm of the oracle and of both device
                copies.  Agreement with an amd64 Go build's math.Log (which has
                an assembly body) is still unpinned: there is no Go toolchain
                to run, as tests/test_oracle_kats.py says for the oracle.
  legacy        Byte in place, float64 multiply; Int16 / UInt16 value * 254 /
                float32(clip); Float32 adds float32(uint8(offset)).

The table (part "cases" below): per integer type the whole value domain,
rolled so that element 0 is the nodata and so that it is not, under six
nodata values and twenty parameter triples, plus five small arrays for auto
mode; for float32 a boundary set per triple (the three float32 around every
byte boundary), special values, log and non-log colour scales and eight
small auto-mode arrays.  Every data set runs under every parameter set.
"""
import functools

import numpy as np
import pytest

from .test_oracle_kats import SCALE_KATS

f32 = np.float32
INT_TYPES = (np.uint8, np.int8, np.int16, np.uint16)
NAN, INF = float("nan"), float("inf")


# ---------------------------------------------------------------- Go conversions
def go_cvtt32(x):
    """CVTTSD2SL / CVTTSS2SL: truncate to int32; NaN or out of range -> -2^31."""
    x = float(x)
    if not (x > -2147483649.0 and x < 2147483648.0):
        return -2 ** 31
    return int(x)


def go_conv(x, dt):
    """Go's T(x) of a float: int32 conversion, then the low bits of T."""
    dt = np.dtype(dt)
    if dt == np.float32:
        with np.errstate(over="ignore"):
            return f32(x)
    bits = dt.itemsize * 8
    u = go_cvtt32(x) & ((1 << bits) - 1)
    if dt.kind == "i" and u >> (bits - 1):
        u -= 1 << bits
    return dt.type(u)


def _wrap(v, dt):
    """int64 array -> its low bits read as T (Go's wrapping integer add)."""
    dt = np.dtype(dt)
    bits = dt.itemsize * 8
    u = v & ((1 << bits) - 1)
    if dt.kind == "i":
        u = np.where(u >> (bits - 1), u - (1 << bits), u)
    return u


def go_u8(x):
    """uint8() of a float array (float32 or float64)."""
    d = np.asarray(x, np.float64)
    ok = (d > -2147483649.0) & (d < 2147483648.0)
    i = np.where(ok, np.trunc(np.where(ok, d, 0.0)), -2.0 ** 31).astype(np.int64)
    return (i & 0xFF).astype(np.uint8)


# ---------------------------------------------------------------- math.Log10
def go_log(x):
    """math.Log, the portable body (log.go: FreeBSD's e_log.c), elementwise."""
    x = np.asarray(x, np.float64)
    Ln2Hi, Ln2Lo = 6.93147180369123816490e-01, 1.90821492927058770002e-10
    L1, L2, L3, L4 = 6.666666666666735130e-01, 3.999999999940941908e-01, 2.857142874366239149e-01, 2.222219843214978396e-01
    L5, L6, L7 = 1.818357216161805012e-01, 1.531383769920937332e-01, 1.479819860511658591e-01
    with np.errstate(all="ignore"):
        f1, ki = np.frexp(x)
        low = f1 < 1.41421356237309504880168872420969808 / 2
        f1 = np.where(low, f1 * 2, f1)
        k = (ki - low).astype(np.float64)
        f = f1 - 1
        s = f / (2 + f)
        s2 = s * s
        s4 = s2 * s2
        t1 = s2 * (L1 + s4 * (L3 + s4 * (L5 + s4 * L7)))
        t2 = s4 * (L2 + s4 * (L4 + s4 * L6))
        R = t1 + t2
        hfsq = 0.5 * f * f
        r = k * Ln2Hi - ((hfsq - (s * (hfsq + R) + k * Ln2Lo)) - f)
    r = np.where(x == 0, -np.inf, r)
    r = np.where(x < 0, np.nan, r)
    return np.where(np.isnan(x) | (x == np.inf), x, r)


def go_log10(x):
    """math.Log10 = log2(x) * (Ln2 / Ln10); log2 by Frexp (log10.go)."""
    x = np.asarray(x, np.float64)
    frac, e = np.frexp(x)
    e = np.where(np.isfinite(x) & (x != 0), e, 0)      # Go's Frexp: 0, Inf and NaN come back with exponent 0
    with np.errstate(all="ignore"):
        l2 = np.where(frac == 0.5, (e - 1).astype(np.float64),
                      go_log(frac) * (1.0 / 0.693147180559945309417232121458176568) + e.astype(np.float64))
        return l2 * 0.301029995663981195213738894724493026768189881462108541310


def normalise(val, colour_scale, nodata):
    """normalise() (raster_scaler.go:15-28) of a float64 array."""
    with np.errstate(all="ignore"):
        v = go_log10(val) if colour_scale == 1 else val.copy()
        v = np.where(np.isinf(v) | np.isnan(v), nodata, v)
        return np.where(val == nodata, val, v)


# ---------------------------------------------------------------- the rule
def scale_const(scale, clip):
    """raster_scaler.go:31-38, float32 arithmetic."""
    with np.errstate(all="ignore"):
        sc = f32(scale)
        if sc <= 0.0:
            sc = f32(1.0) if clip <= 0.0 else f32(f32(254.0) / f32(clip))
    return sc


def is_auto(offset, scale, clip):
    return scale == 0.0 and clip == 0.0 and offset == 0.0


def auto_minmax(vals, valid):
    """The sequential loop of raster_scaler.go:48-67 (268-293), literally.
    vals: the float32 values as Python floats; valid: not skipped by the
    nodata tests."""
    min_val = max_val = 0.0
    for i, value in enumerate(vals):
        if not valid[i]:
            continue
        if i == 0:
            min_val = value
            max_val = value
        else:
            if value < min_val:
                min_val = value
            if value > max_val:
                max_val = value
    return f32(min_val), f32(max_val)


def auto_consts(vals, valid):
    """(scale, dfOffset, maxVal + dfOffset), all float32 (69-77, 295-302)."""
    min_val, max_val = auto_minmax(vals, valid)
    with np.errstate(all="ignore"):
        if min_val == max_val:
            max_val = f32(max_val + f32(0.1))
        sc = f32(254.0) / f32(max_val - min_val)
        df_offset = f32(-min_val)
        return f32(sc), df_offset, f32(max_val + df_offset)


def scale_rule(data, nodata, offset, scale, clip, colour_scale=0, signed_byte=False):
    """utils.scale of one raster -> uint8 array of the same shape."""
    data = np.asarray(data)
    if signed_byte and data.dtype == np.uint8:
        data = data.view(np.int8)
    shape = data.shape
    d = np.ascontiguousarray(data).reshape(-1)
    sc = scale_const(scale, clip)
    auto = is_auto(offset, scale, clip)
    if d.dtype == np.float32:
        nd32 = go_conv(nodata, np.float32)
        with np.errstate(all="ignore"):
            is_nd = d == nd32                                       # 306
            value = d
            if colour_scale > 0:                                    # 309-316
                v = normalise(d.astype(np.float64), colour_scale, float(nodata))
                is_nd = is_nd | (v == float(nodata))
                value = v.astype(np.float32)
            off, clp = f32(offset), f32(clip)
            if auto:
                sc, off, clp = auto_consts(value.astype(np.float64).tolist(), (~is_nd).tolist())
            value = (value + off).astype(np.float32)
            value = np.where(value > clp, clp, value)
            value = np.where(value < 0.0, f32(0.0), value)
            out = go_u8((value * sc).astype(np.float32))
        out[is_nd] = 0xFF
        return out.reshape(shape)
    T = d.dtype
    if T.type not in INT_TYPES:
        raise ValueError("Raster type not implemented")             # 329-331
    nd, off, clp = go_conv(nodata, T), go_conv(offset, T), go_conv(clip, T)
    is_nd = d == nd
    if auto:
        sc, df_offset, top = auto_consts(d.astype(np.float32).astype(np.float64).tolist(), (~is_nd).tolist())
        off, clp = go_conv(df_offset, T), go_conv(top, T)
    value = _wrap(d.astype(np.int64) + int(off), T)                 # value += offset, in T
    value = np.where(value > int(clp), int(clp), value)
    value = np.where(value < 0, 0, value)
    with np.errstate(all="ignore"):
        out = go_u8(value.astype(np.float32) * sc)
    out[is_nd] = 0xFF
    return out.reshape(shape)


def scale_legacy_rule(data, nodata, offset, scale, clip):
    """RasterScaler.Run (tile_scaler.go:17-112) -> uint8 array; a Byte raster
    is rewritten in place by the reference, the result is that raster."""
    data = np.asarray(data)
    d = np.ascontiguousarray(data).reshape(-1)
    with np.errstate(all="ignore"):
        if d.dtype == np.uint8:                                     # 22-41
            nd, clp = go_conv(nodata, np.uint8), go_conv(clip, np.uint8)
            value = np.minimum(d, clp)
            out = go_u8(value.astype(np.float64) * float(scale))
        elif d.dtype in (np.int16, np.uint16):                      # 43-83
            nd, clp = go_conv(nodata, d.dtype), go_conv(clip, d.dtype)
            value = np.maximum(np.minimum(d.astype(np.int64), int(clp)), 0)
            out = go_u8((value.astype(np.float32) * f32(254.0)).astype(np.float32) / f32(clp))
        elif d.dtype == np.float32:                                 # 85-109
            nd, sc, clp = f32(nodata), f32(scale), f32(clip)
            value = (d + f32(go_conv(offset, np.uint8))).astype(np.float32)
            value = np.where(value > clp, clp, value)
            value = np.where(value < 0, f32(0.0), value)
            out = go_u8((value * sc).astype(np.float32))
        else:
            raise ValueError("Raster type not implemented")
        out[d == nd] = 0xFF
    return out.reshape(data.shape)


# ---------------------------------------------------------------- cases
def safe_threshold():
    """(lo, hi): the largest float32 scale with float32(65535) * scale < 2^31
    and the next float32 above it -- the two sides of the band kernel's
    `safe` predicate for a UInt16 canvas under clip 65535."""
    s = f32(2.0 ** 31 / 65535.0)
    while f32(65535.0) * s >= 2147483648.0:
        s = np.nextafter(s, f32(0.0))
    while f32(65535.0) * np.nextafter(s, f32(INF)) < 2147483648.0:
        s = np.nextafter(s, f32(INF))
    return float(s), float(np.nextafter(s, f32(INF)))


SAFE_LO, SAFE_HI = safe_threshold()
# (offset, scale, clip, colour_scale)
INT_PARAMS = [(0, 0, 0), (0, 0, 1000), (1, 1, 1000), (3, 2, 2), (-5, 0.5, 300), (0, 0, 10000), (100.5, 0, 254),
              (0, 3.5, 0), (-1e3, 0, 70000), (0, 0, 762), (0, 0, 40000), (7, 0, -3), (-32768, 1, 65535),
              (1e10, 1, 1e10), (0, 1e7, 0), (0, 3e38, 40000), (0, INF, 5), (0, SAFE_LO, 65535), (0, SAFE_HI, 65535),
              (0, 1e7, 65535)]
INT_PARAMS = [(float(o), float(s), float(c), 0) for o, s, c in INT_PARAMS]
INT_NODATA = (0.0, -999.0, 255.0, 1e10, NAN, 65535.0)
SUBNORMAL = (0.0, 3e38, 1.0, 0)
FLOAT_PARAMS = INT_PARAMS[:17] + [INT_PARAMS[19], SUBNORMAL, (0.0, 1.0, 2.0, 1), (30.0, 0.0, 60.0, 1), (0.0, 0.0, 0.0, 1),
                                  (0.0, 0.0, 1000.0, 2), (0.0, 0.0, 0.0, 2)]
FLOAT_NODATA = (-9999.0, -9999.9, NAN, 0.0)
FSIDE = 48     # float32 data sets are FSIDE x FSIDE unless they are small auto-mode arrays


def domain(T):
    info = np.iinfo(T)
    return np.arange(info.min, info.max + 1, dtype=np.int64).astype(T)


@functools.lru_cache(None)
def int_datasets(T):
    """[(name, 2-D array, nodata)]: the whole domain as 256 x 256 (8-bit
    types: tiled 256 times) rolled so that element 0 is T(nodata) ("nd0") and
    so that T(nodata) is element 1 ("v0"), under every nodata; then the small
    auto-mode arrays."""
    T = np.dtype(T).type
    dom = domain(T)
    out = []
    for nd in INT_NODATA:
        at = int(np.nonzero(dom == go_conv(nd, T))[0][0])
        for name, shift in (("nd0", at), ("v0", at - 1)):
            a = np.roll(dom, -shift)
            out.append(("domain %s nodata %r" % (name, nd), np.tile(a, 65536 // a.size).reshape(256, 256).copy(), nd))
    nd = -999.0
    h = go_conv(nd, T)                         # the hole
    a, b = (T(17), T(40)) if h not in (17, 40) else (T(18), T(41))
    out.append(("auto all nodata", np.full((3, 5), h, T), nd))
    out.append(("auto one valid at 0", np.array([[a] + [h] * 6] * 1 + [[h] * 7] * 3, T), nd))
    out.append(("auto one valid elsewhere", np.array([[h] * 4, [h, h, b, h]], T), nd))
    out.append(("auto all equal", np.full((4, 4), a, T), nd))
    info = np.iinfo(T)
    out.append(("auto full range", np.array([[info.min, info.max, a, h, b, info.max, info.min, 0, 1]] * 2, T), nd))
    return out


def _mid(n, off, sc):
    """n valid mid-range values of a parameter set (bytes around 40..200)."""
    with np.errstate(all="ignore"):
        v = (np.linspace(40.0, 200.0, n) / np.float64(sc) - off).astype(np.float32)
    bad = ~np.isfinite(v) | (np.abs(v) > 1e30)
    v[bad] = np.linspace(1.0, 900.0, n).astype(np.float32)[bad]
    return v


def _pad(vals, off, sc, nd32, side=FSIDE):
    vals = np.asarray(vals, np.float32)
    assert vals.size <= side * side - 8, vals.size
    fill = _mid(side * side - vals.size, off, sc)
    fill[fill == nd32] = f32(123.0)
    # the specials in the middle, valid values at both ends (element 0 valid)
    out = np.concatenate([fill[:8], vals, fill[8:]])
    return out.reshape(side, side)


def _around(x):
    x = f32(x)
    return [np.nextafter(x, f32(-INF)), x, np.nextafter(x, f32(INF))]


def _specials(nd):
    nd32 = go_conv(nd, np.float32)
    tiny = np.finfo(np.float32).tiny
    s = [0.0, -0.0, tiny, -tiny, 1e-38, -1e-38, 3e38, -3e38, INF, -INF, NAN, nd32, f32(-9999.9), f32(-9999.0)]
    if np.isfinite(nd32):
        s += _around(nd32)
    return [f32(v) for v in s]


@functools.lru_cache(None)
def float_datasets():
    """[(name, 2-D float32 array, nodata)]."""
    out = []
    with np.errstate(all="ignore"):
        for p in FLOAT_PARAMS[:19]:
            off, scale, clip, _ = p
            if is_auto(off, scale, clip):
                continue
            sc = scale_const(scale, clip)
            b = (np.arange(256, dtype=np.float64) / np.float64(sc) - off).astype(np.float32)
            b = np.concatenate([np.nextafter(b, f32(-INF)), b, np.nextafter(b, f32(INF))])
            b = b[np.isfinite(b)]
            nd = -9999.0
            out.append(("boundaries of %r" % (p[:3],), _pad(np.concatenate([b, _specials(nd)]), off, sc, f32(nd)), nd))
    for nd in FLOAT_NODATA:
        out.append(("specials nodata %r" % nd, _pad(_specials(nd), 0.0, f32(0.254), go_conv(nd, np.float32)), nd))
    # colour scales: exact powers of ten and two, 0, negatives, around 1, +inf
    p10 = [f32(10.0) ** f32(k) for k in range(-30, 31)] + [f32(float("1e%d" % k)) for k in range(-30, 31)]
    p2 = [f32(2.0 ** k) for k in range(-40, 41)]
    logs = p10 + p2 + [0.0, -0.0, -1.0, -1e-30, -3e38] + _around(1.0) + _around(10.0) + [INF, -INF, NAN]
    for nd in (-9999.0, NAN, 2.0):       # 2.0: log10(100) equals the nodata after normalise()
        out.append(("log set nodata %r" % nd, _pad(logs + [f32(100.0)] + _specials(nd), -10.0, f32(0.1), go_conv(nd, np.float32)), nd))
    # auto mode, small arrays of different sizes
    nd, a = -9999.0, np.float32
    out.append(("auto element 0 NaN", np.array([[NAN, 1, 2, 3, 4]], a), nd))
    out.append(("auto NaN elsewhere", np.array([[1, NAN, 5], [NAN, 3, 2]], a), nd))
    out.append(("auto all NaN", np.full((2, 3), NAN, a), nd))
    out.append(("auto single +inf", np.array([[1, 2, INF, 4], [5, 6, 7, 8], [3, 3, 3, 3]], a), nd))
    out.append(("auto -inf and +inf", np.array([[1, -INF, INF, 4, 9, 2, 7]], a), nd))
    out.append(("auto element 0 zero", np.array([[0, 10, 100, 1000], [1, 5, 50, 500]], a), nd))
    out.append(("auto element 0 negative", np.array([[-3, 10, 100], [1000, 1, 5], [50, 500, 7]], a), nd))
    out.append(("auto all equal", np.full((5, 5), 42.5, a), nd))
    out.append(("auto all equal huge", np.full((2, 2), 3e38, a), nd))
    out.append(("auto element 0 nodata", np.array([[nd, 7, 9, 300, nd, 20]], a), nd))
    out.append(("auto NaN nodata NaN data", np.array([[NAN, 1, 2], [3, NAN, 4]], a), NAN))
    out.append(("auto NaN nodata NaN later", np.array([[5, NAN, 2], [3, NAN, 4]], a), NAN))
    return out


def datasets(T):
    return float_datasets() if np.dtype(T) == np.float32 else int_datasets(np.dtype(T).type)


def params(T):
    return FLOAT_PARAMS if np.dtype(T) == np.float32 else INT_PARAMS


@functools.lru_cache(None)
def expected(tname, k, p):
    """scale_rule of data set k of type `tname` under parameter set p, computed once."""
    _, data, nd = datasets(np.dtype(tname))[k]
    out = scale_rule(data, nd, *p)
    out.setflags(write=False)
    return out


LEGACY_TYPES = (np.uint8, np.int16, np.uint16, np.float32)

# Auto mode on the device reduces per wave of 64 with atomics across blocks of
# 256: positions of the single minimum and the single maximum among 1025
# elements -- first / last element, the last lane of a wave and the first of
# the next, either side of a block boundary, and the reverse orders.
EXTREMA = [(0, 1024), (1024, 0), (63, 64), (64, 63), (255, 256), (256, 255), (1, 1023), (511, 512), (1024, 1023)]


def extrema_array(T, at_min, at_max, n=1025):
    d = np.full(n, 500, T)
    d[2::7] = 600
    d[at_min], d[at_max] = -2000, 3000
    return d


# ---------------------------------------------------------------- checks of the rule
def test_conversions_by_hand():
    """The quirks tests/test_oracle_kats.py pins for the oracle, restated."""
    assert go_conv(300.0, np.uint8) == 44 and go_conv(1000.0, np.uint8) == 232
    assert go_conv(-1e10, np.int16) == 0 and go_conv(NAN, np.uint8) == 0 and go_conv(1e10, np.uint16) == 0
    assert go_conv(65535.0, np.int16) == -1 and go_conv(40000.0, np.int16) == -25536
    assert go_conv(-999.0, np.uint8) == 25 and go_conv(-3.0, np.uint16) == 65533 and go_conv(200.0, np.int8) == -56
    assert go_conv(-0.9, np.uint8) == 0 and go_conv(2147483647.9, np.uint8) == 255 and go_conv(2147483648.0, np.uint8) == 0
    got = go_u8(np.array([0.0, 255.9, 256.0, 300.0, -1.0, -0.5, 2147483520.0, 2147483648.0, -2147483648.0, NAN, INF], np.float32))
    assert got.tolist() == [0, 255, 0, 44, 255, 0, 128, 0, 0, 0, 0]


def test_log10_by_hand():
    x = np.array([1.0, 10.0, 100.0, 1e-30, 0.5, 8.0, 0.0, -1.0, INF, NAN])
    got = go_log10(x)
    assert got[:3].tolist() == [0.0, 1.0, 2.0] and got[6] == -INF and np.isnan(got[7]) and got[8] == INF and np.isnan(got[9])
    assert got[4] == -1 * 0.301029995663981195 and got[5] == 3 * 0.301029995663981195       # the frac == 0.5 branch
    assert abs(got[3] + 30.0) < 1e-13
    r = np.random.default_rng(1).uniform(1e-30, 1e30, 2000)
    assert np.max(np.abs(go_log10(r) - np.log10(r))) < 1e-13


@pytest.mark.parametrize("dt,data,sp,exp", SCALE_KATS)
def test_rule_reference_kats(dt, data, sp, exp):
    """The 18 cases of raster_scaler_test.go:18-151."""
    assert scale_rule(np.array(data, dt), 0.0, sp[0], sp[1], sp[2]).tolist() == exp


def test_rule_hand_derived_cases():
    """The hand-derived cases of tests/test_oracle_kats.py: the Byte clip
    wrap, nodata and the i == 0 quirk of auto mode, the log colour scale."""
    assert scale_rule(np.array([250, 10, 0], np.uint8), 0.0, 0.0, 1.0, 1000.0).tolist() == [232, 10, 0xFF]
    out = scale_rule(np.array([-9999, 100, 200], np.float32), -9999.0, 0, 0, 0)
    assert out.tolist() == [255, int(f32(100) * f32(254.0 / 200.0)), 254]
    out2 = scale_rule(np.array([50, 100, 200], np.int16), -9999.0, 0, 0, 0)
    assert out2[0] == 0 and out2[2] == 254
    out3 = scale_rule(np.array([1.0, 10.0, 100.0, 0.0, -1.0], np.float32), -9999.0, 0, 1.0, 2.0, colour_scale=1)
    assert out3.tolist() == [0, 1, 2, 255, 255]


def _of(T, name):
    return next((k, d, nd) for k, (n, d, nd) in enumerate(datasets(T)) if n == name)


def test_special_cases_do_what_they_are_for():
    """Each special case of the table, by hand."""
    u16, i16, u8 = np.dtype(np.uint16), np.dtype(np.int16), np.dtype(np.uint8)
    _, dom, _ = _of(u16, "domain v0 nodata -999.0")
    flat = dom.reshape(-1)
    at = lambda v: int(np.nonzero(flat == v)[0][0])
    # value * scale >= 2^31: Go's uint8(float32) gives 0 (the SAFE == false branch, go_u8_f32)
    # ((0, 1e7, 0) itself clamps every value to its clip of 0: all valid bytes 0, and `safe` holds)
    assert set(scale_rule(dom, -999.0, 0.0, 1e7, 0.0).reshape(-1).tolist()) == {0, 0xFF}
    out = scale_rule(dom, -999.0, 0.0, 1e7, 65535.0).reshape(-1)
    assert f32(214) * f32(1e7) < 2.0 ** 31 <= f32(215) * f32(1e7)
    assert out[at(213)] == (2130000000 & 0xFF) == 0x80 and out[at(214)] == (2140000000 & 0xFF)
    assert out[at(215)] == 0 and out[at(65535)] == 0
    assert (out[flat >= 215] == 0).sum() == 65535 - 215                 # all but the nodata 64537 (0xFF)
    # the two sides of the `safe` predicate
    assert f32(65535) * f32(SAFE_LO) < 2.0 ** 31 <= f32(65535) * f32(SAFE_HI)
    lo = scale_rule(dom, -999.0, 0.0, SAFE_LO, 65535.0).reshape(-1)
    hi = scale_rule(dom, -999.0, 0.0, SAFE_HI, 65535.0).reshape(-1)
    assert lo[at(65535)] == (int(f32(65535) * f32(SAFE_LO)) & 0xFF) and hi[at(65535)] == 0
    assert hi[at(65534)] == (int(f32(65534) * f32(SAFE_HI)) & 0xFF) and (lo != hi).sum() > 1000
    assert f32(65535) * f32(SAFE_HI) == 2.0 ** 31       # exactly on the bound: `<=` in the predicate would call it safe
    # clip 40000 wraps negative on Int16: every valid pixel is 0; nodata 65535 is -1
    _, d16, _ = _of(i16, "domain v0 nodata 65535.0")
    o = scale_rule(d16, 65535.0, 0.0, 0.0, 40000.0)
    assert go_conv(40000.0, np.int16) < 0 and (o[d16 == -1] == 0xFF).all() and (o[d16 != -1] == 0).all()
    assert d16.reshape(-1)[0] == -2 and d16.reshape(-1)[1] == -1
    # offset and clip 1e10 convert to 0 in every integer type: every valid pixel is 0
    for T in INT_TYPES:
        _, d, _ = datasets(T)[2]
        o = scale_rule(d, -999.0, 1e10, 1.0, 1e10)
        assert go_conv(1e10, T) == 0 and set(o.reshape(-1).tolist()) == {0, 0xFF}
    # 254 / 762 is no float32: one ulp in the constant moves bytes on multiples of 3
    sc = scale_const(0.0, 762.0)
    v = np.arange(0, 763, 3).astype(np.float32)
    assert float(sc) != 254.0 / 762.0
    assert (go_u8(v * sc) != go_u8(v * np.nextafter(sc, f32(0)))).any() or (go_u8(v * sc) != go_u8(v * np.nextafter(sc, f32(1)))).any()
    # +inf scale: 0 * inf = NaN -> 0, everything else inf -> 0
    assert set(scale_rule(dom, -999.0, 0.0, INF, 5.0).reshape(-1).tolist()) == {0, 0xFF}
    # Byte offsets wrap in uint8 and a negative clip wraps high
    o = scale_rule(np.array([250, 3], np.uint8), 0.0, 7.0, 0.0, -3.0)
    assert o.tolist() == [1, 10] and go_conv(-3.0, np.uint8) == 253
    # SignedByte: value += offset wraps in int8
    assert scale_rule(np.array([127, -128, 5], np.int8), -999.0, 3.0, 2.0, 2.0).tolist() == [0, 0, 4]
    # auto mode: all nodata -> min = max = 0, scale 254 / 0.1 = 2540
    k, d, nd = _of(u8, "auto all nodata")
    assert auto_consts(d.reshape(-1).astype(np.float64).tolist(), [False] * d.size)[0] == f32(2540.0)
    assert (scale_rule(d, nd, 0, 0, 0) == 0xFF).all()
    # one valid value elsewhere: min stays 0 (element 0 is nodata), one valid at 0: min = max = it
    k, d, nd = _of(i16, "auto one valid elsewhere")
    assert scale_rule(d, nd, 0, 0, 0).reshape(-1)[6] == 254
    k, d, nd = _of(i16, "auto one valid at 0")
    assert scale_rule(d, nd, 0, 0, 0).reshape(-1)[0] == 0
    # full Int16 range: offset -> -32768, clip -> -1, every valid byte 0
    k, d, nd = _of(i16, "auto full range")
    assert set(scale_rule(d, nd, 0, 0, 0).reshape(-1).tolist()) == {0, 0xFF}
    # float32: the subnormal survives (a flush-to-zero build gives 0)
    sub = scale_rule(np.array([1e-38], np.float32), -9999.0, *SUBNORMAL)
    assert f32(1e-38) < np.finfo(np.float32).tiny and sub[0] in (2, 3)
    # a nodata no float32 equals: its float32 is nodata by the first test, its neighbours are values
    x = f32(-9999.9)
    assert float(x) != -9999.9
    o = scale_rule(np.array(_around(x), np.float32), -9999.9, 10000.0, 1.0, 200.0)
    assert o.tolist() == [0, 0xFF, 0]
    # log scale: 0 -> -inf and negatives -> NaN are nodata; NaN nodata lets the NaN through as byte 0
    assert scale_rule(np.array([0, -1, 100, INF], np.float32), -9999.0, 0.0, 1.0, 2.0, 1).tolist() == [255, 255, 2, 255]
    assert scale_rule(np.array([0, -1, 100, INF], np.float32), NAN, 0.0, 1.0, 2.0, 1).tolist() == [0, 0, 2, 0]
    assert scale_rule(np.array([100, 10], np.float32), 2.0, 0.0, 1.0, 2.0, 1).tolist() == [255, 1]
    assert scale_rule(np.array([INF, -INF, NAN, 5], np.float32), -9999.0, 0.0, 1.0, 1000.0, 2).tolist() == [255, 255, 255, 5]
    # auto mode float32: NaN at element 0 makes every valid byte 0; NaN elsewhere is ignored
    assert scale_rule(np.array([NAN, 1, 2], np.float32), -9999.0, 0, 0, 0).tolist() == [0, 0, 0]
    assert scale_rule(np.array([1, NAN, 5], np.float32), -9999.0, 0, 0, 0).tolist() == [0, 0, 254]
    # element 0 unnormalisable under log: min starts at 0, not at log10(element 1)
    o = scale_rule(np.array([0, 10, 100], np.float32), -9999.0, 0, 0, 0, 1)
    assert o.tolist() == [255, 127, 254]


def test_boundary_sets_sit_on_boundaries():
    """Every float32 boundary set holds, for most bytes k, a value that scales
    to k - 1 next to one that scales to k."""
    for k, (name, data, nd) in enumerate(float_datasets()):
        if not name.startswith("boundaries of (0.0, 0.0, 1000.0"):
            continue
        out = scale_rule(data, nd, 0.0, 0.0, 1000.0).reshape(-1)
        steps = np.nonzero(np.diff(out[8:8 + 768].astype(int)[256:512]) == 1)[0]
        assert len(set(out.tolist())) >= 255 and len(steps) >= 250
        break
    else:
        raise AssertionError("boundary set not found")


def _types():
    return [np.dtype(t).name for t in INT_TYPES + (np.float32,)]


@pytest.mark.parametrize("tname", _types())
def test_rule_matches_oracle_on_the_table(oracle, tname):
    """oracle.scale on every (data set, parameter set) of the table:
    identical bytes, nothing left out."""
    T = np.dtype(tname)
    n = px = 0
    for k, (name, data, nd) in enumerate(datasets(T)):
        for p in params(T):
            exp = oracle.scale(data, nd, p[0], p[1], p[2], p[3])
            got = expected(tname, k, p)
            assert np.array_equal(got, exp), (tname, name, p, int((got != exp).sum()),
                                              np.nonzero(got.reshape(-1) != exp.reshape(-1))[0][:5].tolist())
            n += 1
            px += data.size
    assert n == len(datasets(T)) * len(params(T))
    print("\n[scale_rule] %s: %d cases, %d pixels, rule == oracle" % (tname, n, px))


@pytest.mark.parametrize("tname", [np.dtype(t).name for t in LEGACY_TYPES])
def test_legacy_rule_matches_oracle_on_the_table(oracle, tname):
    T = np.dtype(tname)
    n = 0
    for name, data, nd in datasets(T):
        for p in params(T):
            exp = oracle.scale_legacy(data, nd, p[0], p[1], p[2])
            got = scale_legacy_rule(data, nd, p[0], p[1], p[2])
            assert np.array_equal(got, exp), (tname, name, p, int((got != exp).sum()))
            n += 1
    assert n == len(datasets(T)) * len(params(T))


def test_legacy_by_hand():
    assert scale_legacy_rule(np.array([7, 200, 9], np.uint8), 7.0, 0.0, 1.5, 100.0).tolist() == [255, 150, 13]
    assert scale_legacy_rule(np.array([-5, 50, 100, 300], np.int16), -999.0, 0.0, 9.0, 100.0).tolist() == [0, 127, 254, 254]
    assert scale_legacy_rule(np.array([50, 65535], np.uint16), 0.0, 0.0, 9.0, 100.0).tolist() == [127, 254]
    # Float32: the offset goes through uint8 (300 -> 44)
    assert scale_legacy_rule(np.array([1.5, -100], np.float32), -9999.0, 300.0, 2.0, 1000.0).tolist() == [91, 0]


def test_extrema_arrays_hold_one_minimum_and_one_maximum():
    for T in (np.int16, np.float32):
        for at_min, at_max in EXTREMA:
            d = extrema_array(T, at_min, at_max)
            assert (d == d.min()).sum() == 1 and (d == d.max()).sum() == 1
            assert int(np.argmin(d)) == at_min and int(np.argmax(d)) == at_max
            out = scale_rule(d, -999.0, 0, 0, 0)
            # element 0 is valid, so min and max are the array's own
            assert out[at_min] == 0 and out[at_max] == 254 and 0 < out[500] < 254
