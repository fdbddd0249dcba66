"""Overview pyramids (gskyhip_overview_levels / gskyhip_build_overviews), CPU
part: level sizes, argument checks that return before any HIP call, and the
numpy reference pyramid the GPU tests compare against bit for bit.

The reference below is written from the rules in include/gskyhip.h alone (a
plain loop over levels, four strided views per level); it shares no code with
the library.  No kernel is launched in this file."""
import ctypes as C

import numpy as np
import pytest

from gsky_amd import _lib, ingest

MAX_OVR = 12


# ---------------------------------------------------------------- reference
def ref_levels(xsize, ysize, min_size=256):
    if min_size <= 0:
        min_size = 256
    out = []
    w, h = xsize, ysize
    while max(w, h) > min_size and len(out) < MAX_OVR:
        w, h = -(-w // 2), -(-h // 2)
        out.append((w, h))
    return out


def typed_nodata(nodata, dtype):
    """The nodata double as the warp's window fill writes it for the type
    (GDALCopyWords: round half away from zero and clamp; an int8 band is a
    Byte band, clamped to 0..255 and then read as int8)."""
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        return np.float32(nodata)
    lo, hi = (0, 255) if dtype.itemsize == 1 else (np.iinfo(dtype).min, np.iinfo(dtype).max)
    r = int(np.trunc(min(max(nodata + 0.5 if nodata >= 0 else nodata - 0.5, lo), hi)))
    if dtype == np.int8:
        return np.array([r], np.uint8).view(np.int8)[0]
    return dtype.type(r)


def ref_level(a, nodata, method):
    """One level from the one before (stored, typed values)."""
    h, w = a.shape
    oh, ow = -(-h // 2), -(-w // 2)
    if method == "nearest":
        return np.ascontiguousarray(a[::2, ::2])
    is_f = a.dtype == np.float32
    nd = typed_nodata(nodata, a.dtype) if nodata is not None else None
    acc = np.zeros((oh, ow), np.float32 if is_f else np.int64)
    cnt = np.zeros((oh, ow), np.int64)
    with np.errstate(all="ignore"):
        for dy in (0, 1):            # row-major box order
            for dx in (0, 1):
                sub = a[dy::2, dx::2]
                sh, sw = sub.shape   # clipped to the extent
                valid = np.ones(sub.shape, bool)
                if nd is not None:
                    valid &= sub != nd
                if is_f:
                    valid &= ~np.isnan(sub)
                    acc[:sh, :sw] = np.where(valid, acc[:sh, :sw] + sub, acc[:sh, :sw])   # float32 adds
                else:
                    acc[:sh, :sw] += np.where(valid, sub, 0).astype(np.int64)
                cnt[:sh, :sw] += valid
        if is_f:
            empty = nd if nd is not None else np.float32("nan")
            out = np.where(cnt > 0, acc / cnt.astype(np.float32), empty).astype(np.float32)
        else:
            c = np.maximum(cnt, 1)
            q = (2 * np.abs(acc) + c) // (2 * c)            # half away from zero, integers only
            out = np.where(cnt > 0, np.sign(acc) * q, nd if nd is not None else 0).astype(a.dtype)
    return out


def ref_pyramid(a, nodata=None, method="nearest", min_size=256):
    out, cur = [], a
    for (w, h) in ref_levels(a.shape[1], a.shape[0], min_size):
        cur = ref_level(cur, nodata, method)
        assert cur.shape == (h, w) and cur.dtype == a.dtype
        out.append(cur)
    return out


# ---------------------------------------------------------------- level sizes
def test_overview_levels():
    assert ingest.overview_levels(4000, 4000, 256) == [(2000, 2000), (1000, 1000), (500, 500), (250, 250)]
    assert ingest.overview_levels(4000, 4000) == ingest.overview_levels(4000, 4000, 256)
    assert ingest.overview_levels(1, 1, 1) == [] and ingest.overview_levels(1, 1) == []
    assert ingest.overview_levels(3, 5, 1) == [(2, 3), (1, 2), (1, 1)]
    # 2^20 needs 20 halvings to reach 1: capped at 12
    lv = ingest.overview_levels(1 << 20, 7, 1)
    assert len(lv) == 12 and lv[-1] == (1 << 8, 1) and lv[0] == (1 << 19, 4)
    for ms in (0, -5):   # <= 0 means 256
        assert ingest.overview_levels(1000, 300, ms) == [(500, 150), (250, 75)]
    assert ingest.overview_levels(256, 256) == [] and ingest.overview_levels(257, 1) == [(129, 1)]
    for args in ((0, 5, 1), (5, -1, 1)):
        with pytest.raises(_lib.GskyError):
            ingest.overview_levels(*args)
    # the reference's own sizes
    for (w, h, ms) in ((4000, 4000, 256), (3, 5, 1), (129, 257, 1), (7, 1031, 1), (1 << 20, 7, 1), (1000, 300, 0)):
        assert ingest.overview_levels(w, h, ms) == ref_levels(w, h, ms)


def test_overview_levels_count_only():
    L = _lib.lib()
    assert L.gskyhip_overview_levels(4000, 4000, 256, None, None) == 4


# ---------------------------------------------------------------- argument checks (no HIP call)
def _build(dtype=_lib.INT16, method=_lib.OVR_AVERAGE, n=2, sizes=((3, 2), (2, 1)), xsize=5, ysize=3, src=0x1000,
           outs=(0x2000, 0x3000), sb=0, null_arrays=False):
    """gskyhip_build_overviews with made-up device addresses: every call here
    must return from the argument checks, before any HIP call."""
    L = _lib.lib()
    m = max(1, len(sizes), len(outs))
    ptrs = (C.c_void_p * m)(*outs)
    xs = (C.c_int32 * m)(*[w for w, _ in sizes])
    ys = (C.c_int32 * m)(*[h for _, h in sizes])
    if null_arrays:
        ptrs = xs = ys = None
    return L.gskyhip_build_overviews(C.c_void_p(src), dtype, sb, xsize, ysize, 1, -999.0, method, n, ptrs, xs, ys, None)


def test_build_overviews_argument_errors():
    E_ARG, E_TYPE = -1, -2
    assert _build(method=2) == E_ARG and _build(method=-1) == E_ARG
    twelve = ref_levels(1 << 20, 1 << 20, 1)
    assert len(twelve) == 12
    assert _build(n=13, xsize=1 << 20, ysize=1 << 20, sizes=twelve + [(128, 128)], outs=(0x2000,) * 13) == E_ARG
    assert _build(n=-1) == E_ARG
    assert _build(sizes=((2, 2), (1, 1))) == E_ARG          # floor instead of ceil
    assert _build(sizes=((3, 2), (1, 1))) == E_ARG          # second level wrong
    assert _build(sizes=((2, 3), (1, 2))) == E_ARG          # axes swapped
    assert _build(src=0) == E_ARG                           # null source
    assert _build(outs=(0x2000, 0)) == E_ARG                # null level
    assert _build(null_arrays=True) == E_ARG
    assert _build(xsize=0) == E_ARG
    for dt in (_lib.FLOAT64, _lib.UINT32, _lib.INT32):
        assert _build(dtype=dt) == E_TYPE
    assert _build(dtype=0) == E_ARG and _build(dtype=9) == E_ARG


def test_python_keyword_errors():
    with pytest.raises(ValueError):
        _lib.ovr_method("mode")
    assert _lib.ovr_method("nearest") == 0 and _lib.ovr_method("average") == 1
    from gsky_amd.service import WarpService
    svc = WarpService("/nonexistent/gskyhip.sock", start=False)
    a = np.zeros((4, 4), np.int16)
    with pytest.raises(ValueError):
        svc.register_granule("p", 1, a, [0, 1, 0, 0, 0, -1], overviews=[a[::2, ::2]], build_overviews="nearest")
    with pytest.raises(ValueError):
        svc.register_granule("p", 1, a, [0, 1, 0, 0, 0, -1], build_overviews="cubic")


# ---------------------------------------------------------------- the reference on hand-worked cases
def test_reference_typed_nodata():
    assert typed_nodata(-999.0, np.int16) == -999 and typed_nodata(-1e10, np.int16) == -32768
    assert typed_nodata(-1.0, np.uint8) == 0 and typed_nodata(255.4, np.uint8) == 255
    assert typed_nodata(200.0, np.int8) == -56 and typed_nodata(-1.0, np.int8) == 0
    assert typed_nodata(65535.0, np.uint16) == 65535 and typed_nodata(2.5, np.uint16) == 3
    assert typed_nodata(-2.5, np.int16) == -3
    assert typed_nodata(-999.0, np.float32) == np.float32(-999.0)


def test_reference_nearest():
    a = np.arange(15, dtype=np.int16).reshape(3, 5)
    lv = ref_pyramid(a, None, "nearest", 1)
    assert [x.shape for x in lv] == [(2, 3), (1, 2), (1, 1)]
    assert lv[0].tolist() == [[0, 2, 4], [10, 12, 14]] and lv[1].tolist() == [[0, 4]] and lv[2].tolist() == [[0]]
    # level k (i, j) is level-0 (i * 2^k, j * 2^k)
    b = np.arange(129 * 67, dtype=np.uint16).reshape(129, 67)
    for k, x in enumerate(ref_pyramid(b, 5.0, "nearest", 1), 1):
        assert np.array_equal(x, b[::1 << k, ::1 << k])


def test_reference_average_rounding_int():
    def one(vals, dt=np.int16, nodata=None):
        return ref_level(np.array(vals, dt).reshape(2, 2), nodata, "average")[0, 0]
    assert one([-1, -2, 0, 0]) == -1          # -3/4 = -0.75 -> -1
    assert one([-3, 0, 0, -3]) == -2          # -6/4 = -1.5 -> -2
    assert one([1, 2, 3, 0]) == 2             # 6/4 = 1.5 -> 2
    assert one([5, 0, 0, 0]) == 1             # 5/4 = 1.25 -> 1
    assert one([-5, 0, 0, 0]) == -1
    # sum / count with nodata out of the count: -3/2 -> -2, 3/2 -> 2, 5/4 -> 1
    assert one([-1, -2, -999, -999], nodata=-999.0) == -2
    assert one([1, 2, -999, -999], nodata=-999.0) == 2
    assert one([2, 1, 1, 1]) == 1
    assert one([7, -999, 0, 0], nodata=-999.0) == 2      # 7/3 = 2.33 -> 2
    assert one([8, 0, -999, 0], nodata=-999.0) == 3      # 8/3 = 2.67 -> 3
    assert one([65535] * 4, np.uint16) == 65535           # 4 x 65535 does not overflow
    assert one([65535, 65535, 65534, 65534], np.uint16) == 65535   # .5 -> up
    assert one([255, 255, 255, 254], np.uint8) == 255
    assert one([-128, -128, -128, -127], np.int8) == -128
    # one valid pixel returns that pixel; none returns nodata
    assert one([-999, -999, 123, -999], nodata=-999.0) == 123
    assert one([-999] * 4, nodata=-999.0) == -999
    assert one([200, 200, 200, 17], np.uint8, nodata=200.0) == 17
    assert one([-56, -56, -56, -56], np.int8, nodata=200.0) == -56   # int8 nodata 200 -> bits 0xc8


def test_reference_average_3x3_and_cascade():
    a = np.array([[1, 2, 10], [3, 4, 20], [100, 101, 7]], np.int16)
    l1 = ref_level(a, None, "average")
    # boxes clipped to the extent: (1+2+3+4)/4 = 2.5 -> 3, (10+20)/2, (100+101)/2 = 100.5 -> 101, 7
    assert l1.tolist() == [[3, 15], [101, 7]]
    lv = ref_pyramid(a, None, "average", 1)
    assert [x.tolist() for x in lv] == [[[3, 15], [101, 7]], [[32]]]    # 126/4 = 31.5 -> 32: from the rounded level
    # nodata in the corner boxes
    b = a.copy()
    b[0, 0] = b[2, 2] = -999
    assert ref_level(b, -999.0, "average").tolist() == [[3, 15], [101, -999]]


def test_reference_average_float():
    nan = np.float32("nan")
    a = np.array([[1.5, nan], [nan, 2.25]], np.float32)
    assert ref_level(a, None, "average")[0, 0] == np.float32(1.875)
    allnan = np.full((2, 2), nan, np.float32)
    r = ref_level(allnan, None, "average")
    assert r.view(np.uint32)[0, 0] == 0x7FC00000          # no nodata value: the quiet NaN
    assert ref_level(allnan, -999.0, "average")[0, 0] == np.float32(-999.0)
    mixed = np.array([[nan, -999.0], [-999.0, nan]], np.float32)
    assert ref_level(mixed, -999.0, "average")[0, 0] == np.float32(-999.0)
    # fp32 sum in box order, one division: (0.1f + 0.2f + 0.3f) / 3f
    v = np.array([[0.1, 0.2], [0.3, -999.0]], np.float32)
    exp = ((np.float32(0.0) + v[0, 0] + v[0, 1]) + v[1, 0]) / np.float32(3.0)
    got = ref_level(v, -999.0, "average")[0, 0]
    assert got.dtype == np.float32 and got == exp
    # a 3 x 3 float with a clipped NaN column
    f = np.array([[1, 2, nan], [3, 4, nan], [5, nan, 9]], np.float32)
    r = ref_level(f, None, "average")
    assert r[0, 0] == 2.5 and np.isnan(r[0, 1]) and r[1, 0] == 5 and r[1, 1] == 9
