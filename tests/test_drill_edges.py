"""Edge cases of the WPS drill: the zonal reduction (csrc/drill.hip) and the
decile selection (csrc/drill_deciles.hip) against a plain numpy restatement
of the reference, written here from worker/gdalprocess/drill.go:128-273 and
processor/drill_merger.go:79-93 (not from oracle/ and not from the kernels).

The inputs sit where the kernels branch: in-mask counts on every unroll, tile,
segment and cache boundary, band lists around the 32- and 64-band groups, more
than 1024 polygons (the carries of the two scans), special float values, mask
bytes other than 0 / 255, windows outside the stack, and the key distributions
that drive the select's range refinement.

Two tests run without a GPU: the restatement against oracle/ (a second
reading of drill.go by another route) on every NaN-free input used below, and
the wave-split restatement against the sequential one under the 1e-5 bar.

Comparisons (ISSUE "Common rules"): reference-order means NaN at the same
places and otherwise bit-equal as float64, counts equal; deciles equal as
float32 under == (Go's sort may leave -0.0 and +0.0 in either order), Count 1;
wave split counts exact and means within 1e-5 relative -- and, more sharply,
bit-equal to the wave-split restatement (float32 partials over 1024-pixel
segments of the compacted list, combined in float64 in segment order).
"""
from __future__ import annotations

import functools
import math
from collections import namedtuple

import numpy as np
import pytest

F32 = np.float32
FLT_MAX = float(np.finfo(np.float32).max)
NOCLIP = (-FLT_MAX, FLT_MAX)
REFERENCE_ORDER, WAVE_SPLIT = 0, 1
SEG = 1024            # pixels per wave-split segment
WAVE_SPLIT_BAR = 1e-5


# ======================================================================
# 1. The reference: drill.go:128-273 and drill_merger.go:79-93 in numpy
# ======================================================================
class RefPanic(Exception):
    """The reference indexes past a slice (or divides by zero) and panics."""


def _f32sum(x):
    """Strictly sequential float32 sum from 0 (drill.go:150, 164)."""
    if x.size == 0:
        return F32(0)
    with np.errstate(all="ignore"):
        return np.add.accumulate(x, dtype=np.float32)[-1]


def _select(v, mask, nodata, lo, hi):
    """drill.go:154, 160: keep = in the mask and not nodata; inc = keep and
    inside the clip -- float32 comparisons (numpy's have Go's NaN rules)."""
    with np.errstate(invalid="ignore"):
        keep = (mask == 255) & (v != F32(nodata))
        inc = keep & ~((v < F32(lo)) | (v > F32(hi)))
    return keep, inc


def ref_mean(v, mask, nodata, lo, hi, pixel_count):
    """drill.go:150-177 of one band: v, mask flat over the window in row-major
    order -> (Value float64, Count)."""
    keep, inc = _select(v, mask, nodata, lo, hi)
    if pixel_count == 0:
        total, s = int(inc.sum()), _f32sum(v[inc])
    else:
        total, s = int(keep.sum()), F32(int(inc.sum()))   # sum += 1.0 per included pixel: exact below 2^24
    if total <= 0:
        return 0.0, 0
    with np.errstate(all="ignore"):
        return float(F32(s) / F32(total)), total


def ref_mean_wave_split(v, mask, nodata, lo, hi, pixel_count):
    """The wave-split order: float32 partial sums over consecutive
    1024-pixel segments of the compacted in-mask list, combined in float64 in
    segment order, then float32(sum) / float32(total)."""
    sel = mask == 255
    vv = v[sel]
    acc, total = 0.0, 0
    for k0 in range(0, vv.size, SEG):
        seg = vv[k0:k0 + SEG]
        keep, inc = _select(seg, np.full(seg.size, 255, np.uint8), nodata, lo, hi)
        if pixel_count == 0:
            part, n = _f32sum(seg[inc]), int(inc.sum())
        else:
            part, n = F32(int(inc.sum())), int(keep.sum())
        with np.errstate(all="ignore"):
            acc += float(part)
        total += n
    if total <= 0:
        return 0.0, 0
    with np.errstate(all="ignore"):
        return float(F32(acc) / F32(total)), total


def ref_deciles(v, mask, nodata, dc):
    """computeDeciles (drill.go:229-273): float32 (dc,); RefPanic where the
    reference indexes buf[len] (len == dc + 1) or takes i % 0."""
    keep, _ = _select(v, mask, nodata, 0.0, 0.0)
    buf = np.sort(v[keep])
    n = int(buf.size)
    out = np.zeros(dc, np.float32)
    step = n // (dc + 1)
    if step > 0:
        even = n % (dc + 1) == 0
        for i in range(dc):
            j = (i + 1) * step
            if even:
                if j + 1 >= n:
                    raise RefPanic("buf[%d] of %d" % (j + 1, n))
                with np.errstate(all="ignore"):
                    out[i] = (buf[j] + buf[j + 1]) / F32(2.0)
            else:
                out[i] = buf[j]
    else:
        if n == 0:
            raise RefPanic("i % len(buf) with len 0")
        padding = np.bincount(np.arange(dc) % n, minlength=n)   # drill.go:254-261
        out[:] = np.repeat(buf, padding)
    return out


def go_round(x):
    """math.Round: half away from zero."""
    return math.copysign(math.floor(abs(x) + 0.5), x)


def ref_rows(cell, bands, strides, dc):
    """drill.go:128-219: the TimeSeries rows of one polygon.  cell(b) gives
    the nCols (Value, Count) of 1-based band b as two lists."""
    if strides <= 0:
        strides = 1
    nc = 1 + dc
    vals, cnts = [], []
    for ib in range(0, len(bands), strides):
        ie = min(ib + strides, len(bands))
        read = [bands[ib], bands[ie - 1]]
        if strides == 1:
            read = read[:1]
        bound = [cell(b) for b in read]
        vals.append(bound[0][0])
        cnts.append(bound[0][1])
        if strides > 2 and len(bound) > 1:
            with np.errstate(all="ignore"):
                beta = [float((np.float64(bound[1][0][ic]) - np.float64(bound[0][0][ic])) / np.float64(strides - 1))
                        for ic in range(nc)]
                count = [go_round(float(bound[0][1][ic] + bound[1][1][ic]) / 2.0) for ic in range(nc)]
                for ip in range(1, strides - 1):
                    vals.append([float(np.float64(bound[0][0][ic]) + np.float64(ip) * np.float64(beta[ic]))
                                 for ic in range(nc)])
                    cnts.append([int(count[ic]) for ic in range(nc)])
        if len(bound) > 1:
            vals.append(bound[1][0])
            cnts.append(bound[1][1])
    return np.array(vals, np.float64).reshape(-1, nc), np.array(cnts, np.int32).reshape(-1, nc)


def ref_merge(values, counts):
    """drill_merger.go:79-93 per date; NaN = no value."""
    v = np.asarray(values, np.float64)
    c = np.asarray(counts, np.int32)
    out = np.full(v.shape[1], np.nan)
    for d in range(v.shape[1]):
        total, count = np.float64(0.0), 0
        for f in range(v.shape[0]):
            if not np.isnan(v[f, d]):
                with np.errstate(all="ignore"):
                    total = total + v[f, d] * np.float64(int(c[f, d]))
                count += int(c[f, d])
        if not np.isnan(total) and count > 0:
            out[d] = total / np.float64(count)
    return out


# ======================================================================
# Cases: a stack, polygon windows and the calls the GPU tests make
# ======================================================================
Call = namedtuple("Call", "clip pc strides dc bands mode", defaults=(NOCLIP, 0, 1, 0, None, REFERENCE_ORDER))


class Case:
    """One stack with its polygon windows, and the reference's answers."""

    def __init__(self, name, data, nodata, windows, masks, labels=None):
        self.name = name
        self.data = np.ascontiguousarray(data, np.float32)
        self.nodata = float(nodata)
        self.windows = [tuple(int(x) for x in w) for w in windows]
        self.masks = [np.ascontiguousarray(m, np.uint8) for m in masks]
        self.labels = labels or ["poly %d" % i for i in range(len(windows))]
        self._win, self._mean, self._dec = {}, {}, {}

    # the window clipped to the stack, in row-major order (ISSUE "Pixel selection")
    def clipped(self, p):
        if p not in self._win:
            nb, H, W = self.data.shape
            x0, y0, w, h = self.windows[p]
            xa, ya, xb, yb = max(0, x0), max(0, y0), min(W, x0 + w), min(H, y0 + h)
            if w <= 0 or h <= 0 or xa >= xb or ya >= yb:
                self._win[p] = (np.zeros((nb, 0, 0), np.float32), np.zeros((0, 0), np.uint8))
            else:
                m = self.masks[p].reshape(h, w)[ya - y0:yb - y0, xa - x0:xb - x0]
                self._win[p] = (self.data[:, ya:yb, xa:xb], m)
        return self._win[p]

    def mean(self, p, b, clip, pc, mode=REFERENCE_ORDER):
        key = (p, b, F32(clip[0]).tobytes(), F32(clip[1]).tobytes(), pc, mode)
        if key not in self._mean:
            sub, m = self.clipped(p)
            f = ref_mean_wave_split if mode == WAVE_SPLIT else ref_mean
            self._mean[key] = f(sub[b].reshape(-1), m.reshape(-1), self.nodata, clip[0], clip[1], pc)
        return self._mean[key]

    def deciles(self, p, b, dc):
        key = (p, b, dc)
        if key not in self._dec:
            sub, m = self.clipped(p)
            try:
                self._dec[key] = ref_deciles(sub[b].reshape(-1), m.reshape(-1), self.nodata, dc)
            except RefPanic:
                self._dec[key] = None
        if self._dec[key] is None:
            raise RefPanic()
        return self._dec[key]

    def band_list(self, call):
        return list(call.bands) if call.bands is not None else list(range(1, self.data.shape[0] + 1))

    def expect_poly(self, p, call):
        """(values (rows, nCols) float64, counts int32) of polygon p; RefPanic."""
        def cell(b):
            v, c = self.mean(p, b - 1, call.clip, call.pc, call.mode)
            rv, rc = [v], [c]
            if call.dc > 0:
                if c > 0:   # drill.go:179-191
                    rv += [float(x) for x in self.deciles(p, b - 1, call.dc)]
                    rc += [1] * call.dc
                else:
                    rv += [0.0] * call.dc
                    rc += [0] * call.dc
            return rv, rc
        return ref_rows(cell, self.band_list(call), call.strides, call.dc)

    def expect(self, call):
        """All polygons: (values, counts, panics) shaped as read_data's."""
        vs, cs, panics = [], [], []
        for p in range(len(self.windows)):
            try:
                v, c = self.expect_poly(p, call)
            except RefPanic:
                panics.append(p)
                v = c = None
            vs.append(v)
            cs.append(c)
        if panics:
            return None, None, panics
        v, c = np.stack(vs), np.stack(cs)
        if call.dc == 0:
            v, c = v[..., 0], c[..., 0]
        return v, c, panics


def row_mask(n, k, rng):
    """A 1-row window mask of width n + k with exactly n bytes 255: k zeros at
    scattered positions, so the compaction has work to do."""
    m = np.full(n + k, 255, np.uint8)
    if k:
        m[rng.choice(n + k, k, replace=False)] = 0
    return m.reshape(1, n + k)


# ---------------------------------------------------------------- sizes
SIZES_N = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049)
SIZES_LISTS = (1, 31, 32, 33, 63, 64, 65, 129)
SIZES_MODES = ((0, NOCLIP), (1, (0.3, 0.8)))   # (pixel_count, clip)


def band_list(length, nb=129):
    """Odd lengths: random 1-based bands with repeats; even: reversed order."""
    if length % 2:
        return [int(b) for b in np.random.default_rng(1000 + length).integers(1, nb + 1, length)]
    return [int(b) for b in (np.arange(length)[::-1] * 2) % nb + 1]


@functools.lru_cache(None)
def case_sizes():
    """129 bands x 3 rows x 2112 columns, uniform in [0.1, 1] (the wave-split
    family: one sign, nothing cancels), nodata -9999 at 2 % right of column
    200; one polygon per n in SIZES_N as a 1-row window of width n + k.  The
    polygons below 63 pixels lie left of column 200, so their lengths are
    exactly n (never decile_count + 1 = 10)."""
    rng = np.random.default_rng(20240611)
    nb, H, W = 129, 3, 2112
    data = rng.uniform(0.1, 1.0, (nb, H, W)).astype(np.float32)
    nd = rng.random((nb, H, W)) < 0.02
    nd[:, :, :200] = False
    data[nd] = -9999.0
    wins, masks, labels = [], [], []
    for i, n in enumerate(SIZES_N):
        k = 3 + (5 * i) % 11
        w = n + k
        hi = (200 if n < 63 else W) - w
        wins.append((int(rng.integers(0, hi + 1)), i % 3, w, 1))
        masks.append(row_mask(n, k, rng))
        labels.append("n=%d" % n)
    return Case("sizes", data, -9999.0, wins, masks, labels)


# ---------------------------------------------------------------- many polygons
@functools.lru_cache(None)
def case_many(max_count):
    """2050 polygons (two carries of the 1024-polygon scan rounds) of 0 to
    max_count in-mask pixels in 3 x 2 windows, empty masks among them; values
    of the wave-split family, nodata in band 2 only."""
    rng = np.random.default_rng(77 + max_count)
    nb, H, W = 3, 64, 64
    data = rng.uniform(0.1, 1.0, (nb, H, W)).astype(np.float32)
    data[1][rng.random((H, W)) < 0.1] = -9999.0
    wins, masks = [], []
    for i in range(2050):
        cnt = int(rng.integers(0, max_count + 1))
        m = np.zeros(6, np.uint8)
        m[rng.choice(6, cnt, replace=False)] = 255
        wins.append((int(rng.integers(0, W - 3)), int(rng.integers(0, H - 2)), 3, 2))
        masks.append(m.reshape(2, 3))
    return Case("many%d" % max_count, data, -9999.0, wins, masks)


# ---------------------------------------------------------------- special values
SPECIAL_BANDS = ("plus_inf", "minus_inf", "nan", "both_inf", "flt_max_twice", "zeros", "subnormals", "all_nodata")
SPECIAL_NODATA = {"m9999": -9999.0, "zero": 0.0, "nan": float("nan"), "plus_inf": float("inf")}
SPECIAL_CLIPS = {"none": NOCLIP, "inf_bounds": (float("-inf"), float("inf")), "lo_eq_hi": (0.5, 0.5),
                 "lo_gt_hi": (0.75, 0.25), "nan_lo": (float("nan"), 0.6), "nan_hi": (0.4, float("nan")),
                 "nan_both": (float("nan"), float("nan"))}


@functools.lru_cache(None)
def case_special(nd_name):
    """A 16 x 16 window in a 20 x 22 stack, one scenario per band (see
    SPECIAL_BANDS); every band holds some nodata values, several exact 0.5
    (the lo == hi clip) and, for nodata 0.0, values of -0.0."""
    nodata = SPECIAL_NODATA[nd_name]
    rng = np.random.default_rng(5)
    H, W = 20, 22
    data = np.zeros((len(SPECIAL_BANDS), H, W), np.float32)
    for b, name in enumerate(SPECIAL_BANDS):
        v = rng.uniform(0.0, 1.0, (H, W)).astype(np.float32)
        flat = v.reshape(-1)
        pos = rng.permutation(flat.size)
        flat[pos[:9]] = 0.5
        if name == "plus_inf":
            flat[pos[9:12]] = np.inf
        elif name == "minus_inf":
            flat[pos[9:12]] = -np.inf
        elif name == "nan":
            flat[pos[9:11]] = np.nan
        elif name == "both_inf":
            flat[pos[9:15]] = np.inf
            flat[pos[15:21]] = -np.inf
        elif name == "flt_max_twice":
            flat[pos[9:40]] = FLT_MAX
        elif name == "zeros":
            flat[:] = np.where(rng.random(flat.size) < 0.5, F32(0.0), F32(-0.0))
        elif name == "subnormals":
            flat[:] = rng.choice(np.array([1e-40, 3e-41, -1e-40, 1.4e-45], np.float32), flat.size)
        elif name == "all_nodata":
            flat[:] = nodata
        if name not in ("zeros", "all_nodata"):
            if nodata == nodata:   # (NaN nodata values would poison every band: it excludes nothing)
                flat[pos[40:52]] = nodata
            flat[pos[52:58]] = -0.0
        data[b] = v
    mask = np.full((16, 16), 255, np.uint8)
    mask[rng.random((16, 16)) < 0.1] = 0
    return Case("special_" + nd_name, data, nodata, [(3, 2, 16, 16)], [mask])


# ---------------------------------------------------------------- masks and windows
@functools.lru_cache(None)
def case_maskwin():
    """A 24 x 31 stack of 5 bands; the windows are named in `labels`."""
    rng = np.random.default_rng(11)
    H, W = 24, 31
    data = rng.normal(0.0, 3.0, (5, H, W)).astype(np.float32)
    data[rng.random(data.shape) < 0.05] = -9999.0
    wm = []

    def add(label, win, mask=None):
        w, h = win[2], win[3]
        if mask is None:
            mask = rng.choice(np.array([0, 1, 127, 254, 255], np.uint8), (max(h, 0), max(w, 0)),
                              p=[0.1, 0.1, 0.1, 0.1, 0.6])
        wm.append((label, win, mask))
    add("mask bytes {0,1,127,254,255}", (4, 3, 13, 11))
    add("mask all zero", (2, 2, 7, 5), np.zeros((5, 7), np.uint8))
    add("mask all 255", (9, 8, 7, 5), np.full((5, 7), 255, np.uint8))
    add("mask all 254", (9, 8, 7, 5), np.full((5, 7), 254, np.uint8))
    add("1 x 1", (30, 23, 1, 1), np.full((1, 1), 255, np.uint8))
    add("1 x 1 masked out", (0, 0, 1, 1), np.full((1, 1), 1, np.uint8))
    add("1 x n", (1, 5, 29, 1))
    add("n x 1", (6, 1, 1, 22))
    add("outside left", (-9, 4, 8, 6))
    add("outside right", (31, 4, 8, 6))
    add("outside above", (5, -7, 8, 6))
    add("outside below", (5, 24, 8, 6))
    add("beyond the corner", (40, 30, 5, 5))
    add("beyond the far corner", (-20, -20, 5, 5))
    add("straddles left", (-4, 6, 9, 7))
    add("straddles right", (26, 6, 9, 7))
    add("straddles top", (8, -3, 9, 7))
    add("straddles bottom", (8, 20, 9, 7))
    add("straddles top-left corner", (-3, -2, 8, 6))
    add("straddles top-right corner", (27, -2, 8, 6))
    add("straddles bottom-left corner", (-3, 21, 8, 6))
    add("straddles bottom-right corner", (27, 21, 8, 6))
    add("covers the whole stack and more", (-2, -2, 35, 28))
    add("zero width", (5, 5, 0, 4), np.zeros((4, 0), np.uint8))
    add("zero height", (5, 5, 4, 0), np.zeros((0, 4), np.uint8))
    return Case("maskwin", data, -9999.0, [w for _, w, _ in wm], [m for _, _, m in wm], [l for l, _, _ in wm])


# ---------------------------------------------------------------- decile lengths
DECILE_COUNTS = (1, 4, 9, 16)


def decile_lengths(dc):
    q = dc + 1
    near = int(round(2048 / q)) * q   # the multiple of dc + 1 nearest to 2048
    return sorted({1, dc - 1, dc, dc + 2, 2 * q - 1, 2 * q, 2 * q + 1, 64, 65, near - 1, near, near + 1})


@functools.lru_cache(None)
def case_lengths(dc, panic=False):
    """One polygon per length of decile_lengths(dc), on its own row: in-mask
    count len + 3, of which 3 pixels are nodata in either band (at different
    places).  panic: one polygon more, of length dc + 1."""
    rng = np.random.default_rng(100 + dc)
    lens = decile_lengths(dc) + ([dc + 1] if panic else [])
    H, W = len(lens), 2080
    data = rng.normal(10.0, 50.0, (2, H, W)).astype(np.float32)
    wins, masks, labels = [], [], []
    for i, ln in enumerate(lens):
        n, k = ln + 3, 4 + i % 5
        x0 = int(rng.integers(0, W - n - k + 1))
        m = row_mask(n, k, rng)
        inside = x0 + np.flatnonzero(m[0] == 255)
        for b in range(2):
            data[b, i, rng.choice(inside, 3, replace=False)] = -9999.0
        wins.append((x0, i, n + k, 1))
        masks.append(m)
        labels.append("len=%d" % ln)
    return Case("lengths%d%s" % (dc, "p" if panic else ""), data, -9999.0, wins, masks, labels)


# ---------------------------------------------------------------- decile key distributions
KEY_N = (340, 5100, 2210)   # in-mask counts: inside the 2048-key LDS cache, streamed, streamed
KEY_DCS = (6, 9, 16)        # 340, 5100 and 2210 are multiples of 10 and 17 (even picks) but not of 7 (odd)


def _shuffled(v, rng):
    v = np.asarray(v, np.float32).copy()
    rng.shuffle(v)
    return v


def kd_all_equal(n, rng):
    return np.full(n, 0.25, np.float32)


def kd_two_values(n, rng):
    return _shuffled(np.where(np.arange(n) < n // 2, 1.5, -2.0), rng)


def kd_full_range(n, rng):
    half = n // 2
    pos = np.linspace(0, 0x7F800000, n - half).astype(np.uint32)   # +0.0 ... +inf
    pos[1], pos[2] = 1, 0x007FFFFF                                  # smallest and largest subnormal
    neg = np.linspace(0, 0x7F800000, half).astype(np.uint32)
    neg[1], neg[2] = 1, 0x007FFFFF
    bits = np.concatenate([pos, neg | np.uint32(0x80000000)])
    assert np.unique(bits).size == n
    v = bits.view(np.float32)
    assert not np.isnan(v).any() and not (v == F32(-9999.0)).any()
    return _shuffled(v, rng)


def kd_negative(n, rng):
    return (-rng.uniform(1.0, 1000.0, n)).astype(np.float32)


def kd_nextafter(n, rng):
    m = min(n, 1500)   # consecutive floats from 1.0: the key span stays under 2048
    return _shuffled((np.uint32(0x3F800000) + (np.arange(n) % m).astype(np.uint32)).view(np.float32), rng)


def kd_dominant(n, rng):
    v = np.full(n, 0.5, np.float32)
    k = max(2, n // 40)
    v[:k] = rng.uniform(-100.0, -1.0, k)
    v[k:2 * k] = rng.uniform(1.0, 100.0, k)
    return _shuffled(v, rng)


def _kd_tie(n, rng, size):
    """`size` equal values at sorted positions [r - 31, r - 31 + size) around
    r = 5 * (n // 10), decile 5's rank at decile_count 9; all others distinct."""
    r = 5 * (n // 10)
    s = np.unique(rng.uniform(0.0, 1.0, 2 * n).astype(np.float32))[: n - size]
    assert s.size == n - size
    s = np.sort(_shuffled(s, rng))
    start = r - 31
    tie = F32((np.float64(s[start - 1]) + np.float64(s[start])) / 2)
    assert s[start - 1] < tie < s[start]
    return _shuffled(np.concatenate([s[:start], np.full(size, tie, np.float32), s[start:]]), rng)


def kd_tie64(n, rng):
    return _kd_tie(n, rng, 64)


def kd_tie65(n, rng):
    return _kd_tie(n, rng, 65)


def kd_ties32(n, rng):
    """32 widely spaced values; with n a multiple of 17 the multiplicities put
    each of the 32 ranks decile_count 16 reads (step .. 16 step, each with its
    successor) into a tie of its own: at least 65 copies each once step >=
    130 (n = 2210, 5100)."""
    step = n // 17
    vals = np.array(sorted([-(4.0 ** k) for k in range(16)] + [4.0 ** k for k in range(16)]), np.float32)
    mult = [step + 1]
    for _ in range(15):
        mult += [step // 2, step - step // 2]
    mult.append(n - sum(mult))
    assert len(mult) == 32 and min(mult) >= 1
    return _shuffled(np.repeat(vals, mult), rng)


def kd_nodata_most(n, rng):
    v = rng.uniform(0.0, 1.0, n).astype(np.float32)
    v[rng.random(n) < 0.6] = -9999.0
    return v


def kd_nodata_between(n, rng):
    v = rng.uniform(-20000.0, 0.0, n).astype(np.float32)
    v[rng.random(n) < 0.05] = -9999.0
    return v


def kd_nodata_adjacent(n, rng):
    """Consecutive floats within 150 ulps of the nodata value, 10 % exactly
    nodata, 5 % outliers at +-1e30: the wide key range puts nodata and the picks
    into one bucket, which the select refines from its cached keys."""
    bits = np.float32(-9999.0).view(np.uint32) + rng.integers(-150, 151, n).astype(np.int64)
    v = bits.astype(np.uint32).view(np.float32).copy()
    u = rng.random(n)
    v[u < 0.10] = -9999.0
    v[(u >= 0.10) & (u < 0.125)] = -1e30
    v[(u >= 0.125) & (u < 0.15)] = 1e30
    return v


def kd_zero_tiny(n, rng):
    """Nodata 0.0: both zeros (10 % each) among subnormals of both signs (15 %
    each) that share their bucket, the rest at +-1e20..1e30: the middle picks
    are subnormals whose bucket also holds the keys of -0.0 / +0.0."""
    u = rng.random(n)
    v = np.where(u < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(20, 30, n)
    tiny = rng.integers(1, 1000, n).astype(np.uint32).view(np.float32).astype(np.float64)
    v = np.where(u < 0.15, -tiny, v)
    v = np.where((u >= 0.85), tiny, v)
    v = v.astype(np.float32)
    v[(u >= 0.15) & (u < 0.25)] = -0.0
    v[(u >= 0.75) & (u < 0.85)] = 0.0
    return v


def kd_uniform(n, rng):
    return rng.uniform(-1.0, 1.0, n).astype(np.float32)


def kd_both_zeros(n, rng):
    v = rng.normal(0.0, 1.0, n).astype(np.float32)
    u = rng.random(n)
    v[u < 0.1] = 0.0
    v[(u >= 0.1) & (u < 0.2)] = -0.0
    return v


def kd_only_zeros(n, rng):
    return _shuffled(np.where(np.arange(n) < n // 2, F32(0.0), F32(-0.0)), rng)


# (nodata group, scenario): the band's values
KEY_SCENARIOS = {
    "m9999": [("all_equal", kd_all_equal), ("two_values", kd_two_values), ("full_range_inf_to_inf", kd_full_range),
              ("negative_only", kd_negative), ("nextafter_span_under_2048", kd_nextafter),
              ("dominant_95_percent", kd_dominant), ("tie_of_64_at_rank", kd_tie64), ("tie_of_65_at_rank", kd_tie65),
              ("dc16_every_rank_in_own_tie", kd_ties32), ("nodata_most_frequent", kd_nodata_most),
              ("nodata_between_picks", kd_nodata_between), ("nodata_adjacent_to_picks", kd_nodata_adjacent)],
    "zero": [("nodata_zero_both_zeros", kd_both_zeros), ("nodata_zero_full_range", kd_full_range),
             ("nodata_zero_only_zeros", kd_only_zeros), ("nodata_zero_dominant", kd_dominant),
             ("nodata_zero_among_subnormal_picks", kd_zero_tiny)],
    "nan": [("nodata_nan_uniform", kd_uniform), ("nodata_nan_full_range", kd_full_range),
            ("nodata_nan_all_equal", kd_all_equal)],
}
KEY_NODATA = {"m9999": -9999.0, "zero": 0.0, "nan": float("nan")}
KEY_IDS = [(g, i, name) for g, lst in KEY_SCENARIOS.items() for i, (name, _) in enumerate(lst)]


@functools.lru_cache(None)
def case_keys(group):
    """One band per scenario, three polygons (1-row windows) with KEY_N
    in-mask pixels; masked-out pixels hold 777 (must be ignored)."""
    scen = KEY_SCENARIOS[group]
    W = max(KEY_N) + 64
    data = np.full((len(scen), len(KEY_N), W), 777.0, np.float32)
    rng = np.random.default_rng(31)
    wins, masks = [], []
    for row, n in enumerate(KEY_N):
        k = 9 + 7 * row
        m = row_mask(n, k, rng)
        x0 = 3 + row
        wins.append((x0, row, n + k, 1))
        masks.append(m)
        inside = x0 + np.flatnonzero(m[0] == 255)
        for b, (_, gen) in enumerate(scen):
            data[b, row, inside] = gen(n, np.random.default_rng(1000 * b + n))
    return Case("keys_" + group, data, KEY_NODATA[group], wins, masks, ["n=%d" % n for n in KEY_N])


# ---------------------------------------------------------------- strides
STRIDES_LIST = [6, 1, 2, 3, 4, 5, 8]   # strides 3: groups (6,1,2) (3,4,5) (8); band 5 is all nodata


@functools.lru_cache(None)
def case_strides():
    rng = np.random.default_rng(9)
    data = rng.uniform(-5.0, 5.0, (8, 12, 14)).astype(np.float32)
    data[rng.random(data.shape) < 0.05] = -9999.0
    data[4] = -9999.0   # band 5: total 0 in every polygon
    wins = [(1, 1, 7, 6), (5, 3, 9, 8), (0, 0, 14, 12)]
    masks = [np.where(rng.random((h, w)) < 0.85, 255, 0).astype(np.uint8) for _, _, w, h in wins]
    return Case("strides", data, -9999.0, wins, masks)


STRIDES_CALLS = [("strides_greater_than_list", STRIDES_LIST, 9), ("strides_equal_to_list", STRIDES_LIST, 7),
                 ("strides_one_less_than_list", STRIDES_LIST, 6), ("strides_3_bound_band_total_0", STRIDES_LIST, 3),
                 ("strides_2", STRIDES_LIST, 2), ("one_band_strides_3", [7], 3), ("all_bands_strides_3", None, 3)]


# ---------------------------------------------------------------- every call the GPU tests make
def sizes_calls(pc, clip, length):
    bl = band_list(length)
    return [Call(clip, pc, 1, 0, tuple(bl), REFERENCE_ORDER), Call(clip, pc, 1, 9, tuple(bl), REFERENCE_ORDER),
            Call(clip, pc, 1, 0, tuple(bl), WAVE_SPLIT), Call(clip, pc, 1, 9, tuple(bl), WAVE_SPLIT)]


def special_calls(clip_name):
    return [Call(SPECIAL_CLIPS[clip_name], pc) for pc in (0, 1)]


EXCLUDE_ALL = (1e30, 2e30)


MASKWIN_DC = 7   # no (window, band) of case_maskwin holds exactly 8 values (the reference would panic)


def maskwin_calls():
    return [Call(dc=dc) for dc in (0, MASKWIN_DC)] + [Call(EXCLUDE_ALL, pc, 1, MASKWIN_DC) for pc in (0, 1)] + \
           [Call((-1.0, 2.0), pc, 1, dc) for pc in (0, 1) for dc in (0, MASKWIN_DC)]


def strides_calls(bands, strides):
    return [Call(NOCLIP, pc, strides, dc, None if bands is None else tuple(bands))
            for dc in (0, 4) for pc in (0, 1)]


def all_reference_order_calls():
    """(case, call, thorough) of every reference-order call below.  thorough
    False: the oracle is compared on a subset (see test_reference_agrees...)."""
    out = []
    for pc, clip in SIZES_MODES:
        for length in SIZES_LISTS:
            for call in sizes_calls(pc, clip, length)[:2]:
                out.append((case_sizes(), call, length in (33, 129)))
    for mx, dcs in ((5, (0,)), (4, (0, 4))):
        for dc in dcs:
            out.append((case_many(mx), Call(dc=dc), True))
    for nd in SPECIAL_NODATA:
        for cn in SPECIAL_CLIPS:
            for call in special_calls(cn):
                out.append((case_special(nd), call, True))
    for call in maskwin_calls():
        out.append((case_maskwin(), call, True))
    for dc in DECILE_COUNTS:
        out.append((case_lengths(dc), Call(dc=dc), True))
        out.append((case_lengths(dc, True), Call(dc=dc), True))
    for g, b, _ in KEY_IDS:
        for dc in KEY_DCS:
            out.append((case_keys(g), Call(dc=dc, bands=(b + 1,)), True))
    for _, bands, strides in STRIDES_CALLS:
        for call in strides_calls(bands, strides):
            out.append((case_strides(), call, True))
    return out


# ======================================================================
# CPU tests
# ======================================================================
def _same_rows(a_v, a_c, b_v, b_c):
    """NaN at the same places, every other value bit-equal, counts equal."""
    if a_v.shape != b_v.shape or not np.array_equal(a_c, b_c):
        return False
    if not np.array_equal(np.isnan(a_v), np.isnan(b_v)):
        return False
    ok = ~np.isnan(a_v)
    return np.array_equal(np.ascontiguousarray(a_v[ok]).view(np.uint64), np.ascontiguousarray(b_v[ok]).view(np.uint64))


def test_reference_by_hand():
    """The restatement on cases small enough to work out on paper, the
    special-value rules of drill.go:153-177 among them."""
    m = np.full(6, 255, np.uint8)
    v = np.array([1.0, 2.0, np.nan, 4.0, -9999.0, 3.0], np.float32)
    val, cnt = ref_mean(v, m, -9999.0, *NOCLIP, 0)
    assert np.isnan(val) and cnt == 5                      # a NaN value is not nodata and passes the clip
    val, cnt = ref_mean(v, m, float("nan"), *NOCLIP, 0)
    assert np.isnan(val) and cnt == 6                      # a NaN nodata excludes nothing
    z = np.array([0.0, -0.0, 1.0, 3.0], np.float32)
    assert ref_mean(z, m[:4], 0.0, *NOCLIP, 0) == (2.0, 2)   # nodata 0.0 also excludes -0.0
    big = np.array([FLT_MAX, FLT_MAX], np.float32)
    assert ref_mean(big, m[:2], -1.0, *NOCLIP, 0) == (float("inf"), 2)
    both = np.array([np.inf, -np.inf, 1.0], np.float32)
    assert ref_mean(both, m[:3], -1.0, *NOCLIP, 0) == (1.0, 1)        # the default clip is +-FLT_MAX: no infinities
    assert np.isnan(ref_mean(both, m[:3], -1.0, -np.inf, np.inf, 0)[0])   # inf + -inf
    assert ref_mean(both, m[:3], -1.0, 0.0, np.inf, 0) == (float("inf"), 2)
    w = np.array([1.0, 2.0, 3.0, 4.0], np.float32)
    assert ref_mean(w, m[:4], -1.0, 2.0, 2.0, 0) == (2.0, 1)         # both clip ends inclusive
    assert ref_mean(w, m[:4], -1.0, 3.0, 2.0, 0) == (0.0, 0)         # lo > hi: nothing, mean mode
    assert ref_mean(w, m[:4], -1.0, 3.0, 2.0, 1) == (0.0, 4)         # pixel-count mode: 0 of 4
    assert ref_mean(w, m[:4], -1.0, float("nan"), 2.5, 0) == (1.5, 2)   # a NaN bound passes every value
    assert ref_mean(w, m[:4], -1.0, 1.5, 3.5, 1) == (0.5, 4)
    assert ref_mean(w, np.array([255, 254, 1, 255], np.uint8), -1.0, *NOCLIP, 0) == (2.5, 2)
    # computeDeciles: 9 of 1..20 (step 2, even: means of neighbours), 3 values padded to 4 slots
    d = ref_deciles(np.arange(1, 21, dtype=np.float32)[::-1].copy(), np.full(20, 255, np.uint8), -1.0, 9)
    assert np.array_equal(d, np.arange(1, 10, dtype=np.float32) * 2 + 1.5)
    d = ref_deciles(np.arange(1, 22, dtype=np.float32), np.full(21, 255, np.uint8), -1.0, 9)
    assert np.array_equal(d, np.arange(1, 10, dtype=np.float32) * 2 + 1)
    assert np.array_equal(ref_deciles(np.array([3, 1, 2], np.float32), m[:3], -1.0, 4), [1, 1, 2, 3])
    with pytest.raises(RefPanic):
        ref_deciles(np.arange(5, dtype=np.float32), m[:5], -1.0, 4)
    assert [go_round(x) for x in (0.5, 1.5, 2.5, -0.5, 2.4)] == [1.0, 2.0, 3.0, -1.0, 2.0]
    # rows: strides 3 over [a, b, c, d]: a, mid, c, then the 1-band group d read twice -> d, mid, d
    stats = {1: 1.0, 2: 99.0, 3: 4.0, 4: 7.0}
    rv, rc = ref_rows(lambda b: ([stats[b]], [b]), [1, 2, 3, 4], 3, 0)
    assert rv[:, 0].tolist() == [1.0, 2.5, 4.0, 7.0, 7.0, 7.0] and rc[:, 0].tolist() == [1, 2, 3, 4, 4, 4]
    rv, rc = ref_rows(lambda b: ([stats[b]], [b]), [1, 2, 3, 4], 2, 0)
    assert rv[:, 0].tolist() == [1.0, 99.0, 4.0, 7.0]
    # the sequential float32 sum is the Python loop of float32 additions
    x = np.random.default_rng(0).uniform(0.1, 1.0, 3000).astype(np.float32)
    s = F32(0)
    for t in x:
        s = F32(s + t)
    assert s == _f32sum(x)
    # merge
    out = ref_merge([[1.0, np.nan, np.inf, 2.0], [3.0, np.nan, 1.0, 5.0]], [[1, 4, 0, 0], [3, 4, 2, 0]])
    assert out[0] == 2.5 and np.isnan(out[1:]).all()


def test_reference_agrees_with_oracle(oracle):
    """(a) On every NaN-free input of the GPU tests this restatement and the
    oracle agree bit for bit: oracle.drill_read_data_full (it calls
    oracle.drill_read_data and oracle.compute_deciles per read band) on every
    reference-order call -- of the sizes case the 33- and 129-band lists, the
    other lists select from the same (polygon, band) results -- plus
    oracle.drill_read_data and oracle.compute_deciles directly on every band
    of the sizes case, and oracle.drill_merge on the merge inputs."""
    checked = 0
    for case, call, thorough in all_reference_order_calls():
        if not thorough:
            continue
        for p in range(len(case.windows)):
            sub, m = case.clipped(p)
            bl = case.band_list(call)
            if call.strides == 1:   # rows are per band: keep the NaN-free ones
                bl = [b for b in bl if not np.isnan(sub[b - 1]).any()]
                call = call._replace(bands=tuple(bl))
            if m.size == 0 or not bl or np.isnan(sub[np.asarray(bl) - 1]).any():
                continue   # the oracle takes a window inside the stack, and NaN-free values
            try:
                ev, ec = case.expect_poly(p, call)
            except RefPanic:
                ev = None
            got = oracle.drill_read_data_full(sub, m, case.nodata, call.clip[0], call.clip[1], call.pc, call.strides,
                                              call.dc, bl)
            if ev is None or got is None:
                assert ev is None and got is None, (case.name, call, p)
                continue
            assert _same_rows(ev, ec, got[0], got[1]), (case.name, call, case.labels[p])
            checked += 1
    assert checked > 3000
    case = case_sizes()
    for p in range(len(case.windows)):
        sub, m = case.clipped(p)
        for pc, clip in SIZES_MODES:
            ov, oc = oracle.drill_read_data(sub, m, case.nodata, clip[0], clip[1], pc, 1)
            mine = [case.mean(p, b, clip, pc) for b in range(sub.shape[0])]
            assert np.array_equal(oc, [c for _, c in mine])
            assert np.array_equal(ov.view(np.uint64), np.array([v for v, _ in mine]).view(np.uint64))
        for b in range(0, sub.shape[0], 8):
            assert np.array_equal(oracle.compute_deciles(sub[b], m, case.nodata, 9), case.deciles(p, b, 9))
    for v, c in merge_inputs().values():
        exp, got = ref_merge(v, c), oracle.drill_merge(v, c)
        assert np.array_equal(np.isnan(exp), np.isnan(got))
        assert np.array_equal(exp[~np.isnan(exp)], got[~np.isnan(got)])


def wave_split_inputs():
    """(case, polygon, band, pc, clip) of every wave-split mean below."""
    out = []
    for case in (case_sizes(), case_many(5)):
        for pc, clip in SIZES_MODES:
            for p in range(len(case.windows)):
                for b in range(case.data.shape[0]):
                    out.append((case, p, b, pc, clip))
    return out


def test_wave_split_bar_on_cpu():
    """(b) On the wave-split inputs (uniform in [0.1, 1], one sign) the
    wave-split restatement stays within the 1e-5 relative bar of the
    sequential one: so the bar tests the kernel, not the data.  Worst here
    2.16e-6."""
    worst = 0.0
    for case in (case_sizes(), case_many(5)):
        kept = case.data[case.data != F32(-9999.0)]
        assert kept.min() >= 0.1 and kept.max() <= 1.0
    for case, p, b, pc, clip in wave_split_inputs():
        sv, sc = case.mean(p, b, clip, pc)
        wv, wc = case.mean(p, b, clip, pc, WAVE_SPLIT)
        assert sc == wc
        if sv == 0.0:   # no value (or, in pixel-count mode, none inside the clip)
            assert wv == 0.0
        else:
            worst = max(worst, abs(wv - sv) / abs(sv))
    print("wave split restatement vs sequential: worst relative %.3g" % worst)
    assert worst <= WAVE_SPLIT_BAR


# ======================================================================
# GPU tests
# ======================================================================
_GPU = {}


def gpu_objects(dev, case):
    import torch

    from gsky_amd import drill
    if case.name not in _GPU:
        st = drill.DrillStack(torch.from_numpy(case.data), case.nodata, dev)
        _GPU[case.name] = (st, drill.pack_masks(case.windows, case.masks, dev))
    return _GPU[case.name]


def run(dev, case, call):
    from gsky_amd import drill
    st, mb = gpu_objects(dev, case)
    v, c = drill.read_data(st, mb, clip_lower=call.clip[0], clip_upper=call.clip[1], pixel_count=call.pc,
                           band_strides=call.strides, decile_count=call.dc,
                           bands=None if call.bands is None else list(call.bands), mode=call.mode)
    return v.cpu().numpy(), c.cpu().numpy()


def assert_means(got, exp, what):
    assert got.shape == exp.shape, what
    bad = np.isnan(got) != np.isnan(exp)
    assert not bad.any(), (what, "NaN places", np.argwhere(bad)[:5].tolist())
    ok = ~np.isnan(exp)
    bad = ok & (np.where(ok, got, 0.0).view(np.uint64) != np.where(ok, exp, 0.0).view(np.uint64))
    assert not bad.any(), (what, "means", np.argwhere(bad)[:5].tolist(), got[bad][:5], exp[bad][:5])


def assert_deciles(got, exp, what):
    bad = ~((got == exp) | (np.isnan(got) & np.isnan(exp)))
    assert not bad.any(), (what, "deciles", np.argwhere(bad)[:5].tolist(), got[bad][:5], exp[bad][:5])


def check(dev, case, call, what=""):
    """One read_data call against the reference (module docstring).  Returns
    the worst relative distance of a wave-split mean from reference order."""
    what = (case.name, what, call)
    ev, ec, panics = case.expect(call)
    assert not panics, (what, "the reference panics for", [case.labels[p] for p in panics])
    gv, gc = run(dev, case, call)
    assert gv.shape == ev.shape, what
    bad = gc != ec
    assert not bad.any(), (what, "counts", np.argwhere(bad)[:5].tolist(), gc[bad][:5], ec[bad][:5])
    means = (gv[..., 0], ev[..., 0]) if call.dc else (gv, ev)
    assert_means(means[0], means[1], what)   # wave split: bit-equal to the wave-split restatement
    if call.dc:
        assert_deciles(gv[..., 1:], ev[..., 1:], what)
    worst = 0.0
    if call.mode == WAVE_SPLIT:   # the project's bar, against the reference order
        sv, sc, _ = case.expect(call._replace(mode=REFERENCE_ORDER))
        smean = sv[..., 0] if call.dc else sv
        assert np.array_equal(sc, gc), what
        nz = smean != 0
        rel = np.abs(means[0][nz] - smean[nz]) / np.abs(smean[nz])
        worst = float(rel.max()) if rel.size else 0.0
        assert worst <= WAVE_SPLIT_BAR, (what, worst)
        assert not means[0][~nz].any(), what
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("length", SIZES_LISTS, ids=["bands%d" % n for n in SIZES_LISTS])
@pytest.mark.parametrize("pc,clip", SIZES_MODES, ids=["mean", "pixel_count"])
def test_sizes(gpu, pc, clip, length):
    """In-mask counts n on the walks' boundaries -- the 16- and 32-pixel
    unrolls (15..17, 31..33), the 32-pixel emit tile and the 64-pixel transpose
    chunk (63..65), the 256-pixel compaction rounds (255..257), the 1024-pixel
    wave-split segments (1023..1025) and the select's 2048-key cache (2047..
    2049) -- with band lists of 1, 31..33, 63..65 and 129 entries (repeats,
    reversed order; more than 64 bands on the fused-emit path, ragged last
    groups of 32 and 64), on (i) read_data without deciles, (ii) with 9
    deciles (fused emit + select), (iii) WAVE_SPLIT without and with deciles
    (the transposing path).  Wave-split means are bit-equal to the wave-split
    restatement; against the reference order the worst measured on an MI355X
    is 2.16e-6 relative (bar 1e-5)."""
    case = case_sizes()
    worst = 0.0
    for call in sizes_calls(pc, clip, length):
        worst = max(worst, check(gpu, case, call))
    print("wave split vs reference order: worst relative %.3g" % worst)


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [1, 33, 64])
def test_sizes_compute_deciles_band_chunk(gpu, chunk):
    """(iv) compute_deciles over the 129-band list in chunks of 1, 33 (a group
    of 32 and a ragged one) and 64 bands (last chunk: 1 band) gives the fused
    path's deciles of (ii), and the reference's."""
    from gsky_amd import drill
    case = case_sizes()
    call = Call(dc=9, bands=tuple(band_list(129)))
    fv, fc = run(gpu, case, call)
    st, mb = gpu_objects(gpu, case)
    import torch
    dec, stt = drill.compute_deciles(st, mb, torch.from_numpy(np.ascontiguousarray(fc[..., 0])).to(gpu), 9,
                                     list(call.bands), band_chunk=chunk)
    dec, stt = dec.cpu().numpy(), stt.cpu().numpy()
    assert (stt == 0).all() and (fc[..., 0] > 0).all()
    assert_deciles(dec, fv[..., 1:].astype(np.float32), "against the fused path")
    ev, _, _ = case.expect(call)
    assert_deciles(dec, ev[..., 1:].astype(np.float32), "against the reference")


@pytest.mark.gpu
def test_many_polygons(gpu):
    """2050 polygons of 0 to 5 in-mask pixels (empty masks among them):
    drill_seg_scan_kernel and decile_chunk_scan_kernel carry twice.  Reference
    order and wave split on counts 0..5; compute_deciles (decile_count 4)
    reports -7 exactly where a band has 5 values; read_data with 4 deciles,
    reference order (fused) and wave split (transposing), on the same layout
    with counts 0..4."""
    import torch

    from gsky_amd import drill
    case = case_many(5)
    check(gpu, case, Call())
    check(gpu, case, Call(mode=WAVE_SPLIT))
    mv, mc = run(gpu, case, Call())
    st, mb = gpu_objects(gpu, case)
    dec, stt = drill.compute_deciles(st, mb, torch.from_numpy(mc).to(gpu), 4)
    dec, stt = dec.cpu().numpy(), stt.cpu().numpy()
    n_panic = 0
    for p in range(len(case.windows)):
        for b in range(3):
            if mc[p, b] == 0:
                assert stt[p, b] == 1 and not dec[p, b].any()
                continue
            try:
                exp = case.deciles(p, b, 4)
            except RefPanic:
                n_panic += 1
                assert stt[p, b] == -7, (p, b)
                continue
            assert stt[p, b] == 0 and np.array_equal(dec[p, b], exp), (p, b)
    assert n_panic > 100 and (mc == 0).all(axis=1).sum() > 100
    case4 = case_many(4)
    check(gpu, case4, Call(dc=4))
    check(gpu, case4, Call(dc=4, mode=WAVE_SPLIT))


@pytest.mark.gpu
@pytest.mark.parametrize("clip_name", list(SPECIAL_CLIPS))
@pytest.mark.parametrize("nd_name", list(SPECIAL_NODATA))
def test_special_values(gpu, nd_name, clip_name):
    """Reference order, mean and pixel-count mode, one scenario per band
    (SPECIAL_BANDS): +inf / -inf among finite values, a NaN among finite
    values (mean NaN, counted), +inf and -inf together (NaN), FLT_MAX more
    than once (+inf), only +0.0 and -0.0, subnormals, all values nodata (0,
    Count 0) -- under nodata -9999, 0.0 (with -0.0 in the data: excluded too),
    NaN (excludes nothing) and +inf, and the clips none, lo == hi == a value
    present (both ends inclusive), lo > hi (mean mode 0 / Count 0, pixel-count
    mode 0 / Count = non-nodata pixels) and a NaN bound (every value
    passes).  The default clip, +-FLT_MAX, drops infinities: they reach the sum
    under the clip (-inf, +inf) and under NaN bounds."""
    case = case_special(nd_name)
    for call in special_calls(clip_name):
        check(gpu, case, call, SPECIAL_BANDS)
    # the rules the scenarios are there for, spelled out on the reference
    ev, ec, _ = case.expect(Call(SPECIAL_CLIPS[clip_name], 0))
    col = {n: i for i, n in enumerate(SPECIAL_BANDS)}
    if clip_name == "none" and nd_name == "m9999":
        assert 0 < ev[0, col["plus_inf"]] < 1 and 0 < ev[0, col["both_inf"]] < 1 and np.isnan(ev[0, col["nan"]])
    if clip_name in ("inf_bounds", "nan_both") and nd_name == "m9999":
        assert ev[0, col["plus_inf"]] == np.inf and ev[0, col["minus_inf"]] == -np.inf
        assert np.isnan(ev[0, col["nan"]]) and np.isnan(ev[0, col["both_inf"]])
        assert ev[0, col["flt_max_twice"]] == np.inf and ev[0, col["zeros"]] == 0.0
        assert 0 < abs(ev[0, col["subnormals"]]) < 1.2e-38
        assert ev[0, col["all_nodata"]] == 0.0 and ec[0, col["all_nodata"]] == 0
    if nd_name == "zero":
        assert ec[0, col["zeros"]] == 0
    if nd_name == "plus_inf" and clip_name == "inf_bounds":
        assert 0 < ev[0, col["plus_inf"]] < 1 and ev[0, col["both_inf"]] == -np.inf
    if nd_name == "nan" and clip_name == "none":
        assert np.isnan(ev[0, col["all_nodata"]]) and ec[0, col["all_nodata"]] == ec[0, col["zeros"]] > 200
    if clip_name == "lo_eq_hi" and nd_name == "m9999":
        assert ev[0, col["plus_inf"]] == 0.5 and ec[0, col["plus_inf"]] >= 1
    if clip_name == "lo_gt_hi":   # (a NaN value passes even this clip: the "nan" band stays NaN)
        fin = [col[n] for n in SPECIAL_BANDS if n != "nan" and not (n == "all_nodata" and nd_name == "nan")]
        assert not ev[0, fin].any() and not ec[0, fin].any()
        ev1, ec1, _ = case.expect(Call(SPECIAL_CLIPS[clip_name], 1))
        assert not ev1[0, fin].any() and ec1[0, col["minus_inf"]] > 200


@pytest.mark.gpu
def test_masks_and_windows(gpu):
    """Mask bytes from {0, 1, 127, 254, 255} (only 255 is inside), all-zero,
    all-255 and all-254 masks; windows of 1 x 1, 1 x n and n x 1; wholly
    outside the stack on each of the four sides and beyond a corner;
    straddling each side and each corner; covering the whole stack; zero
    width and zero height (rows of zeros, Count 0) -- without and with 7
    deciles, with a clip, and (totals and deciles, drill.go:179-191) with a
    clip that excludes everything: mean mode gives zero deciles with Count 0,
    pixel-count mode computes them."""
    case = case_maskwin()
    for call in maskwin_calls():
        check(gpu, case, call, case.labels)
    ev, ec, _ = case.expect(Call(EXCLUDE_ALL, 0, 1, MASKWIN_DC))
    assert not ev.any() and not ec.any()
    ev, ec, _ = case.expect(Call(EXCLUDE_ALL, 1, 1, MASKWIN_DC))
    assert not ev[..., 0].any() and (ec[..., 1:] == 1).any() and ev[..., 1:].any()
    empty = [case.labels.index(s) for s in ("mask all zero", "mask all 254", "outside left", "outside right",
                                            "outside above", "outside below", "beyond the corner", "zero width",
                                            "zero height", "1 x 1 masked out")]
    ev, ec, _ = case.expect(Call(dc=MASKWIN_DC))
    assert not ev[empty].any() and not ec[empty].any()


@pytest.mark.gpu
@pytest.mark.parametrize("dc", DECILE_COUNTS)
def test_decile_lengths(gpu, dc):
    """decile_count 1, 4, 9 and 16 at lengths 1, dc - 1, dc, dc + 2 (around
    the padding branch), 2 (dc + 1) - 1, 2 (dc + 1), 2 (dc + 1) + 1 (around
    the even picks), 64, 65 and the multiple of dc + 1 nearest to 2048 with its
    two neighbours.  Length dc + 1: status -7 from compute_deciles for that
    polygon alone, GskyError from read_data."""
    import torch

    from gsky_amd import GskyError, drill
    check(gpu, case_lengths(dc), Call(dc=dc), decile_lengths(dc))
    case = case_lengths(dc, True)
    _, _, panics = case.expect(Call(dc=dc))
    assert panics == [len(case.windows) - 1]
    with pytest.raises(GskyError):
        run(gpu, case, Call(dc=dc))
    _, mc = run(gpu, case, Call())
    st, mb = gpu_objects(gpu, case)
    dec, stt = drill.compute_deciles(st, mb, torch.from_numpy(mc).to(gpu), dc)
    dec, stt = dec.cpu().numpy(), stt.cpu().numpy()
    assert (stt[-1] == -7).all()
    for p in range(len(case.windows) - 1):
        for b in range(2):
            if mc[p, b] == 0:
                assert stt[p, b] == 1
            else:
                assert stt[p, b] == 0 and np.array_equal(dec[p, b], case.deciles(p, b, dc)), (case.labels[p], b)


@pytest.mark.gpu
def test_decile_count_17_is_refused(gpu):
    """decile_count 17 needs 34 ranks, more than the select holds: GskyError."""
    from gsky_amd import GskyError
    with pytest.raises(GskyError):
        run(gpu, case_lengths(16), Call(dc=17))
    with pytest.raises(GskyError):
        run(gpu, case_lengths(16), Call(dc=17, mode=WAVE_SPLIT))


@pytest.mark.gpu
@pytest.mark.parametrize("group,band,name", KEY_IDS, ids=[k[2] for k in KEY_IDS])
def test_decile_key_distributions(gpu, group, band, name):
    """The select's range refinement on extreme key distributions, NaN-free,
    each at 340 in-mask pixels (inside the 2048-key LDS cache), 5100 and 2210
    (streamed), decile_count 6 (odd picks), 9 and 16 (even picks): all values
    equal (L == Hk on the first pass); two values, half each; all distinct
    from -inf to +inf through both signs, subnormals and both zeros; negative
    values only; consecutive floats from nextafter (span under 2048 keys, sh
    == 0); one value making up 95 % with outliers on each side; a tie of
    exactly 64 and of exactly 65 equal values straddling decile 5's rank
    (kCandMax); 32 widely spaced values tied so that each of the 32 ranks of
    decile_count 16 ends in a tie of its own, of at least 65 copies at 2210
    and 5100 pixels (32 x 65 = 2080 keys cannot fit the cache: at 340 pixels
    the ties are shorter); nodata as the most frequent value; nodata lying
    between two picks, and within a few ulps of the picks (the select refines a
    bucket that holds both from its cached keys); nodata 0.0 with both zeros in
    the data (with only zeros: total 0; among subnormal picks that share the
    zeros' bucket); NaN nodata (excludes nothing).  Both decile paths: fused
    with the reference-order walk, transposing under WAVE_SPLIT."""
    case = case_keys(group)
    for dc in KEY_DCS:
        check(gpu, case, Call(dc=dc, bands=(band + 1,)), name)
    gv, gc = run(gpu, case, Call(dc=9, bands=(band + 1,), mode=WAVE_SPLIT))
    ev, ec, _ = case.expect(Call(dc=9, bands=(band + 1,)))
    assert np.array_equal(gc, ec)
    assert_deciles(gv[..., 1:], ev[..., 1:], (name, "transposing path"))


@pytest.mark.gpu
@pytest.mark.parametrize("name,bands,strides", STRIDES_CALLS, ids=[s[0] for s in STRIDES_CALLS])
def test_strides(gpu, name, bands, strides):
    """band_strides greater than, equal to and one less than the list length,
    3 (a group whose bound band 5 has total 0; a 1-band last group read
    twice) and 2, a list of one band with strides 3 -- with decile_count 0 and
    4, mean and pixel-count mode; Counts math.Round half away from zero."""
    case = case_strides()
    for call in strides_calls(bands, strides):
        check(gpu, case, call, name)


def merge_inputs():
    rng = np.random.default_rng(3)
    out = {}
    v = rng.normal(0.3, 0.1, (5, 257))
    v[rng.random(v.shape) < 0.2] = np.nan
    c = rng.integers(0, 1000, v.shape).astype(np.int32)
    v[:, 7] = np.nan                      # every file NaN
    c[:, 9] = 0                           # all counts 0
    v[2, 11], c[2, 11] = np.inf, 0        # inf x 0 = NaN poisons the total
    v[1, 13] = np.inf                     # inf with a count: +inf
    v[0, 15], v[1, 15], c[0, 15], c[1, 15] = np.inf, -np.inf, 1, 1
    out["nan_skipped_257_dates"] = (v, c)
    out["one_file"] = (v[:1].copy(), c[:1].copy())
    out["one_date"] = (v[:, 11:12].copy(), c[:, 11:12].copy())
    out["all_counts_0"] = (rng.normal(size=(3, 5)), np.zeros((3, 5), np.int32))
    out["inf_times_0"] = (np.array([[np.inf], [1.0]]), np.array([[0], [4]], np.int32))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["nan_skipped_257_dates", "one_file", "one_date", "all_counts_0", "inf_times_0"])
def test_drill_merge(gpu, name):
    """drill_merge against the restatement of drill_merger.go:79-93: NaN
    values skipped, all counts 0 gives NaN, inf x 0 gives NaN, one file, 1 and
    257 dates."""
    import torch

    from gsky_amd import drill
    v, c = merge_inputs()[name]
    exp = ref_merge(v, c)
    got = drill.drill_merge(torch.from_numpy(v).to(gpu), torch.from_numpy(c).to(gpu)).cpu().numpy()
    assert_means(got, exp, name)
    if name in ("all_counts_0", "inf_times_0"):
        assert np.isnan(exp).all()
