"""Edge rules of nearest-neighbour resampling (GSKYHIP_RESAMPLE_NEAREST) on
every code path that takes it, against the rule in numpy (tests/test_nn_rule.py).

The paths, and the call that reaches each:

  (i)   nn_index (resample.h) in warp_window_kernel       batch.warp_windows(0)
  (ii)  render_nn_kernel (render_nn.h), RGBA              batch.render(sp, pal); batches of fewer than 256
        workgroups pick the one-row-per-wave kernel, larger ones four rows per wave
  (iii) render_nn_kernel, typed canvases                  render(..., rgba=False) and render_coverage(..., resample=0)
  (iv)  the MASK variants of (ii) and (iii)               the same calls of a config with mask=
  (v)   the generic kernels (nn_fetch, render_common.h)   batch.typed = False; three namespaces; promoted types
  (vi)  the A/B shapes of (ii) and (iv): 4 and 8 rows per wave, the single-entry ONE path on and off, masked
        stacks at 1 and 4 rows per wave -- libgskyhip_ab.so in one child process per knob set (four), each
        running every part-A and part-B case through every path and printing the differing tiles per case.
        The fixed-point row (nn_fix_row) is live only on the ONE path, which production picks from 32768
        workgroups up, so it is these children that run it

Bodies of render_nn.h and the cases built for them: nn_fix_row, full and
window-edge form, and its hand-over to fp64 (A1: shifts inside and outside
kFixMargin; the anisotropic case mixes both in one row group, the ONE path's
redo loop); the fp64 fast body and nn_partial_row (A1 redo rows, A2 4100-wide
window and coordinates past 2^20, which have no fixed-point form); the span
path (A3); nn_masked_same_row 8- and 16-bit (A6 a), the general body with
mask_fast_pair and its flat-index remap (A6 b, c); nn_fold_row_stack in 2 and
3 rounds (A7); the output stage (A9).

Bar: nearest neighbour moves values and computes none: identical window
boxes, identical bytes of every window, canvas (float32 as bit patterns) and
RGBA tile, no pixel left out, no tolerance.  Each case asserts on the CPU
that the rule yields the pixels it exists for before the GPU is asked.

Part A is same-CRS (EPSG:3857 on both sides, the geometry of
tests/test_nn_rule.py); part B reprojects EPSG:3577 -> EPSG:3857 (POOL rows)
with oracle.warp and oracle.render_tiles as the reference.  Not covered:
failed leaves -- no CRS the oracle knows puts a failed point inside a window
(a window is the bounding box of transformed points, and the geostationary
CRS, whose windows do hold such points, is not in the oracle); Mask types
Int16 / SignedByte; nn_axis() itself, which only the service's warp batch
(bytesRead) calls.

Part A found one departure, fixed with this module: in fill mode the fast
bodies folded float32 with (c == nd) ? v : c, which stores an older entry's
-0.0 over a canvas +0.0 under a nodata of 0.0 (A4_negative_zero: 568 of 1920
pixels differed on each tile, through the fp64 fast body and through the
fixed-point row's fold alike).

Measured on an MI355X (-s prints the running counts): pixels compared per
path over all cases, differences 0 on every one:

  (i)   windows                   1 050 019
  (ii)  band kernel RGBA          1 373 987
  (iii) typed canvases            1 343 267   coverages 1 339 427
  (iv)  masked RGBA / canvases       17 280 each
  (v)   generic RGBA / canvases   1 391 267 / 1 360 547, coverages 1 339 427; RGB 3 840 (+ 11 520 canvas pixels)
  (vi)  each of the four children: the same counts again, differences 0

The module's 62 tests take 15 s; the slowest in-process test is 0.3 s; each
child takes 2.8-3.5 s, start-up of the interpreter and torch included
(tests/test_gpu_variants.py's children: 2.4-2.7 s in the same run).

Deliberate one-line breaks, each tried on a scratch build, and the first case
that noticed: "+ 1e-10" dropped from the fp64 fast body -- A1 (the 40 x 10
tiles); the s < 0 test dropped from the rule -- A1; <= for < in nn_index_sxy's
band bound -- A3 (NaN nodata: the span path is off); the flat-index remap
skipped -- A6c; only the first 64 entries folded -- A7 (130 entries);
kFixMargin = 0 -- A1 (the 40 x 10 tiles), in the child that forces the ONE
path only: the in-process kernels take no fixed-point row.
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from gsky_amd import synth

from .helpers import cast_cfg, gpu_batch, oracle_inputs, oracle_render
from .test_cubic import TYPE_NAME, _fnv32a
from .test_nn_rule import (CORNERS, GRID_TILE, ND, SHIFTS_X, SHIFTS_Y, SRS, STEP, T0, NnRef, bits, expected_rgba,
                           grid_granule, merge_nodata, nn_gran, nn_tile, tile_reference, window_type)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DAY = 86400.0
PAL = synth.PALETTE_GSKY
TILE = nn_tile(80, 24)
COUNTS = {}
# polygon names by FNV-1a hash, largest first: the merge orders a stack by
# timestamp + hash, and these hashes lie further apart than any two timestamps
# used here, so POLYS[0] is first in every stack
POLYS = []
for _p in sorted(("P%d" % k for k in range(400)), key=_fnv32a, reverse=True):
    if not POLYS or _fnv32a(POLYS[-1]) - _fnv32a(_p) > 400 * 86400:
        POLYS.append(_p)
POLYS = POLYS[:16]
assert len(POLYS) == 16


# ---------------------------------------------------------------- cases
class Case:
    """One config, the paths it runs through ("i" windows, "rgba", "canvas",
    "cov" render_coverage, "generic": rgba / canvas again with typed = False)
    and its reference, computed once."""

    def __init__(self, cfg, paths=("i", "rgba", "canvas", "cov", "generic")):
        self.cfg, self.paths = cfg, tuple(paths)
        if cfg.mask is not None or len(cfg.namespaces) != 1:
            self.paths = tuple(p for p in self.paths if p != "cov")

    @functools.cached_property
    def ref(self):
        return [tile_reference(self.cfg, t) for t in range(len(self.cfg.tiles))]

    def rgba(self, O):
        if not hasattr(self, "_rgba"):
            self._rgba = [expected_rgba(O, [m[0] for m in merged], [m[1] for m in merged], self.cfg.scale,
                                        self.cfg.palette) for _, merged in self.ref]
        return self._rgba


def _cfg(name, granules, tiles, pairs, namespaces=("",), mask=None, scale=(0.0, 0.0, 3000.0, 0), palette=PAL):
    return synth.SynthConfig(name, granules, SRS, tiles, pairs, list(namespaces), scale, palette, resample=0, mask=mask)


def _vals(rng, ny, nx, dt, nodata, p_holes=0.3):
    """Values over the type's whole range (float32: [-1000, 1000]) that differ
    from the merge's nodata, with `p_holes` of the pixels holding it."""
    nd = merge_nodata(nodata, dt)
    if dt == np.float32:
        v = rng.uniform(-1000.0, 1000.0, (ny, nx)).astype(np.float32)
    else:
        info = np.iinfo(dt)
        v = rng.integers(info.min, info.max + 1, (ny, nx)).astype(dt)
        v.reshape(-1)[:2] = (info.min, info.max)
        v[v == nd] = dt(1) if nd != 1 else dt(2)
    if p_holes:
        v[rng.random((ny, nx)) < p_holes] = nd
    return v


def _near(r, tol):
    """Window pixels of a reference whose x coordinate lies within `tol` of an integer."""
    near = np.abs(r.sx - np.round(r.sx)) <= tol
    return int((r.inwin & near[None, :]).sum())


CASES = {}


def case(fn):
    CASES[fn.__name__] = functools.lru_cache(None)(fn)
    return CASES[fn.__name__]


# A1: the truncation boundary
def _grid(ratio):
    cells = [(c, dx, dy) for c in CORNERS for dx in SHIFTS_X for dy in SHIFTS_Y]
    gs = [grid_granule(ratio, c, dx, dy) for c, dx, dy in cells]
    # every granule under the 80 x 24 tile (its window ends inside the tile: the last column and row hold no
    # source pixel, so no row is `inside`: the span path) and under a 40 x 10 tile the granule overhangs to the
    # right and below (rows `inside`: the fixed-point row and the fp64 fast body; the corner at (-7.5, -3.5)
    # covers it, the other two start inside it: the window-edge forms)
    n = len(gs)
    c = Case(_cfg("A1 ratio %g" % ratio, gs, [GRID_TILE] * n + [nn_tile(40, 10)] * n, [[k] for k in range(n)] * 2))
    exact = margin = outside = eps = nofill = rows_in = 0
    for k, (corner, dx, dy) in enumerate(cells):
        nofill += int((c.ref[k][0][0].inwin & ~c.ref[k][0][0].has).sum())
        r = c.ref[n + k][0][0]
        x, y, w, h = r.win
        assert (x + w, y + h) == (40, 10) and (x == 0) == (corner[0] < 0)
        inside = r.has[:, x:].all(axis=1)
        rows_in += int(inside.sum())
        cnt = lambda near: int(inside.sum()) * int(near[x:].sum())
        frac = np.abs(r.sx - np.round(r.sx))
        exact += cnt(frac == 0)
        if abs(dx) == 2.0 ** -20:
            margin += cnt((frac <= 2.0 ** -19) & (frac > 2.0 ** -21))
        if abs(dx) == 2.0 ** -18:
            outside += cnt((frac <= 2.0 ** -17) & (frac > 2.0 ** -19))
        if 0 < abs(dx) <= 2.0 ** -33:
            eps += cnt(frac <= 2 * STEP)
    # `inside` rows with pixels exactly on a boundary, inside kFixMargin (2^-19) of one, outside it, astride the
    # epsilon; window-fill pixels of the larger tiles
    assert min(exact, margin, outside, eps, nofill) >= 400 and rows_in >= 400, (exact, margin, outside, eps, nofill,
                                                                                rows_in)
    return c


for _r in (1.0, 2.0, 0.5, 4.0):
    CASES["A1_ratio_%g" % _r] = functools.lru_cache(None)(functools.partial(_grid, _r))


@case
def A1_anisotropic():
    """x ratio 1 at an integer corner (no column near a boundary), y ratio 2
    at a half-pixel corner: every other tile row sits on a y boundary, so one
    row group mixes fixed-point rows and rows handed to fp64."""
    rng = np.random.default_rng(41)
    gs = [nn_gran(_vals(rng, 18, 70, np.int16, -1.0, 0.05), 1.0, 5.0, 3.5, -1.0, ratio_y=2.0, sy=dy, poly="P%d" % k)
          for k, dy in enumerate((0.0, -STEP, 2.0 ** -20))]
    # 60 x 32: the granule overhangs to the right and below, so its rows are `inside`; 80 x 40: they leave the band
    c = Case(_cfg("A1 anisotropic", gs, [nn_tile(60, 32)] * 3 + [nn_tile(80, 40)] * 3, [[0], [1], [2]] * 2))
    for t, (refs, _) in enumerate(c.ref):
        r = refs[0]
        on = np.abs(r.sy - np.round(r.sy)) <= 2.0 ** -19
        rows = slice(r.win[1], r.win[1] + r.win[3])
        assert on[rows].sum() >= 13 and (~on[rows]).sum() >= 13 and (on[rows][:-1] != on[rows][1:]).sum() >= 26
        assert not (np.abs(r.sx - np.round(r.sx)) < 0.25).any()
        if t < 3:
            assert r.has[rows, r.win[0]:].all(axis=1).sum() >= r.win[3] - 1 and r.win[0] + r.win[2] == 60
    return c


# A2: block shapes
WIDTHS = (1, 63, 64, 65, 511, 512, 513, 1100)
HEIGHTS = (1, 3, 4, 5, 17, 33)


@case
def A2_block_shapes():
    rng = np.random.default_rng(42)
    full = nn_gran(_vals(rng, 40, 1110, np.int16, -1.0, 0.05), 1.0, -3.5, -2.5, -1.0, poly="F")
    part = nn_gran(_vals(rng, 40, 600, np.int16, -1.0, 0.05), 1.0, 100.5, -2.5, -1.0, poly="P")      # 100.5 .. 700.5
    second = nn_gran(_vals(rng, 40, 530, np.int16, -1.0, 0.05), 1.0, 500.5, -2.5, -1.0, poly="S")    # 500.5 .. 1030.5
    tiles = [nn_tile(w, h) for w in WIDTHS for h in HEIGHTS]
    pairs = [[0]] * len(tiles)
    for w in (511, 512, 513, 1100):
        for h in (5, 33):
            tiles.append(nn_tile(w, h))
            pairs.append([1])
    for h in (4, 17):
        tiles += [nn_tile(1100, h), nn_tile(1100, h)]
        pairs += [[2], [2, 1]]
    c = Case(_cfg("A2 block shapes", [full, part, second], tiles, pairs))
    for t, (refs, _) in enumerate(c.ref):
        r = refs[0]
        if pairs[t] == [0]:
            assert r.has.all()                                      # cover (and, at 512 columns, full)
        elif pairs[t] == [1]:
            assert r.win[0] == 100 and not r.has[:, :100].any() and r.has[:, 101:min(700, r.val.shape[1])].all()
        else:
            assert r.win[0] == 500 and r.has[:, 512:1024].all() and not r.has[:, :500].any() and not r.has[:, 1031:].any()
    return c


@case
def A2_window_wider_than_4096():
    """4100 x 4: wider than kFixMaxW, no fixed-point form."""
    rng = np.random.default_rng(43)
    g = nn_gran(_vals(rng, 6, 4110, np.int16, -1.0, 0.05), 1.0, -3.5, -0.5, -1.0)
    c = Case(_cfg("A2 4100 wide", [g], [nn_tile(4100, 4)], [[0]]))
    assert c.ref[0][0][0].win == [0, 0, 4100, 4] and c.ref[0][0][0].has.all()
    return c


@case
def A2_coordinates_past_2_20():
    """A uint8 granule of 2 rows x (2^20 + 128) columns; the tile looks at its
    last 100 columns: source coordinates exceed 2^20 (fix_range_ok fails)."""
    rng = np.random.default_rng(44)
    nx = 2 ** 20 + 128
    data = rng.integers(1, 256, (2, nx)).astype(np.uint8)
    g = nn_gran(data, 1.0, -float(nx - 100), 0.0, 0.0)
    c = Case(_cfg("A2 past 2^20", [g], [nn_tile(120, 2)], [[0]], scale=(0.0, 0.0, 250.0, 0)))
    r = c.ref[0][0][0]
    assert r.sx[0] == nx - 99.5 and r.has[:, :100].all() and not r.has[:, 100:].any() and r.win == [0, 0, 101, 2]
    assert np.array_equal(r.val[:, :100], data[:, -100:])
    return c


# A3: rows that leave the band
def _leaving(dt, nodata, hole, nan_data=False):
    rng = np.random.default_rng(45)

    def gran(ny, nx, ratio, left, top, ts, poly):
        v = _vals(rng, ny, nx, dt, nodata, 0.0)
        v[rng.random((ny, nx)) < 0.2] = hole
        if nan_data:
            v[rng.random((ny, nx)) < 0.1] = np.nan
        return nn_gran(v, ratio, left, top, nodata, ts, poly)

    gs = [gran(12, 40, 1.0, 5.5, 3.5, T0 + DAY, POLYS[0]), gran(7, 20, 2.0, 7.5, 4.5, T0, POLYS[1]),
          gran(20, 60, 0.5, 20.5, 6.5, T0 + 2 * DAY, POLYS[2])]
    return gs, [TILE] * 5, [[0], [1], [2], [0, 1], [1, 2]]


def _assert_leaving(c, fill_is_nd):
    for t, (refs, merged) in enumerate(c.ref):
        for r in refs:     # the window's last column and row hold no source pixel
            x, y, w, h = r.win
            assert not r.has[y:y + h, x + w - 1].any() and not r.has[y + h - 1, x:x + w].any() and r.has.any()
            assert (r.fill == r.nd) == fill_is_nd or (fill_is_nd is None)
        assert fill_is_nd is None or all(m[1] > 0 for m in merged[0][2])


@case
def A3_leaving_nodata_in_range():
    c = Case(_cfg("A3 nd -1", *_leaving(np.int16, -1.0, -1)))
    _assert_leaving(c, True)
    assert any(m[0] for _, merged in c.ref for m in merged[0][2])
    return c


@case
def A3_leaving_nodata_wraps():
    """int16 nodata 40000: the window fill is 32767, the merge's nodata
    -25536, so window-fill pixels are values and the span path must stay off."""
    c = Case(_cfg("A3 nd 40000", *_leaving(np.int16, 40000.0, -25536)))
    _assert_leaving(c, False)
    r = c.ref[0][0][0]
    assert r.fill == 32767 and r.nd == -25536 and (c.ref[0][1][0][0] == 32767).sum() >= r.win[2] + r.win[3] - 1
    return c


@case
def A3_leaving_nan_nodata():
    """float32, NaN nodata, NaN among the data: a NaN nodata equals nothing,
    so no entry fills and an overwriting entry takes every window pixel."""
    c = Case(_cfg("A3 nd NaN", *_leaving(np.float32, float("nan"), np.nan, True), scale=(1000.0, 0.0, 2000.0, 0)))
    _assert_leaving(c, None)
    modes = [m for _, merged in c.ref for m in merged[0][2]]
    assert any(fill for fill, _, _ in modes) and all((taken == 0) if fill else taken > 0 for fill, taken, _ in modes)
    assert np.isnan(c.ref[3][1][0][0]).sum() > 50
    return c


# A4: types and nodata
def _two_entries(dt, nodata, seed=46):
    """Granules covering the whole tile (`inside` rows, cover: the fast
    bodies), 30 % holes each: `new`; `old` and `old_fix`, older and after it
    in the stack (fill mode) -- `old` with every coordinate on a truncation
    boundary (the fp64 fast body), `old_fix` at phase 1/4 (the fixed-point
    row); `edge`, older still, starting inside the tile (the window-edge
    forms); `late`, the newest but last in the stack (overwrite mode)."""
    rng = np.random.default_rng(seed)
    new = nn_gran(_vals(rng, 30, 90, dt, nodata), 1.0, -3.25, -2.25, nodata, T0 + DAY, POLYS[0])
    old = nn_gran(_vals(rng, 30, 90, dt, nodata), 1.0, -4.5, -3.5, nodata, T0, POLYS[1])
    old_fix = nn_gran(_vals(rng, 30, 90, dt, nodata), 1.0, -4.25, -3.25, nodata, T0, POLYS[2])
    edge = nn_gran(_vals(rng, 30, 50, dt, nodata), 1.0, 20.0, -3.0, nodata, T0 - DAY, POLYS[3])
    late = nn_gran(_vals(rng, 30, 90, dt, nodata), 1.0, -5.75, -4.25, nodata, T0 + 2 * DAY, POLYS[15])
    return [new, old, old_fix, edge, late], [TILE] * 5, [[0, 1], [2, 0], [0, 3, 1], [0, 2, 4], [1, 3]]


INT_SCALE = {np.uint8: (0.0, 0.0, 250.0, 0), np.int8: (100.0, 0.0, 200.0, 0), np.int16: (20000.0, 0.0, 50000.0, 0),
             np.uint16: (0.0, 0.0, 60000.0, 0), np.float32: (1000.0, 0.0, 2000.0, 0)}
A4_TYPES = [(np.uint8, 7.0), (np.int8, -3.0), (np.int16, -999.0), (np.uint16, 65535.0), (np.float32, ND)]


def _types(dt, nodata):
    c = Case(_cfg("A4 %s nodata %r" % (np.dtype(dt).name, nodata), *_two_entries(dt, nodata), scale=INT_SCALE[dt]))
    for refs, merged in c.ref:
        canvas, _, modes = merged[0]
        assert refs[0].has.all() and any(m[0] and m[1] > 100 for m in modes) and any(not m[0] and m[1] > 100 for m in modes)
    assert sum(1 for m in c.ref[3][1][0][2] if not m[0] and m[1] > 100) == 2      # overwrite over a filled canvas
    assert (c.ref[0][1][0][0] == c.ref[0][0][0].nd).sum() > 50     # holes of both entries stay nodata
    return c


for _dt, _nd in A4_TYPES:
    for _n in (_nd, None):
        CASES["A4_%s_%s" % (np.dtype(_dt).name, "none" if _n is None else "nd")] = functools.lru_cache(None)(
            functools.partial(_types, _dt, _n))


def _source_of(g, tile_mask):
    """Indices into g.data of the source pixels of the tile pixels in `tile_mask` (g covers TILE at 1:1)."""
    r = NnRef(g, TILE)
    assert r.has.all()
    iy, ix = np.trunc(r.sy + 1e-10).astype(int), np.trunc(r.sx + 1e-10).astype(int)
    rr, cc = np.nonzero(tile_mask)
    return iy[rr], ix[cc]


@case
def A4_negative_zero():
    """float32, nodata 0.0: the canvas holds +0.0 where the newer granule has
    holes, the older granules hold -0.0 exactly there, on `inside` rows.
    -0.0 == 0.0, so the reference takes nothing and the canvas keeps +0.0."""
    gs, tiles, pairs = _two_entries(np.float32, 0.0, 47)
    holes = NnRef(gs[0], TILE).val == 0.0
    assert 300 < holes.sum() < 0.5 * holes.size
    for old in gs[1:3]:
        old.data[_source_of(old, holes)] = -0.0
    c = Case(_cfg("A4 -0.0", gs, tiles[:2], pairs[:2], scale=INT_SCALE[np.float32]))
    for t, (refs, merged) in enumerate(c.ref):
        canvas, _, modes = merged[0]
        r_old = refs[pairs[t].index(t + 1)]
        assert (bits(r_old.val)[holes] == 0x80000000).all() and r_old.has.all()
        assert modes[1][0]      # the older entry folds in fill mode
        assert (bits(canvas)[holes] == 0).all() and not (bits(canvas) == 0x80000000).any()
    return c


# A5: merge order
def _stack(n, equal_ts, seed):
    rng = np.random.default_rng(seed)
    days = {2: (1, 0), 3: (1, 0, 2), 5: (2, 0, 3, 1, 4)}[n]
    gs = []
    for k in range(n):   # the stack is in this order (POLYS); an entry fills where its day is below an earlier one's
        gs.append(nn_gran(_vals(rng, 26, 70, np.int16, -999.0), 1.0, 2.25 + 3 * k, 1.5 - k, -999.0,
                          T0 if equal_ts else T0 + DAY * days[k], POLYS[k]))
    order = list(range(n))
    return gs, [TILE] * 2, [order, order[::-1]]


def _merge_case(n, equal_ts):
    c = Case(_cfg("A5 %d entries %s" % (n, "equal ts" if equal_ts else "distinct ts"), *_stack(n, equal_ts, 48 + n)),
             paths=("rgba", "canvas", "cov", "generic"))
    for refs, merged in c.ref:
        modes = merged[0][2]
        assert len(modes) == n and all(m[1] > 0 for m in modes)
        if equal_ts:
            assert not any(m[0] for m in modes)
        else:
            assert any(m[0] for m in modes) and (n == 2 or any(not m[0] for m in modes[1:]))
    assert np.array_equal(c.ref[0][1][0][0], c.ref[1][1][0][0]) or equal_ts
    return c


for _n in (2, 3, 5):
    for _eq in (False, True):
        CASES["A5_%d_%s" % (_n, "equal" if _eq else "distinct")] = functools.lru_cache(None)(
            functools.partial(_merge_case, _n, _eq))


@case
def A5_rgb_three_namespaces():
    """Three namespaces in one render: launch_render has no band kernel for
    it, the generic dispatch_render_3 renders every tile."""
    rng = np.random.default_rng(55)
    gs = []
    for k, ns in enumerate("rgb"):
        gs.append(nn_gran(_vals(rng, 26, 70, np.int16, -999.0), 1.0, 2.5 + k, 1.5 - k, -999.0, T0 + DAY, POLYS[k], ns))
        gs.append(nn_gran(_vals(rng, 30, 90, np.int16, -999.0), 1.0, -3.5, -2.5, -999.0, T0, POLYS[8 + k], ns))
    c = Case(_cfg("A5 rgb", gs, [TILE], [list(range(6))], namespaces=("r", "g", "b"), scale=(0.0, 0.0, 30000.0, 0),
                  palette=None), paths=("i", "generic"))
    assert all(any(m[0] for m in merged[2]) and all(m[1] > 0 for m in merged[2]) for merged in c.ref[0][1])
    return c


# A6: the mask layer
def _mask_case(name, mdt, mask, m_ratio=1.0, m_extra=0, two=False, data_dt=np.int16):
    """A data granule (two: and an older one) on TILE, each with a mask
    granule of the same stamp: on the data's grid (m_ratio 1), at another
    pixel ratio over the same footprint, or m_extra columns wider."""
    rng = np.random.default_rng(56)
    gs, pairs = [], []
    for k in range(2 if two else 1):
        ny, nx = 16, 48
        left, top = 6.5 + 5 * k, 2.5 + 2 * k
        ts, poly = T0 + DAY * (1 - k), POLYS[k]
        gs.append(nn_gran(_vals(rng, ny, nx, data_dt, -999.0), 1.0, left, top, -999.0, ts, poly))
        my, mx = int(ny / m_ratio), int(nx / m_ratio) + m_extra
        qa = rng.integers(0, 8, (my, mx)).astype(mdt)
        gs.append(nn_gran(qa, m_ratio, left, top, None, ts, poly, ns="qa"))
    c = Case(_cfg(name, gs, [TILE], [list(range(len(gs)))], mask=mask))
    refs, merged = c.ref[0]
    modes = merged[0][2]
    assert all(m[1] > 50 and m[2] > 50 for m in modes) and (not two or modes[1][0])
    return c


VALUE = dict(id="qa", value="00000001", inclusive=False)
TESTS = dict(id="qa", bit_tests=["00000011", "00000010", "00000100", "00000100"], inclusive=False)


@case
def A6a_same_grid_byte():
    c = _mask_case("A6a byte", np.uint8, VALUE, two=True)
    assert c.ref[0][0][0].win == c.ref[0][0][1].win
    return c


@case
def A6a_same_grid_uint16_bit_tests():
    c = _mask_case("A6a uint16", np.uint16, TESTS, two=True)
    assert c.ref[0][0][0].win == c.ref[0][0][1].win
    return c


@case
def A6a_same_grid_inclusive():
    """An inclusive mask layer is a stack entry of its own namespace as well;
    Byte data and a Byte mask keep the tile on the band kernel."""
    return _mask_case("A6a inclusive", np.uint8, dict(VALUE, inclusive=True), two=True, data_dt=np.uint8)


@case
def A6b_other_ratio():
    c = _mask_case("A6b ratio 2", np.uint8, TESTS, m_ratio=2.0, two=True)
    assert c.ref[0][0][0].win == c.ref[0][0][1].win      # same footprint, another row record
    return c


@case
def A6c_wider_mask_window():
    c = _mask_case("A6c remap", np.uint8, VALUE, m_extra=9, two=True)
    assert c.ref[0][0][1].win[2] == c.ref[0][0][0].win[2] + 9
    return c


# A7: stacks past 64 entries
def _big_stack(n, masked):
    rng = np.random.default_rng(57)
    gs = []
    for k in range(n):
        ny, nx = int(rng.integers(8, 17)), int(rng.integers(8, 25))
        left, top = float(rng.integers(-4, 90)) + 0.25 * (k % 4), float(rng.integers(-4, 34)) + 0.25 * (k % 3)
        ts, poly = T0 + DAY * int(rng.integers(0, 6)), "S%d" % k
        gs.append(nn_gran(_vals(rng, ny, nx, np.int16, -999.0), 1.0, left, top, -999.0, ts, poly))
        if masked:
            gs.append(nn_gran(rng.integers(0, 4, (ny, nx)).astype(np.uint8), 1.0, left, top, None, ts, poly, ns="qa"))
    c = Case(_cfg("A7 %d entries%s" % (n, " masked" if masked else ""), gs, [nn_tile(96, 40)], [list(range(len(gs)))],
                  mask=VALUE if masked else None), paths=("rgba", "canvas", "generic"))
    modes = c.ref[0][1][0][2]
    assert len(modes) == n and sum(1 for m in modes if m[0] and m[1] > 0) > n // 4
    assert sum(1 for m in modes[64:] if m[1] > 0) >= 3 and (n < 130 or sum(1 for m in modes[128:] if m[1] > 0) >= 1)
    assert not masked or sum(m[2] for m in modes) > 500
    return c


CASES["A7_70_masked"] = functools.lru_cache(None)(functools.partial(_big_stack, 70, True))
CASES["A7_130_masked"] = functools.lru_cache(None)(functools.partial(_big_stack, 130, True))
CASES["A7_70_serial"] = functools.lru_cache(None)(functools.partial(_big_stack, 70, False))


# A9: scale and palette on the band kernel's own output stage
SCALES = [(0.0, 0.0, 0.0, 0), (0.0, 0.0, 1000.0, 0), (-5.0, 0.5, 300.0, 0), (-1e3, 0.0, 70000.0, 0)]


def _scale_case(dt, k, pal):
    rng = np.random.default_rng(58)
    nodata = -999.0
    off, _, clip, _ = SCALES[k]
    v = _vals(rng, 30, 90, dt, nodata, 0.1)
    lo, hi = (-3.0e38, 3.0e38) if dt == np.float32 else (np.iinfo(dt).min, np.iinfo(dt).max)
    special = [0, clip - off, clip - off + 1, clip, clip + 1, -off, -off - 1, lo, hi, nodata]
    special = np.clip(special, lo, hi).astype(dt)
    v[5, 10:10 + len(special)] = special
    g = nn_gran(v, 1.0, -3.25, -2.25, nodata)
    c = Case(_cfg("A9 %s scale %d %s" % (np.dtype(dt).name, k, "palette" if pal else "grey"), [g], [TILE], [[0]],
                  scale=SCALES[k], palette=PAL if pal else None), paths=("rgba", "generic"))
    assert set(special.tolist()) <= set(c.ref[0][0][0].val.reshape(-1).tolist())
    return c


for _dt in (np.int16, np.float32):
    for _k in range(4):
        for _p in (True, False):
            CASES["A9_%s_%d_%s" % (np.dtype(_dt).name, _k, "pal" if _p else "grey")] = functools.lru_cache(None)(
                functools.partial(_scale_case, _dt, _k, _p))


# ---------------------------------------------------------------- part B: reprojected, the oracle as reference
class _OracleWindow:
    def __init__(self, arr, bbox):
        self.window, self.win = arr, [int(v) for v in bbox]


class OracleCase(Case):
    """A reprojected config: the windows are oracle.warp's, the canvases and
    the RGBA oracle.render_tiles's (same shapes as Case.ref / Case.rgba)."""

    @functools.cached_property
    def ref(self):
        from oracle import oracle as O
        cfg = self.cfg
        gr, crs, ts, ph, ns, geots, slots, mask_ns = oracle_inputs(O, cfg)
        self._rgba, cv, created = oracle_render(O, cfg, canvas=True)
        assert created[:, 0].all()
        dt = window_type(cfg.granules[0].data.dtype)
        mw, mh = max(w for _, w, _ in cfg.tiles), max(h for _, _, h in cfg.tiles)
        out = []
        for t, (_, w, h) in enumerate(cfg.tiles):
            refs = []
            for gi in cfg.pairs[t]:
                arr, bbox, nd, _ = O.warp(gr[gi], crs[gi], O.crs(cfg.dst_srs), geots[t], w, h, 0)
                refs.append(_OracleWindow(arr, bbox))
            canvas = cv[t, 0, : mw * mh * np.dtype(dt).itemsize].view(dt).reshape(mh, mw)[:h, :w].copy()
            out.append((refs, [(canvas, cfg.granules[0].nodata, [])]))
        return out

    def rgba(self, O):
        self.ref
        return [self._rgba[t, :h, :w] for t, (_, w, h) in enumerate(self.cfg.tiles)]


B_CASES = {}
POOL_SIZES = [(513, 48), (77, 50), (77, 33), (513, 17)]


def _pool(dt):
    """EPSG:3577 -> EPSG:3857: rows the approximate transformer splits (POOL
    rows: linear leaves), tiles 513 and 77 px wide, seams of up to four entries."""
    cfg = synth.config_c2(scale=0.05, tiles_per_side=2, tile_px=64)
    if dt != np.int16:
        cfg = cast_cfg(cfg, dt)
        cfg.scale = (0.0, 0.0, 250.0, 0)
    cfg.tiles = [(bb, *POOL_SIZES[i]) for i, (bb, _, _) in enumerate(cfg.tiles)]
    return OracleCase(cfg)


for _dt in (np.int16, np.uint8):
    B_CASES["B_pool_%s" % np.dtype(_dt).name] = functools.lru_cache(None)(functools.partial(_pool, _dt))


# ---------------------------------------------------------------- the comparison
def _count(path, n):
    COUNTS[path] = COUNTS.get(path, 0) + int(n)


def _canvas(cv, b, dt, k=0):
    n = b.max_h * b.max_w * np.dtype(dt).itemsize
    return cv.cpu().numpy()[:, k, :n].copy().view(dt).reshape(-1, b.max_h, b.max_w)


def differing(c, O):
    """Every path of case `c` against its reference: the list of (path, tile
    or pair, what) that differ -- empty when all bytes agree."""
    import torch

    import gsky_amd
    cfg = c.cfg
    b = gpu_batch(cfg)
    sp = gsky_amd.ScaleParams(*cfg.scale)
    pal = gsky_amd.Palette(cfg.palette, True) if cfg.palette else None
    bad = []
    n_ns = len(cfg.namespaces)
    if "i" in c.paths:
        wins = b.warp_windows(0)
        p = 0
        for t, (refs, _) in enumerate(c.ref):
            for k, gi in enumerate(cfg.pairs[t]):
                arr, bbox, tname, nd = wins[p]
                p += 1
                r, g = refs[k], cfg.granules[gi]
                a = arr.cpu().numpy()
                gnd = -1e10 if g.nodata is None else g.nodata
                if bbox != r.win or tname != TYPE_NAME[window_type(g.data.dtype)] or not (nd == gnd or (nd != nd and gnd != gnd)):
                    bad.append(("(i)", t, gi, "box / type / nodata", bbox, r.win, tname, nd))
                elif a.dtype != r.window.dtype or not np.array_equal(bits(a), bits(r.window)):
                    bad.append(("(i)", t, gi, "bytes"))
                _count("(i) windows", a.size)
        assert p == len(wins)

    def canvases(path, cv):
        for k in range(n_ns):
            for t, (_, merged) in enumerate(c.ref):
                exp = merged[k][0]
                h, w = exp.shape
                got = _canvas(cv, b, exp.dtype, k)[t, :h, :w]
                if not np.array_equal(bits(got), bits(exp)):
                    bad.append((path, t, k, "canvas", int((bits(got) != bits(exp)).sum())))
                _count(path, exp.size)

    def rgba(path, got):
        for t, exp in enumerate(c.rgba(O)):
            h, w = exp.shape[:2]
            if not np.array_equal(got[t, :h, :w], exp):
                bad.append((path, t, "rgba", int((got[t, :h, :w] != exp).any(-1).sum())))
            _count(path, h * w)

    tag = "(iv)" if cfg.mask else "(ii)/(iii)"
    for typed in (True, False):
        if not typed and "generic" not in c.paths:
            continue
        b.typed = typed
        name = tag if typed else "(v)"
        if n_ns == 3:
            out, cv = b.render(sp, None, canvas=True)
            rgba("(v) rgb", out.cpu().numpy())
            canvases("(v) rgb canvas", cv)
        else:
            if "rgba" in c.paths:
                rgba(name + " rgba", b.render(sp, pal).cpu().numpy().copy())
                if b.status() != 0:
                    bad.append((name, "status", b.status()))
            if "canvas" in c.paths:
                canvases(name + " canvas", b.render(sp, pal, rgba=False))
            if "cov" in c.paths:
                exp0 = c.ref[0][1][0][0]
                out = torch.from_numpy(np.full((len(cfg.tiles) * b.max_h, b.max_w), 77, exp0.dtype)).to(b.device)
                b.render_coverage(sp, out, [t * b.max_h * b.max_w for t in range(len(cfg.tiles))], resample=0)
                got = out.cpu().numpy().reshape(len(cfg.tiles), b.max_h, b.max_w)
                for t, (_, merged) in enumerate(c.ref):
                    exp = merged[0][0]
                    h, w = exp.shape
                    if not np.array_equal(bits(got[t, :h, :w]), bits(exp)):
                        bad.append((name + " coverage", t, int((bits(got[t, :h, :w]) != bits(exp)).sum())))
                    _count(name + " coverage", exp.size)
        if b.status() != 0:
            bad.append((name, "status", b.status()))
    b.typed = True
    c.batch = b
    return bad


def _show(what):
    print("\n[nn_edges] %s: pixels compared so far, no difference: %s"
          % (what, ", ".join("%s %d" % kv for kv in sorted(COUNTS.items()))))


# ---------------------------------------------------------------- part A
@pytest.mark.parametrize("name", sorted(CASES))
def test_part_a(gpu, oracle, name):
    c = CASES[name]()
    assert differing(c, oracle) == []
    _show(name)


@pytest.mark.parametrize("name", sorted(B_CASES))
def test_part_b(gpu, oracle, name):
    c = B_CASES[name]()
    assert differing(c, oracle) == []
    info = c.batch.tile_info()
    assert (info[:, 0] == 0).all()
    if name.startswith("B_pool"):
        assert c.batch.plan_counters["pool_leaves"] > 0 and (info[:, 1] == 0).all()
    print("\n[nn_edges] %s: plan counters %r, complex tiles %r" % (name, c.batch.plan_counters, info[:, 1].tolist()))
    _show(name)


def a8_case():
    """A8: Int32, UInt32 and Float64 granules: the warp promotes them to a
    float32 window (warp.go:339-343), the value is float32(source); their
    tiles are complex (no typed band kernel)."""
    rng = np.random.default_rng(60)
    datas = [rng.integers(-2 ** 31, 2 ** 31 - 1, (14, 50)).astype(np.int32),
             rng.integers(0, 2 ** 32 - 1, (14, 50)).astype(np.uint32), rng.uniform(-1e9, 1e9, (14, 50))]
    for d in datas:
        d[rng.random(d.shape) < 0.2] = 5
    gs = [nn_gran(d, 1.0, 5.5, 3.5, 5.0, poly=POLYS[k]) for k, d in enumerate(datas)]
    c = Case(_cfg("A8 promoted", gs, [TILE] * 3, [[0], [1], [2]], scale=(2.0e9, 0.0, 4.0e9, 0)),
             paths=("i", "rgba", "canvas", "generic"))
    for (refs, merged), d in zip(c.ref, datas):
        r = refs[0]
        assert r.val.dtype == np.float32 and r.win[:2] == [5, 3]
        assert (r.window[:12, :40].astype(np.float64) != d[:12, :40]).sum() > 200     # the promotion rounds
        assert merged[0][2][0][1] > 300 and (merged[0][0] == np.float32(5.0)).sum() > 100
    return c


def test_a8_promoted_types(gpu, oracle, monkeypatch):
    """TileBatch has no name for a UInt32 tensor: the library's type code is
    registered for the test's duration (as tests/test_cubic.py does)."""
    import torch

    from gsky_amd import _lib, tiles as tiles_mod
    monkeypatch.setitem(tiles_mod.DTYPE_OF_TORCH, torch.uint32, _lib.UINT32)
    c = a8_case()
    assert differing(c, oracle) == []
    info = c.batch.tile_info()
    assert (info[:, 0] == 0).all() and (info[:, 1] == 1).all()       # complex: the general kernel rendered them
    _show("A8")


def test_a4_negative_zero_runs_on_an_inside_row(gpu):
    """The -0.0 case reaches the fast bodies: its tiles are simple, single
    typed, and the older entry covers every column."""
    c = CASES["A4_negative_zero"]()
    b = gpu_batch(c.cfg)
    import gsky_amd
    b.render(gsky_amd.ScaleParams(*c.cfg.scale), rgba=False)
    info = b.tile_info()
    assert (info[:, 0] == 0).all() and (info[:, 1] == 0).all() and b.plan_counters["complex_tiles"] == 0


def test_a6d_smaller_mask_footprint_is_refused(gpu, oracle):
    """A6 (d): a mask raster with fewer window pixels than its data raster:
    the reference indexes the mask past its end (Go panics); the planner
    answers GSKYHIP_E_RANGE for the tile, as the merge stage does."""
    import gsky_amd
    E_RANGE = -7      # GSKYHIP_E_RANGE, include/gskyhip.h
    rng = np.random.default_rng(59)
    data = nn_gran(_vals(rng, 16, 48, np.int16, -999.0), 1.0, 6.5, 2.5, -999.0, T0, "M")
    qa = nn_gran(rng.integers(0, 4, (10, 30)).astype(np.uint8), 1.0, 6.5, 2.5, None, T0, "M", ns="qa")
    ok = nn_gran(_vals(rng, 16, 48, np.int16, -999.0), 1.0, 6.5, 2.5, -999.0, T0, "K")
    cfg = _cfg("A6d", [data, qa, ok], [TILE, TILE], [[0, 1], [2]], mask=VALUE)
    rd, rm = NnRef(data, TILE), NnRef(qa, TILE)
    assert rd.win[2] * rd.win[3] > rm.win[2] * rm.win[3]
    with pytest.raises(RuntimeError):     # the oracle restates the panic as an error of the whole call
        oracle_render(oracle, cfg)
    b = gpu_batch(cfg)
    for typed in (True, False):
        b.typed = typed
        b.render(gsky_amd.ScaleParams(*cfg.scale), gsky_amd.Palette(PAL, True))
        assert b.status() == E_RANGE
        info = b.tile_info()
        assert info[0, 0] == E_RANGE and info[1, 0] == 0


# ---------------------------------------------------------------- (vi): the A/B shapes
CHILD = r"""
import json, sys
sys.path.insert(0, %(root)r)
from oracle import oracle as O
from tests import test_nn_edges as M
res = {}
for name, build in sorted(list(M.CASES.items()) + list(M.B_CASES.items())):
    res[name] = [repr(d) for d in M.differing(build(), O)]
print(json.dumps({"differ": res, "counts": M.COUNTS}))
"""

KNOBS = [{"GSKYHIP_NN_RPW": "4", "GSKYHIP_NN_MASK_RPW": "4"},
         {"GSKYHIP_NN_RPW": "8", "GSKYHIP_NN_ONE": "1", "GSKYHIP_NN_MASK_RPW": "1"},
         {"GSKYHIP_NN_RPW": "8", "GSKYHIP_NN_ONE": "0", "GSKYHIP_NN_MASK_RPW": "1", "GSKYHIP_NN_MASK_WPE": "0"},
         {"GSKYHIP_NN_RPW": "1", "GSKYHIP_NN_MASK_RPW": "1", "GSKYHIP_NN_MASK_WPE": "8"}]


@pytest.mark.parametrize("knobs", KNOBS, ids=lambda k: "-".join("%s%s" % (n[8:], v) for n, v in sorted(k.items())))
def test_ab_shapes(gpu, knobs):
    lib = os.path.join(ROOT, "gsky_amd", "libgskyhip_ab.so")
    if not os.path.exists(lib):
        pytest.fail("A/B build not present (build() makes it: make -C gsky_amd/csrc ab)")
    env = dict(os.environ, GSKYHIP_LIB="ab", **knobs)
    p = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], env=env, capture_output=True, text=True,
                       timeout=240, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    assert len(res["differ"]) == len(CASES) + len(B_CASES)
    print("\n[nn_edges] (vi) %r: %s" % (knobs, ", ".join("%s %d" % kv for kv in sorted(res["counts"].items()))))
    assert {k: v for k, v in res["differ"].items() if v} == {}, knobs
