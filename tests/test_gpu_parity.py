"""GPU parity tests: the MI355X path (libgskyhip.so through its C-ABI) against
the CPU oracle on the same seeded inputs.

Bars (BASELINE.json north_star): scale, palette, merge, mask, drill -- bit
exact; nearest-neighbour warp and the fused tile path -- 100 % of pixels
identical (the north_star admits 99.99 %; every case here measures 100 %, so
the bar is exact and any future drift fails); bilinear -- identical nodata
positions and every valid value within 1e-4 relative.
"""
import numpy as np
import pytest

from gsky_amd import synth

from .helpers import bilinear_tie_masks, gpu_batch, identity, oracle_inputs, oracle_render
from .helpers import cast_cfg as _cast_cfg

pytestmark = pytest.mark.gpu

NN_IDENTITY = 1.0
BILINEAR_RTOL = 1e-4
TYPES = [np.uint8, np.int8, np.int16, np.uint16, np.float32]


def _rand(dt, n, rng):
    if dt == np.float32:
        v = rng.normal(300, 400, n).astype(np.float32)
        v[rng.random(n) < 0.05] = -9999.0
        v[rng.random(n) < 0.01] = np.nan
        v[:3] = [0.0, -0.0, 1e30]
        return v
    info = np.iinfo(dt)
    v = rng.integers(info.min, int(info.max) + 1, n).astype(dt)
    return v


SCALE_PARAMS = [(0, 0, 0), (0, 0, 1000), (1, 1, 1000), (3, 2, 2), (-5, 0.5, 300), (0, 0, 10000),
                (100.5, 0, 254), (0, 3.5, 0), (-1e3, 0, 70000)]


@pytest.mark.parametrize("dt", TYPES)
@pytest.mark.parametrize("sp", SCALE_PARAMS)
def test_scale_parity(gpu, oracle, dt, sp):
    import torch

    import gsky_amd
    rng = np.random.default_rng(hash((dt.__name__, sp)) & 0xFFFF)
    n = 100003
    data = _rand(dt, n, rng)
    nodata = -9999.0 if dt == np.float32 else float(data[17])
    for first_valid in (True, False):
        d = data.copy()
        if not first_valid:
            d[0] = d[17] if dt != np.float32 else np.float32(-9999.0)
        exp = oracle.scale(d, nodata, *sp)
        t = torch.from_numpy(d).to(gpu)
        tname = "SignedByte" if dt == np.int8 else None
        got = gsky_amd.scale([t], [nodata], gsky_amd.ScaleParams(*sp), [tname] if tname else None)[0]
        assert np.array_equal(got.cpu().numpy(), exp), (dt, sp, first_valid)


def test_scale_log_parity(gpu, oracle):
    import torch

    import gsky_amd
    rng = np.random.default_rng(7)
    d = rng.lognormal(2, 2, 50000).astype(np.float32)
    d[::97] = 0.0
    d[::101] = -3.0
    d[::103] = -9999.0
    for sp in [(0, 0, 0, 1), (0, 1, 5, 1), (1, 20, 6, 1), (0, 0, 0, 2)]:
        exp = oracle.scale(d, -9999.0, sp[0], sp[1], sp[2], colour_scale=sp[3])
        got = gsky_amd.scale([torch.from_numpy(d).to(gpu)], [-9999.0], gsky_amd.ScaleParams(*sp))[0]
        assert np.array_equal(got.cpu().numpy(), exp), sp


@pytest.mark.parametrize("dt", [np.uint8, np.int16, np.uint16, np.float32])
def test_scale_legacy_parity(gpu, oracle, dt):
    import torch

    import gsky_amd
    rng = np.random.default_rng(3)
    d = _rand(dt, 20000, rng)
    for sp in [(0, 0.5, 200), (2, 1.5, 1000)]:
        exp = oracle.scale_legacy(d, -9999.0 if dt == np.float32 else 7, *sp)
        got = gsky_amd.scale_legacy(torch.from_numpy(d.copy()).to(gpu), -9999.0 if dt == np.float32 else 7,
                                    gsky_amd.ScaleParams(*sp))
        assert np.array_equal(got.cpu().numpy(), exp)


def test_palette_and_rgba_parity(gpu, oracle):
    import torch

    import gsky_amd
    rng = np.random.default_rng(11)
    for n in (2, 3, 5, 7, 13, 200, 300):
        cols = rng.integers(0, 256, (n, 4)).astype(np.uint8)
        for interp in (True, False):
            if interp and n > 257:   # sectionLength 0: the reference panics (palette.go:12)
                continue
            exp = oracle.gradient_palette(cols, interp)
            got = gsky_amd.gradient_rgba_palette(gsky_amd.Palette(cols.tolist(), interp))
            assert np.array_equal(got, exp)
    b = [rng.integers(0, 256, (123, 77)).astype(np.uint8) for _ in range(3)]
    for bb in b:
        bb[rng.random(bb.shape) < 0.3] = 255
    pal = gsky_amd.Palette(synth.PALETTE_GSKY, True)
    ramp = oracle.gradient_palette(synth.PALETTE_GSKY, True)
    cases = [([b[0]], pal, ramp), ([b[0]], None, None), (b, None, None)]
    for bands, p, r in cases:
        exp = oracle.encode_rgba(bands, 77, 123, r)
        got = gsky_amd.encode_rgba([torch.from_numpy(x).to(gpu) for x in bands], p)
        assert np.array_equal(got.cpu().numpy(), exp)


MASKS = [("00000001", ()), ("110", ()), ("11111111", ()), ("", ("1", "1", "110", "10")),
         ("1000000000000000", ()), ("-1", ()), ("", ("11111111", "-1"))]


@pytest.mark.parametrize("dt", [np.uint8, np.int8, np.int16, np.uint16])
@pytest.mark.parametrize("mv", MASKS)
def test_compute_mask_parity(gpu, oracle, dt, mv):
    import torch

    import gsky_amd
    rng = np.random.default_rng(5)
    d = _rand(dt, 4096, rng)
    value, tests = mv
    exp = oracle.compute_mask(d, value or None, tests)
    tname = "SignedByte" if dt == np.int8 else None
    got = gsky_amd.compute_mask(gsky_amd.Mask("qa", value, list(tests)), torch.from_numpy(d).to(gpu), tname)
    assert np.array_equal(got.cpu().numpy(), exp)


@pytest.mark.parametrize("seed", range(6))
def test_merge_parity(gpu, oracle, seed):
    """RasterMerger.Run: random windows, timestamps, polygon hashes, masks."""
    import torch

    import gsky_amd
    rng = np.random.default_rng(seed)
    W, H = 97, 61
    dt = [np.int16, np.float32, np.uint8, np.uint16, np.int8, np.int16][seed]
    tname = {np.int16: "Int16", np.float32: "Float32", np.uint8: "Byte", np.uint16: "UInt16",
             np.int8: "SignedByte"}[dt]
    n = 9
    nodata = -9999.0 if dt == np.float32 else (0.0 if dt in (np.uint8, np.uint16) else -1.0)
    polys = ["A", "B", "C"]
    rasters_o, rasters_g = [], []
    use_mask = seed % 2 == 1
    for k in range(n):
        w, h = int(rng.integers(1, W)), int(rng.integers(1, H))
        ox, oy = int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1))
        d = _rand(dt, w * h, rng).reshape(h, w)
        d[rng.random((h, w)) < 0.3] = nodata if dt != np.float32 else -9999.0
        ts = float(rng.integers(0, 4)) * 86400.0
        pg = polys[int(rng.integers(0, 3))]
        ns = "" if rng.random() < 0.8 else "b2"
        rasters_o.append(dict(data=d, off_x=ox, off_y=oy, nodata=nodata, timestamp=ts,
                              polygon_hash=oracle.fnv32a(pg), ns=0 if ns == "" else 1,
                              signed_byte=dt == np.int8))
        rasters_g.append(gsky_amd.FlexRaster(torch.from_numpy(d).to(gpu), W, H, ox, oy, tname, nodata, ns, ts, pg))
        if use_mask:
            q = rng.integers(0, 4, (h, w)).astype(np.uint8)
            rasters_o.append(dict(data=q, off_x=ox, off_y=oy, nodata=255.0, timestamp=ts,
                                  polygon_hash=oracle.fnv32a(pg), ns=2))
            rasters_g.append(gsky_amd.FlexRaster(torch.from_numpy(q).to(gpu), W, H, ox, oy, "Byte", 255.0, "qa",
                                                 ts, pg))
    mask = gsky_amd.Mask("qa", "01") if use_mask else None
    try:
        exp = oracle.merge_batch(rasters_o, 3, W, H, mask_ns=2 if use_mask else -1,
                                 mask_value="01" if use_mask else None)
    except ValueError as ex:
        # mask[iSrc] beyond the mask raster: the reference panics; both sides must refuse
        assert "-3" in str(ex)
        with pytest.raises(gsky_amd.GskyError):
            gsky_amd.raster_merger_run(rasters_g, ["", "b2"], mask)
        return
    got = gsky_amd.raster_merger_run(rasters_g, ["", "b2"], mask)
    for k, ns in enumerate(["", "b2"]):
        e = exp[k]
        g = got[ns]
        if e[0] is None:
            assert g is None
            continue
        assert g is not None and g[1] == e[1]
        ga = g[0].cpu().numpy()
        if dt == np.float32:
            assert np.array_equal(ga.view(np.uint32), e[0].astype(np.float32).view(np.uint32))
        else:
            assert np.array_equal(ga, e[0])


# ---------------------------------------------------------------- warp / render
def _check_windows(O, cfg, batch, resample=0):
    """Every warped window (FlexRaster) of the batch against oracle.warp:
    identical bbox; NN -> identical bytes (returns the identical fraction);
    bilinear -> asserts identical nodata and <= 1e-4 relative everywhere."""
    gr, crs, ts, ph, ns, geots, slots, mask_ns = oracle_inputs(O, cfg)
    wins = batch.warp_windows(resample)
    p = 0
    tot = same = 0
    for t, (bb, w, h) in enumerate(cfg.tiles):
        for gi in cfg.pairs[t]:
            arr, bbox, nd, dt = O.warp(gr[gi], crs[gi], O.crs(cfg.dst_srs), geots[t], w, h, resample)
            g_arr, g_bbox, g_type, g_nd = wins[p]
            p += 1
            assert list(bbox) == g_bbox, (t, gi)
            ga = g_arr.cpu().numpy()
            if resample == 1:
                a64, g64 = arr.astype(np.float64), ga.astype(np.float64)
                assert np.array_equal(a64 == nd, g64 == nd), (t, gi)
                v = a64 != nd
                rel = np.abs(g64[v] - a64[v]) / np.maximum(np.abs(a64[v]), 1e-30)
                assert rel.size == 0 or rel.max() <= BILINEAR_RTOL, (t, gi, rel.max())
                same += ga.size
            else:
                same += int((ga.view(np.uint8) == arr.view(np.uint8)).reshape(ga.shape[0], ga.shape[1], -1).all(-1).sum())
            tot += ga.size
    return same / max(1, tot)


def test_warp_windows_c1(gpu, oracle):
    cfg = synth.config_c1(scale=0.5)
    frac = _check_windows(oracle, cfg, gpu_batch(cfg))
    assert frac >= NN_IDENTITY


def test_warp_windows_c2_small(gpu, oracle):
    cfg = synth.config_c2(scale=0.05, tiles_per_side=3, tile_px=128)
    frac = _check_windows(oracle, cfg, gpu_batch(cfg))
    assert frac >= NN_IDENTITY


def test_warp_windows_bilinear_c3_small(gpu, oracle):
    cfg = synth.config_c3(scale=0.05, chunk_px=96, out_px=288, grid=3)
    frac = _check_windows(oracle, cfg, gpu_batch(cfg), resample=1)
    assert frac >= NN_IDENTITY


def test_warp_windows_utm_small(gpu, oracle):
    """GDA94 / MGA zone 55 (Transverse Mercator) granules -> EPSG:3857."""
    cfg = synth.config_utm(scale=0.05, tiles_per_side=4, tile_px=128)
    frac = _check_windows(oracle, cfg, gpu_batch(cfg))
    assert frac >= NN_IDENTITY


def test_warp_windows_lambert_small(gpu, oracle):
    """GDA94 / Geoscience Australia Lambert (EPSG:3112) granules -> EPSG:3857."""
    cfg = synth.config_lambert(scale=0.05, tiles_per_side=4, tile_px=128)
    frac = _check_windows(oracle, cfg, gpu_batch(cfg))
    assert frac >= NN_IDENTITY


@pytest.mark.parametrize("srs,origin", [("EPSG:3031", (-2400000.0, 1400000.0)),
                                        ("EPSG:3413", (-200000.0, -2000000.0)),
                                        ("EPSG:32761", (-400000.0, 4400000.0))])
def test_warp_windows_polar_small(gpu, oracle, srs, origin):
    """Polar stereographic granules (Antarctic, NSIDC North, UPS South) -> EPSG:3857."""
    cfg = synth.config_polar(scale=0.05, tiles_per_side=4, tile_px=128, srs=srs, origin=origin)
    frac = _check_windows(oracle, cfg, gpu_batch(cfg))
    assert frac >= NN_IDENTITY


def test_render_polar_small(gpu, oracle):
    import gsky_amd
    cfg = synth.config_polar(scale=0.1, tiles_per_side=4, tile_px=256)
    b = gpu_batch(cfg)
    got = b.render(gsky_amd.ScaleParams(*cfg.scale), gsky_amd.Palette(cfg.palette, True)).cpu().numpy()
    assert b.status() == 0
    exp = oracle_render(oracle, cfg)
    assert identity(got, exp) >= NN_IDENTITY
    assert (exp[..., 3] > 0).mean() > 0.3


def test_render_lambert_small(gpu, oracle):
    import gsky_amd
    cfg = synth.config_lambert(scale=0.1, tiles_per_side=4, tile_px=256)
    b = gpu_batch(cfg)
    got = b.render(gsky_amd.ScaleParams(*cfg.scale), gsky_amd.Palette(cfg.palette, True)).cpu().numpy()
    assert b.status() == 0
    exp = oracle_render(oracle, cfg)
    assert identity(got, exp) >= NN_IDENTITY
    assert (exp[..., 3] > 0).mean() > 0.3


def test_render_utm_small(gpu, oracle):
    import gsky_amd
    cfg = synth.config_utm(scale=0.1, tiles_per_side=4, tile_px=256)
    b = gpu_batch(cfg)
    got = b.render(gsky_amd.ScaleParams(*cfg.scale), gsky_amd.Palette(cfg.palette, True)).cpu().numpy()
    assert b.status() == 0
    exp = oracle_render(oracle, cfg)
    assert identity(got, exp) >= NN_IDENTITY
    assert (exp[..., 3] > 0).mean() > 0.3


def test_warp_operation_fast_utm_dropin(gpu, oracle):
    """warp.go:82 for a UTM granule given as WKT (the source SRS a GDAL
    dataset reports), to EPSG:3857 and to another MGA zone."""
    import torch

    from gsky_amd import worker
    from gsky_amd.tiles import bbox_to_geot
    cfg = synth.config_utm(scale=0.1, tiles_per_side=4, tile_px=256)
    g = cfg.granules[0]
    wkt = ('PROJCS["GDA94 / MGA zone 55",GEOGCS["GDA94",DATUM["Geocentric_Datum_of_Australia_1994",'
           'SPHEROID["GRS 1980",6378137,298.257222101]],PRIMEM["Greenwich",0],UNIT["degree",0.0174532925199433]],'
           'PROJECTION["Transverse_Mercator"],PARAMETER["latitude_of_origin",0],PARAMETER["central_meridian",147],'
           'PARAMETER["scale_factor",0.9996],PARAMETER["false_easting",500000],'
           'PARAMETER["false_northing",10000000],UNIT["metre",1]]')
    worker.register_granule("/g/data/utm/g0.tif", 1, torch.from_numpy(g.data).to(gpu), g.geot, wkt, g.nodata,
                            block=(128, 64))
    try:
        og = oracle.make_granule(g.data, g.geot, g.nodata, block=(128, 64))
        bb, w, h = cfg.tiles[5]
        for dst, dst_gt in (("EPSG:3857", bbox_to_geot(w, h, bb)),
                            ("EPSG:28354", [830000.0, 40.0, 0.0, 5880000.0, 0.0, -40.0])):
            res = worker.warp_raster(worker.GeoRPCGranule(path="/g/data/utm/g0.tif", bands=[1], width=w, height=h,
                                                          dstSRS=dst, dstGeot=dst_gt))
            assert res.error == "OK", (dst, res.error)
            arr, bbox, nd, dt = oracle.warp(og, oracle.crs("EPSG:28355"), oracle.crs(dst), dst_gt, w, h)
            assert res.raster.bbox == list(bbox), (dst, res.raster.bbox, bbox)
            got = worker.raster_array(res.raster)
            assert identity(got, arr) >= NN_IDENTITY, dst
            assert (got != g.nodata).mean() > 0.3, dst
            assert res.bytesRead == oracle.warp.bytes_read > 0
    finally:
        worker.unregister_all()


def test_render_c1(gpu, oracle):
    import gsky_amd
    cfg = synth.config_c1(scale=1.0)
    b = gpu_batch(cfg)
    got = b.render(gsky_amd.ScaleParams(*cfg.scale)).cpu().numpy()
    assert b.status() == 0
    exp = oracle_render(oracle, cfg)
    assert identity(got, exp) >= NN_IDENTITY


@pytest.mark.parametrize("n_tiles", [1, 2, 3])
def test_render_small_batch_complex_tiles(gpu, oracle, n_tiles):
    """Small batches (the one-workgroup planner, one-row-per-wave band
    kernel) with a complex tile beside simple ones: an Int32 granule, which
    the merge promotes to a Float32 canvas (vt 0: render_general_kernel's
    body); the other tiles are the same request moved east over float32
    data.  One tile also takes the planner's one-tile schedule (tile plan
    beside the row records)."""
    import dataclasses

    import gsky_amd
    cfg = synth.config_c1(scale=0.5)
    g0 = cfg.granules[0]
    gi = dataclasses.replace(g0, data=np.where(g0.data == -9999.0, -9999, g0.data * 7.0).astype(np.int32))
    x0, y0, x1, y1 = cfg.tiles[0][0]
    tiles = [((x0 + k * (x1 - x0), y0, x1 + k * (x1 - x0), y1), 256, 256) for k in range(n_tiles)]
    cfg = dataclasses.replace(cfg, granules=[gi, g0], tiles=tiles, pairs=[[0]] + [[1]] * (n_tiles - 1),
                              scale=(0.0, 0.0, 7000.0, 0))
    b = gpu_batch(cfg)
    got = b.render(gsky_amd.ScaleParams(*cfg.scale)).cpu().numpy()
    assert b.status() == 0
    exp = oracle_render(oracle, cfg)
    assert identity(got, exp) >= NN_IDENTITY
    assert (exp[0, ..., 3] > 0).mean() > 0.5


def test_render_c2_small(gpu, oracle):
    import gsky_amd
    cfg = synth.config_c2(scale=0.1, tiles_per_side=4, tile_px=256)
    b = gpu_batch(cfg)
    got = b.render(gsky_amd.ScaleParams(*cfg.scale), gsky_amd.Palette(cfg.palette, True)).cpu().numpy()
    assert b.status() == 0
    exp = oracle_render(oracle, cfg)
    assert identity(got, exp) >= NN_IDENTITY
    assert (exp[..., 3] > 0).mean() > 0.3      # the test exercises real data


@pytest.mark.parametrize("nodata", [40000.0, -999.0])
def test_render_seams_window_fill(gpu, oracle, nodata):
    """Granule seams (tiles with 2+ stack entries whose window rows leave the
    band): with the nodata in range the band kernel folds those rows over
    their in-band spans (RowRec.v[4]); with an int16 nodata out of range the
    window fill (GDALCopyWords: clamped, 32767) differs from the merge nodata
    (Go int16(): wrapped, -25536), the pixels off the span fold the fill, and
    the span path must stay off.  Both against the oracle."""
    import dataclasses

    import gsky_amd
    cfg = synth.config_c2(scale=0.1, tiles_per_side=4, tile_px=256)
    cfg = dataclasses.replace(cfg, granules=[dataclasses.replace(g, nodata=nodata) for g in cfg.granules])
    assert any(len(p) >= 2 for p in cfg.pairs)   # the batch has seam tiles
    b = gpu_batch(cfg)
    got = b.render(gsky_amd.ScaleParams(*cfg.scale), gsky_amd.Palette(cfg.palette, True)).cpu().numpy()
    assert b.status() == 0
    exp = oracle_render(oracle, cfg)
    assert identity(got, exp) >= NN_IDENTITY


def test_render_acceptance_requests(gpu, oracle):
    """The reference's own 500 acceptance GetMap requests
    (acceptance_tests/acpt_url.tpl -> tests/golden/acpt_bboxes.json: 256^2
    EPSG:3857 tiles at zooms 6-9 over Australia, 179 distinct) as one tile
    batch over six overlapping synthetic EPSG:4326 granules: every RGBA
    pixel identical to the oracle's."""
    import json
    import os

    import gsky_amd
    reqs = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "acpt_bboxes.json")))
    assert len(reqs) == 500
    cfg = synth.config_acpt(reqs)
    assert all(cfg.pairs) and max(len(p) for p in cfg.pairs) >= 2
    b = gpu_batch(cfg, gpu)
    got = b.render(gsky_amd.ScaleParams(*cfg.scale), gsky_amd.Palette(cfg.palette, True)).cpu().numpy()
    assert b.status() == 0
    exp = oracle_render(oracle, cfg)
    assert identity(got, exp) == 1.0
    assert (exp[..., 3] > 0).mean() > 0.5


def test_render_auto_scale(gpu, oracle):
    import gsky_amd
    cfg = synth.config_c2(scale=0.05, tiles_per_side=3, tile_px=128)
    cfg.scale = (0.0, 0.0, 0.0, 0)
    b = gpu_batch(cfg)
    got = b.render(gsky_amd.ScaleParams(*cfg.scale), gsky_amd.Palette(cfg.palette, True)).cpu().numpy()
    exp = oracle_render(oracle, cfg)
    assert identity(got, exp) >= NN_IDENTITY


def test_render_c5_small_masks_overviews(gpu, oracle):
    import gsky_amd
    cfg = synth.config_c5(scale=0.05, dates=2, zooms=((4, 11, 8, 2), (5, 22, 16, 3)), tile_px=128)
    b = gpu_batch(cfg)
    got = b.render(gsky_amd.ScaleParams(*cfg.scale)).cpu().numpy()
    assert b.status() == 0
    exp = oracle_render(oracle, cfg)
    assert identity(got, exp) >= NN_IDENTITY
    assert (exp[..., 3] > 0).mean() > 0.05


def test_render_c3_small_bilinear_canvas(gpu, oracle):
    """Typed float canvases of the bilinear chunk batch against the oracle's
    merged canvases: identical nodata, every valid value within 1e-4."""
    import gsky_amd
    cfg = synth.config_c3(scale=0.05, chunk_px=96, out_px=288, grid=3)
    b = gpu_batch(cfg)
    _, cv = b.render(gsky_amd.ScaleParams(*cfg.scale), resample=1, canvas=True)
    _, ecv, created = oracle_render(oracle, cfg, canvas=True)
    assert created[:, 0].all()
    g = cv.cpu().numpy()[:, 0, : b.max_h * b.max_w * 4].view(np.float32)
    e = ecv[:, 0, : b.max_h * b.max_w * 4].view(np.float32)
    assert np.array_equal(g == -9999.0, e == -9999.0)
    v = e != -9999.0
    rel = np.abs(g[v].astype(np.float64) - e[v]) / np.maximum(np.abs(e[v].astype(np.float64)), 1e-30)
    assert v.mean() > 0.5 and rel.max() <= BILINEAR_RTOL


def test_render_mixed_tile_sizes(gpu, oracle):
    """Tiles of different sizes in one batch land in their own max_h x max_w
    slot (row stride max_w) and match the oracle exactly."""
    import gsky_amd
    cfg = synth.config_c2(scale=0.1, tiles_per_side=4, tile_px=128)
    sizes = [(128, 96), (64, 128), (100, 77), (127, 127), (5, 9), (128, 128)]
    cfg.tiles = [(bb, *sizes[i % len(sizes)]) for i, (bb, _, _) in enumerate(cfg.tiles)]
    b = gpu_batch(cfg)
    got = b.render(gsky_amd.ScaleParams(*cfg.scale), gsky_amd.Palette(cfg.palette, True)).cpu().numpy()
    assert b.status() == 0
    exp = oracle_render(oracle, cfg)
    for t, (_, w, h) in enumerate(cfg.tiles):
        assert np.array_equal(got[t, :h, :w], exp[t, :h, :w]), t
    assert (exp[..., 3] > 0).mean() > 0.2


@pytest.mark.parametrize("typed", [True, False])
def test_render_empty_tiles_written(gpu, oracle, typed):
    """A tile no granule covers (an empty MAS answer) is still written:
    transparent RGBA like the oracle, whatever the output buffer held (the
    caching allocator hands back used memory), on the typed band path and the
    generic one."""
    import torch

    import gsky_amd
    cfg = synth.config_c2(scale=0.1, tiles_per_side=3, tile_px=128)
    far = (-1.0e7, 8.0e6, -9.9e6, 8.1e6)   # EPSG:3857 box far from the Albers granules
    cfg.tiles = list(cfg.tiles) + [(far, 128, 128)]
    cfg.pairs = list(cfg.pairs) + [[]]
    cfg.tiles.insert(2, (far, 128, 128))
    cfg.pairs.insert(2, [0])              # a granule listed but not intersecting
    b = gpu_batch(cfg)
    b.typed = typed
    out = torch.full((len(cfg.tiles), b.max_h, b.max_w, 4), 0xAB, dtype=torch.uint8, device="cuda")
    got = b.render(gsky_amd.ScaleParams(*cfg.scale), gsky_amd.Palette(cfg.palette, True), out=out).cpu().numpy()
    assert b.status() == 0
    exp = oracle_render(oracle, cfg)
    assert np.array_equal(got, exp)
    assert not got[-1].any() and not got[2].any()


@pytest.mark.parametrize("dst", ["EPSG:3857", "EPSG:4326", "EPSG:3577", "EPSG:28355", "EPSG:3112", "EPSG:3031", ""])
def test_compute_reproject_extent(gpu, oracle, dst):
    """The worker's `extent` op (ComputeReprojectExtent, warp.go:433-487)
    through the C-ABI, against the oracle restatement, for the C1 / C2 / C5
    granule kinds (lon/lat, Albers, MODIS sinusoidal), a GDA94 / MGA zone 55,
    a GA Lambert and an Antarctic polar stereographic granule and several
    bboxes."""
    import torch

    import gsky_amd.worker as W
    cases = [synth.config_c1(scale=0.2).granules[0], synth.config_c2(scale=0.05, tiles_per_side=2).granules[0],
             synth.config_c5(scale=0.05, dates=1, zooms=((4, 11, 8, 1),), tile_px=64).granules[0],
             synth.config_utm(scale=0.05, tiles_per_side=2).granules[0],
             synth.config_lambert(scale=0.05, tiles_per_side=2).granules[0],
             synth.config_polar(scale=0.05, tiles_per_side=2).granules[0]]
    W.unregister_all()
    try:
        for k, g in enumerate(cases):
            path = "NETCDF:/g%d.nc:band" % k
            W.register_granule(path, 1, torch.from_numpy(np.ascontiguousarray(g.data)).cuda(), g.geot, g.srs,
                               g.nodata)
            og = oracle.make_granule(np.ascontiguousarray(g.data), g.geot)
            src = oracle.crs(g.srs)
            dc = oracle.crs(dst) if dst else src
            for bb in ([12245143.98, -4865942.28, 15584728.71, -1118889.97], [110.0, -45.0, 155.0, -10.0],
                       [-2000000.0, -4000000.0, 2200000.0, -1000000.0], [200000.0, 5700000.0, 500000.0, 5950000.0],
                       [1350000.0, -4100000.0, 1700000.0, -3750000.0],
                       [-2500000.0, 1100000.0, -2100000.0, 1500000.0],
                       [0.0, 0.0, 0.0, 0.0]):
                req = W.GeoRPCGranule(operation="extent", path=path, dstSRS=dst, dstGeot=list(bb))
                res = W.compute_reproject_extent(req)
                exp = oracle.compute_reproject_extent(og, src, dc, bb)
                if exp is None:
                    assert res.error == "GDALSuggestedWarpOutput() failed", (k, bb)
                    continue
                assert res.error == "OK" and res.raster.rasterType == "Int", (k, bb, res.error)
                got = tuple(int(v) for v in np.frombuffer(res.raster.data, dtype="<i8"))
                assert got == exp, (k, dst, bb, got, exp)
        assert W.compute_reproject_extent(W.GeoRPCGranule(path="missing.tif", dstSRS=dst,
                                                          dstGeot=[0, 0, 1, 1])).error.startswith("Failed to open")
    finally:
        W.unregister_all()


# (W, H, source, destination, geotransform, bbox, adjusted axis: 0 right / x, 1 bottom / y)
BORDER_TRIAL_CASES = [
    (100, 7, "EPSG:4326", "EPSG:3857", [131.5265740588777, 0.5, 0, -31.269165207466465, 0, -0.5],
     [0.0, 0.0, 3.45e9, 3.45e9], 0),
    (100, 7, "EPSG:3577", "EPSG:3857", [1772224.4222894707, 50000, 0, -2710353.5651497347, 0, -50000],
     [0.0, 0.0, 3.45e9, 3.45e9], 0),
    # also the 21 x 21 grid fallback: rows run past the pole
    (512, 300, "EPSG:4326", "EPSG:3577", [131.5265740588777, 0.5, 0, -31.269165207466465, 0, -0.5],
     [0.0, 0.0, 4.36e8, 4.36e8], 1),
]


def test_compute_reproject_extent_border_trials(gpu, oracle):
    """GDALSuggestedWarpOutput2's right / bottom border adjustment beyond its
    first trial (must_adjust / must_adjust2 over border_bad, plan.hip), which
    the granules of test_compute_reproject_extent never take: zero-filled
    int16 granules for which the oracle answers gt[1] != -gt[5] (one border
    settled on a later trial), with a bbox of about 10^4 pixels so that the
    0.1-1 % the trial changes the resolution by moves the pixel count.  The
    extent op feeds psx / psy straight into the counts: a wrong trial is a
    wrong integer."""
    import torch

    import gsky_amd.worker as W
    prepared = []
    for w, h, srs, dst, gt, bb, axis in BORDER_TRIAL_CASES:
        data = np.zeros((h, w), np.int16)
        og, src, dc = oracle.make_granule(data, gt), oracle.crs(srs), oracle.crs(dst)
        rc, ogt, _, _, _ = oracle.suggested_warp_output(og, src, dc, [0.0, 1.0, 0.0, 0.0, 0.0, 1.0])
        psx, psy = float(ogt[1]), -float(ogt[5])
        assert rc == 0 and psx != psy, (srs, dst, psx, psy)
        assert (psx < psy) == (axis == 0), (srs, dst, psx, psy)   # the adjusted border has the smaller pixel
        exp = oracle.compute_reproject_extent(og, src, dc, bb)
        big = max(psx, psy)   # the resolution before any adjustment
        assert exp[axis] != int((bb[2 + axis] - bb[axis] + big / 2.0) / big), (srs, dst, exp)
        prepared.append((data, srs, dst, gt, bb, exp))
    assert {c[6] for c in BORDER_TRIAL_CASES} == {0, 1}
    W.unregister_all()
    try:
        for k, (data, srs, dst, gt, bb, exp) in enumerate(prepared):
            path = "NETCDF:/border%d.nc:band" % k
            W.register_granule(path, 1, torch.from_numpy(data).cuda(), gt, srs, 0.0)
            res = W.compute_reproject_extent(W.GeoRPCGranule(operation="extent", path=path, dstSRS=dst,
                                                             dstGeot=list(bb)))
            assert res.error == "OK" and res.raster.rasterType == "Int", (k, res.error)
            got = tuple(int(v) for v in np.frombuffer(res.raster.data, dtype="<i8"))
            assert got == exp, (k, srs, dst, got, exp)
    finally:
        W.unregister_all()


def test_warp_operation_fast_dropin(gpu, oracle):
    """warp.go:82 drop-in through the worker mirror (WarpRaster)."""
    import torch

    from gsky_amd import worker
    from gsky_amd.tiles import bbox_to_geot
    cfg = synth.config_c2(scale=0.1, tiles_per_side=4, tile_px=256)
    g = cfg.granules[5]
    worker.register_granule("/g/data/c2/g5.tif", 1, torch.from_numpy(g.data).to(gpu), g.geot, "EPSG:3577",
                            g.nodata, block=(128, 64))
    bb, w, h = cfg.tiles[5]
    dst_gt = bbox_to_geot(w, h, bb)
    res = worker.warp_raster(worker.GeoRPCGranule(path="/g/data/c2/g5.tif", bands=[1], width=w, height=h,
                                                  dstSRS="EPSG:3857", dstGeot=dst_gt))
    assert res.error == "OK", res.error
    og = oracle.make_granule(g.data, g.geot, g.nodata, block=(128, 64))
    arr, bbox, nd, dt = oracle.warp(og, oracle.crs("EPSG:3577"), oracle.crs("EPSG:3857"), dst_gt, w, h)
    assert res.raster.bbox == list(bbox) and res.raster.rasterType == "Int16" and res.raster.noData == nd
    got = worker.raster_array(res.raster)
    assert identity(got, arr) >= NN_IDENTITY
    assert res.bytesRead == oracle.warp.bytes_read > 0           # warp.go:347
    req = dict(bands=[1], width=w, height=h, dstSRS="EPSG:3857", dstGeot=dst_gt)
    assert worker.warp_raster(worker.GeoRPCGranule(path="/nope", **req)).error == "warp_operation() fail: 1"
    # a registered GeoTIFF without band 3: GDALGetRasterBand fails (warp.go:114-118)
    req3 = dict(req, bands=[3])
    assert worker.warp_raster(worker.GeoRPCGranule(path="/g/data/c2/g5.tif", **req3)).error == \
        "warp_operation() fail: 2"
    # netCDF paths are opened per band (band_query, warp.go:89-101): band 3 not there -> open fails
    worker.register_granule("NETCDF:/g/data/c2/g5.nc:v", 1, torch.from_numpy(g.data).to(gpu), g.geot,
                            "EPSG:3577", g.nodata)
    assert worker.warp_raster(worker.GeoRPCGranule(path="NETCDF:/g/data/c2/g5.nc:v", **req3)).error == \
        "warp_operation() fail: 1"
    assert worker.warp_raster(worker.GeoRPCGranule(path="NETCDF:/g/data/c2/g5.nc:v", **req)).error == "OK"
    worker.unregister_all()


@pytest.mark.parametrize("dtype,rtype", [("uint8", "Byte"), ("int16", "Int16"), ("float32", "Float32")])
@pytest.mark.parametrize("w,h", [(256, 256), (257, 131), (33, 7)])
def test_warp_operation_fast_dtypes_and_ragged_windows(gpu, oracle, dtype, rtype, w, h):
    """warp.go:82 through the warp batch for 1-, 2- and 4-byte rasters and
    window sizes whose pixel count is not a multiple of the kernel's pixels
    per thread (the packed wide stores and the per-pixel tail)."""
    import torch

    from gsky_amd import worker
    from gsky_amd.tiles import bbox_to_geot
    cfg = synth.config_c2(scale=0.1, tiles_per_side=4, tile_px=256)
    g = cfg.granules[5]
    nod = g.data == g.nodata
    if dtype == "uint8":
        data, nodata = np.clip(g.data // 16, 0, 254).astype(np.uint8), 255.0
    elif dtype == "float32":
        data, nodata = g.data.astype(np.float32) * np.float32(0.25), float(g.nodata) * 0.25
    else:
        data, nodata = g.data, float(g.nodata)
    data = data.copy()
    data[nod] = nodata
    path = "/g/data/c2/dt_%s.tif" % dtype
    worker.register_granule(path, 1, torch.from_numpy(data).to(gpu), g.geot, "EPSG:3577", nodata, block=(128, 64))
    try:
        bb, _, _ = cfg.tiles[5]
        dst_gt = bbox_to_geot(w, h, bb)
        res = worker.warp_raster(worker.GeoRPCGranule(path=path, bands=[1], width=w, height=h,
                                                      dstSRS="EPSG:3857", dstGeot=dst_gt))
        assert res.error == "OK", res.error
        og = oracle.make_granule(data, g.geot, nodata, block=(128, 64))
        arr, bbox, nd, dt = oracle.warp(og, oracle.crs("EPSG:3577"), oracle.crs("EPSG:3857"), dst_gt, w, h)
        assert res.raster.bbox == list(bbox) and res.raster.rasterType == rtype and res.raster.noData == nd
        got = worker.raster_array(res.raster)
        assert got.dtype == np.dtype(dtype) and got.size == arr.size
        assert identity(got, arr) >= NN_IDENTITY
        assert res.bytesRead == oracle.warp.bytes_read
    finally:
        worker.unregister_all()


# ---------------------------------------------------------------- drill
@pytest.mark.parametrize("strides,pc,clip", [(1, 0, (-1e30, 1e30)), (1, 1, (0.21, 0.26)), (3, 0, (0.2, 0.3)),
                                             (2, 0, (-1e30, 1e30))])
def test_drill_parity(gpu, oracle, strides, pc, clip):
    import torch

    from gsky_amd import drill
    dc = synth.config_c4(n_bands=37, size=256, n_polys=12, rmin=4, rmax=40)
    st = drill.DrillStack(torch.from_numpy(dc.bands), dc.nodata, gpu)
    win, off, masks = drill.pack_masks(dc.windows, dc.masks, gpu)
    vals, cnts = drill.read_data(st, win, off, masks, clip[0], clip[1], pc, strides)
    vals, cnts = vals.cpu().numpy(), cnts.cpu().numpy()
    for p, (x0, y0, w, h) in enumerate(dc.windows):
        sub = dc.bands[:, y0:y0 + h, x0:x0 + w]
        ev, ec = oracle.drill_read_data(sub, dc.masks[p], dc.nodata, clip[0], clip[1], pc, strides)
        assert np.array_equal(cnts[p], ec), p
        assert np.array_equal(vals[p].view(np.uint64), ev.view(np.uint64)), p   # bit exact


@pytest.mark.parametrize("dcount,pc,clip", [(9, 0, (-1e30, 1e30)), (4, 0, (0.21, 0.24)), (3, 1, (-1e30, 1e30))])
def test_drill_deciles_parity(gpu, oracle, dcount, pc, clip):
    """computeDeciles (drill.go:229-273) by radix selection: every decile
    of every (polygon, band) equal to the oracle's float32 value, the
    [mean, deciles] rows and their Counts as the reference's TimeSeries, small
    polygons exercising the padding branch; a band list and a small band chunk
    (several sort passes)."""
    import torch

    from gsky_amd import drill
    dc = synth.config_c4(n_bands=23, size=200, n_polys=15, rmin=1, rmax=30)
    # two tiny polygons: 2 and 3 in-mask pixels -> the padding branch (len < dc + 1)
    dc.windows = list(dc.windows) + [(10, 12, 2, 1), (150, 40, 2, 2)]
    dc.masks = list(dc.masks) + [np.full((1, 2), 255, np.uint8), np.array([[255, 0], [255, 255]], np.uint8)]
    st = drill.DrillStack(torch.from_numpy(dc.bands), dc.nodata, gpu)
    mb = drill.pack_masks(dc.windows, dc.masks, gpu)
    bands = [1, 4, 5, 9, 23, 17, 2]
    vals, cnts = drill.read_data(st, mb, clip_lower=clip[0], clip_upper=clip[1], pixel_count=pc,
                                 decile_count=dcount, bands=bands)
    vals, cnts = vals.cpu().numpy(), cnts.cpu().numpy()
    assert vals.shape == (len(dc.windows), len(bands), 1 + dcount)
    mv, mc = drill.read_data(st, mb, clip_lower=clip[0], clip_upper=clip[1], pixel_count=pc, bands=bands)
    assert np.array_equal(vals[..., 0], mv.cpu().numpy()) and np.array_equal(cnts[..., 0], mc.cpu().numpy())
    small = 0
    for p, (x0, y0, w, h) in enumerate(dc.windows):
        for j, b in enumerate(bands):
            sub = dc.bands[b - 1, y0:y0 + h, x0:x0 + w]
            if cnts[p, j, 0] == 0:
                assert not vals[p, j, 1:].any() and not cnts[p, j, 1:].any()
                continue
            exp = oracle.compute_deciles(sub, dc.masks[p], dc.nodata, dcount)
            assert exp is not None
            assert np.array_equal(vals[p, j, 1:].astype(np.float32), exp), (p, b)
            assert (cnts[p, j, 1:] == 1).all()
            small += int(((dc.masks[p] == 255) & (sub != dc.nodata)).sum() < dcount + 1)
    assert small >= len(bands)
    # wave-split means: the deciles take the transposing path (the fused
    # band-major rows come with the reference-order walk only) -- same picks
    vw, cw = drill.read_data(st, mb, clip_lower=clip[0], clip_upper=clip[1], pixel_count=pc,
                             decile_count=dcount, bands=bands, mode=drill.WAVE_SPLIT)
    assert np.array_equal(vw.cpu().numpy()[..., 1:], vals[..., 1:]) and np.array_equal(cw.cpu().numpy(), cnts)
    # several sort passes over the band list
    dec, stt = drill.compute_deciles(st, mb, mc, dcount, bands, band_chunk=2)
    assert np.array_equal(dec.cpu().numpy()[stt.cpu().numpy() == 0],
                          vals[..., 1:].astype(np.float32)[stt.cpu().numpy() == 0])


@pytest.mark.parametrize("side", [100, 150, 290])
def test_drill_deciles_large_polygon(gpu, oracle, side):
    """Long segments: 100 x 100, 150 x 150 and 290 x 290 in-mask windows
    (~9.5k / ~21k / ~80k keys), all past the 2048 keys a select workgroup
    caches in LDS: decile_select_kernel, one 256-thread workgroup per
    (polygon, band), streams the segment on every pass; all equal to the
    oracle for every band, nodata values (-9999 at 1 %) skipped.  Bands 0/1/3
    resolve their ranks in one pass: a 2048-bucket histogram of the key range,
    then the 64-lane counting select of each rank's bucket (band 3: both signs,
    no shared key bits); bands 2 and 4 (a handful of distinct values) overflow
    the 64-key buckets and continue by range refinement on the bucket's key
    range, down to a single key."""
    import torch

    from gsky_amd import drill
    rng = np.random.default_rng(side)
    sz = side + 10
    data = rng.uniform(0.0, 0.05, size=(5, sz, sz)).astype(np.float32)
    data[3] = rng.normal(size=(sz, sz)) * 1000.0          # both signs, every exponent: no shared key bits
    data[4] = rng.choice(np.array([-1.0, 0.0, 2.5, 7.0], np.float32), size=(sz, sz))   # 4 values: huge buckets
    data[rng.uniform(size=data.shape) < 0.01] = -9999.0
    data[2] = np.round(data[2] * 100) / 100   # many equal values: ties across the ranks
    st = drill.DrillStack(torch.from_numpy(data), -9999.0, gpu)
    mask = np.full((side, side), 255, np.uint8)
    mask[::7, ::3] = 0
    mb = drill.pack_masks([(3, 4, side, side)], [mask], gpu)
    vals, cnts = drill.read_data(st, mb, decile_count=9)
    vals = vals.cpu().numpy()
    for b in range(5):
        exp = oracle.compute_deciles(data[b, 4:4 + side, 3:3 + side], mask, -9999.0, 9)
        assert np.array_equal(vals[0, b, 1:].astype(np.float32), exp), b


@pytest.mark.parametrize("strides,dcount,pc,nb", [(2, 9, 0, 23), (3, 9, 0, 23), (3, 4, 1, 22), (5, 9, 0, 21),
                                                  (1, 9, 0, 23)])
def test_drill_deciles_strides_parity(gpu, oracle, strides, dcount, pc, nb):
    """readData with decileCount and bandStrides together (drill.go:128-219,
    gskyhip_drill_read_data): bound bands read, deciles of both bounds,
    every column interpolated for bandStrides > 2 with Counts math.Round of
    the bounds' mean, the 1-band last group read twice -- values bit-exact
    and Counts equal to the oracle's restatement, for every polygon."""
    import torch

    from gsky_amd import drill
    dc = synth.config_c4(n_bands=nb, size=200, n_polys=14, rmin=1, rmax=30)
    dc.windows = list(dc.windows) + [(10, 12, 2, 1)]            # 2 values: the padding branch
    dc.masks = list(dc.masks) + [np.full((1, 2), 255, np.uint8)]
    st = drill.DrillStack(torch.from_numpy(dc.bands), dc.nodata, gpu)
    mb = drill.pack_masks(dc.windows, dc.masks, gpu)
    clip = (0.21, 0.26) if pc else (-3.4e38, 3.4e38)
    vals, cnts = drill.read_data(st, mb, clip_lower=clip[0], clip_upper=clip[1], pixel_count=pc,
                                 band_strides=strides, decile_count=dcount)
    vals, cnts = vals.cpu().numpy(), cnts.cpu().numpy()
    for p, (x0, y0, w, h) in enumerate(dc.windows):
        ev, ec = oracle.drill_read_data_full(dc.bands[:, y0:y0 + h, x0:x0 + w], dc.masks[p], dc.nodata, clip[0],
                                             clip[1], pc, strides, dcount)
        assert vals[p].shape == ev.shape, (p, vals[p].shape, ev.shape)
        assert np.array_equal(cnts[p], ec), p
        assert np.array_equal(vals[p].view(np.uint64), ev.view(np.uint64)), p


def test_drill_deciles_reference_panic(gpu, oracle):
    """len == decileCount + 1 values: the reference reads buf[len] and panics
    (drill.go:244-249); the GPU path reports GSKYHIP_E_RANGE instead."""
    import torch

    from gsky_amd import GskyError, drill
    data = np.full((3, 64, 64), 0.25, np.float32)
    st = drill.DrillStack(torch.from_numpy(data), -9999.0, gpu)
    mb = drill.pack_masks([(5, 5, 2, 2)], [np.full((2, 2), 255, np.uint8)], gpu)
    assert oracle.compute_deciles(data[0, 5:7, 5:7], np.full((2, 2), 255, np.uint8), -9999.0, 3) is None
    with pytest.raises(GskyError):
        drill.read_data(st, mb, decile_count=3)
    _, stt = drill.compute_deciles(st, mb, torch.full((1, 3), 4, dtype=torch.int32, device=gpu), 3)
    assert (stt.cpu().numpy() == -7).all()


@pytest.mark.parametrize("expr", ["(nir - red) / (nir + red)", "nir * 0.0001 - red * 2 + qa", "nir > red ? nir : -red",
                                  "(nir % 7 + 1) ** 0.5", "3.25", "!(qa == 1) && nir >= 100 || red < 10",
                                  "red / (nir - nir)"])
def test_band_math_parity(gpu, oracle, expr):
    """gskyhip_band_math against the oracle's restatement on merged-canvas-like
    int16 / uint8 / float32 inputs with nodata: bit-identical (pow within 2
    ulp: device powf vs numpy)."""
    import torch

    from gsky_amd import GskyError, band_math
    rng = np.random.default_rng(7)
    n = 300 * 257
    nir = rng.integers(-50, 10000, n).astype(np.int16)
    nir[rng.random(n) < 0.05] = -999
    red = (rng.random(n) * 500).astype(np.float32)
    red[rng.random(n) < 0.05] = -9999.0
    qa = rng.integers(0, 3, n).astype(np.uint8)
    vs = [("nir", nir, -999.0), ("red", red, -9999.0), ("qa", qa, 2.0)]
    got = band_math(expr, [(nm, torch.from_numpy(a).to(gpu), nd) for nm, a, nd in vs], -999.0).cpu().numpy()
    exp = oracle.band_math(expr, vs, -999.0)
    if "**" in expr:
        np.testing.assert_array_max_ulp(got, exp, maxulp=2)
    else:
        assert np.array_equal(got.view(np.uint32), exp.view(np.uint32))
    if "(nir - nir)" in expr:   # division by zero everywhere: every pixel nodata
        assert (exp == -999.0).all()
    else:
        assert (exp == -999.0).mean() < 0.6
    with pytest.raises(GskyError):
        band_math("nir + swir", [(nm, torch.from_numpy(a).to(gpu), nd) for nm, a, nd in vs], -999.0)


def test_drill_merge_parity(gpu, oracle):
    import torch

    from gsky_amd import drill
    rng = np.random.default_rng(2)
    v = rng.normal(0.3, 0.1, (5, 365))
    v[rng.random(v.shape) < 0.1] = np.nan
    c = rng.integers(0, 1000, v.shape).astype(np.int32)
    exp = oracle.drill_merge(v, c)
    got = drill.drill_merge(torch.from_numpy(v).to(gpu), torch.from_numpy(c).to(gpu)).cpu().numpy()
    assert np.array_equal(np.isnan(exp), np.isnan(got))
    assert np.allclose(got[~np.isnan(got)], exp[~np.isnan(exp)], rtol=0, atol=0)


# ---------------------------------------------------------------- typed LDS band kernel
@pytest.mark.parametrize("dt", [np.int16, np.uint16, np.uint8, np.int8, np.float32])
def test_lds_kernel_types(gpu, oracle, dt):
    """The typed LDS band kernel (value-type hint) and the generic kernels give
    the oracle's tiles exactly, for every value type the warp keeps."""
    import gsky_amd
    cfg = _cast_cfg(synth.config_c2(scale=0.1, tiles_per_side=4, tile_px=256), dt)
    if dt == np.uint8:
        cfg.scale = (0.0, 0.0, 250.0, 0)
    b = gpu_batch(cfg)
    assert bin(b.value_types).count("1") == 1
    sp, pal = gsky_amd.ScaleParams(*cfg.scale), gsky_amd.Palette(cfg.palette, True)
    got = b.render(sp, pal).cpu().numpy().copy()
    b.typed = False
    gen = b.render(sp, pal).cpu().numpy()
    exp = oracle_render(oracle, cfg)
    assert np.array_equal(got, exp)
    assert np.array_equal(gen, exp)
    assert (exp[..., 3] > 0).mean() > 0.3


@pytest.mark.parametrize("resample", [0, 1])
def test_lds_kernel_wide_tiles(gpu, oracle, resample):
    """Tiles wider than one 512-column block of the band kernel (1100 px:
    three blocks, the last ragged), RGBA and typed canvases, NN and bilinear.
    Bilinear int16: equal to the oracle except, by 1, where a stack entry's
    unrounded sample sits on a rounding tie (helpers.bilinear_tie_masks)."""
    import gsky_amd
    cfg = synth.config_c2(scale=0.1, tiles_per_side=2, tile_px=1100)
    cfg.resample = resample
    b = gpu_batch(cfg)
    sp, pal = gsky_amd.ScaleParams(*cfg.scale), gsky_amd.Palette(cfg.palette, True)
    got = b.render(sp, pal, resample=resample).cpu().numpy().copy()
    cv = b.render(sp, pal, resample=resample, rgba=False).cpu().numpy().copy()
    exp, ecv, created = oracle_render(oracle, cfg, canvas=True)
    if resample == 0:
        assert np.array_equal(got, exp)
        assert np.array_equal(cv[:, 0, :1100 * 1100 * 2], ecv[:, 0, :1100 * 1100 * 2])
    else:
        e = ecv[:, 0, :1100 * 1100 * 2].view(np.int16)
        g = cv[:, 0, :1100 * 1100 * 2].view(np.int16)
        assert np.array_equal(e == -999, g == -999)
        d = np.abs(e.astype(np.int32) - g.astype(np.int32)).reshape(-1, 1100, 1100)
        assert d.max() <= 1
        tie = np.stack(bilinear_tie_masks(oracle, cfg))
        assert not d[~tie].any()
        assert (got[..., 3] > 0).sum() == (exp[..., 3] > 0).sum()
    assert (exp[..., 3] > 0).mean() > 0.3


def test_lds_kernel_many_entries_multipass(gpu, oracle):
    """40 overlapping granules on one tile: more entries per band than the
    kernel stages at once (16), so the band folds in several passes."""
    import gsky_amd
    base = synth.config_c2(scale=0.05, tiles_per_side=2, tile_px=128, grid=2)
    gs = []
    for k in range(40):
        g = base.granules[k % len(base.granules)]
        gt = list(g.geot)
        gt[0] += 731.0 * (k % 7)
        gt[3] -= 517.0 * (k % 5)
        d = np.roll(g.data, k * 13, axis=1).copy()
        gs.append(synth.SynthGranule(d, gt, g.srs, g.nodata, 1577836800.0 + 3600.0 * ((k * 7) % 11),
                                     "P%d" % (k % 3)))
    cfg = synth.SynthConfig("many", gs, base.dst_srs, base.tiles, [list(range(40))] * len(base.tiles), [""],
                            base.scale, base.palette)
    b = gpu_batch(cfg)
    sp, pal = gsky_amd.ScaleParams(*cfg.scale), gsky_amd.Palette(cfg.palette, True)
    got = b.render(sp, pal).cpu().numpy().copy()
    exp = oracle_render(oracle, cfg)
    assert np.array_equal(got, exp)
    b.typed = False
    assert np.array_equal(b.render(sp, pal).cpu().numpy(), exp)


def test_lds_kernel_masks(gpu, oracle):
    """C5-style QA masks (non-inclusive mask layer, overviews) on the typed path."""
    import gsky_amd
    cfg = synth.config_c5(scale=0.05, dates=2, zooms=((4, 11, 8, 2), (5, 22, 16, 3)), tile_px=128)
    b = gpu_batch(cfg)
    assert b.value_types == 4          # Int16 only: the Byte QA layer is not merged
    got = b.render(gsky_amd.ScaleParams(*cfg.scale)).cpu().numpy()
    exp = oracle_render(oracle, cfg)
    assert np.array_equal(got, exp)


@pytest.mark.parametrize("strides", [1, 3])
def test_drill_band_list(gpu, oracle, strides):
    """readData's `bands []int32` (drill.go:90, 128-143): an arbitrary 1-based
    band list, in list order, with bandStrides grouping over list positions."""
    import torch

    from gsky_amd import drill
    dc = synth.config_c4(n_bands=37, size=256, n_polys=12, rmin=4, rmax=40)
    st = drill.DrillStack(torch.from_numpy(dc.bands), dc.nodata, gpu)
    mb = drill.pack_masks(dc.windows, dc.masks, gpu)
    blist = [5, 3, 17, 1, 2, 36, 37, 9, 9, 20, 11]
    vals, cnts = drill.read_data(st, mb, clip_lower=-1e30, clip_upper=1e30, band_strides=strides, bands=blist)
    vals, cnts = vals.cpu().numpy(), cnts.cpu().numpy()
    sel = np.asarray(blist) - 1
    for p, (x0, y0, w, h) in enumerate(dc.windows):
        sub = dc.bands[sel][:, y0:y0 + h, x0:x0 + w]
        ev, ec = oracle.drill_read_data(sub, dc.masks[p], dc.nodata, -1e30, 1e30, 0, strides)
        assert np.array_equal(cnts[p], ec), p
        assert np.array_equal(vals[p].view(np.uint64), ev.view(np.uint64)), p


@pytest.mark.parametrize("pc,clip", [(0, (-1e30, 1e30)), (1, (0.21, 0.26))])
def test_drill_wave_split_mode(gpu, oracle, pc, clip):
    """Mode 1 (wave-split reduction): counts exact, means within 1e-5 relative
    of the reference summation order."""
    import torch

    from gsky_amd import drill
    dc = synth.config_c4(n_bands=70, size=512, n_polys=20, rmin=20, rmax=120)
    st = drill.DrillStack(torch.from_numpy(dc.bands), dc.nodata, gpu)
    mb = drill.pack_masks(dc.windows, dc.masks, gpu)
    vals, cnts = drill.read_data(st, mb, clip_lower=clip[0], clip_upper=clip[1], pixel_count=pc,
                                 mode=drill.WAVE_SPLIT)
    vals, cnts = vals.cpu().numpy(), cnts.cpu().numpy()
    for p, (x0, y0, w, h) in enumerate(dc.windows):
        sub = dc.bands[:, y0:y0 + h, x0:x0 + w]
        ev, ec = oracle.drill_read_data(sub, dc.masks[p], dc.nodata, clip[0], clip[1], pc, 1)
        assert np.array_equal(cnts[p], ec), p
        rel = np.abs(vals[p] - ev) / np.maximum(np.abs(ev), 1e-30)
        assert rel.max() <= 1e-5, (p, rel.max())


def test_drill_window_past_stack_edge(gpu, oracle):
    """A window reaching past the stack reads nothing outside it:
    equals the reference on the clipped window."""
    import torch

    from gsky_amd import drill
    dc = synth.config_c4(n_bands=9, size=128, n_polys=1, rmin=4, rmax=8)
    st = drill.DrillStack(torch.from_numpy(dc.bands), dc.nodata, gpu)
    wins = [(118, 120, 30, 20), (-5, -3, 12, 9)]
    masks = [np.full((20, 30), 255, np.uint8), np.full((9, 12), 255, np.uint8)]
    vals, cnts = drill.read_data(st, drill.pack_masks(wins, masks, gpu))
    vals, cnts = vals.cpu().numpy(), cnts.cpu().numpy()
    for p, (x0, y0, w, h) in enumerate(wins):
        xa, ya, xb, yb = max(0, x0), max(0, y0), min(128, x0 + w), min(128, y0 + h)
        sub = dc.bands[:, ya:yb, xa:xb]
        ev, ec = oracle.drill_read_data(sub, np.full((yb - ya, xb - xa), 255, np.uint8), dc.nodata, -1e30, 1e30)
        assert np.array_equal(cnts[p], ec) and np.array_equal(vals[p].view(np.uint64), ev.view(np.uint64))


def test_pair_info_footprint_covers_samples(gpu):
    """gskyhip_render_pair_info (bench.py's C5 algorithmic bytes): each pair's
    source footprint lies inside its picked level and holds every value its
    warped window sampled (C2-style pairs, int16 data with few repeats)."""
    import gsky_amd
    cfg = synth.config_c2(scale=0.05, tiles_per_side=3, tile_px=128)
    b = gpu_batch(cfg)
    b.render(gsky_amd.ScaleParams(*cfg.scale), gsky_amd.Palette(cfg.palette, True))
    info = b.pair_info()
    assert info.shape == (b.n_pairs, 8)
    wins = b.warp_windows()
    flat = [k for ks in cfg.pairs for k in ks]
    n_checked = 0
    for p, (win, bbox, tname, nd) in enumerate(wins):
        g, lx, ly, es, x0, y0, x1, y1 = info[p].tolist()
        gr = cfg.granules[flat[p]]
        levels = [gr.data] + list(gr.overviews)
        lv = [a for a in levels if (a.shape[1], a.shape[0]) == (lx, ly)]
        assert g == flat[p] and lv and es == 2
        assert 0 <= x0 <= x1 <= lx and 0 <= y0 <= y1 <= ly
        vals = win.cpu().numpy().ravel()
        vals = vals[vals != nd]
        if vals.size == 0:
            continue
        inside = np.isin(vals, lv[0][y0:y1, x0:x1])
        assert inside.all(), (p, bbox, (x0, y0, x1, y1))
        n_checked += 1
    assert n_checked > 0


def test_render_touched_bytes_match_warped_windows(gpu):
    """gskyhip_render_touched (bench.py's C5 algorithmic bytes) against the
    warped windows themselves: float32 granules whose every element holds its
    own index, so the distinct values of all windows of a granule are exactly
    the source elements its pairs pick -- their count x 4 B and the 128-B
    lines holding them must equal what the device bitmaps count."""
    import dataclasses

    import gsky_amd
    cfg = synth.config_c2(scale=0.05, tiles_per_side=3, tile_px=128)
    gran = []
    for g in cfg.granules:
        n = g.data.shape[0] * g.data.shape[1]
        gran.append(dataclasses.replace(g, data=np.arange(n, dtype=np.float32).reshape(g.data.shape), nodata=-1.0,
                                        overviews=[]))
    cfg = dataclasses.replace(cfg, granules=gran)
    b = gpu_batch(cfg)
    b.render(gsky_amd.ScaleParams(0.0, 0.0, 40000.0, 0), None)
    flat = [k for ks in cfg.pairs for k in ks]
    seen = {}
    for p, (win, bbox, tname, nd) in enumerate(b.warp_windows()):
        vals = win.cpu().numpy().ravel()
        vals = vals[vals != nd].astype(np.int64)
        seen.setdefault(flat[p], set()).update(vals.tolist())
    exp_bytes = sum(len(v) * 4 for v in seen.values())
    exp_lines = sum(len({x * 4 // 128 for x in v}) * 128 for v in seen.values())
    assert exp_bytes > 0
    assert b.touched_bytes() == (exp_bytes, exp_lines)
