"""Overview pyramids built on the GPU (overview.hip): bit-exact against the
numpy reference of tests/test_overviews.py, and through every way in --
registered tensors, render_tiles, files, the drop-in's own ingest and the
per-node service -- the zoomed-out warp equals the one over explicit
overviews and differs from the one without any."""
import math
import multiprocessing as mp
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from tests.test_overviews import ref_pyramid, typed_nodata

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(2, 2), (3, 5), (63, 65), (64, 64), (65, 63), (129, 257), (7, 1031)]   # (ysize, xsize)
# and one whose pitch allows the wide loads for every type while its tiles are clipped in x and y
# and its height is odd (the shapes above reach the wide loads only with the single full 64 x 64 tile)
SHAPES.append((67, 200))
NODATA = {"uint8": 255.0, "int8": 200.0, "int16": -999.0, "uint16": 65535.0, "float32": -999.0}


def _data(dtype, shape, nodata, seed, nans=False):
    """Seeded values with ~30 % nodata, whole all-nodata 8 x 8 blocks (so "no
    valid pixel" survives three levels) and, for float32, some NaNs."""
    rng = np.random.default_rng(seed)
    dt = np.dtype(dtype)
    h, w = shape
    if dt == np.float32:
        a = (rng.standard_normal(shape) * 1000).astype(np.float32)
    else:
        ii = np.iinfo(dt)
        a = rng.integers(ii.min, ii.max + 1, shape).astype(dt)
    bad = rng.random(shape) < 0.3
    by, bx = -(-h // 8), -(-w // 8)
    blocks = rng.random((by, bx)) < 0.25
    blocks[0, 0] = h >= 16 and w >= 16   # (tiny shapes keep some valid pixels)
    bad |= np.kron(blocks.astype(np.uint8), np.ones((8, 8), np.uint8))[:h, :w].astype(bool)
    if nodata is not None:
        a[bad] = typed_nodata(nodata, dt)
    if dt == np.float32 and nans:
        nan_at = bad if nodata is None else (rng.random(shape) < 0.1)
        a[nan_at] = np.float32("nan")
    return a


def _to_gpu(a):
    import torch
    if a.dtype == np.uint16:   # through the int16 bits (older torch has no uint16 from_numpy)
        return torch.from_numpy(a.view(np.int16).copy()).cuda().view(torch.uint16)
    return torch.from_numpy(a.copy()).cuda()


def _to_host(t):
    import torch
    if t.dtype == torch.uint16:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy()


def _check(a, nodata, method, where=""):
    from gsky_amd import ingest
    got = ingest.build_overviews(_to_gpu(a), nodata, method, 1)
    exp = ref_pyramid(a, nodata, method, 1)
    assert len(got) == len(exp) and len(exp) >= 1, where
    assert exp[-1].shape == (1, 1)
    for k, (g, e) in enumerate(zip(got, exp)):
        gh = _to_host(g)
        assert gh.dtype == e.dtype and gh.shape == e.shape, (where, k)
        if gh.tobytes() != e.tobytes():
            bad = np.argwhere(gh.view(np.uint8).reshape(e.shape + (-1,)) != e.view(np.uint8).reshape(e.shape + (-1,)))
            y, x = bad[0][:2]
            raise AssertionError("%s level %d (%dx%d): %d bytes differ, first at (%d, %d): got %r, expected %r"
                                 % (where, k + 1, e.shape[1], e.shape[0], len(bad), y, x, gh[y, x], e[y, x]))


@pytest.mark.parametrize("method", ["nearest", "average"])
@pytest.mark.parametrize("dtype", ["uint8", "int8", "int16", "uint16", "float32"])
def test_pyramid_bit_exact(gpu, dtype, method):
    for i, shape in enumerate(SHAPES):
        a = _data(dtype, shape, NODATA[dtype], 100 + i, nans=True)
        _check(a, NODATA[dtype], method, "%s %s %s" % (dtype, method, shape))


@pytest.mark.parametrize("method", ["nearest", "average"])
def test_pyramid_float_nan_without_nodata(gpu, method):
    for i, shape in enumerate(SHAPES):
        a = _data("float32", shape, None, 200 + i, nans=True)
        assert np.isnan(a[:8, :8]).all() or min(shape) < 16
        _check(a, None, method, "float32 no-nodata %s %s" % (method, shape))


def test_pyramid_int_without_nodata(gpu):
    for dtype in ("int16", "uint8"):
        a = _data(dtype, (65, 63), None, 7)
        _check(a, None, "average", dtype)


def test_pyramid_on_a_side_stream(gpu):
    import torch

    from gsky_amd import ingest
    a = _data("int16", (129, 257), -999.0, 11)
    t = _to_gpu(a)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = ingest.build_overviews(t, -999.0, "average", 1)
    s.synchronize()
    exp = ref_pyramid(a, -999.0, "average", 1)
    assert len(got) == len(exp)
    for g, e in zip(got, exp):
        assert g.cpu().numpy().tobytes() == e.tobytes()


def test_unsupported_type_is_an_error(gpu):
    import torch

    from gsky_amd import _lib, ingest
    for dt in (torch.int32, torch.float64):
        with pytest.raises(_lib.GskyError) as e:
            ingest.build_overviews(torch.zeros((8, 8), dtype=dt, device="cuda"), None, "nearest", 1)
        assert e.value.code == -2


# ---------------------------------------------------------------- end to end
GEOT = [130.0, 0.01, 0.0, -20.0, 0.0, -0.01]    # 512 x 512 lon / lat granule


def _merc(lon, lat):
    r = 6378137.0
    return r * math.radians(lon), r * math.log(math.tan(math.pi / 4 + math.radians(lat) / 2))


def _zoomed_out(n=512, px=64, geot=GEOT):
    """A px x px EPSG:3857 tile over the whole n x n granule (ratio n / px)."""
    from gsky_amd.tiles import bbox_to_geot
    x0, y1 = _merc(geot[0], geot[3])
    x1, y0 = _merc(geot[0] + n * geot[1], geot[3] + n * geot[5])
    bbox = (x0, y0, x1, y1)
    return bbox, bbox_to_geot(px, px, bbox)


def _pattern(n=512, nodata=-999):
    """int16 values that depend on (x & 3, y & 3) inside slowly varying 4 x 4
    cells: a pick from an overview can never equal a sparse full-resolution pick
    everywhere."""
    y, x = np.mgrid[0:n, 0:n]
    a = (((x >> 2) * 7 + (y >> 2) * 13) % 500 * 16 + (x & 3) + 4 * (y & 3)).astype(np.int16)
    rng = np.random.default_rng(5)
    a[rng.random(a.shape) < 0.2] = nodata
    return a


def _warp(worker, path, dst_geot, px=64, band=1):
    r = worker.warp_raster(worker.GeoRPCGranule(path=path, bands=[band], width=px, height=px, dstSRS="EPSG:3857",
                                                 dstGeot=list(dst_geot)))
    assert r.error == "OK", (path, r.error)
    return worker.raster_array(r.raster), r.raster.bbox


def test_registered_granule_nearest(gpu, oracle):
    import torch

    from gsky_amd import worker
    a = _pattern()
    ovr = ref_pyramid(a, -999.0, "nearest", 32)
    assert len(ovr) == 4
    _, dst_geot = _zoomed_out()
    worker.unregister_all()
    try:
        t = torch.from_numpy(a).cuda()
        worker.register_granule("built", 1, t, GEOT, "EPSG:4326", -999.0, build_overviews="nearest", min_size=32)
        worker.register_granule("explicit", 1, t, GEOT, "EPSG:4326", -999.0,
                                overviews=[torch.from_numpy(o).cuda() for o in ovr])
        worker.register_granule("plain", 1, t, GEOT, "EPSG:4326", -999.0)
        with pytest.raises(ValueError):
            worker.register_granule("both", 1, t, GEOT, "EPSG:4326", -999.0, overviews=[t[::2, ::2]],
                                    build_overviews="nearest")
        built, bb = _warp(worker, "built", dst_geot)
        explicit, be = _warp(worker, "explicit", dst_geot)
        plain, _ = _warp(worker, "plain", dst_geot)
        assert bb == be and built.tobytes() == explicit.tobytes()
        og = oracle.make_granule(a, GEOT, -999.0, ovr)
        arr, obox, _, _ = oracle.warp(og, oracle.crs("EPSG:4326"), oracle.crs("EPSG:3857"), dst_geot, 64, 64)
        assert list(obox) == bb and arr.tobytes() == built.tobytes()
        # a level-2-or-deeper nearest pick only ever sees pixels with x & 3 == y & 3 == 0
        valid = built != -999
        assert valid.any() and ((built[valid] & 15) == 0).all()
        assert not np.array_equal(plain, built)
    finally:
        worker.unregister_all()


def test_render_tiles_average(gpu):
    import torch

    from gsky_amd import GranuleSet, ScaleParams, TileBatch
    a = _pattern()
    ovr = ref_pyramid(a, -999.0, "average", 32)
    bbox, _ = _zoomed_out()
    t = torch.from_numpy(a)
    out = {}
    for name, kw in (("built", dict(build_overviews="average", min_size=32)),
                     ("explicit", dict(overviews=[torch.from_numpy(o) for o in ovr])), ("plain", {})):
        gs = GranuleSet("cuda:0")
        gs.add(t, GEOT, "EPSG:4326", -999.0, **kw)
        tb = TileBatch(gs, "EPSG:3857", [(bbox, 64, 64)], [[0]])
        rgba, cv = tb.render(ScaleParams(0.0, 0.03, 8000.0), None, resample=0, canvas=True)   # bilinear off
        torch.cuda.synchronize()
        assert tb.status() == 0
        out[name] = (rgba.cpu().numpy().copy(), tb.canvas_view(cv, 0, 0, "Int16").cpu().numpy().copy())
    with pytest.raises(ValueError):
        GranuleSet("cuda:0").add(t, GEOT, "EPSG:4326", -999.0, overviews=[t[::2, ::2]], build_overviews="average")
    assert out["built"][1].tobytes() == out["explicit"][1].tobytes()
    assert out["built"][0].tobytes() == out["explicit"][0].tobytes()
    assert not np.array_equal(out["built"][1], out["plain"][1])
    assert (out["built"][0][..., 3] > 0).any()


# ---------------------------------------------------------------- files
def _small(n=128):
    a = _pattern(n, -1)
    geot = [130.0, 0.04, 0.0, -20.0, 0.0, -0.04]
    return a, geot


def _write_nc(path, a, geot):
    from tests import test_ingest as TI
    n = a.shape[0]
    lon = geot[0] + geot[1] * (np.arange(n) + 0.5)
    lat = geot[3] + geot[5] * (np.arange(n) + 0.5)
    TI._write_nc(path, "v", a, lon, lat, fill=-1)


def _write_tif(path, a, geot, overviews=()):
    from tests import test_ingest as TI
    geo = [(33550, 12, [geot[1], -geot[5], 0.0]), (33922, 12, [0, 0, 0, geot[0], geot[3], 0]),
           TI.geokeys(2, 1, [(2048, 4326)])]
    TI.write_tiff(path, [a], tile=(64, 64), compression=8, geo=geo, nodata="-1", overviews=overviews)


@pytest.mark.parametrize("kind", ["nc", "tif"])
def test_file_register_average(gpu, tmp_path, kind):
    import torch

    from gsky_amd import ingest, worker
    a, geot = _small()
    p = str(tmp_path / ("g." + kind))
    (_write_nc if kind == "nc" else _write_tif)(p, a, geot)
    inf = ingest.info(p)
    assert inf.overviews == [] and inf.nodata == -1.0
    ovr = ref_pyramid(a, -1.0, "average", 8)
    assert len(ovr) == 4
    _, dst_geot = _zoomed_out(128, 16, list(inf.geot))
    worker.unregister_all()
    try:
        ingest.register(p, 1, overviews="average", min_size=8)
        t = torch.from_numpy(a).cuda()
        worker.register_granule("explicit", 1, t, inf.geot, "EPSG:4326", -1.0,
                                overviews=[torch.from_numpy(o).cuda() for o in ovr])
        worker.register_granule("plain", 1, t, inf.geot, "EPSG:4326", -1.0)
        built, bb = _warp(worker, p, dst_geot, 16)
        explicit, be = _warp(worker, "explicit", dst_geot, 16)
        plain, _ = _warp(worker, "plain", dst_geot, 16)
        assert bb == be and built.tobytes() == explicit.tobytes()
        assert not np.array_equal(built, plain)
        # the file changes on disk: the drop-in reads it again and builds the same kind of pyramid
        a2 = (a // 2).astype(np.int16)
        st = os.stat(p)
        (_write_nc if kind == "nc" else _write_tif)(p, a2, geot)
        os.utime(p, ns=(st.st_atime_ns, st.st_mtime_ns + 2 * 10 ** 9))
        worker.register_granule("explicit2", 1, torch.from_numpy(a2).cuda(), inf.geot, "EPSG:4326", -1.0,
                                overviews=[torch.from_numpy(o).cuda() for o in ref_pyramid(a2, -1.0, "average", 8)])
        built2, _ = _warp(worker, p, dst_geot, 16)
        explicit2, _ = _warp(worker, "explicit2", dst_geot, 16)
        assert built2.tobytes() == explicit2.tobytes() and built2.tobytes() != built.tobytes()
        worker.register_granule("plain", 1, torch.from_numpy(a2).cuda(), inf.geot, "EPSG:4326", -1.0)
        plain, _ = _warp(worker, "plain", dst_geot, 16)
        assert not np.array_equal(built2, plain)
        # registered again without the keyword: today's behaviour
        ingest.register(p, 1)
        again, _ = _warp(worker, p, dst_geot, 16)
        assert again.tobytes() == plain.tobytes()
    finally:
        worker.unregister_all()


def test_file_overviews_win(gpu, tmp_path):
    """A GeoTIFF with overviews of its own keeps them: a marker value that
    only the file's overview levels hold fills the zoomed-out warp."""
    from gsky_amd import ingest, worker
    a, geot = _small()
    p = str(tmp_path / "own.tif")
    marker = [np.full((128 >> k, 128 >> k), 7777, np.int16) for k in (1, 2, 3, 4)]
    _write_tif(p, a, geot, overviews=[[m] for m in marker])
    assert len(ingest.info(p).overviews) == 4
    _, dst_geot = _zoomed_out(128, 16, geot)
    worker.unregister_all()
    try:
        ingest.register(p, 1, overviews="average", min_size=8)
        got, _ = _warp(worker, p, dst_geot, 16)
        assert (got[got != -1] == 7777).all() and (got == 7777).any()
    finally:
        worker.unregister_all()


_CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from gsky_amd import worker
path, out = sys.argv[2], sys.argv[3]
geot = [float(v) for v in sys.argv[4:10]]
r = worker.warp_raster(worker.GeoRPCGranule(path=path, bands=[1], width=18, height=18, dstSRS="EPSG:3857",
                                             dstGeot=geot))
assert r.error == "OK", r.error
np.save(out, worker.raster_array(r.raster))
worker.unregister_all()
"""


def test_drop_in_environment(gpu, tmp_path):
    """GSKYHIP_BUILD_OVERVIEWS in a fresh process: the drop-in's own ingest of
    an unregistered path builds the pyramid; without it, today's result."""
    import torch

    from gsky_amd import worker
    a, geot = _small()
    p = str(tmp_path / "auto.nc")
    _write_nc(p, a, geot)
    from gsky_amd import ingest
    inf_geot = list(ingest.info(p).geot)
    _, dst_geot = _zoomed_out(128, 18, inf_geot)   # ratio 7.1: a plain pick leaves the 4 x 4 cell corners
    ovr = ref_pyramid(a, -1.0, "nearest", 8)
    worker.unregister_all()
    try:
        t = torch.from_numpy(a).cuda()
        worker.register_granule("explicit", 1, t, inf_geot, "EPSG:4326", -1.0,
                                overviews=[torch.from_numpy(o).cuda() for o in ovr])
        worker.register_granule("plain", 1, t, inf_geot, "EPSG:4326", -1.0)
        explicit, _ = _warp(worker, "explicit", dst_geot, 18)
        plain, _ = _warp(worker, "plain", dst_geot, 18)
    finally:
        worker.unregister_all()
    assert not np.array_equal(explicit, plain)
    base = {k: v for k, v in os.environ.items() if k not in ("GSKYHIP_BUILD_OVERVIEWS", "GSKYHIP_OVERVIEW_MIN_SIZE",
                                                             "GSKYHIP_SERVICE")}
    runs = {"on": dict(base, GSKYHIP_BUILD_OVERVIEWS="nearest", GSKYHIP_OVERVIEW_MIN_SIZE="8"), "off": base,
            "empty": dict(base, GSKYHIP_BUILD_OVERVIEWS="")}
    procs = {}
    for name, env in runs.items():   # fresh children, side by side
        out = str(tmp_path / (name + ".npy"))
        procs[name] = (subprocess.Popen([sys.executable, "-c", _CHILD, ROOT, p, out] + ["%r" % v for v in dst_geot],
                                        env=env), out)
    got = {}
    for name, (pr, out) in procs.items():
        assert pr.wait(timeout=240) == 0, name
        got[name] = np.load(out)
    assert got["on"].tobytes() == explicit.tobytes()
    assert got["off"].tobytes() == plain.tobytes() and got["empty"].tobytes() == plain.tobytes()


# ---------------------------------------------------------------- service
def _client(sock, paths, dst_geot, q):
    """The one worker process of the service test (no HIP context of its own)."""
    os.environ["GSKYHIP_SERVICE"] = sock
    from gsky_amd import worker as W
    res = []
    for path in paths:
        r = W.warp_raster(W.GeoRPCGranule(path=path, bands=[1], width=64, height=64, dstSRS="EPSG:3857",
                                          dstGeot=list(dst_geot)))
        res.append((r.error, r.raster.data if r.raster else b"", r.raster.bbox if r.raster else []))
    q.put(res)


def test_service_builds_overviews(gpu):
    from gsky_amd import WarpService
    a = _pattern()
    ovr = ref_pyramid(a, -999.0, "nearest", 32)
    _, dst_geot = _zoomed_out()
    sock = os.path.join(tempfile.mkdtemp(prefix="gskyhip-"), "svc.sock")
    svc = WarpService(sock, max_batch=8, window_us=0)
    try:
        svc.register_granule("/g/built.tif", 1, a, GEOT, "EPSG:4326", -999.0, build_overviews="nearest", min_size=32)
        assert svc.stats()["granules"] == 1          # the pyramid is part of its granule
        svc.register_granule("/g/explicit.tif", 1, a, GEOT, "EPSG:4326", -999.0, overviews=ovr)
        svc.register_granule("/g/plain.tif", 1, a, GEOT, "EPSG:4326", -999.0)
        assert svc.stats()["granules"] == 3
        ctx = mp.get_context("spawn")
        q = ctx.Queue()
        p = ctx.Process(target=_client, args=(sock, ["/g/built.tif", "/g/explicit.tif", "/g/plain.tif"], dst_geot, q))
        p.start()
        built, explicit, plain = q.get(timeout=240)
        p.join(60)
        assert p.exitcode == 0
        assert built[0] == "OK" and explicit[0] == "OK" and plain[0] == "OK"
        assert built[1] == explicit[1] and built[2] == explicit[2]
        assert built[1] != plain[1]
        # a refresh under the same key replaces the upload and its pyramid
        svc.register_granule("/g/built.tif", 1, a, GEOT, "EPSG:4326", -999.0, build_overviews="average", min_size=32)
        assert svc.stats()["granules"] == 3
    finally:
        assert svc.shutdown() == 0
