"""The opt-in Deflate GeoTIFF of the WCS writer with the tiles gathered,
predicted and deflated in HBM (gskyhip_encode_geotiff_opts,
encode.encode_geotiff(..., compression="deflate")).  The yardstick is the
host writer on the same arrays (encode.encode_geotiff_host, checked without a
device by tests/test_geotiff_deflate.py): the device file must be that file,
byte for byte, whatever the slab size, and the device decoder of the ingest
side must read it back bit for bit.  compression="packbits" through the new
entry point is the unchanged writer's file."""
import numpy as np
import pytest

from gsky_amd import encode, ingest

from .test_geotiff import read_bigtiff
from .test_geotiff_deflate import GT, _band

pytestmark = pytest.mark.gpu


def _dev(a):
    import torch
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def _roundtrip_arrays(dtype, w, h, nb):
    """The coverages of tests/test_geotiff.py::test_geotiff_roundtrip."""
    rng = np.random.default_rng(hash((dtype, w, h)) & 0xFFFF)
    if dtype == "float32":
        arrs = [rng.normal(size=(h, w)).astype(np.float32) for _ in range(nb)]
        arrs[0][:, : w // 3] = -999.0
    else:
        info = np.iinfo(dtype)
        arrs = [rng.integers(info.min, info.max, size=(h, w), endpoint=True).astype(dtype) for _ in range(nb)]
        arrs[0][h // 2:, :] = arrs[0][0, 0]
        arrs[-1][:, ::7] = 3
    return arrs


@pytest.mark.parametrize("dtype,w,h,nb", [("float32", 1500, 300, 2), ("int16", 700, 530, 1), ("uint8", 1024, 256, 3),
                                           ("int8", 33, 17, 1), ("uint16", 1030, 260, 2)])
def test_packbits_is_the_unchanged_file(dtype, w, h, nb):
    arrs = _roundtrip_arrays(dtype, w, h, nb)
    dev = [_dev(a) for a in arrs]
    nodata = [-999.0] * nb if dtype == "float32" else [0.0] * nb
    names = ["band_%d&<x>" % i for i in range(nb)]
    old = encode.encode_geotiff(dev, GT, 3577, nodata, names, uint16=(dtype == "uint16"))
    new, stats = encode.encode_geotiff(dev, GT, 3577, nodata, names, uint16=(dtype == "uint16"),
                                       compression="packbits", return_stats=True)
    assert new == old
    assert stats[:3] == (0, 0, 0)
    # and the host writer's PackBits file is the same again
    assert encode.encode_geotiff_host(arrs, GT, 3577, nodata, names) == old


@pytest.mark.parametrize("w,h,block", [(33, 40, (16, 16)), (700, 530, (1024, 256))])
@pytest.mark.parametrize("dtype,predictor", [("int16", 2), ("uint16", 2), ("uint8", 1), ("int8", 2), ("float32", 2),
                                             ("float32", 3)])
def test_device_file_is_the_host_file(dtype, predictor, w, h, block):
    a = _band(dtype, h, w, seed=predictor + w)
    nodata = [-999.0] if dtype in ("int16", "float32") else [7.0]
    want = encode.encode_geotiff_host([a], GT, 3577, nodata, ["b"], block=block, compression="deflate",
                                      predictor=predictor)
    got, stats = encode.encode_geotiff([_dev(a)], GT, 3577, nodata, ["b"], block=block, uint16=(dtype == "uint16"),
                                       compression="deflate", predictor=predictor, return_stats=True)
    assert got == want
    tags = read_bigtiff(got)
    n_tiles = -(-w // block[0]) * -(-h // block[1])
    assert stats[0] == n_tiles == len(tags[325])
    assert stats[2] == sum(tags[325])
    assert stats[1] > 0 and stats[3] > 0


def test_slabs_and_host_mode_give_the_same_file():
    arrs = [_band("float32", 300, 1500, seed=s) for s in (31, 32)]   # 2 x 2 tiles a band
    dev = [_dev(a) for a in arrs]
    kw = dict(nodata=[-1.0, -2.0], names=["a", "b"], compression="deflate", predictor=3)
    whole, s0 = encode.encode_geotiff(dev, GT, 3577, slab_tiles=0, return_stats=True, **kw)
    single, s1 = encode.encode_geotiff(dev, GT, 3577, slab_tiles=1, return_stats=True, **kw)
    assert single == whole
    assert s0[:3] == s1[:3] and s0[0] == 8 and s1[3] < s0[3]   # the workspace follows the slab
    assert encode.encode_geotiff(dev, GT, 3577, slab_tiles=3, **kw) == whole   # a slab that does not divide the band
    host, sh = encode.encode_geotiff(dev, GT, 3577, deflate="host", return_stats=True, **kw)
    assert host == whole and sh == (0, 0, 0, 0)
    assert encode.encode_geotiff_host(arrs, GT, 3577, **kw) == whole


@pytest.mark.parametrize("dtype,predictor", [("int16", 2), ("float32", 3)])
def test_closed_loop_through_the_device_decoder(tmp_path, dtype, predictor):
    a = _band(dtype, 530, 700, seed=5)
    t = _dev(a)
    buf = encode.encode_geotiff([t], GT, 3577, [-999.0], ["b"], block=(256, 128), compression="deflate",
                                predictor=predictor)
    path = str(tmp_path / "loop.tif")
    with open(path, "wb") as f:
        f.write(buf)
    back, stats = ingest.read(path, 1, decode="device", return_stats=True)
    assert back.dtype == t.dtype and back.shape == t.shape
    assert back.cpu().numpy().tobytes() == a.tobytes()
    n_tiles = 3 * 5
    assert stats[0] == n_tiles and stats[1] == 0   # every block decoded on the device


def test_device_extremes():
    const = np.full((40, 33), -7, np.int16)
    noise = np.random.default_rng(5).integers(0, 256, (530, 700)).astype(np.uint8)
    for a, block, predictor in ((const, (16, 16), 2), (noise, (256, 128), 1)):
        want = encode.encode_geotiff_host([a], GT, 3577, None, None, block=block, compression="deflate",
                                          predictor=predictor)
        assert encode.encode_geotiff([_dev(a)], GT, 3577, None, None, block=block, compression="deflate",
                                     predictor=predictor) == want
    # stored blocks, and an EmptyTile band between two real ones
    arrs = [_band("int16", 40, 33, seed=s) for s in (1, 2, 3)]
    names = ["red", "EmptyTile_green", "blue"]
    for zlevel in (0, 6):
        kw = dict(nodata=[1.0, 2.0, 7.0], names=names, block=(16, 16), compression="deflate", predictor=2,
                  zlevel=zlevel)
        want = encode.encode_geotiff_host(arrs, GT, 4326, **kw)
        got, stats = encode.encode_geotiff([_dev(a) for a in arrs], GT, 4326, return_stats=True, **kw)
        assert got == want and stats[0] == 18   # the empty band's tiles never reach the device
