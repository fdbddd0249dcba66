"""The WCS netCDF output with the chunks shuffled and deflated on the GPU
(gskyhip_encode_netcdf_deflate, encode.encode_netcdf(..., deflate="device")):
the file reads back bit-exact through the host reader and through the device
decode path, reports what the host-path file reports, and is the host-path
file of the same arguments in everything but the chunk payloads.

"Everything but the payloads" is checked on a skeleton of each file: the
chunks are found by walking the file (superblock -> root group links -> each
band's layout message -> its chunk B-tree), their bytes (and the padding to
the next 8-byte boundary) are cut out, every address the writer stores after
the first chunk (B-tree children, the layout's B-tree address, the root
group's links, the superblock's root and end-of-file addresses) is rewritten
to its position in the cut file, the chunk sizes and addresses in the B-tree
leaves are zeroed, and the lookup3 checksums that cover such fields are
verified and then zeroed.  The two skeletons must be equal byte for byte."""

import numpy as np
import pytest

from gsky_amd import encode, ingest

from .h5write import lookup3

GT = [1400000.0, 25.0, 0.0, -3800000.0, 0.0, -25.0]


def _u(blob, at, n):
    return int.from_bytes(blob[at:at + n], "little")


def _ohdr(blob, addr):
    """(messages [(type, body position, size)], checksum position) of a version-2 object header."""
    assert blob[addr:addr + 4] == b"OHDR" and blob[addr + 4] == 2 and blob[addr + 5] == 0x02
    size = _u(blob, addr + 6, 4)
    at, end, msgs = addr + 10, addr + 10 + size, []
    while at < end:
        t, n = blob[at], _u(blob, at + 1, 2)
        msgs.append((t, at + 4, n))
        at += 4 + n
    assert at == end
    assert _u(blob, end, 4) == lookup3(blob[addr:end]), "object header checksum"
    return msgs, end


def skeleton(blob):
    """(the file without its chunk payloads, addresses normalised; [[(row, addr, size)] per band])."""
    out = bytearray(blob)
    assert blob[:8] == b"\x89HDF\r\n\x1a\n" and blob[8] == 2
    assert _u(blob, 44, 4) == lookup3(blob[:44]), "superblock checksum"
    assert _u(blob, 28, 8) == len(blob)
    addr_fields = [28, 36]   # positions of 8-byte addresses to rewrite
    zero = [(44, 4)]         # (position, length) to zero
    root = _u(blob, 36, 8)
    msgs, ck = _ohdr(blob, root)
    zero.append((ck, 4))
    links = {}
    for t, at, n in msgs:
        if t == 0x06:
            nl = blob[at + 2]
            links[blob[at + 3:at + 3 + nl].decode()] = at + 3 + nl
            addr_fields.append(at + 3 + nl)
    bands, k = [], 1
    while "Band%d" % k in links:
        bmsgs, bck = _ohdr(blob, _u(blob, links["Band%d" % k], 8))
        zero.append((bck, 4))
        lay = [at for t, at, n in bmsgs if t == 0x08]
        assert len(lay) == 1 and blob[lay[0]] == 3 and blob[lay[0] + 1] == 2
        addr_fields.append(lay[0] + 3)
        chunks = []

        def walk(node):
            assert blob[node:node + 4] == b"TREE" and blob[node + 4] == 1
            level, n = blob[node + 5], _u(blob, node + 6, 2)
            for i in range(n):
                key = node + 24 + i * 40
                child = key + 32
                if level == 0:
                    chunks.append((_u(blob, key + 8, 8), _u(blob, child, 8), _u(blob, key, 4)))
                    zero.append((key, 4))
                    zero.append((child, 8))
                else:
                    addr_fields.append(child)
                    walk(_u(blob, child, 8))

        walk(_u(blob, lay[0] + 3, 8))
        bands.append(chunks)
        k += 1
    cuts = sorted((a, (a + s + 7) & ~7) for ch in bands for _, a, s in ch)
    for (a0, a1), (b0, _) in zip(cuts, cuts[1:]):
        assert a1 <= b0, "chunks overlap"

    def compact(addr):
        return addr - sum(min(addr, e) - s for s, e in cuts if s < addr)

    for at in addr_fields:
        out[at:at + 8] = compact(_u(blob, at, 8)).to_bytes(8, "little")
    for at, n in zero:
        out[at:at + n] = bytes(n)
    keep, prev = [], 0
    for s, e in cuts:
        keep.append(bytes(out[prev:s]))
        prev = min(e, len(out))
    keep.append(bytes(out[prev:]))
    return b"".join(keep), bands


def _bands(dt, n=2, h=37, w=53, seed=3):
    rng = np.random.default_rng(seed)
    if np.dtype(dt).kind == "f":
        return [rng.normal(size=(h, w)).astype(dt) * 100 for _ in range(n)]
    info = np.iinfo(dt)
    return [rng.integers(info.min, info.max, size=(h, w), endpoint=True).astype(dt) for _ in range(n)]


def _to_device(bands, gpu):
    import torch
    u16 = bands[0].dtype == np.uint16
    return [torch.from_numpy(b.view(np.int16) if u16 else b).to(gpu) for b in bands], u16


def _write(tmp_path, name, data):
    p = str(tmp_path / name)
    with open(p, "wb") as f:
        f.write(data)
    return p


def _check(tmp_path, gpu, bands, names, nodata, epsg=3577, slab_rows=0, zlevel=6):
    """Encode on the device and on the host; every per-file check of the issue."""
    dev, u16 = _to_device(bands, gpu)
    blob, stats = encode.encode_netcdf(dev, GT, epsg, nodata=nodata, names=names, zlevel=zlevel, uint16=u16,
                                       deflate="device", slab_rows=slab_rows, return_stats=True)
    host = encode.encode_netcdf(dev, GT, epsg, nodata=nodata, names=names, zlevel=zlevel, uint16=u16)
    assert host == encode.encode_netcdf_host(bands, GT, epsg, nodata=nodata, names=names, zlevel=zlevel, threads=16)
    p, ph = _write(tmp_path, "dev.nc", blob), _write(tmp_path, "host.nc", host)
    h, w = bands[0].shape
    es = 4 if bands[0].dtype == np.uint16 else bands[0].dtype.itemsize
    for k, b in enumerate(bands):
        vp, vh = "NETCDF:%s:Band%d" % (p, k + 1), "NETCDF:%s:Band%d" % (ph, k + 1)
        want = ingest.read_host(vh, 1)
        empty = names is not None and names[k].startswith("EmptyTile")
        if not empty and b.dtype == np.uint16:   # widened to NC_INT
            assert np.array_equal(want.astype(np.int64), b.astype(np.int64))
        elif not empty:   # the same bits (NC_BYTE reads back as Byte)
            assert np.array_equal(want.view(np.uint8), b.view(np.uint8))
        got = ingest.read_host(vp, 1)
        assert got.dtype == want.dtype and np.array_equal(got.view(np.uint8), want.view(np.uint8))
        if bands[0].dtype == np.float32:
            gd = ingest.read(vp, 1, device=gpu, decode="device").cpu().numpy()
            assert np.array_equal(gd.view(np.uint8), want.view(np.uint8))
        assert ingest.info(vp) == ingest.info(vh)
        assert ingest.netcdf_srs(vp, 0) == ingest.netcdf_srs(vh, 0)
        assert ingest.netcdf_srs(vp, 1) == ingest.netcdf_srs(vh, 1)
    sk_d, ch_d = skeleton(blob)
    sk_h, ch_h = skeleton(host)
    assert sk_d == sk_h
    bound = encode.deflate_bound(w * es)
    n_dev = 0
    total = 0
    for k, ch in enumerate(ch_d):
        assert [r for r, _, _ in ch] == list(range(h))
        assert all(0 < s <= bound for _, _, s in ch)
        if not (names is not None and names[k].startswith("EmptyTile")):
            n_dev += h
            total += sum(s for _, _, s in ch)
    assert stats[0] == n_dev
    assert stats[1] == n_dev * w * bands[0].dtype.itemsize
    assert stats[2] == total
    assert stats[3] > 0
    return blob


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [np.uint8, np.int8, np.int16, np.uint16, np.float32])
def test_device_deflate_dtypes(tmp_path, gpu, dt):
    bands = _bands(dt)
    nd = [float(np.asarray(bands[0]).ravel()[7]), 0.0]
    _check(tmp_path, gpu, bands, ["ls8", "qa"], nd)


@pytest.mark.gpu
def test_device_deflate_five_slabs(tmp_path, gpu):
    """300 rows in slabs of 64: five slabs, the last short."""
    bands = _bands(np.float32, n=2, h=300, w=257)
    _check(tmp_path, gpu, bands, ["a", "b"], [-9999.0, -9999.0], epsg=4326, slab_rows=64)


@pytest.mark.gpu
def test_device_deflate_64k_chunks(tmp_path, gpu):
    rng = np.random.default_rng(5)
    x = np.linspace(0, 40, 16384)
    b = (280 + 10 * np.sin(x)[None, :] + rng.normal(0, 0.05, (3, 16384))).astype(np.float32)
    b[1, 100:9000] = -9999.0   # a long nodata run
    _check(tmp_path, gpu, [b], ["t"], [-9999.0])


@pytest.mark.gpu
def test_device_deflate_one_row(tmp_path, gpu):
    _check(tmp_path, gpu, _bands(np.int16, n=1, h=1, w=31), ["v"], [-1.0])


@pytest.mark.gpu
def test_device_deflate_level_zero_stored_blocks(tmp_path, gpu):
    _check(tmp_path, gpu, _bands(np.int16, n=1, h=5, w=40), ["v"], [-1.0], zlevel=0)


@pytest.mark.gpu
def test_device_deflate_empty_tile(tmp_path, gpu):
    bands = _bands(np.int16, n=2, h=8, w=8)
    blob = _check(tmp_path, gpu, bands, ["ok", "EmptyTile_1"], [-5.0, -6.0], epsg=4326)
    p = _write(tmp_path, "e.nc", blob)
    assert np.array_equal(ingest.read_host("NETCDF:%s:Band2" % p, 1), np.zeros((8, 8), np.int16))
    assert ingest.info("NETCDF:%s:Band1" % p).nodata == -5.0


@pytest.mark.gpu
def test_device_deflate_file_does_not_depend_on_slabs(gpu):
    dev, _ = _to_device(_bands(np.float32, n=1, h=37, w=53), gpu)
    a = encode.encode_netcdf(dev, GT, 3577, nodata=[0.0], names=["v"], deflate="device")
    b = encode.encode_netcdf(dev, GT, 3577, nodata=[0.0], names=["v"], deflate="device", slab_rows=7)
    assert a == b


@pytest.mark.gpu
def test_default_is_the_host_path(gpu):
    bands = _bands(np.int16, n=1, h=9, w=20)
    dev, _ = _to_device(bands, gpu)
    want = encode.encode_netcdf_host(bands, GT, 3577, nodata=[1.0], names=["v"], threads=16)
    assert encode.encode_netcdf(dev, GT, 3577, nodata=[1.0], names=["v"]) == want
    got, stats = encode.encode_netcdf(dev, GT, 3577, nodata=[1.0], names=["v"], deflate="host", return_stats=True)
    assert got == want and stats == (0, 0, 0, 0)
    with pytest.raises(ValueError):
        encode.encode_netcdf(dev, GT, 3577, deflate="gpu")


def test_skeleton_of_a_host_file():
    """The file walker itself, without a GPU: the skeleton of a host-path file
    is found, and two host files that differ in payload only (zlevel) differ
    in their skeletons only where the filter message and history record it."""
    b = _bands(np.float32, n=2, h=70, w=33)
    f6 = encode.encode_netcdf_host(b, GT, 3577, nodata=[1.0, 2.0], names=["a", "b"], zlevel=6)
    f6b = encode.encode_netcdf_host(b, GT, 3577, nodata=[1.0, 2.0], names=["a", "b"], zlevel=6, threads=3)
    f1 = encode.encode_netcdf_host(b, GT, 3577, nodata=[1.0, 2.0], names=["a", "b"], zlevel=1)
    s6, ch = skeleton(f6)
    assert skeleton(f6b)[0] == s6
    assert [len(c) for c in ch] == [70, 70]
    s1, _ = skeleton(f1)
    assert len(s1) == len(s6)
    diff = [i for i in range(len(s1)) if s1[i] != s6[i]]
    assert 0 < len(diff) <= 3   # two filter messages and the history attribute
