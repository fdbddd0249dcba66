"""The Deflate encoder of independent blocks (gskyhip_deflate_blocks[_host],
deflate_core.h / deflate.hip): every block of tests/deflate_corpus.py as a
zlib stream and as a raw stream, at level 0 (stored) and 6, decoded by
Python's zlib and by the product's own inflate; the size bound; the exact
capacity check; determinism; the derived size bounds of compressible chunks.
The CPU tests run the host twin, which gives the device's bytes bit for bit
(the GPU tests at the end assert exactly that)."""
import zlib

import numpy as np
import pytest

from gsky_amd import encode, ingest

from .deflate_corpus import corpus, half_compressible, shuffle

E_CAP = 5   # GSKYHIP_INFLATE_E_CAP
MODES = [(True, 6), (False, 6), (True, 0), (False, 0)]


def _names():
    return [n for n, _ in corpus()]


def _blocks():
    return [b for _, b in corpus()]


_HOST = {}


def host_streams(wrapper, level):
    """The host twin's streams of the whole corpus, one call per mode, shared."""
    key = (wrapper, level)
    if key not in _HOST:
        _HOST[key] = encode.deflate_blocks(_blocks(), zlib_wrapper=wrapper, level=level, where="host")
    return _HOST[key]


def _inflate(stream, wrapper):
    return zlib.decompress(stream) if wrapper else zlib.decompress(stream, wbits=-15)


def test_bound_formula():
    for n in (0, 1, 65534, 65535, 65536, 131070, 1 << 20):
        assert encode.deflate_bound(n) == n + 5 * (n // 65535 + 1) + 6


@pytest.mark.parametrize("wrapper,level", MODES)
def test_corpus_decodes_and_is_bounded(wrapper, level):
    for (name, block), out in zip(corpus(), host_streams(wrapper, level)):
        assert _inflate(out, wrapper) == block, name
        assert len(out) <= encode.deflate_bound(len(block)), name
        if wrapper:
            assert out[:2] == b"\x78\x9c", name


@pytest.mark.parametrize("wrapper,level", MODES)
def test_status_zero_and_lengths(wrapper, level):
    st, ln, outs = encode.deflate_blocks(_blocks(), zlib_wrapper=wrapper, level=level, where="host",
                                         return_status=True)
    assert st == [0] * len(st)
    for k, out in enumerate(host_streams(wrapper, level)):
        assert ln[k] == len(out)
        assert outs[k][:ln[k]].tobytes() == out
        assert (outs[k][ln[k]:] == 0xA5).all(), "bytes past the stream were written"


@pytest.mark.parametrize("wrapper,level", MODES)
def test_capacity_one_short_writes_nothing(wrapper, level):
    caps = [len(s) - 1 for s in host_streams(wrapper, level)]
    st, ln, outs = encode.deflate_blocks(_blocks(), zlib_wrapper=wrapper, level=level, where="host", out_caps=caps,
                                         return_status=True)
    assert st == [E_CAP] * len(st)
    for k, o in enumerate(outs):
        assert (o == 0xA5).all(), _names()[k]
        assert ln[k] == caps[k] + 1


@pytest.mark.parametrize("wrapper,level", MODES)
def test_own_inflate_reads_the_streams(wrapper, level):
    streams = host_streams(wrapper, level)
    sizes = [len(b) for b in _blocks()]
    st, ln, outs, _ = ingest.inflate_blocks(streams, sizes, zlib_wrapper=wrapper, where="host")
    assert st == [0] * len(st)
    for k, block in enumerate(_blocks()):
        assert ln[k] == len(block) and outs[k].tobytes() == block, _names()[k]


def test_level_zero_stored_blocks():
    """level 0: stored blocks only -- n + 5 per 65535 bytes + the wrapper."""
    for block, out in zip(_blocks(), host_streams(True, 0)):
        n = len(block)
        assert len(out) == n + 5 * max(1, -(-n // 65535)) + 6


def test_random_bytes_fall_back_to_stored():
    """Incompressible data: never above the bound (zlib level 6 gives exactly
    the bound, 8,203 bytes, for 8,192 random bytes)."""
    d = dict(zip(_names(), host_streams(True, 6)))
    assert len(d["random8192"]) <= 8203
    assert len(zlib.compress(dict(corpus())["random8192"], 6)) == 8203


def test_constant_chunks_are_small():
    """A constant row: at most n / 32 + 64 bytes (a match token costs at most
    18 bits under the fixed code, and the encoder covers a run with matches of
    72 bytes or more).  zlib level 6 gives 38 and 15 bytes for these rows."""
    blocks = [shuffle(np.full(2048, 273.15, np.float32)), shuffle(np.full(67, -999, np.int16))]
    assert [len(b) for b in blocks] == [8192, 134]
    for wrapper in (True, False):
        for b, out in zip(blocks, encode.deflate_blocks(blocks, zlib_wrapper=wrapper, where="host")):
            print("constant chunk", len(b), "->", len(out), "zlib", len(zlib.compress(b, 6)))
            assert len(out) <= len(b) // 32 + 64


def test_half_compressible_chunk():
    """High byte constant, low byte random: at most 0.6 n + 256 (literals cost
    at most 9 bits under the fixed code, the constant plane next to nothing).
    zlib level 6 gives 2,119 bytes for this row."""
    b = half_compressible()
    assert len(b) == 4096
    out = encode.deflate_blocks([b], where="host")[0]
    print("half compressible", len(b), "->", len(out), "zlib", len(zlib.compress(b, 6)))
    assert len(out) <= 0.6 * len(b) + 256


def test_no_distance_past_the_window():
    """Period 40,000 > 32,768: zlib rejects a stream with a longer distance."""
    d = dict(zip(_names(), host_streams(False, 6)))
    block = dict(corpus())["period40000"]
    assert zlib.decompress(d["period40000"], wbits=-15) == block


def test_deterministic_alone_among_many_and_twice():
    blocks = _blocks()
    base = host_streams(True, 6)
    pick = [_names().index(n) for n in ("row_f32_257", "fibonacci", "run516", "half_compressible")]
    many = []
    for k in range(300):
        many.append(blocks[pick[k % len(pick)]] if k % 3 == 0 else blocks[(k * 7) % 5 + 16])
    got = encode.deflate_blocks(many, where="host")
    for k in range(0, 300, 3):
        assert got[k] == base[pick[k % len(pick)]]
    for i in pick:
        assert encode.deflate_blocks([blocks[i]], where="host")[0] == base[i]
    assert encode.deflate_blocks(blocks, where="host") == base


def test_levels_one_to_nine_are_one_encoding():
    blocks = [b for n, b in corpus() if n in ("row_i16_2048", "fibonacci", "len3")]
    ref = encode.deflate_blocks(blocks, level=6, where="host")
    for level in (1, 9):
        assert encode.deflate_blocks(blocks, level=level, where="host") == ref


def test_bad_arguments():
    from gsky_amd._lib import GskyError
    with pytest.raises(GskyError):
        encode.deflate_blocks([b"abc"], level=10, where="host")
    with pytest.raises(ValueError):
        encode.deflate_blocks([b"abc"], where="nowhere")
    assert encode.deflate_blocks([], where="host") == []


# ---------------------------------------------------------------- the device
@pytest.mark.gpu
@pytest.mark.parametrize("wrapper,level", MODES)
def test_device_matches_host_one_launch(gpu, wrapper, level):
    got = encode.deflate_blocks(_blocks(), zlib_wrapper=wrapper, level=level, where="device")
    for name, a, b in zip(_names(), got, host_streams(wrapper, level)):
        assert a == b, name


@pytest.mark.gpu
def test_device_matches_host_block_per_launch(gpu):
    for name, block, ref in zip(_names(), _blocks(), host_streams(True, 6)):
        assert encode.deflate_blocks([block], where="device")[0] == ref, name


@pytest.mark.gpu
def test_device_on_a_side_stream(gpu):
    import torch
    s = torch.cuda.Stream(device=gpu)
    with torch.cuda.stream(s):
        got = encode.deflate_blocks(_blocks(), where="device")
        raw = encode.deflate_blocks(_blocks(), zlib_wrapper=False, where="device")
    s.synchronize()
    assert got == host_streams(True, 6)
    assert raw == host_streams(False, 6)


@pytest.mark.gpu
@pytest.mark.parametrize("level", [6, 0])
def test_device_capacity_one_short_writes_nothing(gpu, level):
    caps = [len(s) - 1 for s in host_streams(True, level)]
    st, ln, outs = encode.deflate_blocks(_blocks(), level=level, where="device", out_caps=caps, return_status=True)
    assert st == [E_CAP] * len(st)
    for k, o in enumerate(outs):
        assert (o == 0xA5).all(), _names()[k]
        assert ln[k] == caps[k] + 1


@pytest.mark.gpu
def test_device_writes_nothing_past_the_streams(gpu):
    st, ln, outs = encode.deflate_blocks(_blocks(), where="device", return_status=True)
    assert st == [0] * len(st)
    for k, ref in enumerate(host_streams(True, 6)):
        assert outs[k][:ln[k]].tobytes() == ref
        assert (outs[k][ln[k]:] == 0xA5).all(), _names()[k]


@pytest.mark.gpu
def test_device_among_300_blocks(gpu):
    blocks = _blocks()
    base = host_streams(True, 6)
    idx = [(k * 7) % 5 + 16 for k in range(300)]
    got = encode.deflate_blocks([blocks[i] for i in idx], where="device")
    assert got == [base[i] for i in idx]
