"""The GPU DEFLATE encoder of gskyhip_encode_png (csrc/encode.hip) at the edges
tests/test_png.py never reaches: all three paths (dynamic / fixed codes on the
GPU, host zlib behind GSKYHIP_PNG_ZLIB=1 or past 4096 rows), degenerate
shapes, matches at the 32 KiB window edge, chained 258-byte matches, Huffman
length limiting, and -- what no inflate-only check can see -- that matches are
emitted at all: every stream is bounded by sizes derived from the reference
rows (oracle.go_png_rows), never from what the encoder gives.

The reference of every case is CPU-only: oracle.go_png_rows, zlib's inflate
and PIL.  deflate_header() below reads the block header of a stream so a test
can tell which path and which codes produced it.

The bytes themselves are held to tests/golden/png_streams.json, recorded on an
MI355X at the last commit whose PNG encoder was a copy of its own: the host
twin gskyhip_png_deflate_rows_host on the CPU, the kernels inside check_case.

Recorded (test_size_table prints it at -s; the gpu column is what the golden
file pins): bytes of the default path's zlib stream on an MI355X against
len(zlib.compress(rows, 6)).

    case         w x h          rows      gpu  zlib -6  ratio
    tiny         1x1               4       12       12   1.00
    tiny         1x1               5       11       11   1.00
    tiny         1x1               5       13       13   1.00
    tiny         2x1               7       15       15   1.00
    tiny         1x2              10       18       18   1.00
    tiny         3x1              13       20       20   1.00
    one_column   1x120           600      297      263   1.13
    one_row      300x1           901      959      912   1.05
    constant     64x64         12352      133      101   1.32
    constant     64x64         16448      141      155   0.91
    long_runs    700x8         16808       63       70   0.90
    noise        200x100       80100    80110    80131   1.00
    upsampled    131x67        35175     3509     3373   1.04
    upsampled    131x67        26398     2787     2668   1.04
    upsampled    131x67        26398      175      175   1.00   (gradient)
    skewed       200x200      120200    46663    46717   1.00
    window_a     5461x3        49152    18695    30003   0.62
    window_b     2800x4        44804    19987    22050   0.91
    window_c     2730x4        32764    13986    15047   0.93
    rows_4096    2x4096        36864    35448    35585   1.00
    rows_4097    2x4097        36873    35598    35598   1.00   (host zlib)

The skewed tile read 111898 bytes (2.40 x zlib) before huff_lengths counted the
internal nodes past the length limit: every tree more than one level too deep
came out incomplete and the tile fell back to the fixed codes.  Its code-length
code was 5 bits deep; a 7-bit one was never seen.
"""
import hashlib
import heapq
import io
import json
import os
import zlib
from fractions import Fraction

import numpy as np
import pytest

from .test_png import _check, _chunks

E_ARG = -1   # GSKYHIP_E_ARG (include/gskyhip.h)

# lengths and SHA-256 of the streams of both Deflate encoders at the commit
# before they shared deflate_core.h (tests/golden/make_png_streams.py)
with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "png_streams.json")) as _f:
    GOLDEN = json.load(_f)


def record(stream):
    return {"len": len(stream), "sha256": hashlib.sha256(stream).hexdigest()}


# ------------------------------------------------------------------ header reader
class _Bits:
    """LSB-first bit reader (RFC 1951 3.1.1)."""

    def __init__(self, data, pos=0):
        self.d, self.p = data, pos * 8

    def get(self, n):
        v = 0
        for k in range(n):
            v |= ((self.d[self.p >> 3] >> (self.p & 7)) & 1) << k
            self.p += 1
        return v


def _canonical(lens):
    """{(length, code): symbol} of the canonical code (RFC 1951 3.2.2)."""
    count = [0] * 16
    for n in lens:
        count[n] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    table = {}
    for s, n in enumerate(lens):
        if n:
            table[(n, nxt[n])] = s
            nxt[n] += 1
    return table


def _symbol(br, table):
    code = 0
    for n in range(1, 16):
        code = (code << 1) | br.get(1)   # Huffman codes are packed MSB first
        if (n, code) in table:
            return table[(n, code)]
    raise AssertionError("no code-length code matches")


CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)


def deflate_header(z):
    """The first block header of a zlib stream: btype, final and, for a
    dynamic block, the code-length-code lengths (by symbol), the HLIT
    literal/length lengths and the HDIST distance lengths."""
    br = _Bits(z, 2)
    out = {"final": br.get(1), "btype": br.get(2), "cl_lens": [], "lit_lens": [], "dist_lens": []}
    if out["btype"] != 2:
        return out
    hlit, hdist, hclen = br.get(5) + 257, br.get(5) + 1, br.get(4) + 4
    cl = [0] * 19
    for k in range(hclen):
        cl[CL_ORDER[k]] = br.get(3)
    table = _canonical(cl)
    lens = []
    while len(lens) < hlit + hdist:
        s = _symbol(br, table)
        if s < 16:
            lens.append(s)
        elif s == 16:
            assert lens, "repeat code with no previous length"
            lens += [lens[-1]] * (3 + br.get(2))
        elif s == 17:
            lens += [0] * (3 + br.get(3))
        else:
            lens += [0] * (11 + br.get(7))
    assert len(lens) == hlit + hdist, "code-length run crosses the end of the alphabets"
    out.update(cl_lens=cl, lit_lens=lens[:hlit], dist_lens=lens[hlit:])
    return out


def kraft(lens):
    return sum(Fraction(1, 1 << n) for n in lens if n)


def huffman_lengths(freq):
    """Unconstrained Huffman code lengths of the non-zero frequencies."""
    heap = [(f, i, (i,)) for i, f in enumerate(freq) if f]
    lens = [0] * len(freq)
    if len(heap) == 1:
        lens[heap[0][1]] = 1
        return lens
    heapq.heapify(heap)
    tie = len(freq)
    while len(heap) > 1:
        fa, _, a = heapq.heappop(heap)
        fb, _, b = heapq.heappop(heap)
        for s in a + b:
            lens[s] += 1
        heapq.heappush(heap, (fa + fb, tie, a + b))
        tie += 1
    return lens


def literal_only_bytes(rows):
    """Lower bound on the zlib stream of any block that codes `rows` with
    literals only (the best prefix code of its bytes plus one end of block;
    the dynamic header counted as free): 2 + ceil(bits / 8) + 4."""
    freq = np.bincount(np.frombuffer(rows, np.uint8), minlength=256).tolist() + [1]
    lens = huffman_lengths(freq)
    bits = sum(f * n for f, n in zip(freq, lens))
    return 2 + (bits + 7) // 8 + 4


def gpu_size_cap(n):
    """No token of the fixed codes costs more than 9 bits per byte it covers
    (the dearest: a 3-byte match, 7 + 5 + 13 = 25 bits against 27), and a
    dynamic block is used only where it is shorter: zlib header, 3 header
    bits, 9 n, end of block, byte padding, Adler-32."""
    return 2 + (3 + 9 * n + 7 + 7) // 8 + 4


# ------------------------------------------------------------------ tiles (h, w, 4) uint8
def _noise(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)


def noise_tile():
    """200 x 100 RGBA uniform noise, alpha from 1..255: an alpha of 0 turns a
    pixel into four zero bytes, a run the matcher takes, and this tile is the
    one that must leave the distance alphabet (all but) empty."""
    a = _noise(24, 100, 200)
    a[..., 3] = np.random.default_rng(38).integers(1, 256, (100, 200), dtype=np.uint8)
    return a


def _opaque(a):
    a = a.copy()
    a[..., 3] = 255
    return a


def _const(h, w, rgba):
    return np.broadcast_to(np.asarray(rgba, np.uint8), (h, w, 4)).copy()


def _centred_rows(seed, w, k, transparent=0.0):
    """k independent rows (k, w, 4) of colours drawn from -10..10 mod 256,
    alpha 255 (or 0 for a fraction `transparent` of the pixels): bytes near
    zero in int8, so Go's heuristic leaves every row unfiltered (None, or Up
    over the zero row above row 0) and equal pixel rows give equal bytes."""
    rng = np.random.default_rng(seed)
    out = np.full((k, w, 4), 255, np.uint8)
    out[..., :3] = (rng.integers(-10, 11, (k, w, 3)) % 256).astype(np.uint8)
    if transparent:
        out[rng.random((k, w)) < transparent] = 0
    return out


def upsampled_tiles():
    h, w = 67, 131
    t3 = np.repeat(np.repeat(_noise(11, h // 4 + 1, w // 4 + 1), 4, 0), 4, 1)[:h, :w]
    gy, gx = np.mgrid[0:h, 0:w]
    t1 = np.stack([(gx * 3) % 256, (gy * 5) % 256, (gx + gy) % 256, np.full((h, w), 255)], -1).astype(np.uint8)
    return [np.ascontiguousarray(t3), _opaque(t3), t1]


FIB_K = 30


def fibonacci_tile(k=FIB_K, side=200):
    """An opaque tile whose bytes follow a Fibonacci histogram over k values
    0, 1, 255, 2, 254, ... (most frequent first), shuffled: its unconstrained
    Huffman tree is deeper than the 15 bits DEFLATE allows."""
    n = side * side * 3
    fib = [1, 1]
    while len(fib) < k:
        fib.append(fib[-1] + fib[-2])
    values = [0] + [v for j in range(1, k) for v in (j, 256 - j)][:k - 1]
    counts = [max(1, c * n // sum(fib)) for c in reversed(fib)]
    data = np.zeros(n, np.uint8)
    p = 0
    for v, c in zip(values[1:], counts[1:]):   # value 0 takes the rest (the padding)
        data[p:p + c] = v
        p += c
    assert p < n
    np.random.default_rng(7).shuffle(data)
    out = np.full((side, side, 4), 255, np.uint8)
    out[..., :3] = data.reshape(side, side, 3)
    return out


def tiny_tiles():
    return [np.array([[[200, 100, 50, 255]]], np.uint8),
            np.array([[[9, 8, 7, 0]]], np.uint8),
            np.array([[[10, 60, 30, 77]]], np.uint8),
            _opaque(_noise(21, 1, 2)),                                             # 2 x 1
            np.array([[[1, 2, 3, 77]], [[250, 251, 252, 255]]], np.uint8),         # 1 x 2
            np.array([[[5, 6, 7, 0], [70, 60, 50, 77], [1, 2, 3, 255]]], np.uint8)]   # 3 x 1


def window_a():
    r = _centred_rows(31, 5461, 2)
    return np.stack([r[0], r[1], r[0]])


def window_b():
    """Row 2 repeats row 0 in its left half only (distance 2 * stride = 22402)
    and row 3 repeats row 0 in its right half only, which only 3 * stride =
    33603 > 32768 could reach: those bytes must go out as literals."""
    r = _centred_rows(32, 2800, 4, transparent=0.02)
    r[2, :1400] = r[0, :1400]
    r[3, 1400:] = r[0, 1400:]
    return r


def window_c():
    r = _centred_rows(33, 2730, 3)
    return np.stack([r[0], r[1], r[2], r[0]])


CONST_A = (10, 200, 30, 255)
CONST_B = (10, 60, 30, 77)

# every case of the default path: name -> tiles of one encode_png call
CASES = {
    "tiny": tiny_tiles,
    "one_column": lambda: [np.repeat(_noise(22, 40, 1), 3, 0)],
    "one_row": lambda: [_opaque(_noise(23, 1, 300))],
    "constant": lambda: [_const(64, 64, CONST_A), _const(64, 64, CONST_B)],
    "long_runs": lambda: [_const(8, 700, CONST_A)],
    "noise": lambda: [noise_tile()],
    "upsampled": upsampled_tiles,
    "skewed": lambda: [fibonacci_tile()],
    "window_a": lambda: [window_a()],
    "window_b": lambda: [window_b()],
    "window_c": lambda: [window_c()],
    "rows_4096": lambda: [_noise(25, 4096, 2)],
    "rows_4097": lambda: [_noise(26, 4097, 2)],
    "mixed": lambda: [tiny_tiles()[2], _const(64, 64, CONST_A), noise_tile(), upsampled_tiles()[0]],
}
OTHER_PATH_CASES = ("constant", "noise", "upsampled", "skewed", "tiny")
_tiles = {}


def tiles_of(name):
    if name not in _tiles:
        _tiles[name] = CASES[name]()
    return _tiles[name]


def pack(tiles, fill=0xA5):
    """The tiles in the top-left corners of one (n, max_h, max_w, 4) batch,
    the rest of every slot filled with bytes no tile may pick up."""
    mh, mw = max(t.shape[0] for t in tiles), max(t.shape[1] for t in tiles)
    batch = np.full((len(tiles), mh, mw, 4), fill, np.uint8)
    for i, t in enumerate(tiles):
        batch[i, :t.shape[0], :t.shape[1]] = t
    return batch, [(t.shape[1], t.shape[0]) for t in tiles]


class _Rows:
    """oracle.go_png_rows computed once per tile."""

    def __init__(self, oracle):
        self.oracle, self.cache = oracle, {}

    def go_png_rows(self, rgba):
        key = (rgba.shape, rgba.tobytes())
        if key not in self.cache:
            self.cache[key] = self.oracle.go_png_rows(rgba)
        return self.cache[key]


@pytest.fixture(scope="module")
def ref(oracle):
    return _Rows(oracle)


@pytest.fixture(scope="module")
def enc(gpu):
    """enc(name, mode) -> the PNGs of a case's tiles encoded in one call,
    mode "default", "fixed" (GSKYHIP_PNG_FIXED=1) or "zlib"
    (GSKYHIP_PNG_ZLIB=1); each (case, mode) is encoded once."""
    import torch

    from gsky_amd.encode import encode_png
    done = {}

    def run(name, mode="default", tiles=None):
        key = (name, mode)
        if tiles is not None or key not in done:
            batch, sizes = pack(tiles if tiles is not None else tiles_of(name))
            with pytest.MonkeyPatch.context() as mp:
                mp.delenv("GSKYHIP_PNG_FIXED", raising=False)
                mp.delenv("GSKYHIP_PNG_ZLIB", raising=False)
                if mode != "default":
                    mp.setenv({"fixed": "GSKYHIP_PNG_FIXED", "zlib": "GSKYHIP_PNG_ZLIB"}[mode], "1")
                pngs = encode_png(torch.from_numpy(batch).to(gpu), sizes)
            if tiles is not None:
                return pngs
            done[key] = pngs
        return done[key]
    return run


# ------------------------------------------------------------------ the per-tile check
def check_tile(png, rgba, ref, path="gpu"):
    """test_png._check plus: the stream ends exactly where zlib says it does
    (Adler-32 right, nothing after it), the path that made it, well-formed
    dynamic codes, the derived size cap and gskyhip_png_bound.  Returns
    (z, header, rows)."""
    from gsky_amd import lib
    _check(png, rgba, ref)
    _, rows = ref.go_png_rows(rgba)
    z = b"".join(d for t, d in _chunks(png) if t == b"IDAT")
    d = zlib.decompressobj()
    assert d.decompress(z) == rows
    assert d.eof and d.unused_data == b""
    assert lib().gskyhip_png_bound(rgba.shape[1], rgba.shape[0]) >= len(png)
    if path == "zlib":
        assert z[:2] == b"\x78\x9c"
        return z, None, rows
    hd = deflate_header(z)
    assert z[:2] == b"\x78\x01" and hd["final"] == 1   # the first block is the last: exactly one
    assert hd["btype"] in (1, 2)
    if hd["btype"] == 2:
        assert max(hd["lit_lens"]) <= 15 and max(hd["dist_lens"]) <= 15 and max(hd["cl_lens"]) <= 7
        assert kraft(hd["lit_lens"]) == 1 and kraft(hd["cl_lens"]) == 1
        assert hd["lit_lens"][256] > 0
    assert len(z) <= gpu_size_cap(len(rows))
    return z, hd, rows


def check_case(name, enc, ref, mode="default", path="gpu"):
    tiles = tiles_of(name)
    pngs = enc(name, mode)
    assert len(pngs) == len(tiles)
    out = [check_tile(p, t, ref, path) for p, t in zip(pngs, tiles)]
    if mode in GOLDEN["png"] and path == "gpu":   # the bytes are the recorded ones
        assert [record(z) for z, _, _ in out] == GOLDEN["png"][mode][name]
    return out


def filter_types(rows, h):
    n = len(rows) // h
    return [rows[y * n] for y in range(h)]


# ------------------------------------------------------------------ CPU tests
def _skewed_buffer():
    rng = np.random.default_rng(3)
    return (rng.geometric(0.3, 50000) % 256).astype(np.uint8).tobytes()


def test_header_reader_on_zlib_dynamic_block():
    c = zlib.compressobj(6)
    z = c.compress(_skewed_buffer()) + c.flush()
    hd = deflate_header(z)
    assert hd["btype"] == 2 and hd["final"] == 1
    assert len(hd["cl_lens"]) == 19 and len(hd["lit_lens"]) >= 257 and 1 <= len(hd["dist_lens"]) <= 30
    assert max(hd["lit_lens"]) <= 15 and max(hd["cl_lens"]) <= 7 and hd["lit_lens"][256] > 0
    assert kraft(hd["lit_lens"]) == 1 and kraft(hd["cl_lens"]) == 1
    used = [n for n in hd["dist_lens"] if n]
    assert kraft(used) == 1 or used == [1]


def test_header_reader_on_zlib_fixed_block():
    c = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_FIXED)
    z = c.compress(_skewed_buffer()) + c.flush()
    hd = deflate_header(z)
    assert hd["btype"] == 1 and hd["final"] == 1 and hd["lit_lens"] == []


def test_header_reader_decodes_repeat_codes():
    """A histogram of two plateaus (Huffman only): the 256 literal lengths
    come in long runs, which zlib writes with the repeat code 16; all are read
    back."""
    data = np.concatenate([np.tile(np.arange(128), 120), np.tile(np.arange(128, 256), 40)])
    data = np.random.default_rng(4).permutation(data).astype(np.uint8).tobytes()
    c = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_HUFFMAN_ONLY)
    z = c.compress(data) + c.flush()
    hd = deflate_header(z)
    assert hd["btype"] == 2 and hd["cl_lens"][16] > 0
    assert all(hd["lit_lens"][:257]) and kraft(hd["lit_lens"]) == 1


def test_literal_only_bytes_bounds(oracle):
    _, noise = oracle.go_png_rows(tiles_of("noise")[0])
    assert literal_only_bytes(noise) >= 0.99 * len(noise)
    _, const = oracle.go_png_rows(tiles_of("long_runs")[0])
    assert literal_only_bytes(const) <= len(const) // 8 + 16
    for t in tiles_of("constant"):   # what `len(z) < n // 8` of the constant cases rests on
        _, const = oracle.go_png_rows(t)
        assert len(const) // 8 <= literal_only_bytes(const) <= len(const) // 8 + 24
    assert literal_only_bytes(b"\x00") == 2 + 1 + 4
    # a code of two symbols, 1 bit each; a dyadic histogram is coded at its entropy
    assert huffman_lengths([5, 0, 9]) == [1, 0, 1]
    assert sorted(huffman_lengths([8, 4, 2, 1, 1])) == [1, 2, 3, 4, 4]


def test_fibonacci_tile_histogram(oracle):
    """The skewed tile's own precondition: the byte histogram of the rows
    the encoder receives has an unconstrained Huffman depth above 15."""
    _, rows = oracle.go_png_rows(tiles_of("skewed")[0])
    freq = np.bincount(np.frombuffer(rows, np.uint8), minlength=256).tolist() + [1]
    assert max(huffman_lengths(freq)) > 15


def test_window_tiles_meet_their_preconditions(oracle):
    """Every row of the window-edge tiles is left unfiltered, so the repeated
    pixel rows are repeated bytes at exactly the distances the cases name."""
    for name, w, bpp, h in (("window_a", 5461, 3, 3), ("window_b", 2800, 4, 4), ("window_c", 2730, 3, 4)):
        opaque, rows = oracle.go_png_rows(tiles_of(name)[0])
        assert opaque == (bpp == 3)
        s = 1 + bpp * w
        assert len(rows) == h * s and set(filter_types(rows, h)) <= {0, 2}
        r = [rows[y * s + 1:(y + 1) * s] for y in range(h)]
        if name == "window_a":
            assert s == 16384 and r[2] == r[0] and r[1] != r[0]
        elif name == "window_b":
            half = 4 * 1400
            assert s == 11201 and 3 * s > 32768 and r[2][:half] == r[0][:half] and r[3][half:] == r[0][half:]
        else:
            assert 3 * s == 24573 and r[3] == r[0] and r[1] != r[0] and r[2] != r[0]


def host_twin_stream(rgba, ref, fixed):
    """gskyhip_png_deflate_rows_host over the reference rows of a tile."""
    import ctypes as C

    from gsky_amd import lib
    opaque, rows = ref.go_png_rows(rgba)
    h = rgba.shape[0]
    src = np.frombuffer(rows, np.uint8).copy()
    out = np.empty(gpu_size_cap(len(rows)), np.uint8)
    n = C.c_int64(-1)
    rc = lib().gskyhip_png_deflate_rows_host(C.c_void_p(src.ctypes.data), h, len(rows) // h, 3 if opaque else 4,
                                             int(fixed), C.c_void_p(out.ctypes.data), out.size, C.byref(n))
    assert rc == 0
    return out[:n.value].tobytes()


@pytest.mark.parametrize("mode", ["default", "fixed"])
def test_host_twin_gives_the_recorded_streams(ref, mode):
    """The functions the PNG kernels run, on the host, give the bytes the GPU
    gave before the encoders were merged -- every case but rows_4097 (host
    zlib), in both modes."""
    assert set(GOLDEN["png"][mode]) == set(CASES) - {"rows_4097"}
    for name, recs in GOLDEN["png"][mode].items():
        got = [host_twin_stream(t, ref, mode == "fixed") for t in tiles_of(name)]
        assert [record(z) for z in got] == recs, name
        for z, t in zip(got, tiles_of(name)):
            assert zlib.decompress(z) == ref.go_png_rows(t)[1]
            assert z[:2] == b"\x78\x01" and deflate_header(z)["btype"] in ((1,) if mode == "fixed" else (1, 2))
    (one_row,), tiny = GOLDEN["png"]["default"]["one_row"], GOLDEN["png"]["default"]["tiny"]
    assert one_row["len"] == 959   # a stored block would take 912
    assert [r["len"] for r in tiny] == [12, 11, 13, 15, 18, 20]


def test_tiny_tiles_take_the_fixed_fallback_on_the_host_twin(ref):
    for t in tiles_of("tiny"):
        assert deflate_header(host_twin_stream(t, ref, False))["btype"] == 1


def test_block_encoder_gives_the_recorded_streams():
    """gskyhip_deflate_blocks_host over tests/deflate_corpus.py: the bytes of
    the commit before plan_block was split."""
    from gsky_amd import encode

    from .deflate_corpus import corpus
    modes = {"zlib6": (True, 6), "raw6": (False, 6), "zlib0": (True, 0), "raw0": (False, 0)}
    assert set(GOLDEN["deflate_host"]) == set(modes)
    names, blocks = [n for n, _ in corpus()], [b for _, b in corpus()]
    for mode, (wrapper, level) in modes.items():
        streams = encode.deflate_blocks(blocks, zlib_wrapper=wrapper, level=level, where="host")
        assert [dict(record(z), name=n) for n, z in zip(names, streams)] == GOLDEN["deflate_host"][mode], mode


# ------------------------------------------------------------------ GPU cases, default path
@pytest.mark.gpu
def test_tiny_tiles_take_the_fixed_fallback(enc, ref):
    for z, hd, rows in check_case("tiny", enc, ref):
        assert hd["btype"] == 1


@pytest.mark.gpu
def test_one_column(enc, ref):
    (z, hd, rows), = check_case("one_column", enc, ref)
    assert len(rows) == 120 * 5   # stride 5: every candidate distance but 1 reaches into the rows above


@pytest.mark.gpu
def test_one_row(enc, ref):
    (z, hd, rows), = check_case("one_row", enc, ref)
    assert len(rows) == 901


@pytest.mark.gpu
def test_constant_tiles_are_coded_with_matches(enc, ref):
    for z, hd, rows in check_case("constant", enc, ref):
        assert len(z) < len(rows) // 8   # no literal-only coding goes below 1 bit per byte


@pytest.mark.gpu
def test_long_runs_chain_258_byte_matches(enc, ref):
    (z, hd, rows), = check_case("long_runs", enc, ref)
    assert len(rows) == 8 * 2101
    assert len(z) < len(rows) // 8


@pytest.mark.gpu
def test_noise(enc, ref):
    (z, hd, rows), = check_case("noise", enc, ref)
    png, = enc("noise")
    assert sum(1 for t, _ in _chunks(png) if t == b"IDAT") >= 3
    assert hd["btype"] == 2
    # no distance code or one in use: the second leaf is forced, both 1 bit
    assert [n for n in hd["dist_lens"] if n] == [1, 1]


@pytest.mark.gpu
def test_upsampled_tiles_are_coded_with_matches(enc, ref):
    for z, hd, rows in check_case("upsampled", enc, ref):
        assert len(z) < literal_only_bytes(rows)


@pytest.mark.gpu
def test_skewed_histogram_reaches_the_length_limit(enc, ref):
    (z, hd, rows), = check_case("skewed", enc, ref)
    assert hd["btype"] == 2   # not the fixed fallback of a code that came out incomplete
    print("skewed: max lit %d, max dist %d, max cl %d" % (max(hd["lit_lens"]), max(hd["dist_lens"]),
                                                          max(hd["cl_lens"])))
    assert hd["btype"] == 2 and max(hd["lit_lens"]) == 15


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["window_a", "window_b", "window_c"])
def test_window_edge(enc, ref, name):
    """A: a match at 2 * stride = 32768, the largest legal distance.  B: 2 *
    stride used, 3 * stride = 33603 skipped (an encoder that took it would
    write a distance no inflater accepts).  C: 3 * stride = 24573 used."""
    (z, hd, rows), = check_case(name, enc, ref)
    assert len(z) < literal_only_bytes(rows)


@pytest.mark.gpu
def test_row_limit_switches_to_the_host_path(enc, ref):
    (z, hd, rows), = check_case("rows_4096", enc, ref)
    assert z[:2] == b"\x78\x01"
    (z, hd, rows), = check_case("rows_4097", enc, ref, path="zlib")
    assert z[:2] == b"\x78\x9c"


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["default", "fixed"])
def test_mixed_batch_tiles_equal_tiles_encoded_alone(enc, ref, mode):
    tiles = tiles_of("mixed")
    batch, sizes = pack(tiles)
    assert batch.shape == (4, 100, 200, 4)
    pngs = enc("mixed", mode)
    for p, t in zip(pngs, tiles):
        check_tile(p, t, ref)
        alone, = enc(None, mode, tiles=[t])
        assert alone == p


# ------------------------------------------------------------------ the other two paths
@pytest.mark.gpu
@pytest.mark.parametrize("name", OTHER_PATH_CASES)
def test_fixed_codes_only(enc, ref, name):
    fixed = check_case(name, enc, ref, mode="fixed")
    default = check_case(name, enc, ref)
    for (zf, hf, _), (zd, _, _) in zip(fixed, default):
        assert hf["btype"] == 1
        assert len(zd) <= len(zf)   # the default path falls back whenever fixed is not longer


@pytest.mark.gpu
@pytest.mark.parametrize("name", OTHER_PATH_CASES + ("mixed",))
def test_host_zlib_path(enc, ref, name):
    from PIL import Image
    check_case(name, enc, ref, mode="zlib", path="zlib")
    for ph, pd in zip(enc(name, "zlib"), enc(name)):
        zh = b"".join(d for t, d in _chunks(ph) if t == b"IDAT")
        zd = b"".join(d for t, d in _chunks(pd) if t == b"IDAT")
        assert zlib.decompress(zh) == zlib.decompress(zd)
        assert _chunks(ph)[0] == _chunks(pd)[0]   # IHDR
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(ph))), np.asarray(Image.open(io.BytesIO(pd))))


# ------------------------------------------------------------------ argument errors
def _raw_encode(gpu, w, h, size, cap_short=0, ws_short=0):
    """gskyhip_encode_png of one w x h slot through the C ABI; returns its code."""
    import ctypes as C

    import torch

    from gsky_amd import lib
    L = lib()
    rgba = torch.zeros((1, h, w, 4), dtype=torch.uint8, device=gpu)
    ws = torch.empty(int(L.gskyhip_png_workspace_size(1, w, h)), dtype=torch.uint8, device=gpu)
    cap = int(L.gskyhip_png_bound(max(size[0], 1), max(size[1], 1)))
    out = np.empty(cap, np.uint8)
    lens = np.zeros(1, np.int64)
    wh = np.asarray([size], np.int32)
    return L.gskyhip_encode_png(C.c_void_p(rgba.data_ptr()), 1, w, h, w * h * 4, w * 4,
                                wh.ctypes.data_as(C.c_void_p), C.c_void_p(ws.data_ptr()), ws.numel() - ws_short,
                                out.ctypes.data_as(C.c_void_p), cap - cap_short, lens.ctypes.data_as(C.c_void_p), 1,
                                C.c_void_p(torch.cuda.current_stream().cuda_stream))


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(21, 10), (20, 11), (0, 10), (20, 0)])
def test_bad_sizes_are_refused(gpu, size):
    import torch

    from gsky_amd import GskyError
    from gsky_amd.encode import encode_png
    with pytest.raises(GskyError) as e:
        encode_png(torch.zeros((1, 10, 20, 4), dtype=torch.uint8, device=gpu), [size])
    assert e.value.code == E_ARG
    assert _raw_encode(gpu, 20, 10, size) == E_ARG


@pytest.mark.gpu
def test_short_buffers_are_refused(gpu):
    assert _raw_encode(gpu, 20, 10, (20, 10)) == 0
    assert _raw_encode(gpu, 20, 10, (20, 10), cap_short=1) == E_ARG
    assert _raw_encode(gpu, 20, 10, (20, 10), ws_short=1) == E_ARG


# ------------------------------------------------------------------ recorded sizes
@pytest.mark.gpu
def test_size_table(enc, ref):
    """Prints (pytest -s) the default path's zlib bytes of every tile above
    next to zlib level 6 on the same rows.  Recorded, not asserted."""
    print("\n%-12s %-10s %8s %8s %8s %6s" % ("case", "w x h", "rows", "gpu", "zlib -6", "ratio"))
    for name in CASES:
        path = "zlib" if name == "rows_4097" else "gpu"
        for (z, hd, rows), t in zip(check_case(name, enc, ref, path=path), tiles_of(name)):
            ref6 = len(zlib.compress(rows, 6))
            print("%-12s %-10s %8d %8d %8d %6.2f" % (name, "%dx%d" % (t.shape[1], t.shape[0]), len(rows), len(z),
                                                      ref6, len(z) / ref6))
