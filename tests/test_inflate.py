"""The RFC 1950 / 1951 decoder of gsky_amd/csrc/inflate_core.h through
gskyhip_inflate_blocks_host (host threads, no device) and, marked gpu, through
gskyhip_inflate_blocks (one wave64 per stream).  The reference is Python's
zlib.decompress; every comparison is exact.

The streams: what zlib writes at its levels and strategies over inputs chosen
for the corner each reaches (noted per case), and hand-assembled streams for
what zlib never writes (distance 32768, a distance alphabet of one code, none
used, a code-length repeat across the literal / distance boundary)."""
import zlib

import numpy as np
import pytest

from gsky_amd import ingest


def _deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, wbits=15):
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, 8, strategy)
    return c.compress(data) + c.flush()


# ---------------------------------------------------------------- a bit writer for hand-made streams
class Bits:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, value, nbits):
        """nbits of value, least significant first (header fields, extra bits)."""
        self.acc |= (value & ((1 << nbits) - 1)) << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, length):
        """A Huffman code: most significant bit first."""
        for k in range(length - 1, -1, -1):
            self.put((code >> k) & 1, 1)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def raw(self, data):
        self.align()
        self.out += data

    def bytes(self):
        self.align()
        return bytes(self.out)


def _canonical(lens):
    """{symbol: length} -> {symbol: (code, length)} (RFC 1951 3.2.2)."""
    codes, code = {}, 0
    for ln in range(1, 16):
        for s in sorted(k for k, v in lens.items() if v == ln):
            codes[s] = (code, ln)
            code += 1
        code <<= 1
    return codes


def _fixed_lit(sym):
    if sym < 144:
        return 0x30 + sym, 8
    if sym < 256:
        return 0x190 + sym - 144, 9
    if sym < 280:
        return sym - 256, 7
    return 0xC0 + sym - 280, 8


def _dynamic_header(b, lit_lens, dist_lens, n_lit, n_dist, cl_lens, final=1):
    """BFINAL, BTYPE = 2 and the code-length section.  The length sequence is
    run-length coded greedily with 18 / 17 for zeros (a run may cross from the
    literal lengths into the distance lengths) and plain symbols otherwise;
    cl_lens: the (complete) code-length code to write it with."""
    seq = [lit_lens.get(i, 0) for i in range(n_lit)] + [dist_lens.get(i, 0) for i in range(n_dist)]
    ops, i = [], 0
    while i < len(seq):
        if seq[i] == 0:
            j = i
            while j < len(seq) and seq[j] == 0 and j - i < 138:
                j += 1
            run = j - i
            if run >= 11 and 18 in cl_lens:
                ops.append((18, run - 11, 7))
                i = j
                continue
            if run >= 3 and 17 in cl_lens:
                run = min(run, 10)
                ops.append((17, run - 3, 3))
                i += run
                continue
        ops.append((seq[i], 0, 0))
        i += 1
    assert sum(2.0 ** -v for v in cl_lens.values()) == 1.0
    order = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
    n_cl = max(k for k, s in enumerate(order) if s in cl_lens) + 1
    n_cl = max(n_cl, 4)
    b.put(final, 1)
    b.put(2, 2)
    b.put(n_lit - 257, 5)
    b.put(n_dist - 1, 5)
    b.put(n_cl - 4, 4)
    for s in order[:n_cl]:
        b.put(cl_lens.get(s, 0), 3)
    cl = _canonical(cl_lens)
    for s, extra, nb in ops:
        b.code(*cl[s])
        if nb:
            b.put(extra, nb)
    return ops


def _wrap(raw_deflate, payload):
    return b"\x78\x9c" + raw_deflate + zlib.adler32(payload).to_bytes(4, "big")


def _hand_distance_32768(rng):
    """A stored block of 32,768 bytes, then a fixed block with <258, 32768>
    and <3, 1>: the farthest distance there is."""
    first = rng.integers(0, 256, 32768, dtype=np.uint8).tobytes()
    b = Bits()
    b.put(0, 1)
    b.put(0, 2)
    b.align()
    b.put(32768, 16)
    b.put(32768 ^ 0xFFFF, 16)
    b.raw(first)
    b.put(1, 1)
    b.put(1, 2)
    b.code(*_fixed_lit(285))        # length 258
    b.code(29, 5)                   # distance symbol 29: 24577 + 13 extra bits
    b.put(32768 - 24577, 13)
    b.code(*_fixed_lit(257))        # length 3
    b.code(0, 5)                    # distance 1
    b.code(*_fixed_lit(256))
    raw = b.bytes()
    payload = zlib.decompress(raw, -15)
    assert payload == first + first[:258] + first[257:258] * 3
    return _wrap(raw, payload)


_LIT4 = {97: 2, 98: 2, 256: 2, 257: 2}


def _hand_one_distance_code():
    """A dynamic block whose distance alphabet is exactly one code of one bit
    (what libdeflate writes): a, b, <3, 1>, a."""
    b = Bits()
    _dynamic_header(b, _LIT4, {0: 1}, 258, 1, {18: 1, 1: 2, 2: 2})
    lit = _canonical(_LIT4)
    b.code(*lit[97])
    b.code(*lit[98])
    b.code(*lit[257])
    b.code(0, 1)
    b.code(*lit[97])
    b.code(*lit[256])
    return b.bytes()


def _hand_no_distance_code():
    """HDIST = 1 with that one length 0 (literals only); HLIT = 270 so that the
    zero run after the end-of-block code crosses from the literal lengths into
    the distance length as one repeat of 14."""
    lens = {97: 2, 98: 2, 99: 2, 256: 2}
    b = Bits()
    ops = _dynamic_header(b, lens, {}, 270, 1, {18: 1, 0: 2, 2: 2})
    assert ops[-1] == (18, 3, 7)    # 13 literal zeros + 1 distance zero in one run
    lit = _canonical(lens)
    for ch in b"abcabccba":
        b.code(*lit[ch])
    b.code(*lit[256])
    return b.bytes()


def _hand_oversubscribed():
    """A dynamic header whose code-length code has three codes of one bit."""
    b = Bits()
    b.put(1, 1)
    b.put(2, 2)
    b.put(0, 5)
    b.put(0, 5)
    b.put(0, 4)            # four code-length code lengths: 16, 17, 18, 0
    for v in (1, 1, 1, 0):
        b.put(v, 3)
    b.put(0, 32)
    return b"\x78\x9c" + b.bytes() + bytes(8)


def _hand_distance_before_start():
    """A fixed block that opens with <3, 1>: nothing to copy from."""
    b = Bits()
    b.put(1, 1)
    b.put(1, 2)
    b.code(*_fixed_lit(257))
    b.code(0, 5)
    b.code(*_fixed_lit(256))
    return b"\x78\x9c" + b.bytes() + bytes(4)


# ---------------------------------------------------------------- the cases
HELLO = b"hello hello hello world" * 40


def _int16_walk():
    rng = np.random.default_rng(16)
    return np.cumsum(rng.integers(-40, 41, (128, 128)), axis=1).astype(np.int16).tobytes()


def _build_cases():
    rng = np.random.default_rng(20261020)
    rand = lambda n: rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    cases = []   # (name, stream, wrapper)

    def add(name, stream, wrapper=True):
        cases.append((name, stream, wrapper))

    add("empty", zlib.compress(b""))                                     # fixed block, 0 bytes out
    add("one-byte", zlib.compress(b"\x07"))                              # fixed block, 1 byte out
    add("zeros-100k", zlib.compress(bytes(100000), 6))                   # distance 1, length 258, overlapping copies
    r70 = rand(70000)
    add("random-70k-stored", zlib.compress(r70, 0))                      # stored blocks (> 65,535 is split)
    add("random-70k-level6", zlib.compress(r70, 6))
    add("hello-fixed", _deflate(HELLO, 6, zlib.Z_FIXED))                 # fixed block with matches, length 258
    runs = b"".join(bytes([v]) * int(k) for v, k in zip(rng.integers(0, 256, 400), rng.integers(1, 600, 400)))
    add("runs-rle", _deflate(runs, 6, zlib.Z_RLE))                       # distance 1 only
    fib = [1, 1]
    while len(fib) < 24:
        fib.append(fib[-1] + fib[-2])
    sym = np.repeat(np.arange(24, dtype=np.uint8), fib)
    assert sym.size == 121392
    rng.shuffle(sym)
    add("fibonacci-huffman", _deflate(sym.tobytes(), 6, zlib.Z_HUFFMAN_ONLY))   # code length 15, no matches
    add("two-symbols-huffman", _deflate(rng.integers(0, 2, 5000, dtype=np.uint8).tobytes(), 6, zlib.Z_HUFFMAN_ONLY))
    unit = rng.integers(0, 4, 30000, dtype=np.uint8).tobytes()
    add("distance-30000", zlib.compress(unit + unit + unit[:5000], 9))   # distance 30,000, length 258
    add("mixed-blocks", zlib.compress(rand(40000) + bytes(40000) + b"abcabcabd" * 3000 + rand(20000), 6))
    add("int16-walk", zlib.compress(_int16_walk(), 6))                   # the window used across its depth
    add("f32-noise", zlib.compress(np.random.default_rng(32).standard_normal((128, 128)).astype(np.float32).tobytes(), 6))
    add("hand-distance-32768", _hand_distance_32768(rng))
    one = _hand_one_distance_code()
    add("hand-one-distance-code", _wrap(one, zlib.decompress(one, -15)))
    none = _hand_no_distance_code()
    add("hand-no-distance-code", _wrap(none, zlib.decompress(none, -15)))
    add("hand-one-distance-code-raw", one, False)                        # the same payloads as raw streams
    add("hand-no-distance-code-raw", none, False)
    add("hello-raw", _deflate(HELLO, 6, zlib.Z_DEFAULT_STRATEGY, -15), False)
    return cases


CASES = _build_cases()
# the reference, computed once and never changed
EXPECTED = {name: zlib.decompress(stream, 15 if wrapper else -15) for name, stream, wrapper in CASES}
for _v in EXPECTED.values():
    assert isinstance(_v, bytes)

assert EXPECTED["hand-one-distance-code"] == b"abbbba"
assert EXPECTED["hand-no-distance-code"] == b"abcabccba"


def _check_cases(where):
    for wrapper in (True, False):
        sel = [(n, s) for n, s, w in CASES if w == wrapper]
        status, out_len, outs, gaps = ingest.inflate_blocks([s for _, s in sel], [len(EXPECTED[n]) for n, _ in sel],
                                                            zlib_wrapper=wrapper, where=where, gap=64)
        for k, (name, _) in enumerate(sel):
            assert status[k] == 0, (name, status[k])
            assert out_len[k] == len(EXPECTED[name]), name
            assert outs[k].tobytes() == EXPECTED[name], name
        for g in gaps:
            assert (g == 0xA5).all()


def _check_batches(where, counts):
    """One launch of n streams of mixed cases and sizes: every output exact,
    every out_len right, the bytes between the output ranges untouched."""
    pool = [(n, s) for n, s, w in CASES if w]
    for n in counts:
        sel = [pool[(k * 7 + n) % len(pool)] for k in range(n)]
        slack = [k % 3 for k in range(n)]          # some capacities larger than the output
        sizes = [len(EXPECTED[name]) + slack[k] for k, (name, _) in enumerate(sel)]
        need = [len(EXPECTED[name]) for name, _ in sel]
        status, out_len, outs, gaps = ingest.inflate_blocks([s for _, s in sel], sizes, where=where, out_need=need,
                                                            gap=37)
        assert len(gaps) == n + 1
        for k, (name, _) in enumerate(sel):
            assert status[k] == 0, (n, k, name, status[k])
            assert out_len[k] == need[k], (n, k, name)
            assert outs[k][:need[k]].tobytes() == EXPECTED[name], (n, k, name)
        for g in gaps:
            assert g.size == 37 and (g == 0xA5).all(), n


def _malformed():
    """(name, stream, capacity, expected status or None for any non-zero,
    zlib must refuse it)."""
    hello = _deflate(HELLO, 6, zlib.Z_FIXED)
    hello_stored = zlib.compress(HELLO, 0)
    walk = zlib.compress(_int16_walk(), 6)
    nh, nw = len(HELLO), 128 * 128 * 2
    flipped = bytearray(walk)
    flipped[-2] ^= 0x01
    m = [
        ("cut-in-zlib-header", hello[:1], nh, None, True),
        ("cut-in-dynamic-header", walk[:5], nw, None, True),
        ("cut-in-code-lengths", walk[:20], nw, None, True),
        ("cut-mid-symbol", walk[:len(walk) // 2], nw, None, True),
        ("cut-mid-symbol-fixed", hello[:len(hello) // 2], nh, None, True),
        ("cut-in-stored-length", hello_stored[:4], nh, None, True),
        ("cut-before-adler", walk[:-4], nw, None, True),
        ("cut-in-adler", hello[:-1], nh, None, True),
        ("block-type-3", b"\x78\x9c\x07" + bytes(8), 16, 2, True),
        ("adler-flipped", bytes(flipped), nw, 6, True),
        ("distance-before-start", _hand_distance_before_start(), 16, 4, True),
        ("capacity-one-short", hello, nh - 1, 5, False),
        ("over-subscribed", _hand_oversubscribed(), 16, 3, True),
    ]
    return m, hello, walk


def _check_malformed(where):
    bad, hello, walk = _malformed()
    for name, stream, cap, want, zlib_refuses in bad:
        if zlib_refuses:
            with pytest.raises(zlib.error):
                zlib.decompress(stream)
    # every malformed stream between two valid ones, in one launch
    streams = [hello] + [s for _, s, _, _, _ in bad] + [walk]
    sizes = [len(HELLO)] + [c for _, _, c, _, _ in bad] + [128 * 128 * 2]
    status, out_len, outs, gaps = ingest.inflate_blocks(streams, sizes, where=where, gap=16)
    assert status[0] == 0 and outs[0].tobytes() == HELLO
    assert status[-1] == 0 and outs[-1].tobytes() == _int16_walk()
    for k, (name, _, cap, want, _) in enumerate(bad, 1):
        assert status[k] != 0, name
        if want is not None:
            assert status[k] == want, (name, status[k])
        assert 0 <= out_len[k] <= cap, name
    for g in gaps:
        assert (g == 0xA5).all()
    # a valid stream whose output is shorter than required
    status, _, _, _ = ingest.inflate_blocks([hello], [len(HELLO) + 8], where=where, out_need=[len(HELLO) + 1])
    assert status == [7]


# ---------------------------------------------------------------- host threads (no device)
def test_host_cases_match_zlib():
    _check_cases("host")


def test_host_batches():
    _check_batches("host", (1, 63, 64, 65, 300))


def test_host_malformed_streams():
    _check_malformed("host")


def test_arguments():
    with pytest.raises(ValueError):
        ingest.inflate_blocks([b""], [0], where="elsewhere")
    with pytest.raises(ValueError):
        ingest.inflate_blocks([b"", b""], [0])
    from gsky_amd import GskyError
    with pytest.raises(GskyError):   # out_need beyond out_cap
        ingest.inflate_blocks([zlib.compress(b"abc")], [3], where="host", out_need=[4])
    assert ingest.inflate_blocks([], [], where="host")[0] == []


# ---------------------------------------------------------------- the kernel
@pytest.mark.gpu
def test_gpu_cases_match_zlib(gpu):
    _check_cases("device")


@pytest.mark.gpu
def test_gpu_batches(gpu):
    _check_batches("device", (1, 63, 64, 65, 300))


@pytest.mark.gpu
def test_gpu_malformed_streams(gpu):
    """The error path of the kernel: the host build of the same core passes
    these streams (test_host_malformed_streams) and every truncation and bit
    flip of tools/inflate_check.cpp under the address sanitizer first."""
    _check_malformed("device")
