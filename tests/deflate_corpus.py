"""The block corpus of the Deflate encoder tests (tests/test_deflate.py on the
host twin, tests/test_deflate_gpu.py on the device): small, fixed, built
once."""
from __future__ import annotations

import functools

import numpy as np


def shuffle(a: np.ndarray) -> bytes:
    """HDF5 shuffle of a 1-D array: byte b of element e at b * len + e."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(a.shape[0], a.dtype.itemsize).T.copy().tobytes()


def fibonacci_block() -> bytes:
    """Byte counts 1, 1, 2, 3, 5, ... over 25 distinct values in shuffled
    order (196,417 bytes): the Huffman tree stays more than 15 deep after the
    matches thin the counts of the frequent values, so the length limiter has
    to run (tools/deflate_check.cpp reports that it did)."""
    rng = np.random.default_rng(7)
    fib = [1, 1]
    while len(fib) < 25:
        fib.append(fib[-1] + fib[-2])
    vals = rng.permutation(256)[:25]
    b = np.concatenate([np.full(c, v, np.uint8) for c, v in zip(fib, vals)])
    return rng.permutation(b).tobytes()


def half_compressible() -> bytes:
    """int16 row of width 2048, high byte 1, uniformly random low byte."""
    rng = np.random.default_rng(11)
    return shuffle((256 + rng.integers(0, 256, 2048)).astype(np.int16))


@functools.lru_cache(maxsize=None)
def corpus():
    """[(name, bytes)], the same objects on every call."""
    rng = np.random.default_rng(2024)
    out = []
    for n in (0, 1, 2, 3, 4):
        out.append(("len%d" % n, bytes(range(65, 65 + n))))
    for n in (257, 258, 259, 516, 70000):
        out.append(("run%d" % n, b"\x07" * n))
    out.append(("random8192", rng.integers(0, 256, 8192, dtype=np.uint8).tobytes()))
    out.append(("random65535", rng.integers(0, 256, 65535, dtype=np.uint8).tobytes()))
    out.append(("random65536", rng.integers(0, 256, 65536, dtype=np.uint8).tobytes()))
    out.append(("one_value", b"\xee" * 1000))
    out.append(("all256", bytes(range(256))))
    period = rng.integers(0, 256, 40000, dtype=np.uint8).tobytes()
    out.append(("period40000", (period * 3)[:100000]))
    out.append(("fibonacci", fibonacci_block()))
    out.append(("row_i8_53", shuffle(rng.integers(-5, 6, 53).astype(np.int8))))
    x = np.linspace(0, 6, 257)
    out.append(("row_f32_257", shuffle((280 + 10 * np.sin(x) + rng.normal(0, 0.01, 257)).astype(np.float32))))
    out.append(("row_i16_2048", shuffle((1000 + 50 * np.sin(np.linspace(0, 20, 2048)) +
                                         rng.integers(-2, 3, 2048)).astype(np.int16))))
    f = rng.normal(0, 1, 300).astype(np.float32)
    f[::7] = -0.0
    u = f.view(np.uint32)
    u[3::11] = 0x7FC00000 | rng.integers(1, 1 << 20, u[3::11].shape[0]).astype(np.uint32)   # NaN payloads
    u[5::13] = 0xFFC00001
    out.append(("row_f32_nan", shuffle(f)))
    out.append(("const_f32_row", shuffle(np.full(2048, 273.15, np.float32))))
    out.append(("const_i16_67", shuffle(np.full(67, -999, np.int16))))
    out.append(("half_compressible", half_compressible()))
    return out
