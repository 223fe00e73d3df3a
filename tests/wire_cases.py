"""Payloads for the tests of the receiving side (tests/test_wire_scan.py,
tests/test_gpu_wire_unpack.py): seeded random ciphertext words in the
library's own wire layout (wire.encode_words), with the element forms the
index scan has to tell apart, and the scan's ctypes call."""
import ctypes

import numpy as np

WIDTHS = (128, 192, 256, 512)          # n^2 words of the 2048/3072/4096/8192-bit keys
COUNTS = (1, 999, 1000, 1001, 2001)    # around the APPENDS batches of 1000; element 0 has the long header
EXPS = (0, 255, 256, -1, -1074)        # BININT1 ('K') up to 255, BININT ('J') beyond and below 0


def _shape(count, kind):
    """(n,), (n, 1) or a 2-D shape with a dimension above 255"""
    if kind == 0 or count == 1 and kind == 2:
        return (count,)
    if kind == 1:
        return (count, 1)
    for a in (2, 3):
        if count % a == 0:
            return (a, count // a)
    return (1, count)


def make(n2w, count, kind=None, seed=None):
    """-> (words uint32 [count, n2w], exps int32 [count], shape)"""
    rng = np.random.default_rng(1000 * n2w + count if seed is None else seed)
    w = rng.integers(0, 1 << 32, size=(count, n2w), dtype=np.uint64).astype(np.uint32)
    w[:, -1] &= 0x7FFFFFFF  # most values: top bit clear, LONG4 with nb = 4 n2w
    b = w.view(np.uint8)    # little-endian bytes of each row

    def short(i, nbytes, top):
        """row i: a value of nbytes bytes whose top byte is `top`"""
        if i < count:
            b[i, nbytes:] = 0
            if nbytes:
                b[i, nbytes - 1] = top
    # element 0 (the long header) takes another form per case; the rest are
    # spread behind it and around the batch boundaries
    first = (n2w // 64 + count) % 4
    if first == 0:
        short(0, 4 * n2w, 0x80)      # top bit set: the extra sign byte, LONG4 with nb = 4 n2w + 1
    elif first == 1:
        short(0, 0, 0)               # zero: '\x8a\x00'
    elif first == 2:
        short(0, 3, 0x7F)            # LONG1
    for base in (1, 997, 1996):
        short(base, 0, 0)
        short(base + 1, 4 * n2w, 0xFF)
        short(base + 2, 1, 0x01)
        short(base + 3, 254, 0x80)   # nb = 255: the longest LONG1
        short(base + 4, 255, 0x80)   # nb = 256: the shortest LONG4
        short(base + 5, 4 * n2w - 1, 0x80)
        short(base + 6, 17, 0x7F)
    exps = np.array([EXPS[(i + count) % 5] for i in range(count)], dtype=np.int32)
    return w, exps, _shape(count, (n2w // 64 + count) % 3 if kind is None else kind)


def cases():
    """(n2w, count) of every CPU case"""
    return [(n2w, count) for n2w in WIDTHS for count in COUNTS]


def scan(nat, data, n2w, window=None, cap=None):
    """xhe_wire_scan over `data`, whole or through windows of `window` bytes
    (each window a buffer of its own, as a staged chunk is) -> (return code,
    offsets in data, lengths, exponents, shape)"""
    L = nat.lib()
    buf = np.frombuffer(data, dtype=np.uint8)
    cap = len(data) // 16 + 1 if cap is None else cap
    off, ln, ex = np.zeros(cap, np.uint32), np.zeros(cap, np.uint16), np.zeros(cap, np.int32)
    shape, ndim = np.zeros(8, np.int64), ctypes.c_int()
    found, nxt = ctypes.c_int64(), ctypes.c_int64()
    pos = e0 = 0
    while True:
        n = len(data) - pos if window is None else min(window, len(data) - pos)
        last = pos + n == len(data)
        part = buf[pos:pos + n].copy()
        rc = L.xhe_wire_scan(part.ctypes.data, n, e0, int(last), n2w, off[e0:].ctypes.data, ln[e0:].ctypes.data,
                             ex[e0:].ctypes.data, cap - e0, ctypes.byref(found), ctypes.byref(nxt), shape.ctypes.data,
                             ctypes.byref(ndim))
        if rc != nat.XHE_OK:
            return rc, found.value, None, None, None
        m = found.value
        assert 0 <= nxt.value <= n and np.all(off[e0:e0 + m].astype(np.int64) + ln[e0:e0 + m] <= nxt.value)
        off[e0:e0 + m] += pos
        e0 += m
        if last:
            break
        assert nxt.value > 0, "a window without a whole element"
        pos += nxt.value
    return rc, off[:e0], ln[:e0], ex[:e0], tuple(int(s) for s in shape[:ndim.value])


def rows_of(data, off, ln, n2w):
    """the rows the index describes, by numpy slicing"""
    buf = np.frombuffer(data, dtype=np.uint8)
    out = np.zeros((len(off), 4 * n2w), dtype=np.uint8)
    for i, (o, k) in enumerate(zip(off.tolist(), ln.tolist())):
        out[i, :k] = buf[o:o + k]
    return out.view(np.uint32)
