"""Native wire codec for ciphertext arrays (xhe_wire_encode / xhe_wire_decode,
include/xhe.h): Paillier.serialize / ciphertext_from (paillier.py:244-271)
without a Python pickle round of one RawCiphertext object per element. The
bytes are a standard pickle of np.ndarray[object] of RawCiphertext, loadable
by XFL peers (numpy 1.x or 2.x); decoding accepts CPython's pickles of that
graph, including the reference's gmpy2 values. Host-only: no device needed.
"""
import ctypes
import os
import sys
import threading
import time

import numpy as np

from .. import _native as nat

_MAX_WORDS = 512  # n^2 of an 8192-bit key, the largest device key size (context.SUPPORTED_DEVICE_BITS)


def _vp(a):
    return ctypes.c_void_p(a.ctypes.data)


def encode(raws, exps, shape, n2w):
    """pickle bytes of the ndarray (shape) of RawCiphertext(raws[i], exps[i])."""
    ct = nat.ints_to_words(raws, n2w) if len(raws) else np.zeros((0, n2w), np.uint32)
    return encode_words(ct, exps, shape)


def encode_words(ct, exps, shape, compression=False):
    """pickle bytes of the ndarray (shape) of RawCiphertext from flat buffers:
    ct uint32 [count, n2w], exps int32 [count]. compression=True: what
    compat.compress makes of those bytes (paillier.py:244-258) - from
    compat.RAW_FRAME_MIN up the zstd raw-block frame, written in one pass
    (xhe_wire_encode_frame: no intermediate pickle buffer)."""
    ct = np.ascontiguousarray(ct, dtype=np.uint32)
    count, n2w = ct.shape
    if count == 0:
        ct = np.zeros((1, n2w), np.uint32)
    ex = np.ascontiguousarray(exps, dtype=np.int32) if count else np.zeros(1, np.int32)
    shp = np.ascontiguousarray(shape, dtype=np.int64) if len(shape) else np.zeros(1, np.int64)
    L = nat.lib()
    need = ctypes.c_int64()

    def enc(framed, out, cap):
        return L.xhe_wire_encode_frame(_vp(ct), _vp(ex), count, n2w, _vp(shp), len(shape), int(framed), out, cap,
                                       ctypes.byref(need))
    rc = enc(False, None, 0)
    if rc != nat.XHE_EOVERFLOW:
        nat.check(rc, "wire encode")
    from .. import compat
    framed = compression and need.value >= compat.RAW_FRAME_MIN
    if compression and not framed:  # small payloads: libzstd level 3, as before
        return compat.compress(encode_words(ct[:count], ex[:count], shape))
    if framed:
        rc = enc(True, None, 0)
        if rc != nat.XHE_EOVERFLOW:
            nat.check(rc, "wire encode")
    # written straight into the bytes object handed back (every byte of it),
    # from the process heap when large (nat.alloc_bytes)
    out = nat.alloc_bytes(need.value)
    nat.check(enc(framed, ctypes.cast(out, ctypes.c_void_p), need.value), "wire encode")
    return out


PIPE_MIN = 1 << 16    # device arrays from this many rows serialize through the pipeline below
PIPE_CHUNK = 1 << 17  # rows per D2H chunk (64 MB at 2048 bits)
# rows per encryption launch of a pipelined Paillier.encrypt (resident.encrypt_floats);
# $XHE_ENC_SUB overrides it (A/B measurement)
ENC_SUB = int(os.environ.get("XHE_ENC_SUB", 1 << 18))
_stage = {}           # (device, n2w) -> two pinned ([PIPE_CHUNK, n2w] words, [PIPE_CHUNK] bits), kept for the process
_copy_streams = {}    # device -> the pipelines' copy stream
# one pipeline at a time (serialize's or ciphertext_from's) uses the pinned
# buffers; _stage and _copy_streams get their entries only under it
_stage_lock = threading.Lock()
_TRACE = os.environ.get("XHE_PIPE_TRACE", "0") not in ("", "0")  # per-chunk timings on stderr
# $XHE_WIRE_DEV (read once): 0 keeps Paillier.ciphertext_from on the host
# decode (A/B runs against decode_device)
WIRE_DEV = os.environ.get("XHE_WIRE_DEV", "1").strip() != "0"
# payloads from this many elements decode on the device (decode_device)
DEV_DECODE_MIN = PIPE_MIN
DEV_CHUNK = 1 << 26   # payload bytes per H2D chunk of decode_device, at most (and what the pinned pair holds)
_STAGE_MIN_ROWS = 256  # the pinned pair's least size: a received chunk holds whole elements and their index


def _copy_stream(dev):
    """the copy stream of `dev` (call under _stage_lock)"""
    import torch
    s = _copy_streams.get(dev)
    if s is None:
        s = _copy_streams[dev] = torch.cuda.Stream(device=dev)
    return s


def _stage_pair(dev, n2w, rows):
    """the two pinned (words, bits) buffers of (dev, n2w), of at least `rows`
    rows (call under _stage_lock)"""
    import torch
    st = _stage.get((dev, n2w))
    if st is None or st[0][0].shape[0] < rows:
        st = _stage[(dev, n2w)] = [(torch.empty((rows, n2w), dtype=torch.int32, pin_memory=True),
                                    torch.empty(rows, dtype=torch.int16, pin_memory=True)) for _ in range(2)]
    return st


def encode_device(d, exps, shape, compression, dev):
    """encode_words of words held in HBM (an int32 tensor [count, n2w] on
    `dev`, written by kernels on the drop-in stream - e.g. an encryption that
    is still running), chunk by chunk: each chunk's D2H copy, on a copy
    stream, waits only for the encryption launches that write its rows (the
    readiness marks resident.encrypt_floats leaves on the tensor,
    `_xhe_ready`; else for everything queued so far) and lands in a pinned
    double buffer; the host lays the chunk out from the rows' own top words
    (xhe_wire_layout_part_rows: offsets from the previous chunk's end) and
    writes its rows (xhe_wire_rows) while the next chunk is encrypted and
    copied. The copy stream runs copies only - a kernel there would queue
    behind the encryption's blocks for CU slots. The payload is allocated at
    the size its elements could at most need (xhe_wire_begin) and cut to the
    real one at the end (finish, then an in-place shrink). The bytes equal
    encode_words(download(d), ...)."""
    import torch

    from .. import compat
    from . import resident
    count, n2w = int(d.shape[0]), int(d.shape[1])
    ex = np.ascontiguousarray(exps, dtype=np.int32).reshape(-1)
    shp = np.ascontiguousarray(shape, dtype=np.int64) if len(shape) else np.zeros(1, np.int64)
    L = nat.lib()
    off = np.empty(count + 1, dtype=np.int64)
    maxlen = ctypes.c_int64()
    # (count >= PIPE_MIN: the payload is above compat.RAW_FRAME_MIN, framed when compressed)
    framed = bool(compression)
    if count * 16 < compat.RAW_FRAME_MIN:
        raise ValueError("encode_device: below the pipeline's size (use encode_words)")
    nat.check(L.xhe_wire_begin(_vp(ex), count, n2w, _vp(shp), len(shape), int(framed), _vp(off),
                               ctypes.byref(maxlen), None, 0), "wire begin")
    out = nat.alloc_bytes(maxlen.value)
    optr = ctypes.c_void_p(ctypes.cast(out, ctypes.c_void_p).value)  # the address only (no reference)
    nat.check(L.xhe_wire_begin(_vp(ex), count, n2w, _vp(shp), len(shape), int(framed), _vp(off),
                               ctypes.byref(maxlen), optr, maxlen.value), "wire begin")
    marks = getattr(d, "_xhe_ready", None)
    if not marks or marks[-1][0] < count:
        with resident._On(dev):
            ev = torch.cuda.Event()
            ev.record(resident.stream(dev))
        marks = [(count, ev)]
    with _stage_lock:
        size = _pipeline(d, ex, count, n2w, dev, framed, off, maxlen, optr, marks)
    box = [out]
    del out  # the box holds the only reference: the cut is in place
    return nat.shrink_bytes(box, size)


def _pipeline(d, ex, count, n2w, dev, framed, off, maxlen, optr, marks):
    """encode_device's chunk loop (under _stage_lock: the pinned buffers are
    shared by every call); returns the payload's real size"""
    import torch
    L = nat.lib()
    st = _stage_pair(dev, n2w, min(PIPE_CHUNK, count))
    # the bit lengths the encryption computed behind each piece (else the host
    # reads them off the rows' top words)
    bits_d = getattr(d, "_xhe_bits", None)
    if bits_d is not None and bits_d.shape[0] != count:
        bits_d = None
    chunks = [(lo, min(count, lo + PIPE_CHUNK)) for lo in range(0, count, PIPE_CHUNK)]
    cs = _copy_stream(dev)
    evs = [None, None]
    waited = [0]  # marks the copy stream already waits for

    def issue(k):
        lo, hi = chunks[k]
        with torch.cuda.device(dev), torch.cuda.stream(cs):
            # every launch up to the one that writes row hi - 1 (launches on
            # two streams may finish out of order)
            while waited[0] < len(marks) and (waited[0] == 0 or marks[waited[0] - 1][0] < hi):
                cs.wait_event(marks[waited[0]][1])
                waited[0] += 1
            st[k % 2][0][:hi - lo].copy_(d[lo:hi], non_blocking=True)
            if bits_d is not None:
                st[k % 2][1][:hi - lo].copy_(bits_d[lo:hi], non_blocking=True)
            evs[k % 2] = torch.cuda.Event()
            evs[k % 2].record(cs)
    trace = _TRACE and []
    t0 = time.perf_counter()
    try:
        issue(0)
        for k, (lo, hi) in enumerate(chunks):
            if k + 1 < len(chunks):
                issue(k + 1)  # its buffer held chunk k - 1, written in the previous iteration
            evs[k % 2].synchronize()
            t1 = time.perf_counter()
            rp = ctypes.c_void_p(st[k % 2][0].data_ptr())
            if bits_d is not None:
                nat.check(L.xhe_wire_layout_part(ctypes.c_void_p(st[k % 2][1].data_ptr()), _vp(ex), lo, hi, count,
                                                 n2w, _vp(off)), "wire layout")
            else:
                nat.check(L.xhe_wire_layout_part_rows(rp, _vp(ex), lo, hi, count, n2w, _vp(off)), "wire layout")
            t2 = time.perf_counter()
            nat.check(L.xhe_wire_rows(rp, _vp(ex), lo, hi, count, n2w, _vp(off), int(framed), optr, maxlen.value),
                      "wire rows")
            if trace is not False:
                t3 = time.perf_counter()
                trace.append((k, round((t1 - t0) * 1e3, 2), round((t2 - t1) * 1e3, 2), round((t3 - t2) * 1e3, 2)))
        if trace:
            print("pipeline (chunk, ready_ms, layout_ms, rows_ms):", trace, file=sys.stderr, flush=True)
    finally:
        cs.synchronize()  # no copy still landing in the shared pinned buffers (an error mid-way)
    size = ctypes.c_int64()
    nat.check(L.xhe_wire_finish(count, _vp(off), int(framed), optr, maxlen.value, ctypes.byref(size)), "wire finish")
    return size.value


class _Source:
    """The content bytes of a received payload: the bytes themselves, or the
    content of a closed-form raw-block zstd frame (compat.raw_frame_size),
    read range by range straight out of the frame."""

    def __init__(self, data, content=None):
        self.data = data
        self.framed = content is not None
        self.size = len(data) if content is None else int(content)

    def read(self, lo, hi, dst):
        """content bytes [lo, hi) -> the memory at address dst; False when the
        frame is not what its probe saw"""
        L = nat.lib()
        if self.framed:
            return L.xhe_zstd_raw_extract_range(self.data, len(self.data), lo, hi, ctypes.c_void_p(dst)) == nat.XHE_OK
        src = ctypes.cast(self.data, ctypes.c_void_p).value + lo  # (the address only: data outlives the call)
        return L.xhe_host_memcpy(ctypes.c_void_p(dst), ctypes.c_void_p(src), hi - lo) == nat.XHE_OK


def peek_shape(src, n2w):
    """the shape in the header of a payload in the library's own layout
    (xhe_wire_scan of its first bytes), or None for any other payload"""
    n = min(src.size, 512)  # the header with eight 8-byte dimensions is below 200 bytes
    if n < 2:
        return None
    head = np.empty(n, dtype=np.uint8)
    if not src.read(0, n, head.ctypes.data):
        return None
    found, nxt, ndim = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int()
    shape = np.zeros(8, dtype=np.int64)
    rc = nat.lib().xhe_wire_scan(_vp(head), n, 0, int(n == src.size), n2w, None, None, None, 0, ctypes.byref(found),
                                 ctypes.byref(nxt), _vp(shape), ctypes.byref(ndim))
    if rc not in (nat.XHE_OK, nat.XHE_EOVERFLOW):
        return None
    return tuple(int(s) for s in shape[:ndim.value])


def decode_device(src, n2w, dev, shape):
    """decode_words of a payload in the library's own layout, into HBM: ->
    (int32 tensor [count, n2w] on `dev`, int32 exponents, shape), or None when
    the bytes are not that layout after all (a foreign, truncated or corrupt
    payload: the caller decodes on the host, which accepts or rejects it).
    `src` is a _Source, `shape` its peek_shape. The mirror image of
    encode_device, chunk by chunk: host threads copy (or de-frame) the chunk's
    bytes into a pinned buffer; the host scans it for whole elements
    (xhe_wire_scan: value offsets, lengths, exponents - no words are copied);
    bytes and index go up in one copy on the copy stream; xhe_wire_unpack, on
    the drop-in stream behind that copy's event, writes those elements' rows
    of the result. The next chunk starts at the first incomplete element. The
    [count, n2w] words never exist on the host. Returns when the host work is
    done: the last launch may still be queued, as with every resident result."""
    count = 1
    for s in shape:
        count *= s
    # an element is 16 bytes at least: a header that promises more is not worth a tensor
    if count < 1 or min(shape) < 0 or count * 16 > src.size or n2w % 4 or n2w > _MAX_WORDS:
        return None
    with _stage_lock:
        return _recv_pipeline(src, n2w, dev, shape, count)


def _recv_pipeline(src, n2w, dev, shape, count):
    """decode_device's chunk loop (under _stage_lock). A pinned buffer and its
    device twin hold [offsets: 4 cap][lengths: 2 cap][chunk bytes]."""
    import torch

    from . import resident
    L = nat.lib()
    st = _stage_pair(dev, n2w, max(min(PIPE_CHUNK, count), _STAGE_MIN_ROWS))
    pins = [s[0].view(torch.uint8).reshape(-1) for s in st]
    hosts = [p.numpy() for p in pins]
    cap = min(int(st[0][0].shape[0]), count)        # elements one chunk may hold
    o_len = 4 * cap
    o_bytes = (6 * cap + 15) & ~15
    chunk = min(DEV_CHUNK, int(pins[0].shape[0]) - o_bytes, src.size + 15) & ~15
    exps = np.empty(count, dtype=np.int32)
    cs = _copy_stream(dev)
    main = resident.stream(dev)
    with resident._On(dev):
        d = torch.empty((count, n2w), dtype=torch.int32, device=f"cuda:{dev}")
        twins = [torch.empty(o_bytes + chunk, dtype=torch.uint8, device=f"cuda:{dev}") for _ in range(2)]
        # the twins' blocks may come from tensors freed with kernels still queued
        # on the drop-in stream: the copy stream starts behind those
        ready = torch.cuda.Event()
        ready.record(main)
        cs.wait_event(ready)
    copied, unpacked = [None, None], [None, None]
    found, nxt, ndim = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int()
    shp = np.zeros(8, dtype=np.int64)
    trace = _TRACE and []
    pos = e0 = k = 0
    ok = False
    try:
        while True:
            b = k % 2
            t0 = time.perf_counter()
            if copied[b] is not None:
                copied[b].synchronize()  # chunk k - 2 has left the pinned buffer
            t1 = time.perf_counter()
            n = min(chunk, src.size - pos)
            last = pos + n == src.size
            base = hosts[b].ctypes.data
            if not src.read(pos, pos + n, base + o_bytes):
                break
            t2 = time.perf_counter()
            want = min(cap, count - e0)
            rc = L.xhe_wire_scan(ctypes.c_void_p(base + o_bytes), n, e0, int(last), n2w, ctypes.c_void_p(base),
                                 ctypes.c_void_p(base + o_len), ctypes.c_void_p(exps.ctypes.data + 4 * e0), want,
                                 ctypes.byref(found), ctypes.byref(nxt), _vp(shp), ctypes.byref(ndim))
            # a deviation, more elements than the header's shape (or the index)
            # holds, or an element that no chunk holds whole
            if rc != nat.XHE_OK or (not last and nxt.value == 0):
                break
            t3 = time.perf_counter()
            m = found.value
            if m:
                with torch.cuda.device(dev):
                    with torch.cuda.stream(cs):
                        if unpacked[b] is not None:
                            cs.wait_event(unpacked[b])  # chunk k - 2's kernel has read the twin
                        twins[b][:o_bytes + n].copy_(pins[b][:o_bytes + n], non_blocking=True)
                        copied[b] = torch.cuda.Event()
                        copied[b].record(cs)
                    main.wait_event(copied[b])
                    tw = twins[b].data_ptr()
                    nat.check(L.xhe_wire_unpack(ctypes.c_void_p(tw + o_bytes), n, ctypes.c_void_p(tw),
                                                ctypes.c_void_p(tw + o_len), m, n2w,
                                                ctypes.c_void_p(d.data_ptr() + 4 * n2w * e0),
                                                ctypes.c_void_p(main.cuda_stream)), "wire unpack")
                    unpacked[b] = torch.cuda.Event()
                    unpacked[b].record(main)
            if trace is not False:
                t4 = time.perf_counter()
                trace.append((k, m, *(round((y - x) * 1e3, 2) for x, y in ((t0, t1), (t1, t2), (t2, t3), (t3, t4)))))
            e0 += m
            pos += nxt.value
            if last:
                ok = e0 == count
                break
            k += 1
        if trace:
            print("recv pipeline (chunk, elements, ready_ms, stage_ms, scan_ms, issue_ms):", trace, file=sys.stderr,
                  flush=True)
    finally:
        cs.synchronize()  # no copy still reads the shared pinned buffers
    if not ok:
        return None  # (the partial tensor goes back to the allocator on its own stream)
    return d, exps, tuple(shape)


def decode(data, n2w=None):
    """(raw ints, exponents, shape) of a ciphertext-array pickle; raises
    ValueError when the bytes are not that format."""
    ct, ex, shape = _decode(data, n2w or _MAX_WORDS)
    return (nat.words_to_ints(ct) if ct.shape[0] else []), ex, shape


# word widths tried for a payload decoded without a context: n^2 of the
# device key sizes (context.SUPPORTED_DEVICE_BITS), narrowest first
_WIDTHS = (128, 192, 256, 512)


def decode_words(data, n2w=None):
    """(uint32 words [count, n2w], int32 exponents, shape) of a
    ciphertext-array pickle. Without n2w the narrowest device width that
    holds every value is used. Raises ValueError when the bytes are not that
    format."""
    if n2w is not None:
        return _decode(data, n2w)
    err = None
    for w in _WIDTHS:
        try:
            return _decode(data, w)
        except ValueError as e:  # "value too large" -> next width; anything else is final
            err = e
            if "too large" not in str(e):
                raise
    raise err


def _decode(data, n2w):
    L = nat.lib()
    buf = np.frombuffer(data, dtype=np.uint8)
    count = ctypes.c_int64()
    ndim = ctypes.c_int()
    shape = np.zeros(8, dtype=np.int64)
    cap = max(1, len(data) // (4 * n2w) + 16)
    for _ in range(2):
        ct = nat.empty((cap, n2w), np.uint32)
        ex = np.empty(cap, dtype=np.int32)
        rc = L.xhe_wire_decode(_vp(buf), len(data), n2w, _vp(ct), _vp(ex), cap, ctypes.byref(count), _vp(shape),
                               ctypes.byref(ndim))
        if rc != nat.XHE_EOVERFLOW:
            break
        cap = count.value
    if rc != nat.XHE_OK:
        raise ValueError(nat.lib().xhe_last_error().decode(errors="replace"))
    n = count.value
    return ct[:n], ex[:n], tuple(int(s) for s in shape[:ndim.value])
