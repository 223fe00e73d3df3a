"""Device-resident ciphertext storage and the device-buffer forms of the
drop-in's batched operations.

The reference passes one np.ndarray[object] from call to call -
Paillier.encrypt -> + / * / np.matmul -> Paillier.serialize / decrypt
(paillier.py:88-187, 244-258, 289-339, 370-417). Here a PaillierArray keeps
its words where the last operation left them: `Rows` holds the [count, n2w]
uint32 words in HBM, in host memory, or both (identical when both). Results
of device operations stay in HBM; the host copy is made on first host access
(element reads, serialize, pickling, numpy fallbacks) and kept next to the
device copy. Chained calls therefore move only what they must: exponents and
scalars up (4-8 B per element), decrypted floats down (4 B per element).

Device buffers are torch tensors (int32 views of the words) on the context's
own GPU, allocated and used on one stream per device (`stream()`), so the
caching allocator's reuse is ordered with the kernels that read them; every
kernel goes through the C ABI's device-pointer entry points (include/xhe.h).
A context sharded over several GPUs (num_cores > 1, $XHE_DEVICES) stays in
host-buffer mode; so does everything when $XHE_RESIDENT=0 or torch sees no
GPU (the CPU test suite).
"""
import ctypes
import os
import threading

import numpy as np

from .. import _native as nat

_streams = {}
_aux_streams = {}
_lock = threading.Lock()
_cuda_ok = None


def _torch():
    import torch
    return torch


def available():
    global _cuda_ok
    if _cuda_ok is None:
        try:
            _cuda_ok = bool(_torch().cuda.is_available())
        except Exception:  # noqa: BLE001
            _cuda_ok = False
    return _cuda_ok


# Share of the device's spare HBM (free + torch's cached blocks, less the
# context's WIN_MARGIN table headroom) one new resident result may take;
# larger batches stream through the host pipeline instead (xhe_*_host).
RESIDENT_SHARE = 0.5
# Batches up to this size skip the HBM query (torch's allocator statistics
# cost ~0.1 ms per call, a visible share of a 64-element LR batch); the
# context's WIN_MARGIN headroom covers them.
RESIDENT_QUERY_MIN = 64 << 20


def resident_budget(ctx, dev):
    """Bytes a new resident batch may occupy on `dev` ($XHE_RESIDENT_MAX_BYTES
    overrides; None = unknown, no cap)."""
    pin = os.environ.get("XHE_RESIDENT_MAX_BYTES", "").strip()
    if pin:
        return int(pin)
    from .._native import device_free_bytes
    free = device_free_bytes(dev)
    if free is None:
        return None
    torch = _torch()
    try:
        free += int(torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev))
    except Exception:  # noqa: BLE001
        pass
    return int(max(0, free - getattr(ctx, "WIN_MARGIN", 0)) * RESIDENT_SHARE)


def device_for(ctx, num_cores=-1, count=0, elem_bytes=0):
    """The GPU whose HBM holds this context's arrays, or None (host-buffer
    mode: sharded contexts, $XHE_RESIDENT=0, no GPU, or a new batch of
    `count` results of `elem_bytes` each - ciphertext words, exponent and
    the plaintext staged for it - above resident_budget())."""
    if ctx is None or os.environ.get("XHE_RESIDENT", "1").strip() == "0" or not available():
        return None
    devs = ctx.shard_devices(num_cores)
    if len(devs) != 1:
        return None
    nbytes = count * elem_bytes
    if nbytes and (nbytes > RESIDENT_QUERY_MIN or os.environ.get("XHE_RESIDENT_MAX_BYTES", "").strip()):
        cap = resident_budget(ctx, devs[0])
        if cap is not None and count * elem_bytes > cap:
            return None
    return devs[0]


def stream(dev):
    """The drop-in's stream on `dev` (one per device and process)."""
    s = _streams.get(dev)
    if s is None:
        with _lock:
            s = _streams.get(dev)
            if s is None:
                torch = _torch()
                s = _streams[dev] = torch.cuda.Stream(device=dev)
    return s


def aux_stream(dev):
    """A second stream on `dev` for launches that may overlap the drop-in
    stream's (encrypt_floats); work on it is joined back into the drop-in
    stream before the caller sees the result."""
    s = _aux_streams.get(dev)
    if s is None:
        with _lock:
            s = _aux_streams.get(dev)
            if s is None:
                torch = _torch()
                s = _aux_streams[dev] = torch.cuda.Stream(device=dev)
    return s


class _On:
    """with _On(dev): allocations and copies on the drop-in stream of dev"""

    def __init__(self, dev):
        torch = _torch()
        self.ctx = [torch.cuda.device(dev), torch.cuda.stream(stream(dev))]

    def __enter__(self):
        for c in self.ctx:
            c.__enter__()
        return self

    def __exit__(self, *a):
        for c in reversed(self.ctx):
            c.__exit__(*a)


def _sp(dev):
    return ctypes.c_void_p(stream(dev).cuda_stream)


def _dp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def empty(dev, shape, dtype=None):
    torch = _torch()
    with _On(dev):
        return torch.empty(shape, dtype=dtype or torch.int32, device=f"cuda:{dev}")


def upload(a, dev):
    """host array -> device tensor (same bytes; uint32 travels as int32)"""
    torch = _torch()
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    elif a.dtype == np.uint64:
        a = a.view(np.int64)
    with _On(dev):
        return torch.from_numpy(a).to(f"cuda:{dev}", non_blocking=False)


def upload_async(a, dev):
    """upload() without waiting: the bytes go through a pinned copy (torch's
    caching host allocator keeps it until the copy has run) and the copy is
    ordered on the drop-in stream of dev. For operands only the library's
    kernels on that stream read (indices, exponents); a blocking upload
    would wait for every kernel queued before it."""
    torch = _torch()
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    elif a.dtype == np.uint64:
        a = a.view(np.int64)
    with _On(dev):
        return torch.from_numpy(a).pin_memory().to(f"cuda:{dev}", non_blocking=True)


def upload_small(a, dev, limit=1 << 20):
    """upload_async for operands up to `limit` bytes (the host does not wait
    for the kernels queued before the copy - in the LR step's mat-vec two
    blocking uploads each waited for the inversion kernels ahead of them),
    upload() for larger ones (a pinned staging copy of a big array costs more
    than it saves)"""
    a = np.ascontiguousarray(a)
    return upload_async(a, dev) if a.nbytes <= limit else upload(a, dev)


def download(t, dtype=np.uint32):
    """device tensor -> host array of `dtype` (big buffers come from the
    recycled host mappings, xfl_amd._native.empty)"""
    torch = _torch()
    dt = np.dtype(dtype)
    out = nat.empty(tuple(t.shape), dt)
    if out.size:
        view = out.view({4: np.int32, 8: np.int64, 2: np.int16, 1: np.int8}[dt.itemsize]) if dt.kind == "u" else out
        with _On(t.device.index):
            torch.from_numpy(view).copy_(t)
            stream(t.device.index).synchronize()
    return out


class Rows:
    """Word storage shared by a PaillierArray and its views: [count, n2w]
    uint32 in host memory (`h`), in HBM (`d`, int32 tensor), or both."""
    __slots__ = ("h", "d", "__weakref__")

    def __init__(self, h=None, d=None):
        self.h = h
        self.d = d

    @property
    def count(self):
        return (self.h if self.h is not None else self.d).shape[0]

    @property
    def n2w(self):
        return (self.h if self.h is not None else self.d).shape[1]

    def host(self):
        if self.h is None:
            self.h = download(self.d)
        return self.h

    def device(self, dev):
        """the whole buffer in HBM of `dev` (uploaded once, then kept)"""
        if self.d is None or self.d.device.index != dev:
            self.d = upload(self.h if self.h is not None else self.host(), dev)
        return self.d

    def on_device(self, dev):
        return self.d is not None and self.d.device.index == dev

    def host_written(self):
        """the host copy was changed in place: the device copy is stale"""
        self.d = None


# ------------------------------------------------------------ device operations
def _seed():
    from .ops import _seed as s
    return s()


# ------------------------------------------------------------ obfuscator pool
class _DeviceObfOps:
    """What an ObfPool does to its rows on a GPU: all of it queued on the
    drop-in stream of `dev`, so stream order puts a fill before every use of
    its rows and a use before the next fill."""

    def __init__(self, dev):
        self.dev = dev

    def alloc(self, cap, n2w):
        torch = _torch()
        with _On(self.dev):
            return torch.zeros((cap, n2w), dtype=torch.int32, device=f"cuda:{self.dev}")

    def fill(self, dk, rows):
        """rows <- fresh obfuscators, drawn as _encrypt_pipeline draws: a new
        seed per chunk, xhe_rand, then the encryption kernels on m = 0"""
        torch = _torch()
        L = nat.lib()
        n = rows.shape[0]
        c = max(1, min(n, CHUNK))
        with _On(self.dev):
            rnd = torch.empty((c, dk.rand_words), dtype=torch.int32, device=f"cuda:{self.dev}")
        s = _sp(self.dev)
        for lo in range(0, n, c):
            k = min(c, n - lo)
            seed, nonce = _seed()
            nat.check(L.xhe_rand(dk.handle, seed, nonce, k, _dp(rnd), None, s), "rand")
            nat.check(L.xhe_obf_fill(dk.handle, _dp(rnd), k, _dp(rows[lo:]), s), "obf_fill")

    def zero(self, rows):
        with _On(self.dev):
            rows.zero_()

    def copy(self, dst, src):
        with _On(self.dev):
            dst.copy_(src)


class ObfPool:
    """Obfuscators made ahead of time for one device key: a ring of [cap, n2w]
    int32 rows, `available` of them filled starting at row `head`. Every row
    is handed out once: take() moves the head past the rows it returns before
    anything is launched on them, and the kernels that use a row zero it
    (xhe_encrypt_obf's wipe; obfuscate() zeroes its rows after the product).
    The bookkeeping and the queuing of fills and uses happen under one lock:
    a refill cannot be queued between the hand-out of rows and the launch
    that reads them. `ops` (alloc, fill, zero, copy) stands in for the device
    in the host tests."""

    def __init__(self, dev, n2w, ops=None):
        self.dev = dev
        self.n2w = n2w
        self.ops = ops if ops is not None else _DeviceObfOps(dev)
        self.lock = threading.RLock()
        self.rows = None
        self.cap = 0
        self.head = 0
        self.available = 0

    def _spans(self, start, k):
        """the k rows from `start` on as one view, or two at the wrap"""
        first = min(k, self.cap - start)
        return [self.rows[start:start + first]] + ([self.rows[0:k - first]] if k > first else [])

    def reserve(self, dk, count, max_rows=None):
        """fill rows until min(count, max_rows) are available (the ring grows
        when it is smaller; the rows it holds move over) -> rows available"""
        want = int(count) if max_rows is None else min(int(count), int(max_rows))
        with self.lock:
            if want > self.cap:
                new = self.ops.alloc(want, self.n2w)
                if self.rows is not None:
                    off = 0
                    for v in self._spans(self.head, self.available) if self.available else []:
                        self.ops.copy(new[off:off + v.shape[0]], v)
                        off += v.shape[0]
                    self.ops.zero(self.rows)
                self.rows, self.cap, self.head = new, want, 0
            need = want - self.available
            if need > 0:
                for v in self._spans((self.head + self.available) % self.cap, need):
                    self.ops.fill(dk, v)
                self.available += need  # counted once every fill is queued
            return self.available

    def take(self, k):
        """the next min(k, available) rows -> list of views (none, one, or two
        at the wrap). The head has moved past them on return. A caller that
        launches on them holds `lock` from here until the launch is queued
        (consume does)."""
        with self.lock:
            k = min(int(k), self.available)
            if k <= 0:
                return []
            views = self._spans(self.head, k)
            self.head = (self.head + k) % self.cap
            self.available -= k
            return views

    def consume(self, k, launch):
        """take(k), then launch(view, offset) per view (offset: rows handed
        out before it) -> rows served. The rows are gone from the pool even
        when launch raises."""
        with self.lock:
            off = 0
            for v in self.take(k):
                launch(v, off)
                off += v.shape[0]
            return off

    def drop(self):
        """zero the storage and free it"""
        with self.lock:
            if self.rows is not None:
                self.ops.zero(self.rows)
            self.rows, self.cap, self.head, self.available = None, 0, 0, 0


def obf_pool(dk):
    """the pool of obfuscators reserved for the device key dk (None: none)"""
    return getattr(dk, "obf_pool", None)


def obf_pool_rows(ctx, dk, count):
    """`count` clipped to the rows resident_budget() leaves a pool on dk's device"""
    cap = resident_budget(ctx, dk.device)
    return int(count) if cap is None else min(int(count), cap // (4 * dk.n2w))


_OBF_AUTO = None


def obf_auto():
    """$XHE_OBF_POOL=N (read once): a resident Paillier.encrypt / obfuscate
    tops the pool up to N after its own work is queued"""
    global _OBF_AUTO
    if _OBF_AUTO is None:
        v = os.environ.get("XHE_OBF_POOL", "").strip()
        _OBF_AUTO = int(v) if v.isdigit() else 0
    return _OBF_AUTO


def obf_top_up(ctx, dk):
    """the refill behind a resident call ($XHE_OBF_POOL; nothing when unset)"""
    n = obf_auto()
    if n > 0 and ctx is not None:
        ctx.reserve_obfuscators(n, dk.device)


def _encrypt_obf(dk, m, pool, k, ct):
    """ct[:s] = (1 + n m[:s]) X on the next s = min(k, pool rows) obfuscators
    X, wiped by the same launch, on the drop-in stream -> s"""
    L = nat.lib()
    s = _sp(dk.device)

    def launch(rows, off):
        nat.check(L.xhe_encrypt_obf(dk.handle, _dp(m[off:]), _dp(rows), rows.shape[0], 1, _dp(ct[off:]), s),
                  "encrypt_obf")
    return pool.consume(k, launch)


ENC_STREAMS = int(os.environ.get("XHE_ENC_STREAMS", 2))  # streams the pieces of a pipelined encryption alternate on
CHUNK = 1 << 20  # elements per encode/draw/encrypt pass: bounds the m + draw temporaries (~400 MB at 2048 bits)


def encrypt_floats(dk, x, precision, max_exponent, obfuscation):
    """encode + ChaCha20 draws + encrypt of float64 values (paillier.py:273-339)
    -> (device ct [n, n2w], exponents, status), exponents and status on the
    host (they decide the reference's exceptions)."""
    dev = dk.device
    L = nat.lib()
    xd = upload(np.ascontiguousarray(x, dtype=np.float64), dev)
    prec = -1 if precision is None else int(precision)
    has_max = max_exponent is not None

    def encode(lo, k, m, es):
        nat.check(L.xhe_encode_f64(dk.handle, _dp(xd[lo:]), k, prec, int(has_max),
                                   int(max_exponent) if has_max else 0, _dp(m), _dp(es[0, lo:]), _dp(es[1, lo:]),
                                   _sp(dev)), "encrypt")
    return _encrypt_pipeline(dk, x.shape[0], encode, obfuscation)


def encrypt_packed(dk, cols, ib, precision, obfuscation):
    """embed's float64 columns [k, n] -> (device ct [n, n2w], status): packed
    and reduced mod n on the device (xhe_embed_f64), then the draws and the
    encryption as encrypt_floats; every exponent is 0. A nonzero status (4: a
    value does not fit its slot) sends the caller to the host path."""
    dev = dk.device
    L = nat.lib()
    ncols, n = cols.shape

    def encode(lo, k, m, es):
        cd = upload(cols if k == n else cols[:, lo:lo + k], dev)  # the pass's columns, contiguous
        nat.check(L.xhe_embed_f64(dk.handle, _dp(cd), ncols, k, int(ib), int(precision), _dp(m), _dp(es[1, lo:]),
                                  _sp(dev)), "embed")
    ct, _, st = _encrypt_pipeline(dk, n, encode, obfuscation)
    return ct, st


def _encrypt_pipeline(dk, n, encode, obfuscation):
    """The encryption of n values behind an encoder: encode(lo, k, m, es)
    queues the encoding of elements [lo, lo + k) on the drop-in stream - their
    m words into m, exponents into es[0, lo:] (may be left unwritten: the
    caller then ignores them) and statuses into es[1, lo:] -> (device ct,
    exponents, status)."""
    torch = _torch()
    dev = dk.device
    L = nat.lib()
    c = max(1, min(n, CHUNK))
    from . import wire
    # large arrays: the encryption in launches of wire.ENC_SUB rows, each
    # marked by an event on the result tensor, so that a serialize of it copies
    # and encodes the first rows while the later ones encrypt
    # (wire.encode_device); the launches alternate between the drop-in stream
    # and a second one, so each launch's tail overlaps the next one's start
    # (in one stream the four launches of 1 M elements cost 12 % of the rate)
    sub = wire.ENC_SUB if n >= wire.PIPE_MIN else c
    with _On(dev):
        ct = torch.empty((n, dk.n2w), dtype=torch.int32, device=f"cuda:{dev}")
        es = torch.empty((2, n), dtype=torch.int32, device=f"cuda:{dev}")
        m = torch.empty((c, dk.nw), dtype=torch.int32, device=f"cuda:{dev}")
        bits = torch.empty(n, dtype=torch.int16, device=f"cuda:{dev}") if n >= wire.PIPE_MIN else None
        rnds = [torch.empty((min(sub, c), dk.rand_words), dtype=torch.int32, device=f"cuda:{dev}")
                for _ in range(2 if sub < c and ENC_STREAMS > 1 else 1)] if obfuscation else [None, None]
    main = stream(dev)
    streams = [main, aux_stream(dev)] if sub < c and ENC_STREAMS > 1 else [main]
    # Reserved obfuscators (ObfPool) serve the leading elements of a piece in
    # one xhe_encrypt_obf launch on the drop-in stream; what the pool cannot
    # cover is drawn and encrypted as without a pool. Only in a one-pass call,
    # where the statuses are back before anything is encrypted: a bad input
    # raises with the pool untouched.
    pool = obf_pool(dk) if obfuscation and n <= c else None
    direct = False  # some piece went through xhe_rand + xhe_encrypt
    es_h = None
    marks = []
    j = 0
    for lo in range(0, n, c):
        k = min(c, n - lo)
        encode(lo, k, m, es)
        if n <= c:
            # one pass: the exponents and statuses come back as soon as the
            # encoder has run (a bad input raises before any encryption is
            # queued, as the reference raises in encode), and the encryption
            # kernels are left running - the caller's next step (serialize's
            # D2H, another operation) is ordered after them on this stream
            es_h = download(es, np.int32)
            if np.any(es_h[1] != 0):
                return ct, es_h[0].copy(), es_h[1].copy()
        with _On(dev):
            encoded = torch.cuda.Event()
            encoded.record(main)
            for st in streams[1:]:
                st.wait_event(encoded)
        for so in range(0, k, sub):
            ks = min(sub, k - so)
            st = streams[j % len(streams)]
            rnd = rnds[j % len(rnds)] if obfuscation else None
            sp = ctypes.c_void_p(st.cuda_stream)
            served = 0
            if pool is not None and pool.available:
                served = _encrypt_obf(dk, m[so:], pool, ks, ct[lo + so:])
                if served and bits is not None:
                    nat.check(L.xhe_row_bits(_dp(ct[lo + so:]), served, dk.n2w, _dp(bits[lo + so:]), _sp(dev)),
                              "row bits")
                if 0 < served < ks and st is not main:  # the piece's mark (on st) covers its pooled rows too
                    with _On(dev):
                        ev = torch.cuda.Event()
                        ev.record(main)
                        st.wait_event(ev)
            if served < ks:
                direct = True
                a, kr = so + served, ks - served
                if obfuscation:
                    seed, nonce = _seed()
                    nat.check(L.xhe_rand(dk.handle, seed, nonce, kr, _dp(rnd), None, sp), "rand")
                nat.check(L.xhe_encrypt(dk.handle, _dp(m[a:]), _dp(rnd), kr, _dp(ct[lo + a:]), sp), "encrypt")
                if bits is not None:  # the piece's bit lengths for the serializer's layout, behind the piece
                    nat.check(L.xhe_row_bits(_dp(ct[lo + a:]), kr, dk.n2w, _dp(bits[lo + a:]), sp), "row bits")
            if sub < c:
                with _On(dev):
                    ev = torch.cuda.Event()
                    ev.record(st if served < ks else main)
                marks.append((lo + so + ks, ev))
            j += 1
        with _On(dev):  # the next pass's encode (and everything after) waits for both streams
            for st in streams[1:]:
                done = torch.cuda.Event()
                done.record(st)
                main.wait_event(done)
    if marks and direct:  # (a call the pool served whole ran on the drop-in stream alone)
        ct._xhe_ready = marks
    if bits is not None:
        ct._xhe_bits = bits
    if es_h is None:
        es_h = download(es, np.int32)
    return ct, es_h[0].copy(), es_h[1].copy()


def encrypt_encoded(dk, mw, obfuscation):
    """encrypt encoded integers (host words [n, nw]) -> device ct"""
    return encrypt_encoded_dev(dk, upload(np.ascontiguousarray(mw, dtype=np.uint32), dk.device), obfuscation)


def obfuscate(dk, c):
    """c * (fresh encryption of 0) for device ct (paillier.py:189-232)"""
    torch = _torch()
    dev = dk.device
    n = c.shape[0]
    pool = obf_pool(dk)
    served, out = 0, None
    if pool is not None and pool.available:
        # reserved obfuscators are the fresh encryptions of 0 themselves: the
        # product straight on the pool's rows, zeroed behind it
        L = nat.lib()
        with _On(dev):
            out = torch.empty((n, dk.n2w), dtype=torch.int32, device=f"cuda:{dev}")

        def launch(rows, off):
            nat.check(L.xhe_mulmod(dk.handle, _dp(c[off:]), None, _dp(rows), None, rows.shape[0], 0, _dp(out[off:]),
                                   None, _sp(dev)), "add")
            pool.ops.zero(rows)
        served = pool.consume(n, launch)
        if served == n:
            return out
    with _On(dev):
        zero = torch.zeros((n - served, dk.nw), dtype=torch.int32, device=f"cuda:{dev}")
    x = encrypt_encoded_dev(dk, zero, True)
    if not served:
        return mulmod(dk, c, None, x, None, 0)
    nat.check(nat.lib().xhe_mulmod(dk.handle, _dp(c[served:]), None, _dp(x), None, n - served, 0, _dp(out[served:]),
                                   None, _sp(dev)), "add")
    return out


def encrypt_encoded_dev(dk, md, obfuscation):
    """encrypt device m words [n, nw] -> device ct (fresh draws per chunk)"""
    torch = _torch()
    dev = dk.device
    L = nat.lib()
    n = md.shape[0]
    c = max(1, min(n, CHUNK))
    with _On(dev):
        ct = torch.empty((n, dk.n2w), dtype=torch.int32, device=f"cuda:{dev}")
        rnd = torch.empty((c, dk.rand_words), dtype=torch.int32, device=f"cuda:{dev}") if obfuscation else None
    s = _sp(dev)
    pool = obf_pool(dk) if obfuscation else None
    for lo in range(0, n, c):
        k = min(c, n - lo)
        if pool is not None and pool.available:  # the chunk's leading elements on reserved obfuscators
            served = _encrypt_obf(dk, md[lo:], pool, k, ct[lo:])
            lo, k = lo + served, k - served
            if k == 0:
                continue
        if obfuscation:
            seed, nonce = _seed()
            nat.check(L.xhe_rand(dk.handle, seed, nonce, k, _dp(rnd), None, s), "rand")
        nat.check(L.xhe_encrypt(dk.handle, _dp(md[lo:]), _dp(rnd), k, _dp(ct[lo:]), s), "encrypt")
    return ct


def decrypt(dk, c):
    """device ct -> host m words [n, nw] (paillier.py:347-365)"""
    torch = _torch()
    dev = dk.device
    with _On(dev):
        m = torch.empty((c.shape[0], dk.nw), dtype=torch.int32, device=f"cuda:{dev}")
    nat.check(nat.lib().xhe_decrypt(dk.handle, _dp(c), c.shape[0], _dp(m), _sp(dev)), "decrypt")
    return download(m)


def decrypt_decode(dk, c, exps):
    """device ct + host exponents -> host (f64, f32, status): decrypt, decode
    and the float32 cast on the device (paillier.py:370-398, encoder.py:56-64);
    only 16 B per element come back."""
    torch = _torch()
    dev = dk.device
    L = nat.lib()
    n = c.shape[0]
    ed = upload_small(np.ascontiguousarray(exps, dtype=np.int32), dev)
    with _On(dev):
        m = torch.empty((n, dk.nw), dtype=torch.int32, device=f"cuda:{dev}")
        f64 = torch.empty(n, dtype=torch.float64, device=f"cuda:{dev}")
        f32 = torch.empty(n, dtype=torch.float32, device=f"cuda:{dev}")
        st = torch.empty(n, dtype=torch.int32, device=f"cuda:{dev}")
    s = _sp(dev)
    nat.check(L.xhe_decrypt(dk.handle, _dp(c), n, _dp(m), s), "decrypt")
    nat.check(L.xhe_decode(dk.handle, _dp(m), _dp(ed), n, _dp(f64), _dp(f32), _dp(st), s), "decrypt")
    return download(f64, np.float64), download(f32, np.float32), download(st, np.int32)


def decrypt_umbed(dk, c, num, ib, precision):
    """device ct -> host (f32 [num, n], status): decrypt, then the centred
    digits / 2^precision and the float32 cast on the device (xhe_umbed); 4 B
    per digit come back."""
    torch = _torch()
    dev = dk.device
    L = nat.lib()
    n = c.shape[0]
    with _On(dev):
        m = torch.empty((n, dk.nw), dtype=torch.int32, device=f"cuda:{dev}")
        f64 = torch.empty((num, n), dtype=torch.float64, device=f"cuda:{dev}")
        f32 = torch.empty((num, n), dtype=torch.float32, device=f"cuda:{dev}")
        st = torch.empty(n, dtype=torch.int32, device=f"cuda:{dev}")
    s = _sp(dev)
    nat.check(L.xhe_decrypt(dk.handle, _dp(c), n, _dp(m), s), "decrypt")
    nat.check(L.xhe_umbed(dk.handle, _dp(m), n, int(num), int(ib), int(precision), _dp(f64), _dp(f32), _dp(st), s),
              "umbed")
    return download(f32, np.float32), download(st, np.int32)


def mulmod(dk, a, ea, b, eb, dmax):
    """ciphertext add with exponent alignment (paillier.py:79-123) on device
    words; ea/eb host int32 arrays or None (all 0) -> device out"""
    torch = _torch()
    dev = dk.device
    n = a.shape[0]
    eda = upload_async(np.ascontiguousarray(ea, dtype=np.int32), dev) if ea is not None else None
    edb = upload_async(np.ascontiguousarray(eb, dtype=np.int32), dev) if eb is not None else None
    with _On(dev):
        out = torch.empty((n, dk.n2w), dtype=torch.int32, device=f"cuda:{dev}")
    nat.check(nat.lib().xhe_mulmod(dk.handle, _dp(a), _dp(eda), _dp(b), _dp(edb), n, int(dmax), _dp(out), None,
                                   _sp(dev)), "add")
    return out


def invert(dk, c):
    torch = _torch()
    dev = dk.device
    with _On(dev):
        out = torch.empty_like(c)
    nat.check(nat.lib().xhe_invert(dk.handle, _dp(c), c.shape[0], _dp(out), _sp(dev)), "invert")
    return out


def powmod(dk, c, kw_, kbits, invert_first=False):
    """c^k or (c^-1)^k mod n^2 per element, k host words [n, kw]"""
    torch = _torch()
    dev = dk.device
    kw_ = np.ascontiguousarray(kw_, dtype=np.uint32)
    kd = upload_small(kw_, dev)
    base = invert(dk, c) if invert_first else c
    with _On(dev):
        out = torch.empty_like(c)
    nat.check(nat.lib().xhe_powmod(dk.handle, _dp(base), _dp(kd), kw_.shape[1], int(kbits), c.shape[0], _dp(out),
                                   _sp(dev)), "powmod")
    return out


def pack(dk, c, k, shift_bits):
    """device ct [n, n2w] -> device [ceil(n / k), n2w]: groups of k folded into
    one ciphertext, element t of a group shifted up by shift_bits * (k - 1 - t)
    plaintext bits (xhe_pack)"""
    torch = _torch()
    dev = dk.device
    n = c.shape[0]
    with _On(dev):
        out = torch.empty((-(-n // k), dk.n2w), dtype=torch.int32, device=f"cuda:{dev}")
    nat.check(nat.lib().xhe_pack(dk.handle, _dp(c), n, int(k), int(shift_bits), _dp(out), _sp(dev)), "pack")
    return out


def segprod(dk, c, d, seg):
    """out[s] = prod_{i in segment s} c_i^(2^d_i) mod n^2 (device c; host d
    int32 and int64 offsets) -> device [nseg, n2w]"""
    torch = _torch()
    dev = dk.device
    n = c.shape[0]
    d = np.ascontiguousarray(d, dtype=np.int32)
    seg = np.ascontiguousarray(seg, dtype=np.int64)
    dmax = int(d.max()) if n else 0
    dd = upload_async(d, dev) if dmax else None
    with _On(dev):
        out = torch.empty((seg.shape[0] - 1, dk.n2w), dtype=torch.int32, device=f"cuda:{dev}")
        src = c if n else torch.zeros((1, dk.n2w), dtype=torch.int32, device=f"cuda:{dev}")
    # the library reads `seg` while enqueuing and stages its plan through
    # pinned memory: nothing here waits for the kernels
    nat.check(nat.lib().xhe_segprod(dk.handle, _dp(src), _dp(dd), dmax, n, seg.ctypes.data_as(ctypes.c_void_p),
                                    seg.shape[0] - 1, _dp(out), _sp(dev)), "segprod")
    return out


def segscan(dk, c, seg):
    """out[i] = prod of segment s's rows up to i mod n^2 (device c; host int64
    offsets) -> device [count, n2w] (xhe_segscan)"""
    torch = _torch()
    dev = dk.device
    n = c.shape[0]
    seg = np.ascontiguousarray(seg, dtype=np.int64)
    with _On(dev):
        out = torch.empty((n, dk.n2w), dtype=torch.int32, device=f"cuda:{dev}")
        src = c.contiguous()
    if n:
        nat.check(nat.lib().xhe_segscan(dk.handle, _dp(src), n, seg.ctypes.data_as(ctypes.c_void_p), seg.shape[0] - 1,
                                        _dp(out), _sp(dev)), "segscan")
    return out


def multiexp(dk, bases, idx, kw_, kbits, win_bits=0):
    """out[j] = prod_t bases[idx[j][t]]^k[j][t] mod n^2 on device bases; idx
    and k host arrays (validated here: the device entry point trusts them)"""
    torch = _torch()
    dev = dk.device
    iw = np.ascontiguousarray(idx, dtype=np.int32)
    ncols, nterms = iw.shape
    nb = bases.shape[0]
    if ncols == 0 or nterms == 0 or nb == 0:
        raise ValueError("multiexp: empty problem")
    if iw.min() < 0 or iw.max() >= nb:
        raise ValueError("multiexp: base index out of range")
    kw_ = np.ascontiguousarray(kw_, dtype=np.uint32).reshape(ncols * nterms, -1)
    di, dkw = upload_small(iw, dev), upload_small(kw_, dev)
    with _On(dev):
        out = torch.empty((ncols, dk.n2w), dtype=torch.int32, device=f"cuda:{dev}")
    nat.check(nat.lib().xhe_multiexp(dk.handle, _dp(bases), nb, _dp(di), _dp(dkw), kw_.shape[1], int(kbits), ncols,
                                     nterms, int(win_bits), _dp(out), _sp(dev)), "multiexp")
    return out


def take(c, idx):
    """rows of device c at host indices idx (a new tensor; xhe_gather_rows, so
    no torch kernel is loaded on first use - a first index_select of a new
    shape class cost 75 ms in the LR step's 15-row batch)"""
    torch = _torch()
    dev = c.device.index
    idx = np.ascontiguousarray(idx, dtype=np.int64)
    with _On(dev):
        out = torch.empty((idx.shape[0],) + tuple(c.shape[1:]), dtype=c.dtype, device=c.device)
    if idx.shape[0]:
        if idx.min() < 0 or idx.max() >= c.shape[0]:
            raise IndexError(f"take: row index out of range for {c.shape[0]} rows")
        ii = upload_async(idx, dev)
        nat.check(nat.lib().xhe_gather_rows(_dp(c), _dp(ii), idx.shape[0], _row_words(c), _dp(out), _sp(dev)),
                  "gather_rows")
    return out


def cat(parts):
    """rows of the parts one after another (copies, no concatenation kernel)"""
    torch = _torch()
    with _On(parts[0].device.index):
        out = torch.empty((sum(p.shape[0] for p in parts),) + tuple(parts[0].shape[1:]), dtype=parts[0].dtype,
                          device=parts[0].device)
        off = 0
        for p in parts:
            out[off:off + p.shape[0]].copy_(p)
            off += p.shape[0]
    return out


def _row_words(c):
    n = 1
    for d in c.shape[1:]:
        n *= int(d)
    return n


def clone(c):
    with _On(c.device.index):
        return c.clone()


def put_rows(c, idx, rows):
    """c[idx] = rows (device) in place (xhe_scatter_rows; idx distinct)"""
    dev = c.device.index
    idx = np.ascontiguousarray(idx, dtype=np.int64)
    if idx.shape[0]:
        if idx.min() < 0 or idx.max() >= c.shape[0] or np.unique(idx).shape[0] != idx.shape[0]:
            raise IndexError(f"put_rows: indices must be distinct rows of the {c.shape[0]}")
        if tuple(rows.shape) != (idx.shape[0],) + tuple(c.shape[1:]) or rows.dtype != c.dtype:
            raise ValueError(f"put_rows: rows {tuple(rows.shape)} {rows.dtype} for {idx.shape[0]} rows of {tuple(c.shape)} "
                             f"{c.dtype}")
        for t in (c, c._base):  # rows change: an encryption's readiness marks and bit lengths no longer describe them
            if t is not None:
                t.__dict__.pop("_xhe_ready", None)
                t.__dict__.pop("_xhe_bits", None)
        ii = upload_async(idx, dev)
        with _On(dev):  # a copy made on the drop-in stream, ordered before the scatter that reads it
            src = rows.contiguous()
        nat.check(nat.lib().xhe_scatter_rows(_dp(src), _dp(ii), idx.shape[0], _row_words(c), _dp(c), _sp(dev)),
                  "scatter_rows")