"""Prime search for key generation with the candidates tested on the GPU.

The reference draws a random start with the top bit set and takes
`gmpy2.next_prime` of it (utils.py:79-89), one candidate after another on one
host core. Here a whole window above each start is sieved on the host
(`sieve_offsets`), every survivor gets a base-2 Fermat test in one launch
(include/xhe.h xhe_fermat2_host, one lane group per candidate), and the
smallest survivor that passes is confirmed on the host with the test
`mpz_nextprime` itself applies (`mpz_probab_prime_p(s, 25)`).

Exactness: every integer below the returned one has a small factor or failed
the Fermat test (a prime never fails it), and the returned one passed GMP's
test, so the result is the integer `_gmp.next_prime(x)` returns.

`next_primes` never raises for a request the device cannot serve (a width the
library lacks, a start without the top bit of its width, a window that would
reach 2^bits, no library, no GPU): those starts go to the host search.
"""
import os

import numpy as np

from . import _gmp
from .utils import _SMALL_PRIMES

DEVICE_BITS = (1024, 1536, 2048, 4096)  # prime widths xhe_fermat2_host has: half of each key size

SIEVE_LIMIT = 2000  # the sieve's primes: the 302 odd primes below it (utils._SMALL_PRIMES)

# $XHE_KEYGEN=auto searches on the device from this prime width up: the
# smallest width at which tools/bench_keygen.py measured the device's median
# below the host's and its slowest start below the host's fastest (DESIGN.md
# section 7); None would mean auto = host.
AUTO_MIN_BITS = 2048


def default_span(bits):
    """Window length per start: 3 * bits is 4.3 mean prime gaps (ln 2 * bits),
    so one window holds the prime for 98.7 % of the starts, and its ~6.6 %
    sieve survivors (about 800 at 4096 bits, 16 lanes each) are still fewer
    waves than the chip has compute units: a longer window costs no time."""
    return 3 * bits


def sieve_offsets(x, span, prime_limit=SIEVE_LIMIT):
    """Offsets o in [1, span], ascending, for which x + o is odd and has no
    prime factor below prime_limit: one x % p per small prime, then strided
    numpy writes over the odd offsets."""
    x = int(x)
    first = 2 if x & 1 else 1  # smallest o > 0 with x + o odd
    offs = np.arange(first, span + 1, 2, dtype=np.int64)
    alive = np.ones(len(offs), dtype=bool)
    for p in _odd_primes_below(prime_limit):
        # o = first + 2 k = -x (mod p)  <=>  k = (-x - first) / 2 (mod p)
        k0 = (-(x % p) - first) * ((p + 1) // 2) % p
        alive[k0::p] = False
    return offs[alive]


def _odd_primes_below(limit):
    if limit <= 2000:
        return [p for p in _SMALL_PRIMES if p < limit]
    sieve = np.ones(limit, dtype=bool)
    sieve[:2] = False
    for i in range(2, int(limit ** 0.5) + 1):
        if sieve[i]:
            sieve[i * i::i] = False
    return [int(p) for p in np.nonzero(sieve)[0] if p > 2]


def _confirm(n):
    if _gmp.available():
        return _gmp.probab_prime(n, 25)
    from .utils import is_probable_prime
    return is_probable_prime(n)


def _host_next_prime(x):
    from .utils import next_prime
    return next_prime(x)


_ready = None


def device_ready():
    """The library file exists and sees a GPU. Never raises, and does not
    load the library where its file is missing."""
    global _ready
    if _ready is None:
        try:
            from .. import _native
            _ready = os.path.exists(_native.LIB_PATH) and _native.lib().xhe_device_count() > 0
        except Exception:  # noqa: BLE001
            _ready = False
    return _ready


def keygen_on_device(bits):
    """$XHE_KEYGEN for primes of `bits` bits: 'host', 'device', or 'auto'
    (the default: the device from AUTO_MIN_BITS up when it is there)."""
    mode = os.environ.get("XHE_KEYGEN", "auto").strip().lower() or "auto"
    if mode == "host":
        return False
    if mode == "device":
        return True
    return AUTO_MIN_BITS is not None and bits >= AUTO_MIN_BITS and bits in DEVICE_BITS and device_ready()


def _device_fermat(device):
    """fermat(bits, starts, which, offs) on the native library, or None
    without library or GPU. The callable returns None for a width the loaded
    build lacks."""
    if not device_ready():
        return None
    from .. import _native

    def fermat(bits, starts, which, offs):
        return _native.fermat2(bits, starts, which, offs, device=device)
    return fermat


def next_primes(xs, device=0, span=None, fermat=None):
    """[smallest probable prime > x for x in xs], the integers
    `_gmp.next_prime` returns, with the candidates of all starts of one width
    tested in one launch per round of windows. `fermat(bits, starts, which,
    offs)` replaces the native call (tests): the base-2 Fermat verdict of
    starts[which[i]] + offs[i] per candidate, or None when it cannot serve."""
    xs = [int(x) for x in xs]
    out = [None] * len(xs)
    native = fermat is None
    if native:
        fermat = _device_fermat(device)
    by_bits = {}
    for i, x in enumerate(xs):
        bits = x.bit_length() if x > 0 else 0
        # (below 32 bits a candidate could be one of the sieve's own primes)
        if fermat is None or bits < 32 or (native and bits not in DEVICE_BITS):
            out[i] = _host_next_prime(x)
        else:
            by_bits.setdefault(bits, []).append(i)
    for bits, idx in by_bits.items():
        sp = int(span) if span else default_span(bits)
        base = {i: xs[i] for i in idx}  # every integer in (xs[i], base[i]] is composite
        while base:
            starts, which, offs = [], [], []
            for i in list(base):
                if base[i] + sp >= 1 << bits:  # the window would reach 2^bits
                    out[i] = _host_next_prime(base.pop(i))
                    continue
                o = sieve_offsets(base[i], sp)
                which.append(np.full(len(o), len(starts), dtype=np.int32))
                offs.append(o.astype(np.uint32))
                starts.append(i)
            if not starts:
                break
            which, offs = np.concatenate(which), np.concatenate(offs)
            ok = fermat(bits, [base[i] for i in starts], which, offs) if len(offs) else np.zeros(0, dtype=bool)
            if ok is None:  # a width this build lacks
                for i in starts:
                    out[i] = _host_next_prime(base.pop(i))
                break
            ok = np.asarray(ok, dtype=bool)
            for s, i in enumerate(starts):
                for o in offs[(which == s) & ok]:  # ascending
                    if _confirm(base[i] + int(o)):
                        out[i] = base.pop(i) + int(o)
                        break
                else:
                    base[i] += sp
    return out
