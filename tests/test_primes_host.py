"""Host side of the device prime search (xfl_amd/paillier/primes.py): the
sieve against brute force, the window continuation and the host fallbacks of
next_primes with a pure-Python Fermat test in place of the native call, the
GMP confirmation binding, and key generation where no GPU serves it."""
import math
import random

import pytest

from xfl_amd.paillier import _gmp
from xfl_amd.paillier import primes as P
from xfl_amd.paillier import utils as U

needs_gmp = pytest.mark.skipif(not _gmp.available(), reason="no libgmp on this host")


def _small_primes(limit):
    return [p for p in range(2, limit) if all(p % d for d in range(2, int(p ** 0.5) + 1))]


def _starts(bits, n=3):
    r = random.Random(bits)
    return [r.getrandbits(bits) | 1 << (bits - 1) for _ in range(n)]


def py_fermat(bits, starts, which, offs):
    return [pow(2, n - 1, n) == 1 for n in (starts[w] + int(o) for w, o in zip(which, offs))]


@pytest.mark.parametrize("bits", [256, 1024])
@pytest.mark.parametrize("prime_limit", [50, 2000])
def test_sieve_offsets_brute_force(bits, prime_limit):
    span = 2048
    ps = _small_primes(prime_limit)
    for x in _starts(bits, 2) + [_starts(bits, 1)[0] + 1]:  # odd and even starts
        want = [o for o in range(1, span + 1) if (x + o) & 1 and all((x + o) % p for p in ps)]
        got = P.sieve_offsets(x, span, prime_limit)
        assert got.tolist() == want
        assert 0 < len(want) < span // 4


@needs_gmp
def test_next_primes_python_fermat():
    xs = _starts(256)
    calls = []

    def fermat(bits, starts, which, offs):
        calls.append(len(offs))
        return py_fermat(bits, starts, which, offs)

    assert P.next_primes(xs, fermat=fermat) == [_gmp.next_prime(x) for x in xs]
    assert len(calls) == 1 and calls[0] > 3  # the three starts in one call


@needs_gmp
def test_next_primes_window_continuation():
    xs = _starts(256, 6)
    want = [_gmp.next_prime(x) for x in xs]
    assert max(w - x for w, x in zip(want, xs)) > 64  # some start needs more than one window
    calls = []

    def fermat(bits, starts, which, offs):
        calls.append(len(starts))
        return py_fermat(bits, starts, which, offs)

    assert P.next_primes(xs, span=64, fermat=fermat) == want
    assert len(calls) > 1 and calls[-1] < calls[0]  # finished starts leave the later rounds


@needs_gmp
def test_next_primes_host_fallbacks(monkeypatch):
    def no_call(*a):
        raise AssertionError("the Fermat call must not run")

    x = (1 << 256) - 2  # a window from here would reach 2^256
    assert P.next_primes([x], fermat=no_call) == [_gmp.next_prime(x)]
    # a start just below it: windows until the last one would cross, then the host
    x = (1 << 256) - 150
    assert P.next_primes([x], span=64, fermat=py_fermat) == [_gmp.next_prime(x)]
    # a Fermat call that cannot serve the width (returns None)
    xs = _starts(256, 2)
    assert P.next_primes(xs, fermat=lambda *a: None) == [_gmp.next_prime(v) for v in xs]
    # no library or no GPU; a width the device lacks; a start without its width's top bit
    monkeypatch.setattr(P, "_ready", False)
    xs = _starts(1024, 1)
    assert P.next_primes(xs, device=0) == [_gmp.next_prime(xs[0])]
    monkeypatch.setattr(P, "_ready", True)
    monkeypatch.setattr(P, "_device_fermat", lambda device: no_call)
    xs = [_starts(256, 1)[0], _starts(1024, 1)[0] >> 1]
    assert P.next_primes(xs, device=0) == [_gmp.next_prime(v) for v in xs]
    assert U.next_prime(xs[0], device=0) == _gmp.next_prime(xs[0])


def test_next_primes_fermat_liar_rejected():
    """a base-2 pseudoprime in the window is stopped by the confirmation"""
    x = 2 ** 40 + 2 ** 20
    liar = None

    def fermat(bits, starts, which, offs):
        nonlocal liar
        ok = py_fermat(bits, starts, which, offs)
        if liar is None:
            first = ok.index(True)
            assert first > 0
            liar = starts[which[0]] + int(offs[0])
            ok[0] = True  # a composite reported as passing, below the prime
        return ok

    got = P.next_primes([x], fermat=fermat)[0]
    assert liar is not None and liar < got and not U.is_probable_prime(liar)
    n = x + 1
    while not U.is_probable_prime(n):
        n += 1
    assert got == n


@needs_gmp
def test_probab_prime_matches_miller_rabin():
    r = random.Random(512)
    for _ in range(20):
        n = r.getrandbits(512) | 1 | 1 << 511
        assert _gmp.probab_prime(n) == U.is_probable_prime(n)
    for p in (3, 65537, 2 ** 127 - 1, 2 ** 521 - 1, _gmp.next_prime(1 << 511)):
        assert _gmp.probab_prime(p) and U.is_probable_prime(p)
    for c in (1, 9, 341, 561, (2 ** 127 - 1) * (2 ** 61 - 1)):
        assert not _gmp.probab_prime(c)


def _no_gpu():
    return not P.device_ready()


@pytest.mark.parametrize("mode", ["host", None])
def test_keygen_without_device(mode, monkeypatch):
    """$XHE_KEYGEN=host anywhere, and an unset variable where no GPU is
    visible, generate a valid 2048-bit DJN key on the host"""
    from xfl_amd.paillier import PaillierContext
    if mode is None:
        monkeypatch.delenv("XHE_KEYGEN", raising=False)
        if not _no_gpu():
            monkeypatch.setattr(P, "_ready", False)  # on a GPU machine: as if none were visible
    else:
        monkeypatch.setenv("XHE_KEYGEN", mode)
    monkeypatch.setattr(P, "_device_fermat", lambda device: pytest.fail("device search on the host path"))
    c = PaillierContext.generate(2048, djn_on=True, rng=random.Random(5))
    assert 2046 <= c.n.bit_length() <= 2048 and c.djn_on
    assert c.p != c.q and math.gcd(c.p - 1, c.q - 1) == 2
    assert U.is_probable_prime(c.p, rounds=4) and U.is_probable_prime(c.q, rounds=4)
    assert c.h_pow_n == pow(c.h_pow_n, 1, c.n_square) and math.gcd(c.h_pow_n, c.n) == 1


def test_keygen_mode_probe(monkeypatch):
    """the switch: host / device / auto by width; the probe never raises and
    does not load a library that is not there"""
    from xfl_amd import _native
    monkeypatch.setenv("XHE_KEYGEN", "host")
    assert not P.keygen_on_device(4096)
    monkeypatch.setenv("XHE_KEYGEN", "device")
    assert P.keygen_on_device(1024)
    monkeypatch.setenv("XHE_KEYGEN", "auto")
    monkeypatch.setattr(P, "_ready", True)
    for bits in P.DEVICE_BITS:
        assert P.keygen_on_device(bits) == (P.AUTO_MIN_BITS is not None and bits >= P.AUTO_MIN_BITS)
    assert not P.keygen_on_device(512)
    monkeypatch.setattr(P, "_ready", None)
    monkeypatch.setattr(_native, "LIB_PATH", "/nonexistent/libxhe.so")
    monkeypatch.setattr(_native, "lib", lambda: pytest.fail("library loaded without its file"))
    assert P.device_ready() is False
    assert not P.keygen_on_device(4096)
