"""The device prime search: xhe_fermat2_host's verdicts against Python's pow
for every prime width, the carry and argument edge cases, and the search
built on it (primes.next_primes, utils.next_prime / getprimeover with device=,
$XHE_KEYGEN=device key generation) against GMP's mpz_nextprime."""
import math
import random

import numpy as np
import pytest

from tests.conftest import hx, load_fixture

pytestmark = pytest.mark.gpu

KEY_OF = {1024: 2048, 1536: 3072, 2048: 4096, 4096: 8192}  # prime width -> fixture key size


def _want(ns):
    return [pow(2, n - 1, n) == 1 for n in ns]


def _run(bits, starts, which, offs):
    from xfl_amd import _native as nat
    rc, out = nat.fermat2_rc(bits, starts, np.asarray(which, np.int32), np.asarray(offs, np.uint32))
    assert rc == 0, nat.lib().xhe_last_error()
    return out.astype(bool).tolist()


def _batch(bits, count):
    """`count` odd candidates around the fixture key's p and q, as two starts
    with offsets: the primes themselves among their odd neighbours."""
    k = load_fixture(f"paillier_{KEY_OF[bits]}_djn.json")["key"]
    p, q = hx(k["p"]), hx(k["q"])
    assert p.bit_length() == bits and q.bit_length() == bits
    na = (count + 1) // 2
    starts = [p - 2 * (na // 2) - 1, q - 2 * ((count - na) // 2) - 1]  # even: odd offsets make odd candidates
    which = [0] * na + [1] * (count - na)
    offs = [2 * i + 1 for i in range(na)] + [2 * i + 1 for i in range(count - na)]
    return starts, which, offs


@pytest.mark.parametrize("bits,count", [(1024, 1), (1024, 63), (1024, 64), (1024, 65), (1024, 130), (1536, 48),
                                        (2048, 48), (4096, 48)])
def test_verdicts(bits, count):
    starts, which, offs = _batch(bits, count)
    ns = [starts[w] + o for w, o in zip(which, offs)]
    want = _want(ns)
    assert any(want) and (count == 1 or not all(want))  # the fixture prime and composites
    assert _run(bits, starts, which, offs) == want


def test_verdicts_single_composite():
    k = load_fixture("paillier_2048_djn.json")["key"]
    assert _run(1024, [hx(k["p"]) + 1], [0], [1]) == [False]


def test_carries():
    bits = 1024
    r = random.Random(140)
    top = (r.getrandbits(bits) | 1 << (bits - 1)) >> 140 << 140
    ones = top | ((1 << 140) - 1)          # low 140 bits set: the carry crosses four words
    if (ones >> 140) & 1:                  # ... and stops in a word with room
        ones ^= 1 << 140
    zeros = top >> 28 << 28 | 1 << 200     # low 28 bits clear: a whole limb of zeros under the offset
    starts = [ones, zeros, (1 << bits) - 1 - 2 * 40]
    which, offs = [], []
    for s, x in enumerate(starts[:2]):
        for o in range(1 + (x & 1), 24, 2):
            which.append(s)
            offs.append(o)
    for k in range(0, 41):                 # N = 2^bits - 1 - 2k, up to all ones
        which.append(2)
        offs.append(2 * (40 - k))
    ns = [starts[w] + o for w, o in zip(which, offs)]
    assert all(n & 1 and n.bit_length() == bits for n in ns) and max(ns) == (1 << bits) - 1
    assert _run(bits, starts, which, offs) == _want(ns)


def test_carries_wide_rows():
    """all-ones tails at the 16-lane widths: N = 2^bits - 1 - 2k and a carry through 140 bits"""
    for bits in (2048, 4096):
        x = (1 << (bits - 1)) | (1 << 300) | ((1 << 140) - 1)
        starts = [(1 << bits) - 1 - 16, x]
        which = [0] * 9 + [1] * 4
        offs = [2 * i for i in range(9)] + [2, 4, 6, 8]
        ns = [starts[w] + o for w, o in zip(which, offs)]
        assert _run(bits, starts, which, offs) == _want(ns)


def test_argument_errors():
    from xfl_amd import _native as nat
    bits = 1024
    good = (1 << (bits - 1)) + 1

    def rc(b, starts, which, offs):
        code, out = nat.fermat2_rc(b, starts, np.asarray(which, np.int32), np.asarray(offs, np.uint32))
        assert not out.any()  # nothing written
        return code

    assert rc(bits, [good], [0, 0], [0, 1]) == nat.XHE_EINVAL            # an even candidate
    assert rc(bits, [(1 << bits) - 1], [0, 0], [0, 2]) == nat.XHE_EINVAL  # reaches 2^bits
    assert rc(bits, [good, (1 << (bits - 1)) - 1], [0, 1], [0, 0]) == nat.XHE_EINVAL  # a start below 2^(bits-1)
    assert rc(bits, [good], [0, 1], [0, 0]) == nat.XHE_EINVAL            # start index out of range
    assert rc(1000, [1 << 990], [0], [1]) == nat.XHE_ENOTSUP
    assert rc(512, [(1 << 511) + 1], [0], [0]) == nat.XHE_ENOTSUP
    assert rc(bits, [good], [0], [0]) == 0                               # and the library still serves


def _seeded(bits, n=3):
    r = random.Random(bits)
    return [r.getrandbits(bits) | 1 << (bits - 1) for _ in range(n)]


@pytest.mark.parametrize("bits,n", [(1024, 3), (1536, 3), (2048, 3), (4096, 1)])
def test_search_parity(bits, n):
    from xfl_amd.paillier import _gmp, primes, utils
    if not _gmp.available():
        pytest.skip("no libgmp on this host")
    xs = _seeded(bits, n)
    want = [_gmp.next_prime(x) for x in xs]
    assert [utils.next_prime(x, device=0) for x in xs[:1]] == want[:1]
    assert primes.next_primes(xs, device=0) == want  # the starts searched together


def test_search_continuation_on_device():
    from xfl_amd.paillier import _gmp, primes
    if not _gmp.available():
        pytest.skip("no libgmp on this host")
    x = _seeded(2048)[1]
    want = _gmp.next_prime(x)
    assert want - x > 256  # more than one window
    assert primes.next_primes([x], device=0, span=256) == [want]


def test_getprimeover_same_draw():
    from xfl_amd.paillier import utils
    assert utils.getprimeover(1024, rng=random.Random(7), device=0) == utils.getprimeover(1024, rng=random.Random(7))


def test_keygen_on_device_end_to_end(monkeypatch):
    from xfl_amd.paillier import Paillier, PaillierContext, _gmp, primes
    monkeypatch.setenv("XHE_KEYGEN", "device")
    launches = []
    real = primes._device_fermat

    def spy(device):
        f = real(device)
        assert f is not None

        def g(bits, starts, which, offs):
            launches.append((bits, len(starts)))
            return f(bits, starts, which, offs)
        return g

    monkeypatch.setattr(primes, "_device_fermat", spy)
    ctx = PaillierContext.generate(2048, djn_on=True, rng=random.Random(11))
    assert launches and all(b == 1024 for b, _ in launches) and launches[0][1] == 2  # p and q in one launch
    assert ctx.p.bit_length() == 1024 and ctx.q.bit_length() == 1024
    assert math.gcd(ctx.p - 1, ctx.q - 1) == 2
    monkeypatch.setenv("XHE_KEYGEN", "host")
    if _gmp.available():  # (without libgmp the host's Miller-Rabin draws its bases from the same rng)
        host = PaillierContext.generate(2048, djn_on=True, rng=random.Random(11))
        assert (host.p, host.q) == (ctx.p, ctx.q)  # the same draws give the same key on either path
    x = np.array([0.0, 1.0, -1.0, 3.5, -1234.0, 65536.0, 0.25, -0.5])
    ct = Paillier.encrypt(ctx, x, precision=None, max_exponent=None, obfuscation=True)
    back = Paillier.decrypt(ctx, ct, dtype="float")
    assert np.array_equal(np.asarray(back, dtype=np.float64), x)
