"""The key-dependent kernels on keys a random prime search never produces:
p and q exchanged, and the structured keys of tests/structured_keys.py (primes
at the two ends of their range, close primes, an n of K - 1 bits at 4096/8192
and of K bits at 3072, bit-pattern primes). tests/test_structured_keys.py
checks on the CPU that those keys have the properties named there.

Every comparison is word-for-word equality with Python integers:
  swap      the five golden fixtures with p and q exchanged reproduce every
            golden ciphertext and plaintext (the CRT results do not depend on
            the order)
  encrypt   private DJN = oracle.encrypt_m; private and public non-DJN =
            (1 + n m) r^n mod n^2; public DJN = (1 + n m) h^a mod n^2; no
            obfuscation = 1 + n m
  decrypt   those ciphertexts give their m, arbitrary residues give
            oracle.decrypt_raw
  mod n^2   xhe_mulmod / powmod / invert / segprod / multiexp on extremal
            moduli against pow and products; xhe_decode at the sign bounds

The expected values of a key are computed once (pure Python costs 40 ms per
2048-bit encryption, seconds at 8192 bits), so a key has at most DISTINCT[K]
distinct (m, draw) pairs; they are tiled to the batch sizes that select each
kernel shape, and every produced row is compared.

Batch sizes (the thresholds and rules live in xfl_amd/csrc/paths.hpp, where
tests/test_paths.py pins each of them on the CPU; the names below are its):
  2048-bit DJN private encrypt, k_djn_pmd, pmd_split(): 16 lanes per element
    up to 2,048 elements, 4 up to 16,384, 1 beyond -> 1, 65, 3,000, 17,000
  2048-bit public non-DJN: k_nodjn_pub_wave up to kPubWaveMax = 2,048, the
    digit kernels beyond -> the same four sizes fall on both sides
  3072+ bits: DJN private keys always run k_djn_pmdx, private non-DJN
    k_nodjn_crt, public keys k_djn_pub / k_nodjn_pub, whatever the batch (the
    16-lane limit kEncRowMax = 20,480 gates only k_djn_pow_x, which a key with
    digit tables never reaches) -> 3 and 21,000 (past that limit all the same)
    for DJN private, 3 and 6,000 otherwise; 8192 bits: 2 and 21,000 / 300
  decrypt, decrypt(): 2048 bits k_dec_rns up to kDecWaveMax = 1,024, 16
    lanes up to kDecRowMax = 5,120, 4 up to kDecQuadMax = 28,672, one lane
    (k_dec_pmd_*) beyond -> 15, 1,100, 5,200, 29,000; 3072/4096 bits 16 lanes
    up to 5,120, then the digit kernels k_dec_pmdx_* -> 15 and 6,000
  mod n^2, n2_shape(): 16 lanes up to kN2RowMax = 4,096, 4 beyond (equal
    exponents: k_add_barrett); adds up to kWaveAddMax = 256 run k_mulmod_wave
    -> 300 and 6,000
Where the library records a launch (xhe_profile_read) the test asserts once
that the intended kernel ran.

Draws of non-DJN keys are residues in [1, n) (xhe_rand's range, paillier.py:
215,229), so their edge draws are 1, 2, n - 1, n - 2, the top bit of n alone
and all ones below it; 2^rand_bits - 1 (>= n there) is a DJN draw only.
"""
import math
import random

import numpy as np
import pytest

from oracle import paillier_oracle as O
from tests import structured_keys as SK
from tests.conftest import FIXTURES, hx, load_fixture
from tests.test_gpu_add_barrett import _edge
from tests.test_gpu_codec import ST_F32_OVERFLOW, ST_OK, ST_OVERFLOW, device_decode
from tests.test_gpu_parity import DEC_CASES, ENC_CASES, check_decrypt_case, check_encrypt_case
from tests.test_gpu_pub_small import _launches

pytestmark = pytest.mark.gpu

WIN = 8  # fixed-base tables that build in milliseconds
DISTINCT = {2048: 32, 3072: 8, 4096: 8, 8192: 2}
KEYS = [(K, name) for K in (2048, 3072, 4096) for name in SK.names(K)] + [(8192, "top"), (8192, "bottom")]
DEC_KEYS = [c for c in KEYS if c[0] != 8192]
# (DJN private, every other mode)
ENC_BATCHES = {2048: ((1, 65, 3000, 17000),) * 2, 3072: ((3, 21000), (3, 6000)), 4096: ((3, 21000), (3, 6000)),
               8192: ((2, 21000), (2, 300))}
DEC_BATCHES = {2048: (15, 1100, 5200, 29000), 3072: (15, 6000), 4096: (15, 6000)}
PUB_MODULI = {"top": None, "bottom": None, "all_ones_2048": 2 ** 2048 - 159, "sparse_2046": 2 ** 2045 + 1}


def _nat():
    from xfl_amd import _native as nat
    return nat


def _tile(w, count, start=0):
    """count rows: the rows of w repeated, beginning at row `start`"""
    w = np.roll(w, -start, axis=0)
    return np.ascontiguousarray(np.tile(w, (-(-count // w.shape[0]), 1))[:count])


def _same(got, want, what):
    assert got.shape == want.shape, what
    bad = np.nonzero(np.any(got != want, axis=1))[0]
    assert bad.size == 0, f"{what}: {bad.size} of {len(want)} rows differ, first {bad[:6].tolist()}"


class Profile:
    """launch records on for the block; counts read by kernel label"""

    def __enter__(self):
        _nat().lib().xhe_profile(1)
        return self

    def __exit__(self, *exc):
        _nat().lib().xhe_profile(0)

    @staticmethod
    def reset():
        _nat().lib().xhe_profile(1)

    @staticmethod
    def ran(**want):
        for name, n in want.items():
            assert _launches(name) == n, (name, _launches(name), n)


# ---------------------------------------------------------------- expected values
class Vectors:
    """the distinct inputs of one key and what the oracle makes of them"""

    def __init__(self, K, name):
        k = SK.key(K, name)
        self.k, self.K = k, K
        n, n2 = k.n, k.n * k.n
        d = DISTINCT[K]
        rng = random.Random(f"vectors-{K}-{name}")
        self.ok = O.derive_private(k.p, k.q, k.h)
        rb, nb = n.bit_length() // 2, n.bit_length()
        assert self.ok["djn_exp_bound"] == 1 << rb
        pad = lambda edge, draw: (edge[:1] + [draw()] + edge[1:] + [draw() for _ in range(d)])[:d]  # noqa: E731
        self.m = pad([n - 1, n // 3, 0, 1, n - n // 3], lambda: rng.randrange(n))
        self.a = pad([(1 << rb) - 1, 1 << (rb - 1), 1, 2], lambda: rng.randrange(1, 1 << rb))
        self.r = pad([n - 1, 1 << (nb - 1), 1, 2, n - 2, (1 << (nb - 1)) - 1], lambda: rng.randrange(1, n))
        assert all(0 < r < n for r in self.r) and all(0 <= a < 1 << rb for a in self.a)
        raw = [(1 + n * m) % n2 for m in self.m]
        self.ct = {
            "priv_djn": [O.encrypt_m(self.ok, m, a) for m, a in zip(self.m, self.a)],
            "pub_djn": [c * SK.powmod(k.h, a, n2) % n2 for c, a in zip(raw, self.a)],
            "nodjn": [c * SK.powmod(r, n, n2) % n2 for c, r in zip(raw, self.r)],
            "plain": raw,
        }
        # arbitrary residues (tests/test_gpu_parity.py test_decrypt_arbitrary_residues' edges, then random ones)
        p, q = k.p, k.q
        self.arb = [1, n2 - 1, p * p - 1, p * p + 1, q * q - 2, q * q + 3, n + 1, p * q * q + 5]
        self.arb += [rng.randrange(1, n2) for _ in range(8 if K == 2048 else 2)]
        assert all(math.gcd(c, n) == 1 for c in self.arb)
        self._arb_m = None

    def arb_m(self):
        if self._arb_m is None:
            self._arb_m = [O.decrypt_raw(self.ok, c) for c in self.arb]
        return self._arb_m


_vectors = {}


def vectors(K, name):
    if (K, name) not in _vectors:
        _vectors[(K, name)] = Vectors(K, name)
    return _vectors[(K, name)]


def _ids(c):
    return f"{c[0]}-{c[1]}"


# ---------------------------------------------------------------- p and q exchanged
@pytest.mark.parametrize("fx", FIXTURES)
def test_swapped_primes_reproduce_golden(fx):
    """A fixture's key created as (q, p): every private-key case of ENC_CASES
    gives the golden ciphertexts and every decrypt case the golden m. The
    fixtures fix the order (2048-djn, 3072: p > q; the others p < q), so this
    runs each size's kernels in the order they have not seen."""
    nat = _nat()
    g = load_fixture(fx)
    k = g["key"]
    p, q = hx(k["p"]), hx(k["q"])
    h = hx(k["h_pow_n"]) if k["djn_on"] else None
    dk = nat.DeviceKey(g["key_bits"], p * q, q, p, h, win_bits=WIN if h else 0)
    priv = [c for c in ENC_CASES if g["encrypt"][c]["private"]]
    assert len(priv) >= 4
    for case in priv:
        check_encrypt_case(g, case, dk)
    for case in DEC_CASES:
        check_decrypt_case(g, case, dk)


# ---------------------------------------------------------------- encrypt
def _encrypt_batches(dk, v, mode, rand, batches, kernel):
    nat = _nat()
    mw = nat.ints_to_words(v.m, dk.nw)
    rw = None if rand is None else nat.ints_to_words(rand, dk.rand_words)
    want = nat.ints_to_words(v.ct[mode], dk.n2w)
    for count in batches:
        Profile.reset()
        got = dk.encrypt_words(_tile(mw, count, count), None if rw is None else _tile(rw, count, count))
        _same(got, _tile(want, count, count), f"{mode} x {count}")
        if kernel:
            Profile.ran(**kernel(count))


@pytest.mark.parametrize("mode", ["priv_djn", "priv_nodjn", "pub_djn", "pub_nodjn"])
@pytest.mark.parametrize("key", KEYS, ids=_ids)
def test_encrypt_structured(key, mode):
    """one key kind a case (an 8192-bit key takes a second to derive): with
    obfuscation at every batch size, and on the DJN private and the plain
    public key also without (rand = NULL)"""
    nat = _nat()
    K, name = key
    v = vectors(K, name)
    k = v.k
    djn_b, other_b = ENC_BATCHES[K]
    small = K == 2048
    wave = lambda c: int(small and c <= nat.PUB_WAVE_MAX)  # noqa: E731
    with Profile():
        if mode == "priv_djn":
            dk = nat.DeviceKey(K, k.n, k.p, k.q, k.h, win_bits=WIN)
            assert dk.rand_bits == k.n.bit_length() // 2
            lab = "k_djn_pmd" if small else "k_djn_pmdx"
            _encrypt_batches(dk, v, "priv_djn", v.a, djn_b, lambda c: {lab: 1})
            _encrypt_batches(dk, v, "plain", None, djn_b[:2], None)
        elif mode == "priv_nodjn":
            dk = nat.DeviceKey(K, k.n, k.p, k.q, None)
            assert dk.rand_bits == k.n.bit_length()
            _encrypt_batches(dk, v, "nodjn", v.r, other_b, lambda c: {"k_nodjn_crt": 1})
        elif mode == "pub_djn":
            dk = nat.DeviceKey(K, k.n, None, None, k.h, win_bits=WIN)
            _encrypt_batches(dk, v, "pub_djn", v.a, other_b, lambda c: {"k_djn_pub": 1})
        else:
            dk = nat.DeviceKey(K, k.n, None, None, None)
            _encrypt_batches(dk, v, "nodjn", v.r, other_b,
                             lambda c: {"k_nodjn_pub_wave": wave(c), "k_nodjn_pub": 1 - wave(c)})
            _encrypt_batches(dk, v, "plain", None, other_b[:2], None)


# ---------------------------------------------------------------- decrypt
@pytest.mark.parametrize("key", DEC_KEYS, ids=_ids)
def test_decrypt_structured(key):
    nat = _nat()
    K, name = key
    v = vectors(K, name)
    k = v.k
    g1, g2 = v.ct["priv_djn"], v.ct["nodjn"]
    # the first 15 hold every edge residue and genuine ciphertexts of both kinds
    cts = v.arb[:8] + g1[:4] + g2[:3] + v.arb[8:] + g1[4:] + g2[3:] + v.ct["pub_djn"] + v.ct["plain"]
    ms = v.arb_m()[:8] + v.m[:4] + v.m[:3] + v.arb_m()[8:] + v.m[4:] + v.m[3:] + v.m + v.m
    assert len(cts) == len(ms) and all(c < k.n ** 2 for c in cts)
    cw, mw = nat.ints_to_words(cts, 2 * K // 32), nat.ints_to_words(ms, K // 32)
    with Profile():
        dk = nat.DeviceKey(K, k.n, k.p, k.q, k.h, win_bits=WIN)
        for count in DEC_BATCHES[K]:
            Profile.reset()
            got = dk.decrypt_words(_tile(cw, count))
            _same(got, _tile(mw, count), f"decrypt x {count}")
            rns = int(K == 2048 and count <= 1024)
            Profile.ran(k_dec_rns=rns, k_dec_wave=0, k_dec_pow=1 - rns)


# ---------------------------------------------------------------- mod n^2
def _modulus(which):
    return PUB_MODULI[which] or SK.key(2048, which).n


def _pub(which):
    n = _modulus(which)
    assert n.bit_length() == {"top": 2048, "bottom": 2047, "all_ones_2048": 2048, "sparse_2046": 2046}[which]
    return n, _nat().DeviceKey(2048, n, None, None, None, device=0)


def _up(dk, ints):
    from xfl_amd.paillier import resident
    return resident.upload(_nat().ints_to_words(ints, dk.n2w), dk.device)


def _down(t):
    from xfl_amd.paillier import resident
    return _nat().words_to_ints(resident.download(t))


def _units(n, count, rng):
    """count residues mod n^2 coprime to n, the edge ones first"""
    n2 = n * n
    out = [c for c in (1, n2 - 1, n + 1, 2, (1 << 4095) % n2) if math.gcd(c, n) == 1]
    while len(out) < count:
        c = rng.randrange(1, n2)
        if math.gcd(c, n) == 1:
            out.append(c)
    return out[:count]


@pytest.mark.parametrize("which", list(PUB_MODULI))
@pytest.mark.parametrize("count", [6000, 300])
def test_mulmod_extremal_modulus(which, count):
    """c = a b mod n^2 over the cross product of tests/test_gpu_add_barrett.py's
    edge operands (6,000: k_add_barrett, operands up to 2^4096 - 1; 300: the
    16-lane Montgomery shape, which takes residues - the edges mod n^2), then
    one pass with exponent gaps up to 3 against oracle.add_ct"""
    from xfl_amd.paillier import resident
    n, dk = _pub(which)
    n2 = n * n
    rng = random.Random(f"mulmod-{which}-{count}")
    a = [rng.randrange(n2) for _ in range(count)]
    b = [rng.randrange(n2) for _ in range(count)]
    edge = _edge(n2) if count > 4096 else [x % n2 for x in _edge(n2)]
    assert len(edge) ** 2 <= count
    for i, x in enumerate(edge):
        for j, y in enumerate(edge):
            a[len(edge) * i + j], b[len(edge) * i + j] = x, y
    a[-1], b[-1] = n2 - 1, n2 - 1
    da, db = _up(dk, a), _up(dk, b)
    e = np.arange(count, dtype=np.int32) % 5 - 40
    with Profile():
        got = _down(resident.mulmod(dk, da, e, db, e.copy(), 0))
        Profile.ran(k_add_barrett=int(count > 4096))
        bad = [i for i in range(count) if got[i] != a[i] * b[i] % n2]
        assert not bad, f"{len(bad)} wrong, first {bad[:5]}"
        # gaps: residues below n^2, exponents apart by 0..3 in both directions
        a, b = [x % n2 for x in a], [x % n2 for x in b]
        ea = np.asarray([rng.randrange(-3, 1) for _ in range(count)], dtype=np.int32)
        eb = np.asarray([rng.randrange(-3, 1) for _ in range(count)], dtype=np.int32)
        ea[:8], eb[:8] = [0, -3, 0, -1, -2, -3, -1, 0], [-3, 0, 0, -3, -2, 0, -2, -1]
        da, db = _up(dk, a), _up(dk, b)
        Profile.reset()
        got = _down(resident.mulmod(dk, da, ea, db, eb, 3))
        Profile.ran(k_add_barrett=0)
    ok = O.derive_public(n)
    bad = [i for i in range(count) if got[i] != O.add_ct(ok, a[i], int(ea[i]), b[i], int(eb[i]))[0]]
    assert not bad, f"gaps: {len(bad)} wrong, first {bad[:5]}"


@pytest.mark.parametrize("which", list(PUB_MODULI))
def test_powmod_invert_segprod_multiexp_extremal_modulus(which):
    from xfl_amd.paillier import resident
    nat = _nat()
    n, dk = _pub(which)
    n2 = n * n
    rng = random.Random(f"n2ops-{which}")
    # powmod: exponents 0, 1, all 96 bits set, random; 64 distinct pairs tiled to both lane shapes
    KB = 96
    cs = [1, n2 - 1, n + 1, n2 - n - 1] + [rng.randrange(1, n2) for _ in range(60)]
    ks = [0, 1, (1 << KB) - 1, (1 << KB) - 1, 0, 1, (1 << KB) - 1] + [rng.getrandbits(KB) for _ in range(57)]
    ks[-1] = 1 << (KB - 1)
    want = nat.ints_to_words([pow(c, e, n2) for c, e in zip(cs, ks)], dk.n2w)
    cw, kw = nat.ints_to_words(cs, dk.n2w), nat.ints_to_words(ks, KB // 32)
    with Profile():
        for count in (6000, 300):
            Profile.reset()
            out = resident.powmod(dk, resident.upload(_tile(cw, count), dk.device), _tile(kw, count), KB)
            _same(resident.download(out), _tile(want, count), f"powmod x {count}")
            Profile.ran(k_powmod_n2=1)
    # invert: 257 elements, one past the whole-block tree
    cs = _units(n, 257, rng)
    assert _down(resident.invert(dk, _up(dk, cs))) == [pow(c, -1, n2) for c in cs]
    # segprod: segments of 0, 1 and 130 elements, without and with squarings
    cs = _units(n, 131, rng)
    seg = np.asarray([0, 0, 1, 131], dtype=np.int64)
    for d in (np.zeros(131, np.int32), np.arange(131, dtype=np.int32) % 3):
        got = _down(resident.segprod(dk, _up(dk, cs), d, seg))
        want = []
        for s in range(3):
            acc = 1
            for i in range(int(seg[s]), int(seg[s + 1])):
                acc = acc * pow(cs[i], 1 << int(d[i]), n2) % n2
            want.append(acc)
        assert got == want and want[0] == 1
    # multiexp: 24 bases, 5 columns of 24 terms
    bases = _units(n, 24, rng)
    idx = [[rng.randrange(24) for _ in range(24)] for _ in range(5)]
    ex = [[rng.getrandbits(60) for _ in range(24)] for _ in range(5)]
    ex[0][:3] = [0, 1, (1 << 60) - 1]
    got = _down(resident.multiexp(dk, _up(dk, bases), idx, nat.ints_to_words([e for row in ex for e in row], 2), 60))
    for j in range(5):
        acc = 1
        for t in range(24):
            acc = acc * pow(bases[idx[j][t]], ex[j][t], n2) % n2
        assert got[j] == acc, j


@pytest.mark.parametrize("which", ["top", "bottom"])
def test_decode_sign_bounds(which):
    """xhe_decode at exponent 0 on both sides of max_pos = n // 3 and min_neg =
    n - n // 3: the decode-range OverflowError strictly between them, and the
    reference's float32 result (an mpz -> float OverflowError for a value of
    2,046 bits) on them and outside"""
    n, dk = _pub(which)
    ok = O.derive_public(n)
    ms = [n // 3, n // 3 + 1, n - n // 3 - 1, n - n // 3, n // 3 - 1, n - n // 3 + 1, 5, n - 5]
    f64, f32, st = device_decode(dk, ms, [0] * len(ms))
    kinds = []
    for i, m in enumerate(ms):
        try:
            O.signed_value(ok, m)
        except OverflowError:
            assert st[i] == ST_OVERFLOW, i
            kinds.append(ST_OVERFLOW)
            continue
        try:
            want = O.decode_float32(ok, m, 0)
        except OverflowError:
            assert st[i] == ST_F32_OVERFLOW, i
            kinds.append(ST_F32_OVERFLOW)
            continue
        assert st[i] == ST_OK and float(f32[i]) == want and f64[i] == float(O.decode_origin(ok, m, 0)), i
        kinds.append(ST_OK)
    assert kinds == [ST_F32_OVERFLOW, ST_OVERFLOW, ST_OVERFLOW, ST_F32_OVERFLOW, ST_F32_OVERFLOW, ST_F32_OVERFLOW,
                     ST_OK, ST_OK]
