"""Public non-DJN encryption of small batches (k_nodjn_pub_wave, one 16-wave
block per element up to _native.PUB_WAVE_MAX elements of a 2048-bit key)
against the closed form ct = (1 + n m) r^n mod n^2 (paillier.py:228-230, 283)
in Python integers: every element of 1, 15 and 64, sampled elements on both
sides of the threshold, edge operands, and moduli of every accepted bit length
(a public key needs only an odd n). The two shapes must agree word for word,
and the dispatch is read from the library's own launch records."""
import ctypes
import random

import numpy as np
import pytest

from oracle import paillier_oracle as O
from tests.conftest import hx, load_fixture

pytestmark = pytest.mark.gpu

FX = "paillier_2048_nodjn.json"


def _fixture_n():
    return hx(load_fixture(FX)["key"]["n"])


def _moduli():
    return {"fixture": _fixture_n(),
            "all_ones_2048": 2 ** 2048 - 159,
            "sparse_2046": 2 ** 2045 + 1,
            "random_2047": random.Random(2047).getrandbits(2047) | (1 << 2046) | 1}


def _closed(n, m, r):
    n2 = n * n
    return (1 + n * m) * pow(r, n, n2) % n2


def _encrypt(dk, ms, rs):
    from xfl_amd import _native as nat
    return nat.words_to_ints(dk.encrypt_words(nat.ints_to_words(ms, dk.nw), nat.ints_to_words(rs, dk.rand_words)))


def _pairs(n, count, rng):
    """count (m, r) pairs: the cross product of the edge operands first (as
    many as fit), then random ones"""
    er = [1, 2, n - 1, n - 2, 2 ** 2040, rng.randrange(1, n)]
    em = [0, 1, n - 1, n // 3, n - n // 3, rng.randrange(n)]
    cross = [(m, r) for r in er for m in em]
    if count < len(cross):  # the diagonal, then what fits
        cross = [(em[i], er[i]) for i in range(6)] + cross
    pairs = cross[:count]
    while len(pairs) < count:
        pairs.append((rng.randrange(n), rng.randrange(1, n)))
    return [p[0] for p in pairs], [p[1] for p in pairs]


@pytest.mark.parametrize("which", ["fixture", "all_ones_2048", "sparse_2046", "random_2047"])
def test_closed_form(which):
    from xfl_amd import _native as nat
    n = _moduli()[which]
    assert n.bit_length() == {"fixture": 2048, "all_ones_2048": 2048, "sparse_2046": 2046, "random_2047": 2047}[which]
    dk = nat.DeviceKey(2048, n, None, None, None, device=0)
    rng = random.Random(n % 1000003)
    for count in (1, 15, 64):
        ms, rs = _pairs(n, count, rng)
        ct = _encrypt(dk, ms, rs)
        for i in range(count):
            assert ct[i] == _closed(n, ms[i], rs[i]), (count, i)
    W = nat.PUB_WAVE_MAX
    for count in (W, W + 1):
        ms, rs = _pairs(n, count, rng)
        ct = _encrypt(dk, ms, rs)
        for i in (0, 1, 2, 3, count // 2, count - 1):
            assert ct[i] == _closed(n, ms[i], rs[i]), (count, i)


def test_both_shapes_agree():
    from xfl_amd import _native as nat
    n = _fixture_n()
    dk = nat.DeviceKey(2048, n, None, None, None, device=0)
    W = nat.PUB_WAVE_MAX
    ms, rs = _pairs(n, W + 1, random.Random(7))
    mw, rw = nat.ints_to_words(ms, dk.nw), nat.ints_to_words(rs, dk.rand_words)
    alone = dk.encrypt_words(mw[:W], rw[:W])
    head = dk.encrypt_words(mw, rw)[:W]
    assert np.array_equal(alone, head)


def _launches(name):
    from xfl_amd import _native as nat
    tot, cnt = ctypes.c_double(), ctypes.c_int64()
    nat.check(nat.lib().xhe_profile_read(name.encode(), ctypes.byref(tot), ctypes.byref(cnt)))
    return cnt.value


def test_dispatch_by_batch_size():
    """Fails without the feature: small public non-DJN batches run
    k_nodjn_pub_wave, exactly one launch a call."""
    from xfl_amd import _native as nat
    L = nat.lib()
    n = _fixture_n()
    dk = nat.DeviceKey(2048, n, None, None, None, device=0)
    W = nat.PUB_WAVE_MAX
    rng = random.Random(11)
    ms, rs = _pairs(n, W + 1, rng)
    try:
        for count, want in ((15, 1), (W, 1), (W + 1, 0)):
            L.xhe_profile(1)
            _encrypt(dk, ms[:count], rs[:count])
            assert _launches("k_nodjn_pub_wave") == want, count
            assert _launches("k_nodjn_pub") == 1 - want, count
        k = load_fixture("paillier_2048_djn.json")["key"]
        nd, h = hx(k["n"]), hx(k["h_pow_n"])
        djn = nat.DeviceKey(2048, nd, None, None, h, device=0)
        L.xhe_profile(1)
        _encrypt(djn, [m % nd for m in ms[:15]], [r % 2 ** djn.rand_bits for r in rs[:15]])
        assert _launches("k_nodjn_pub_wave") == 0
    finally:
        L.xhe_profile(0)


def test_dropin_public_encrypt_private_decrypt():
    """Paillier.encrypt with the public key (what the regression operators do
    with B, 1 or D elements a batch), decrypted with the private key."""
    from xfl_amd import _native as nat
    from xfl_amd.paillier import Paillier, PaillierContext
    k = load_fixture(FX)["key"]
    priv = PaillierContext().init(hx(k["p"]), hx(k["q"]))
    pub = priv.to_public()
    assert not pub.is_private()
    ok = O.derive_private(hx(k["p"]), hx(k["q"]))
    x = (np.random.default_rng(15).standard_normal(15) * 3).astype(np.float32)
    x[0], x[1] = 0.0, -1.5
    L = nat.lib()
    L.xhe_profile(1)
    try:
        enc = Paillier.encrypt(pub, x, precision=7, obfuscation=True)
        assert _launches("k_nodjn_pub_wave") == 1
    finally:
        L.xhe_profile(0)
    got = Paillier.decrypt(priv, enc)
    want = []
    for v in x:
        m, e = O.encode_element(ok, v.item(), 7)
        want.append(O.decode_float32(ok, m, e))
    assert np.asarray(got, dtype=np.float64).tolist() == want
