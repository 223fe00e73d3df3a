"""Device-resident PaillierArray (xfl_amd/paillier/resident.py): results of
batched operations stay in HBM and chain without PCIe round trips; the host
copy appears only on host access. Every result is compared bit for bit with
the host-buffer path ($XHE_RESIDENT=0) on the same inputs, and that path is
pinned to the reference's golden vectors by tests/test_gpu_dropin.py. A
received array whose values reach above n^2 goes through the same operations
against the oracle on the unreduced integers."""
import math
import random

import numpy as np
import pytest

from tests import dropin_cases as C
from tests.conftest import load_fixture

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def keys():
    return C.ctxs(load_fixture("paillier_2048_djn.json"))


def _host_mode(monkeypatch, on):
    if on:
        monkeypatch.setenv("XHE_RESIDENT", "0")
    else:
        monkeypatch.delenv("XHE_RESIDENT", raising=False)


def _words(a):
    return np.asarray(a.words).copy(), a.exponents.copy()


def test_chain_stays_in_hbm(keys):
    """encrypt -> + -> * -> sum -> matmul -> decrypt: no host copy is made of
    any intermediate, and the decrypted values are the plaintext results"""
    from xfl_amd.paillier import Paillier
    priv, _ = keys
    rng = np.random.default_rng(3)
    x = (rng.random(4096) * 20 - 10).astype(np.float32)
    y = (rng.random(4096) * 20 - 10).astype(np.float32)
    cx, cy = Paillier.encrypt(priv, x, precision=7), Paillier.encrypt(priv, y, precision=7)
    assert cx.is_resident and cx._st.h is None
    s = cx + cy
    m = s * 0.5
    assert s.is_resident and m.is_resident and s._st.h is None and m._st.h is None
    assert np.all(np.abs(Paillier.decrypt(priv, m) - (x + y) * 0.5) < 1e-3)
    X = rng.random((4096, 3))
    mv = cx @ X
    assert mv.is_resident and cx._st.h is None
    assert np.allclose(Paillier.decrypt(priv, mv), x.astype(np.float64) @ X, atol=1e-2)
    tot = np.sum(cx.reshape(64, 64), axis=1)
    assert tot.is_resident
    assert np.allclose(Paillier.decrypt(priv, tot), x.astype(np.float64).reshape(64, 64).sum(axis=1), atol=1e-3)
    assert cx._st.h is None  # nothing above needed the words on the host


def test_resident_equals_host_path(keys, monkeypatch):
    """deterministic encryptions and every batched op: identical words and
    exponents in both modes (mixed exponents, negative scalars, inversions)"""
    from xfl_amd.paillier import Paillier
    priv, pub = keys
    rng = np.random.default_rng(5)
    x = rng.standard_normal(300) * 100
    k = rng.standard_normal(300)
    X = rng.standard_normal((300, 4))
    res = {}
    for host in (True, False):
        _host_mode(monkeypatch, host)
        a = Paillier.encrypt(pub, x, precision=None, obfuscation=False)
        b = Paillier.encrypt(pub, x[::-1].copy(), precision=7, obfuscation=False)
        assert a.is_resident != host
        outs = [a, b, a + b, a - b, a * k, b * -3, a / 7.0, 2.5 - a, a @ X, X.T @ b, np.sum(a.reshape(20, 15), axis=0),
                np.concatenate([a[:10], b[5:9]]), a.reshape(15, 20).T, a[[3, 3, 1]]]
        res[host] = [_words(o) for o in outs]
        res[host].append(_words(Paillier.encrypt(pub, np.arange(-5, 5), obfuscation=False)))
    _host_mode(monkeypatch, False)
    for i, (h, d) in enumerate(zip(res[True], res[False])):
        assert np.array_equal(h[0], d[0]) and np.array_equal(h[1], d[1]), i


def test_views_assignment_and_obfuscate(keys):
    """slices share the storage; assignment goes to the host copy and drops
    the stale device copy; obfuscating a view re-randomises only its rows"""
    from xfl_amd.paillier import Paillier
    priv, _ = keys
    x = np.arange(16, dtype=np.float64) - 8
    c = Paillier.encrypt(priv, x, precision=7)
    v = c[2:6]
    v[0] = c[9]
    assert c[2].raw_ciphertext == c[9].raw_ciphertext
    assert not c.is_resident  # the host copy was written
    want = x.copy()
    want[2] = x[9]
    assert np.allclose(Paillier.decrypt(priv, c + c), 2 * want, atol=1e-5)
    c.to_device()
    before = np.asarray(c.words).copy()
    c._st.h = None
    Paillier.obfuscate(c[4:8])
    after = np.asarray(c.words)
    assert np.array_equal(before[:4], after[:4]) and np.array_equal(before[8:], after[8:])
    assert not np.any(np.all(before[4:8] == after[4:8], axis=1))
    assert np.allclose(Paillier.decrypt(priv, c), want, atol=1e-5)


def test_serialize_resident(keys):
    """serialize downloads lazily and writes the same bytes as the host copy"""
    from xfl_amd.paillier import Paillier, PaillierArray
    priv, _ = keys
    c = Paillier.encrypt(priv, np.linspace(-3, 3, 257), precision=7)
    assert c._st.h is None
    wire = Paillier.serialize(c, compression=False)
    host = PaillierArray.from_buffers(priv, np.asarray(c.words).copy(), c.exponents.copy(), c.shape)
    assert wire == Paillier.serialize(host, compression=False)
    back = Paillier.ciphertext_from(priv, wire, compression=False)
    assert not back.is_resident
    assert np.allclose(Paillier.decrypt(priv, back), np.linspace(-3, 3, 257), atol=1e-6)


def test_received_values_above_n_square(keys, monkeypatch):
    """A payload in the library's own wire layout whose values are mixed from
    tests/wide_cases.py (three in four at or above n^2, up to 2^4096 - 1; the
    codec rejects only wider ones), decoded into HBM: enc + enc, enc * float
    of both signs, np.sum, np.matmul, pack_ciphertexts and Paillier.decrypt
    give the oracle's results for the unreduced integers, word for word, and
    the untouched array serializes back to the bytes it came from."""
    from oracle import paillier_oracle as O
    from tests import wide_cases as W
    from tests.conftest import hx
    from tests.matmul_cases import oracle_matmul
    from tests.pack_cases import pack_ref
    from xfl_amd import _native as nat
    from xfl_amd.paillier import Paillier, wire
    from xfl_amd.paillier_acceleration import pack_ciphertexts
    priv, pub = keys
    key = load_fixture("paillier_2048_djn.json")["key"]
    ok = O.derive_private(hx(key["p"]), hx(key["q"]), hx(key["h_pow_n"]))
    n, n2, n2w, d = ok["n"], ok["n_square"], 128, 32
    assert pub.n == n
    rng = random.Random("received")
    low = [1, n2 - 1, n + 1]
    while len(low) < d // 4:
        c = rng.randrange(2, n2)
        if math.gcd(c, n) == 1:
            low.append(c)
    distinct = W.mixed(W.units_wide(n, n2w, d - d // 4, rng), low)
    assert max(distinct) >= (1 << 4096) - 2 and sum(c >= n2 for c in distinct) == 24
    count = 330  # the 16-lane shapes; neighbouring rows differ
    vals = [distinct[(i + 7) % d] for i in range(count)]
    exps = [(-24, -53, -60, 0)[(i * 5 + i // 32) % 4] for i in range(count)]
    monkeypatch.setattr(wire, "DEV_DECODE_MIN", 1)

    def receive(values, exponents):
        blob = wire.encode_words(nat.ints_to_words(values, n2w), np.asarray(exponents, dtype=np.int32), (len(values),),
                                 compression=False)
        back = Paillier.ciphertext_from(pub, blob, compression=False)
        assert back.is_resident and back._st.h is None
        return blob, back

    def raws(a):
        w, e = _words(a)
        return nat.words_to_ints(w), e.tolist()

    blob, enc = receive(vals, exps)
    _, other = receive(vals[::-1], exps[3:] + exps[:3])
    got = raws(enc + other)
    want = [O.add_ct(ok, a, ea, b, eb) for a, ea, b, eb in zip(vals, exps, vals[::-1], exps[3:] + exps[:3])]
    assert got == ([w[0] for w in want], [w[1] for w in want])
    for scalar in (0.5, -1.75):
        got = raws(enc * scalar)
        once = {(c, e): O.mul_ct(ok, c, e, scalar) for c, e in set(zip(vals, exps))}
        want = [once[(c, e)] for c, e in zip(vals, exps)]
        assert got == ([w[0] for w in want], [w[1] for w in want]), scalar
    got = raws(np.sum(enc.reshape(10, 33), axis=1))
    want = [O.sum_ct(ok, vals[33 * r:33 * r + 33], exps[33 * r:33 * r + 33]) for r in range(10)]
    assert got == ([w[0] for w in want], [w[1] for w in want])
    X = (np.random.default_rng(4).standard_normal((40, 3)) * 8).astype(np.float32)
    X[0, 0], X[5, 1], X[39, 2] = -1.0, 0.0, 3.0
    got = raws(np.matmul(enc[:40], X))
    want = oracle_matmul(ok, vals[:40], exps[:40], (1, 40), X, "left")
    assert got == ([w[0] for w in want], [w[1] for w in want])
    assert enc._st.h is None  # nothing above needed the words on the host
    # decrypt at exponent 0 with out_origin: exact integers. An arbitrary residue's plaintext lies anywhere in
    # [0, n); those between the sign bounds raise in the reference's decode and are left out
    inrange = []
    for c in distinct:
        try:
            inrange.append((c, O.decode_origin(ok, O.decrypt_raw(ok, c), 0)))
        except OverflowError:
            pass
    assert sum(c >= n2 for c, _ in inrange) >= 8
    dvals = [inrange[(i + 3) % len(inrange)] for i in range(70)]
    _, denc = receive([c for c, _ in dvals], [0] * 70)
    assert list(Paillier.decrypt(priv, denc, out_origin=True)) == [v for _, v in dvals]
    # genuine ciphertexts moved up by multiples of n^2 decrypt to their plaintexts
    x = np.linspace(-3, 3, 64)
    sent = Paillier.encrypt(pub, x, precision=7)
    qm = W.q_max(n, n2w)
    sr, se = raws(sent)
    moved = [c + (qm - 1 - i % 2) * n2 for i, c in enumerate(sr)]
    assert qm >= 3 and max(moved) < 1 << 4096
    _, twin = receive(moved, se)
    plain = Paillier.decrypt(priv, twin)
    assert np.array_equal(plain, Paillier.decrypt(priv, sent)) and np.allclose(plain, x, atol=1e-6)
    # pack: exponent 0 throughout, k = 7 slots of 128 bits, a short last group
    _, flat = receive(vals, [0] * count)
    packed = pack_ciphertexts(flat, num=1, interval=1 << 128, k=7)
    assert packed.is_resident
    assert raws(packed) == (pack_ref(vals, 7, 128, n2), [0] * 48)
    # pass-through: the bytes of the untouched array are the received ones, unreduced
    assert Paillier.serialize(enc, compression=False) == blob
    assert nat.words_to_ints(np.asarray(enc.words)) == vals and max(vals) >= n2
