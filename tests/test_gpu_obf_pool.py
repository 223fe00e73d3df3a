"""GPU: obfuscators made ahead of time (xhe_obf_fill), the one-launch online
encryption on them (xhe_encrypt_obf, k_enc_obf) and the pool behind
Paillier.encrypt / Paillier.obfuscate.

Every check is exact: golden ciphertexts word for word, Python integers for
arbitrary residues (the cases tests/test_obf_pool_host.py states on the CPU),
the oracle's float32 rounding for the drop-in.
"""
import ctypes

import numpy as np
import pytest

from oracle import paillier_oracle as O
from tests import obf_cases
from tests import structured_keys as SK
from tests.conftest import FIXTURES, hx, load_fixture
from tests.dropin_cases import ctxs, raw
from tests.test_gpu_parity import ENC_CASES, _okey
from tests.test_gpu_pub_small import _launches

pytestmark = pytest.mark.gpu

WIN = 8  # fixed-base tables that build in milliseconds
# the labels under which the encryption paths time their exponentiations
EXP_LABELS = ("k_djn_pmd", "k_djn_pmdx", "k_djn_pow", "k_djn_pow_lds", "k_djn_pub", "k_nodjn_crt", "k_nodjn_pub",
              "k_nodjn_pub_wave")
GROUPS_PER_BLOCK = {2048: 64, 3072: 64, 4096: 64, 8192: 16}  # 256 threads / lanes per element (4, 4, 4, 16)
OBF_CASES = [c for c in ENC_CASES if load_fixture(FIXTURES[0])["encrypt"][c]["obfuscation"]]


def _nat():
    from xfl_amd import _native as nat
    return nat


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint32)


def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


_keys = {}


def _dkey(fx, private):
    if (fx, private) not in _keys:
        g = load_fixture(fx)
        k = g["key"]
        h = hx(k["h_pow_n"]) if k["djn_on"] else None
        args = (hx(k["p"]), hx(k["q"])) if private else (None, None)
        _keys[(fx, private)] = _nat().DeviceKey(g["key_bits"], hx(k["n"]), *args, h, win_bits=WIN if h else 0)
    return _keys[(fx, private)]


def _fill(dk, rw):
    """xhe_obf_fill on host draws [n, rand_words] -> device obfuscators [n, n2w]"""
    import torch
    nat = _nat()
    n = rw.shape[0]
    obf = torch.empty((n, dk.n2w), dtype=torch.int32, device="cuda")
    rd = _dev(rw)
    nat.check(nat.lib().xhe_obf_fill(dk.handle, _p(rd), n, _p(obf), _stream()), "obf_fill")
    return obf


def _enc_obf(dk, md, obf, count, wipe, ct):
    nat = _nat()
    nat.check(nat.lib().xhe_encrypt_obf(dk.handle, _p(md), _p(obf), count, wipe, _p(ct), _stream()), "encrypt_obf")


@pytest.mark.parametrize("fx", FIXTURES)
def test_fill_then_online_equals_golden(fx):
    """every obfuscated golden case (private and public, DJN and not): the
    fill on the recorded draws is xhe_encrypt of m = 0, and the online
    encryption on it is the golden ciphertext word for word"""
    import torch
    nat = _nat()
    g = load_fixture(fx)
    ok = _okey(g)
    assert len(OBF_CASES) == 6
    for case in OBF_CASES:
        c = g["encrypt"][case]
        dk = _dkey(fx, c["private"])
        xs = [hx(v) for v in c["input"]] if c["kind"] == "int" else [float.fromhex(v) for v in c["input"]]
        ms = [O.encode_element(ok, x, c["precision"], c["max_exponent"])[0] for x in xs]
        rw = nat.ints_to_words([hx(r) for r in c["rand"]], dk.rand_words)
        obf = _fill(dk, rw)
        zero = np.zeros((len(ms), dk.nw), dtype=np.uint32)
        assert np.array_equal(_host(obf), dk.encrypt_words(zero, rw)), case
        ct = torch.empty((len(ms), dk.n2w), dtype=torch.int32, device="cuda")
        _enc_obf(dk, _dev(nat.ints_to_words(ms, dk.nw)), obf, len(ms), 1, ct)
        assert nat.words_to_ints(_host(ct)) == [hx(r) for r in c["raw"]], case
        assert not _host(obf).any(), case  # used once: wiped


@pytest.mark.parametrize("K,name", [(2048, "top"), (2048, "bottom"), (3072, "top"), (4096, "bottom"), (8192, "top")])
def test_arbitrary_residues(K, name):
    """xhe_encrypt_obf on any X < n^2 against (1 + n m) X mod n^2 in Python
    integers: the edge pairs of tests/obf_cases.py tiled to 1 element, one
    below and one above a 256-thread block's elements, and 3,000; wipe = 0
    leaves the obfuscators, wipe = 1 zeroes rows [0, count) and nothing else;
    nothing is written past row count of the output"""
    import torch
    nat = _nat()
    p, q = SK.pq(K, name)
    n = p * q
    assert n.bit_length() == K + SK.N_BITS[name]
    dk = nat.DeviceKey(K, n)  # the kernel reads n alone: a public non-DJN key builds no tables
    pairs = obf_cases.edge_pairs(n)
    want1 = nat.ints_to_words([(1 + n * m) * x % (n * n) for m, x in pairs], dk.n2w)
    m1 = nat.ints_to_words([m for m, _ in pairs], dk.nw)
    x1 = nat.ints_to_words([x for _, x in pairs], dk.n2w)
    gpb = GROUPS_PER_BLOCK[K]
    pad = 8
    for count in (1, gpb - 1, gpb + 1, 3000):
        reps = -(-(count + pad) // len(pairs))
        tile = lambda w: np.ascontiguousarray(np.tile(w, (reps, 1))[:count + pad])  # noqa: E731
        xw, want = tile(x1), tile(want1)[:count]
        md, obf = _dev(tile(m1)), _dev(xw)
        sentinel = np.full((count + pad, dk.n2w), 0x5A5A5A5A, dtype=np.uint32)
        for wipe in (0, 1):
            ct = _dev(sentinel)
            _enc_obf(dk, md, obf, count, wipe, ct)
            got = _host(ct)
            bad = np.nonzero(np.any(got[:count] != want, axis=1))[0]
            assert bad.size == 0, f"count {count} wipe {wipe}: rows {bad[:8].tolist()} differ (pair = row % {len(pairs)})"
            assert np.array_equal(got[count:], sentinel[count:]), (count, wipe)
            left = _host(obf)
            assert np.array_equal(left[count:], xw[count:]), (count, wipe)
            assert np.array_equal(left[:count], xw[:count]) if wipe == 0 else not left[:count].any(), (count, wipe)


def test_abi_errors():
    import torch
    nat = _nat()
    L = nat.lib()
    dk = _dkey(FIXTURES[0], False)
    m = torch.zeros((4, dk.nw), dtype=torch.int32, device="cuda")
    buf = torch.zeros((16, dk.n2w), dtype=torch.int32, device="cuda")  # obfuscators: rows 4..7
    s = _stream()
    row = 4 * dk.n2w  # bytes
    at = lambda off: ctypes.c_void_p(buf.data_ptr() + off)  # noqa: E731
    obf, apart = at(4 * row), at(8 * row)
    assert L.xhe_encrypt_obf(None, _p(m), obf, 4, 0, apart, s) == nat.XHE_EINVAL
    assert L.xhe_encrypt_obf(dk.handle, _p(m), obf, -1, 0, apart, s) == nat.XHE_EINVAL
    assert L.xhe_encrypt_obf(dk.handle, None, obf, 4, 0, apart, s) == nat.XHE_EINVAL
    # ct on the obfuscators, one row in, beginning at their last word, ending on their first word
    for off in (4 * row, 5 * row, 8 * row - 4, 4):
        assert L.xhe_encrypt_obf(dk.handle, _p(m), obf, 4, 0, at(off), s) == nat.XHE_EINVAL, off
    assert L.xhe_encrypt_obf(dk.handle, None, None, 0, 1, None, s) == nat.XHE_OK
    assert L.xhe_obf_fill(None, _p(m), 4, _p(buf), s) == nat.XHE_EINVAL
    assert L.xhe_obf_fill(dk.handle, _p(m), -1, _p(buf), s) == nat.XHE_EINVAL
    assert L.xhe_obf_fill(dk.handle, None, 0, None, s) == nat.XHE_OK
    torch.cuda.synchronize()
    assert not _host(buf).any()  # nothing was launched


class _Profile:
    def __enter__(self):
        _nat().lib().xhe_profile(1)
        return self

    def __exit__(self, *exc):
        _nat().lib().xhe_profile(0)


def _want_f32(g, xs):
    ok = _okey(g)
    return [O.decode_float32(ok, *O.encode_element(ok, float(x), 7)) for x in xs]


@pytest.mark.parametrize("private", [True, False], ids=["priv", "pub"])
def test_dropin_draws_from_the_pool(private):
    from xfl_amd.paillier import Paillier, resident
    g = load_fixture("paillier_2048_djn.json")
    priv, pub = ctxs(g)
    priv.set_device_window(WIN)
    ctx = priv if private else pub
    assert resident.device_for(ctx) is not None, "the drop-in is not in resident mode"
    rng = np.random.default_rng(11)
    x40, x80 = rng.standard_normal(40) * 50, rng.standard_normal(80) * 50
    # no pool: nothing changes
    with _Profile():
        c0 = Paillier.encrypt(ctx, x40, precision=7)
        assert _launches("k_enc_obf") == 0 and sum(_launches(k) for k in EXP_LABELS) >= 1
    assert ctx.obfuscators_available() == 0
    assert ctx.reserve_obfuscators(100) == 100 and ctx.obfuscators_available() == 100
    # a bad input raises as without a pool and takes nothing
    bad = x40.copy()
    bad[7] = np.nan
    with pytest.raises(ValueError):
        Paillier.encrypt(ctx, bad, precision=7)
    assert ctx.obfuscators_available() == 100
    with _Profile():
        c1 = Paillier.encrypt(ctx, x40, precision=7)
        assert _launches("k_enc_obf") == 1 and [k for k in EXP_LABELS if _launches(k)] == []
    assert ctx.obfuscators_available() == 60
    assert c1.is_resident and not hasattr(c1._dw(resident.device_for(ctx)), "_xhe_ready")
    assert Paillier.decrypt(priv, c1).tolist() == _want_f32(g, x40)
    assert Paillier.decrypt(priv, c0).tolist() == _want_f32(g, x40)
    assert set(raw(c0)[0]).isdisjoint(raw(c1)[0])  # the same values, encrypted twice
    with _Profile():
        c2 = Paillier.encrypt(ctx, x80, precision=7)
        assert _launches("k_enc_obf") == 1 and sum(_launches(k) for k in EXP_LABELS) >= 1  # 60 pooled, 20 direct
    assert ctx.obfuscators_available() == 0
    assert Paillier.decrypt(priv, c2).tolist() == _want_f32(g, x80)
    assert len(set(raw(c2)[0])) == 80
    # obfuscate on pool rows: every row changes, the values stay
    assert ctx.reserve_obfuscators(50) == 50
    before = raw(c2)[0]
    with _Profile():
        assert Paillier.obfuscate(c2) is c2
        assert _launches("k_enc_obf") == 0
    assert ctx.obfuscators_available() == 0  # 50 from the pool, 30 encrypted as before
    after = raw(c2)[0]
    assert all(a != b for a, b in zip(before, after))
    assert Paillier.decrypt(priv, c2).tolist() == _want_f32(g, x80)
    # integers go through the same pool
    assert ctx.reserve_obfuscators(10) == 10
    ints = np.arange(-3, 4, dtype=np.int64)
    ci = Paillier.encrypt(ctx, ints)
    assert ctx.obfuscators_available() == 3
    assert Paillier.decrypt(priv, ci, dtype="int").tolist() == ints.tolist()
    # a public copy has its own, empty pool; dropping leaves nothing
    assert priv.to_public().obfuscators_available() == 0 if private else True
    ctx.drop_obfuscators()
    assert ctx.obfuscators_available() == 0
    with _Profile():
        Paillier.encrypt(ctx, x40, precision=7)
        assert _launches("k_enc_obf") == 0


def test_pool_rows_are_wiped_and_capacity_is_clipped(monkeypatch):
    from xfl_amd.paillier import Paillier, resident
    g = load_fixture("paillier_2048_djn.json")
    _, pub = ctxs(g)
    dk = pub.device_key()
    monkeypatch.setenv("XHE_RESIDENT_MAX_BYTES", str(25 * 4 * dk.n2w + 100))
    assert pub.reserve_obfuscators(1000) == 25  # the budget of a resident batch
    monkeypatch.delenv("XHE_RESIDENT_MAX_BYTES")
    pool = resident.obf_pool(dk)
    assert pool.cap == 25 and _host(pool.rows).any(axis=1).all()
    Paillier.encrypt(pub, np.linspace(-1, 1, 10), precision=7)
    rows = _host(pool.rows)
    assert not rows[:10].any() and rows[10:].any(axis=1).all() and pub.obfuscators_available() == 15
    storage = pool.rows
    pub.drop_obfuscators()
    assert not _host(storage).any() and resident.obf_pool(dk) is None
