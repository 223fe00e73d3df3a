"""Device packing / unpacking of SecureBoost grad/hess plaintexts
(xhe_embed_f64, xhe_umbed, embed_packed -> Paillier.encrypt, decrypt_umbed)
against the reference's golden vectors and the oracle restatement of
paillier_acceleration.py, bit for bit."""
import ctypes

import numpy as np
import pytest

from oracle import paillier_oracle as O
from tests import dropin_cases as C
from tests.conftest import FIXTURES, fl, hx, load_fixture

pytestmark = pytest.mark.gpu

EDGE = [0.0, -0.0, 0.5, -0.5, 2.0 ** -70, -(2.0 ** -64), 1 - 2.0 ** -53, 5e-324]
GEOMETRIES = [(1, 128, 64), (2, 128, 64), (3, 128, 64), (10, 128, 64), (2, 64, 32)]
DJN = "paillier_2048_djn.json"


def _dkey(g, private=True):
    from xfl_amd._native import DeviceKey
    k = g["key"]
    h = hx(k["h_pow_n"]) if k["djn_on"] else None
    if private:
        return DeviceKey(g["key_bits"], hx(k["n"]), hx(k["p"]), hx(k["q"]), h)
    return DeviceKey(g["key_bits"], hx(k["n"]), None, None, h)


@pytest.fixture(scope="module")
def djn():
    g = load_fixture(DJN)
    return g, _dkey(g), hx(g["key"]["n"])


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def embed_dev(dk, cols, ib, p):
    """xhe_embed_f64 on device buffers -> (m words [count, nw], status)"""
    import torch

    from xfl_amd import _native as nat
    cols = np.ascontiguousarray(cols, dtype=np.float64)
    k, count = cols.shape
    cd = torch.from_numpy(cols).cuda()
    m = torch.empty((count, dk.nw), dtype=torch.int32, device="cuda")
    st = torch.empty(count, dtype=torch.int32, device="cuda")
    nat.check(nat.lib().xhe_embed_f64(dk.handle, cd.data_ptr(), k, count, ib, p, m.data_ptr(), st.data_ptr(),
                                      _stream()), "embed")
    torch.cuda.synchronize()
    return m.cpu().numpy().view(np.uint32), st.cpu().numpy()


def umbed_dev(dk, mw, num, ib, p, decrypt=False):
    """xhe_umbed (behind xhe_decrypt of ciphertext words when `decrypt`) on
    device buffers -> (f64 [num, count], f32 [num, count], status)"""
    import torch

    from xfl_amd import _native as nat
    L = nat.lib()
    mw = np.ascontiguousarray(mw, dtype=np.uint32)
    count = mw.shape[0]
    md = torch.from_numpy(mw.view(np.int32).copy()).cuda()
    if decrypt:
        ct, md = md, torch.empty((count, dk.nw), dtype=torch.int32, device="cuda")
        nat.check(L.xhe_decrypt(dk.handle, ct.data_ptr(), count, md.data_ptr(), _stream()), "decrypt")
    f64 = torch.empty((num, count), dtype=torch.float64, device="cuda")
    f32 = torch.empty((num, count), dtype=torch.float32, device="cuda")
    st = torch.empty(count, dtype=torch.int32, device="cuda")
    nat.check(L.xhe_umbed(dk.handle, md.data_ptr(), count, num, ib, p, f64.data_ptr(), f32.data_ptr(), st.data_ptr(),
                          _stream()), "umbed")
    torch.cuda.synchronize()
    return f64.cpu().numpy(), f32.cpu().numpy(), st.cpu().numpy()


def _values(seed, k, count, ib):
    """(rand - 0.5) * 2^s, s in [-70, 20], with the edge values spread over
    the columns; scaled by 2^-10 for 64-bit slots"""
    rng = np.random.default_rng(seed)
    v = (rng.random((k, count)) - 0.5) * np.exp2(rng.integers(-70, 21, size=(k, count)))
    for j in range(k):
        m = min(len(EDGE), count)
        v[j, rng.permutation(count)[:m]] = np.roll(EDGE, j)[:m]
    return v * 2.0 ** -10 if ib == 64 else v


def _bits32(cols):
    return [np.array(c, dtype=np.float32).view(np.uint32) for c in cols]


def _assert_umbed(got_f32, got_f64, vs, num, ib, p):
    want = O.umbed_ref(vs, num, 1 << ib, p)
    for j in range(num):
        assert np.array_equal(got_f32[j].view(np.uint32), _bits32(want)[j]), j
    if got_f64 is not None:
        for i, v in enumerate(vs):
            assert [float(x) for x in got_f64[:, i]] == O.unpack_ref(v, num, 1 << ib, p), i


# ---------------------------------------------------------------- 1. golden
@pytest.mark.parametrize("fx", FIXTURES)
def test_golden_packed(fx):
    from xfl_amd._native import ints_to_words, words_to_ints
    g = load_fixture(fx)
    c = g["encrypt"]["priv_packed_p0"]
    n = hx(g["key"]["n"])
    dk = _dkey(g, private=c["private"])
    ins = [hx(v) for v in c["input"]]
    cols = np.array([[fl(v) for v in c["g"]], [fl(v) for v in c["h"]]])
    m, st = embed_dev(dk, cols, 128, 64)
    assert not st.any()
    assert words_to_ints(m) == [v % n for v in ins]
    rw = ints_to_words([hx(r) for r in c["rand"]], dk.rand_words) if c["obfuscation"] else None
    raw = dk.encrypt_words(m, rw)
    assert words_to_ints(raw) == [hx(r) for r in c["raw"]]
    f64, f32, st = umbed_dev(dk if c["private"] else _dkey(g), raw, 2, 128, 64, decrypt=True)
    assert not st.any()
    _assert_umbed(f32, f64, ins, 2, 128, 64)


# ---------------------------------------------------------------- 2. shapes
@pytest.mark.parametrize("geom", GEOMETRIES)
@pytest.mark.parametrize("count", [1, 63, 64, 65, 257])
def test_embed_shapes(djn, count, geom):
    from xfl_amd._native import words_to_ints
    _, dk, n = djn
    k, ib, p = geom
    cols = _values(count * 100 + k, k, count, ib)
    m, st = embed_dev(dk, cols, ib, p)
    assert not st.any()
    assert words_to_ints(m) == [x % n for x in O.embed_ref(list(cols), 1 << ib, p)]


# ---------------------------------------------------------------- 3. unpacking
@pytest.mark.parametrize("geom", GEOMETRIES)
def test_umbed_values(djn, geom):
    from xfl_amd._native import ints_to_words
    _, dk, n = djn
    k, ib, p = geom
    B = 1 << ib
    packed = O.embed_ref(list(_values(7 + k, k, 65, ib)), B, p)
    sums = [sum(packed[:t]) for t in range(1, len(packed) + 1, 5)]  # what a histogram bin holds
    crafted = [B // 2, B // 2 + 1, -(B // 2), B - 1, -1]
    if k > 1:  # the same digits in the upper slots, where they carry into the next one
        crafted += [(B // 2) * B + B // 2 + 1, (B - 1) * B + (B - 1), -(B // 2) * B - B // 2 - 1]
    vs = packed + [-v for v in packed] + sums + crafted
    f64, f32, st = umbed_dev(dk, ints_to_words([v % n for v in vs], dk.nw), k, ib, p)
    assert not st.any()
    _assert_umbed(f32, f64, vs, k, ib, p)


def test_umbed_decode_overflow(djn):
    """max_pos < m < min_neg is status 1 for that element only"""
    from xfl_amd._native import ints_to_words
    _, dk, n = djn
    maxpos = n // 3
    ms = [5, maxpos, maxpos + 1, n - maxpos - 1, n - maxpos, n - 1]
    f64, f32, st = umbed_dev(dk, ints_to_words(ms, dk.nw), 2, 128, 64)
    assert st.tolist() == [0, 0, 1, 1, 0, 0]
    ok = [0, 1, 4, 5]
    vs = [ms[i] if ms[i] <= maxpos else ms[i] - n for i in ok]
    _assert_umbed(f32[:, ok], f64[:, ok], vs, 2, 128, 64)
    assert not f64[:, [2, 3]].any()


# ---------------------------------------------------------------- 4. status 4 and the fallback
@pytest.mark.parametrize("geom", [(2, 128, 64), (2, 64, 32)])
def test_slot_overflow_status_and_fallback(djn, geom, monkeypatch):
    from xfl_amd._native import words_to_ints
    from xfl_amd.paillier import Paillier
    from xfl_amd.paillier_acceleration import embed, embed_packed
    g, dk, n = djn
    k, ib, p = geom
    cols = _values(11, k, 70, ib)
    cols[1, 37] = 2.0 ** (ib - p)  # int(v * 2^p) = 2^ib: past its slot
    cols[0, 5] = -(2.0 ** (ib - p - 1))  # |t| = 2^(ib - 1): the first value that does not fit
    cols[0, 6] = 2.0 ** (ib - p - 1) * (1 - 2.0 ** -53)  # the last one that does
    m, st = embed_dev(dk, cols, ib, p)
    want_st = np.zeros(70, dtype=np.int32)
    want_st[[5, 37]] = 4
    assert st.tolist() == want_st.tolist()
    assert not m[[5, 37]].any()
    ok = np.nonzero(want_st == 0)[0]
    assert words_to_ints(m[ok]) == [x % n for x in O.embed_ref(list(cols[:, ok]), 1 << ib, p)]
    priv, pub = C.ctxs(g)
    want = Paillier.encrypt(pub, embed(list(cols), 1 << ib, p), precision=0, obfuscation=False)
    for host in (False, True):
        if host:
            monkeypatch.setenv("XHE_RESIDENT", "0")
        got = Paillier.encrypt(pub, embed_packed(list(cols), 1 << ib, p), precision=0, obfuscation=False)
        assert np.array_equal(got.words, want.words) and np.array_equal(got.exponents, want.exponents)


# ---------------------------------------------------------------- 5. drop-in
def _dropin_cols(count=257):
    v = _values(21, 2, count, 128)
    v[1] = np.abs(v[1]) + 2.0 ** -20  # hessians
    return list(v)


@pytest.mark.parametrize("host", [False, True])
@pytest.mark.parametrize("fx", [DJN, "paillier_2048_nodjn.json"])
def test_encrypt_packed_equals_embed_path(fx, host, monkeypatch):
    from xfl_amd.paillier import Paillier
    from xfl_amd.paillier_acceleration import embed, embed_packed
    if host:
        monkeypatch.setenv("XHE_RESIDENT", "0")
    else:
        monkeypatch.delenv("XHE_RESIDENT", raising=False)
    priv, pub = C.ctxs(load_fixture(fx))
    cols = _dropin_cols()
    ints = O.embed_ref(cols)
    for ctx in (priv, pub):
        for kw in (dict(precision=0), dict(precision=None), dict(precision=0, max_exponent=3)):
            want = Paillier.encrypt(ctx, embed(cols), obfuscation=False, **kw)
            got = Paillier.encrypt(ctx, embed_packed(cols), obfuscation=False, **kw)
            assert got.is_resident != host and got.shape == want.shape == (257,)
            assert np.array_equal(got.words, want.words) and np.array_equal(got.exponents, want.exponents)
        # a negative max_exponent moves the exponent: the existing path, the same answer
        want = Paillier.encrypt(ctx, embed(cols)[:9], precision=0, max_exponent=-2, obfuscation=False)
        got = Paillier.encrypt(ctx, embed_packed(cols)[:9], precision=0, max_exponent=-2, obfuscation=False)
        assert np.array_equal(got.words, want.words) and np.array_equal(got.exponents, want.exponents)
        # obfuscated: the same plaintexts
        enc = Paillier.encrypt(ctx, embed_packed(cols), precision=0, obfuscation=True)
        assert enc.is_resident != host
        assert [int(v) for v in Paillier.decrypt(priv, enc, out_origin=True)] == ints
        back = Paillier.ciphertext_from(ctx, Paillier.serialize(enc, compression=False), compression=False)
        assert np.array_equal(back.words, enc.words) and np.array_equal(back.exponents, enc.exponents)


def test_encrypt_packed_serialize_pipeline():
    """a packed encryption of pipeline size carries the bit lengths its
    serialize lays the payload out from, and the bytes are the host path's"""
    from xfl_amd.paillier import Paillier, wire
    from xfl_amd.paillier_acceleration import embed, embed_packed
    _, pub = C.ctxs(load_fixture(DJN))
    n = wire.PIPE_MIN + 3
    cols = _dropin_cols(n)
    enc = Paillier.encrypt(pub, embed_packed(cols), precision=0, obfuscation=False)
    assert enc.is_resident and enc._st.h is None and enc._st.d._xhe_bits.shape == (n,)
    got = Paillier.serialize(enc, compression=False)
    sl = slice(n - 300, n)  # the reference path on the tail (one Python pass per element), the codec on all rows
    want = Paillier.encrypt(pub, embed([c[sl] for c in cols]), precision=0, obfuscation=False)
    assert np.array_equal(enc.words[sl], want.words) and not enc.exponents.any()
    assert got == wire.encode_words(enc.words, enc.exponents, enc.shape)


# ---------------------------------------------------------------- 6. histogram round trip
def test_histogram_round_trip(monkeypatch):
    import pandas as pd

    from xfl_amd.paillier import Paillier, PaillierArray
    from xfl_amd.paillier_acceleration import decrypt_umbed, embed_packed, umbed
    priv, pub = C.ctxs(load_fixture(DJN))
    n, nbins = 4096, 16
    rng = np.random.default_rng(9)
    cols = [rng.random(n) - 0.5, rng.random(n) * 0.25]
    bins = [rng.integers(0, nbins, n), (np.arange(n) * 7) % nbins]
    ints = O.embed_ref(cols)
    enc = Paillier.encrypt(pub, embed_packed(cols), precision=0, obfuscation=True)
    assert enc.is_resident
    data = pd.DataFrame(enc, columns=["xfl_grad_hess"])
    for f, b in enumerate(bins):
        sums = [sum(ints[i] for i in np.nonzero(b == k)[0]) for k in range(nbins)]
        want = _bits32(O.umbed_ref(sums, 2))
        if f == 0:  # pandas groupby (decision_tree_trainer.py:151-160)
            data["bin"] = b
            hist = data.groupby(["bin"])["xfl_grad_hess"].agg(["sum"])["sum"].array
            assert isinstance(hist, PaillierArray)
        else:  # np.sum per bin, an object array of ciphertexts
            hist = np.array([np.sum(enc[np.nonzero(b == k)[0]]) for k in range(nbins)], dtype=object)
        got = decrypt_umbed(priv, hist, 2)
        two_step = umbed(Paillier.decrypt(priv, hist, out_origin=True), 2)
        host_copy = PaillierArray(hist).astype(object) if f == 0 else hist
        monkeypatch.setenv("XHE_RESIDENT", "0")
        host = decrypt_umbed(priv, PaillierArray(host_copy), 2)  # host words, no resident device
        monkeypatch.delenv("XHE_RESIDENT")
        for res in (got, host):
            assert len(res) == 2 and all(isinstance(r, np.ndarray) and r.dtype == np.float32 for r in res)
            for j in range(2):
                assert np.array_equal(res[j].view(np.uint32), want[j])
                assert np.array_equal(res[j].view(np.uint32), _bits32(two_step)[j])
    with pytest.raises(TypeError, match="public key"):
        decrypt_umbed(pub, hist, 2)
    # a sum past the decode range raises as Paillier.decrypt does
    big = Paillier.encrypt(pub, np.array([int(priv.n) // 3 + 1, 7], dtype=object), precision=0, obfuscation=False)
    with pytest.raises(OverflowError, match="Overflow detected during decoding encrypted number."):
        decrypt_umbed(priv, big, 2)
    # nonzero exponents and a geometry the device does not unpack: the two-step path, the same floats
    odd = Paillier.encrypt(pub, np.array([1.5, -2.25]), precision=None, obfuscation=False)
    for arr, kw in ((odd, {}), (hist, dict(interval=10 ** 38))):
        want2 = umbed(Paillier.decrypt(priv, arr, out_origin=True), 2, **kw)
        got2 = decrypt_umbed(priv, arr, 2, **kw)
        for j in range(2):
            assert np.array_equal(got2[j].view(np.uint32), _bits32(want2)[j])


# ---------------------------------------------------------------- 7. host entry points
def test_host_entry_points(djn):
    from xfl_amd import _native as nat
    g, dk, n = djn
    L = nat.lib()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    count = 65
    for k, ib, p in ((2, 128, 64), (3, 128, 64), (2, 64, 32)):
        cols = np.ascontiguousarray(_values(31 + k, k, count, ib))
        cols[k - 1, 40] = 2.0 ** (ib - p)  # one status 4
        m = np.empty((count, dk.nw), np.uint32)
        st = np.empty(count, np.int32)
        nat.check(L.xhe_embed_f64_host(dk.handle, vp(cols), k, count, ib, p, vp(m), vp(st)), "embed host")
        m_dev, st_dev = embed_dev(dk, cols, ib, p)
        assert np.array_equal(m, m_dev) and np.array_equal(st, st_dev) and st[40] == 4 and st.sum() == 4
        ct = dk.encrypt_words(m, None)
        f64 = np.empty((k, count), np.float64)
        f32 = np.empty((k, count), np.float32)
        nat.check(L.xhe_decrypt_umbed_host(dk.handle, vp(ct), count, k, ib, p, vp(f64), vp(f32), vp(st)), "umbed host")
        f64_dev, f32_dev, st_dev = umbed_dev(dk, ct, k, ib, p, decrypt=True)
        assert np.array_equal(f64.view(np.uint64), f64_dev.view(np.uint64))
        assert np.array_equal(f32.view(np.uint32), f32_dev.view(np.uint32)) and np.array_equal(st, st_dev)
        ok = [i for i in range(count) if i != 40]
        _assert_umbed(f32[:, ok], f64[:, ok], O.embed_ref(list(cols[:, ok]), 1 << ib, p), k, ib, p)
    # geometry outside the ABI's conditions is EINVAL for every entry point
    cols = np.zeros((17, 4))
    m = np.empty((4, dk.nw), np.uint32)
    st = np.empty(4, np.int32)
    for k, ib, p in ((17, 128, 64), (2, 96 + 8, 64), (2, 32, 8), (2, 288, 64), (2, 128, 127), (2, 128, -1), (0, 128, 64)):
        assert L.xhe_embed_f64_host(dk.handle, vp(cols), k, 4, ib, p, vp(m), vp(st)) == nat.XHE_EINVAL, (k, ib, p)
        ct = np.zeros((4, dk.n2w), np.uint32)
        f64 = np.empty((17, 4), np.float64)
        f32 = np.empty((17, 4), np.float32)
        assert L.xhe_decrypt_umbed_host(dk.handle, vp(ct), 4, k, ib, p, vp(f64), vp(f32), vp(st)) == nat.XHE_EINVAL
