"""What xhe_rand draws, bit for bit against the ChaCha20 stream contract
("Obfuscation draws: the stream contract"; reference
tests/chacha_ref.py, pinned to RFC 8439 by tests/test_chacha_ref.py).

Every other test that calls xhe_rand reads the draws back and hands them to
the oracle as given: they show that encryption is right for whatever was
drawn, not that the draws are the stream's. The paths no real key reaches
(the DJN zero-draw redraw, 64 rejections) are in the rand_selftest harness,
tests/test_gpu_native_selftests.py."""
import functools
import threading

import numpy as np
import pytest

from tests import chacha_ref as R
from tests.conftest import FIXTURES, hx, load_fixture

gpu = pytest.mark.gpu

SEED = bytes(range(1, 33))  # no symmetry between the key words
NONCE = 0x0123456789ABCDEF  # a non-zero high word
COUNT = 333  # DJN: 2-8 lanes per element, so 3-11 blocks of 256 threads with a ragged last one; non-DJN: 2 blocks
FILL = -1515870811  # 0xA5A5A5A5 as int32


def _dkey(fx, private=True, djn=True):
    from xfl_amd._native import DeviceKey
    g = load_fixture(fx)
    k = g["key"]
    h = hx(k["h_pow_n"]) if djn and k["djn_on"] else None
    if private:
        return DeviceKey(g["key_bits"], hx(k["n"]), hx(k["p"]), hx(k["q"]), h)
    return DeviceKey(g["key_bits"], hx(k["n"]), None, None, h)


def _rand(dk, seed, nonce, count, out=None, status=True):
    """xhe_rand into `out` (a fresh tensor when None): (words uint32 [count, rand_words], statuses or None)."""
    import torch

    from xfl_amd import _native as nat
    if out is None:
        out = torch.full((count, dk.rand_words), FILL, dtype=torch.int32, device="cuda")
    st = torch.full((count,), FILL, dtype=torch.int32, device="cuda") if status else None
    nat.check(nat.lib().xhe_rand(dk.handle, seed, nonce, count, out.data_ptr(), st.data_ptr() if status else None,
                                 torch.cuda.current_stream().cuda_stream), "rand")
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32), (st.cpu().numpy() if status else None)


@functools.lru_cache(maxsize=None)
def _ref(words, bits, bound, count=COUNT, seed=SEED, nonce=NONCE):
    """chacha_ref.draw for elements 0..count-1, computed once per shape."""
    return tuple(R.draw(seed, nonce, i, words, bits, bound) for i in range(count))


def _ref_words(ref, words):
    from xfl_amd._native import ints_to_words
    return ints_to_words([v for v, _, _ in ref], words)


def _mismatch(got, want):
    rows = np.flatnonzero((got != want).any(axis=1))
    return f"{rows.size} rows differ, first {rows[:8].tolist()}"


@gpu
@pytest.mark.parametrize("fx", FIXTURES)
def test_rand_matches_reference(fx):
    """Private keys of all five fixtures, 333 elements: every word of every
    draw and every status. blocks = 2, 3, 4, 8 with tpe = 2, 4, 4, 8 (3072
    bits: one idle lane per group); 2047- and 3071-bit n give a 31-bit top
    word (rand_bits 1023 and 1535); 2048_nodjn takes k_rand_below with n as
    the bound."""
    dk = _dkey(fx)
    n = hx(load_fixture(fx)["key"]["n"])
    if dk.djn:
        assert (dk.rand_bits, dk.rand_words) == (n.bit_length() // 2, -(-(n.bit_length() // 2) // 32))
    else:
        assert (dk.rand_bits, dk.rand_words) == (n.bit_length(), -(-n.bit_length() // 32))
    ref = _ref(dk.rand_words, dk.rand_bits, None if dk.djn else n)
    assert all(st == 0 for _, _, st in ref)
    got, st = _rand(dk, SEED, NONCE, COUNT)
    want = _ref_words(ref, dk.rand_words)
    assert np.array_equal(got, want), _mismatch(got, want)
    assert not st.any()


def test_fixtures_cover_the_31_bit_top_word():
    """A condition on the fixtures, not on the kernel: two of them have an n
    one bit short, so their DJN draws end in a 31-bit word."""
    bits = sorted(hx(load_fixture(fx)["key"]["n"]).bit_length() // 2 for fx in FIXTURES if "nodjn" not in fx)
    assert 1023 in bits and 1535 in bits and 2048 in bits


@gpu
def test_rand_rfc8439_known_answer_on_device():
    """All-zero seed, nonce 0, the 4096-bit DJN key (rand_bits = 2048: nothing
    masked): words 0-15 of element 0 are the keystream of RFC 8439 A.1 test
    vector 1, taken from the RFC's text and not from the Python reference."""
    from tests.test_chacha_ref import RFC_A1_1
    dk = _dkey("paillier_4096_djn.json")
    assert (dk.rand_bits, dk.rand_words) == (2048, 64)
    got, st = _rand(dk, bytes(32), 0, 2)
    assert got[0, :16].astype("<u4").tobytes() == RFC_A1_1
    assert not st.any()


NODJN_PUB = ["paillier_2048_nodjn.json", "paillier_4096_djn.json", "paillier_8192_djn.json"]


def _nodjn_ref(fx):
    n = hx(load_fixture(fx)["key"]["n"])
    return n, _ref(-(-n.bit_length() // 32), n.bit_length(), n)


@pytest.mark.parametrize("fx", NODJN_PUB)
def test_nodjn_inputs_reach_the_redraw_path(fx):
    """A condition on SEED/NONCE and the three moduli (acceptance rates
    n / 2^bitlen = 0.690, 0.720, 0.662), on the reference alone: at least 60 of
    the 333 elements are accepted at attempt >= 1 and at least one at >= 3."""
    _, ref = _nodjn_ref(fx)
    attempts = [t for _, t, _ in ref]
    assert sum(t >= 1 for t in attempts) >= 60, attempts
    assert max(attempts) >= 3, attempts


@gpu
@pytest.mark.parametrize("fx", NODJN_PUB)
def test_rand_nodjn_rejection(fx):
    """Public keys without h (r in [1, n), the remote party's mode): draws and
    statuses equal the reference where a third of the elements redraw."""
    n, ref = _nodjn_ref(fx)
    dk = _dkey(fx, private=False, djn=False)
    assert not dk.djn and not dk.private
    assert (dk.rand_bits, dk.rand_words) == (n.bit_length(), -(-n.bit_length() // 32))
    got, st = _rand(dk, SEED, NONCE, COUNT)
    want = _ref_words(ref, dk.rand_words)
    assert np.array_equal(got, want), _mismatch(got, want)
    assert st.tolist() == [s for _, _, s in ref] and not st.any()
    assert all(0 < v < n for v, _, _ in ref)


@gpu
def test_rand_call_shapes():
    """2048-bit DJN key: no status array, an output 4 bytes off 16-byte
    alignment (the scalar-store branch; nothing written outside the range),
    count = 1 and count = 0."""
    import torch

    from xfl_amd import _native as nat
    dk = _dkey("paillier_2048_djn.json")
    rw = dk.rand_words
    want = _ref_words(_ref(rw, dk.rand_bits, None), rw)
    got, st = _rand(dk, SEED, NONCE, COUNT)
    assert np.array_equal(got, want) and not st.any()
    # status_dev = NULL
    got, st = _rand(dk, SEED, NONCE, COUNT, status=False)
    assert st is None and np.array_equal(got, want), _mismatch(got, want)
    # a slice of a larger int32 tensor starting one word in
    tail = 37
    big = torch.full((1 + COUNT * rw + tail,), FILL, dtype=torch.int32, device="cuda")
    assert big.data_ptr() % 16 == 0
    sl = big[1:1 + COUNT * rw].view(COUNT, rw)
    assert sl.data_ptr() % 16 == 4
    got, st = _rand(dk, SEED, NONCE, COUNT, out=sl)
    assert np.array_equal(got, want), _mismatch(got, want)
    assert not st.any()
    host = big.cpu().numpy()
    assert host[0] == FILL and (host[1 + COUNT * rw:] == FILL).all()
    # count = 1
    got, st = _rand(dk, SEED, NONCE, 1)
    assert np.array_equal(got, want[:1]) and st.tolist() == [0]
    # count = 0: XHE_OK, nothing written (with buffers and without)
    buf = torch.full((4, rw), FILL, dtype=torch.int32, device="cuda")
    stt = torch.full((4,), FILL, dtype=torch.int32, device="cuda")
    strm = torch.cuda.current_stream().cuda_stream
    assert nat.lib().xhe_rand(dk.handle, SEED, NONCE, 0, buf.data_ptr(), stt.data_ptr(), strm) == nat.XHE_OK
    assert nat.lib().xhe_rand(dk.handle, SEED, NONCE, 0, None, None, strm) == nat.XHE_OK
    torch.cuda.synchronize()
    assert (buf == FILL).all().item() and (stt == FILL).all().item()


DEEP_COUNT = (1 << 25) + 64
DEEP_ROWS = (0, (1 << 18) - 1, 1 << 18, (1 << 25) - 1, 1 << 25, (1 << 25) + 63)


@gpu
def test_rand_deep_stream_positions():
    """2^25 + 64 draws of the 2048-bit DJN key (a 4.3 GB buffer, freed here):
    at i = 2^25 the block counter i*64*2 reaches 2^32 and the word index
    i*32 passes 2^30, the smallest batch at which a 32-bit counter or index
    would wrap and repeat draws. Row 2^18 is the first row of the host
    pipeline's second chunk: with test_host_encrypt_chunking_is_invisible
    (chunked == one-shot) this pins rand_impl's base offset to the
    reference."""
    import torch
    dk = _dkey("paillier_2048_djn.json")
    rw = dk.rand_words
    assert rw == 32
    free = torch.cuda.mem_get_info()[0]
    assert free > DEEP_COUNT * rw * 4 + (1 << 30), f"{free} bytes free"
    out = torch.zeros((DEEP_COUNT, rw), dtype=torch.int32, device="cuda")
    try:
        from xfl_amd import _native as nat
        nat.check(nat.lib().xhe_rand(dk.handle, SEED, NONCE, DEEP_COUNT, out.data_ptr(), None,
                                     torch.cuda.current_stream().cuda_stream), "rand")
        torch.cuda.synchronize()
        rows = np.stack([out[i].cpu().numpy() for i in DEEP_ROWS]).view(np.uint32)  # one 128-byte copy per row
    finally:
        del out
        torch.cuda.empty_cache()
    ref = [R.draw(SEED, NONCE, i, rw, dk.rand_bits) for i in DEEP_ROWS]
    assert all(t == 0 and st == 0 for _, t, st in ref)
    want = _ref_words(ref, rw)
    bad = [i for k, i in enumerate(DEEP_ROWS) if not np.array_equal(rows[k], want[k])]
    assert not bad, f"rows {bad} differ from the reference"
    assert len({r.tobytes() for r in rows}) == len(DEEP_ROWS)


@gpu
def test_dropin_obfuscation_is_fresh_per_call():
    """Two Paillier.encrypt calls of 512 zeros with obfuscation (2048-bit DJN
    private context): 1024 pairwise distinct ciphertexts that all decrypt to
    0 - every element and every call gets its own draw."""
    from tests import dropin_cases as C
    from xfl_amd.paillier import Paillier
    ctx, _ = C.ctxs(load_fixture("paillier_2048_djn.json"))
    z = np.zeros(512)
    c1 = Paillier.encrypt(ctx, z, precision=7, obfuscation=True)
    c2 = Paillier.encrypt(ctx, z, precision=7, obfuscation=True)
    raws = C.raw(c1)[0] + C.raw(c2)[0]
    assert len(raws) == 1024 and len(set(raws)) == 1024
    assert np.array_equal(Paillier.decrypt(ctx, c1), z) and np.array_equal(Paillier.decrypt(ctx, c2), z)


def test_seed_allocation_is_thread_safe():
    """ops._seed() from 8 threads, 1000 calls each: 32-byte seeds, none
    repeated, and all nonces distinct."""
    from xfl_amd.paillier import ops
    got = [[] for _ in range(8)]
    start = threading.Barrier(8)

    def work(k):
        start.wait()
        got[k] = [ops._seed() for _ in range(1000)]

    ts = [threading.Thread(target=work, args=(k,)) for k in range(8)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    flat = [x for g in got for x in g]
    assert len(flat) == 8000
    assert all(isinstance(s, bytes) and len(s) == 32 for s, _ in flat)
    assert len({s for s, _ in flat}) == 8000
    nonces = [n for _, n in flat]
    assert len(set(nonces)) == 8000 and all(isinstance(n, int) and 0 <= n < 1 << 64 for n in nonces)
