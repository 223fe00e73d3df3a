"""tests/chacha_ref.py, the reference the GPU draw tests compare with
(tests/test_gpu_rand.py, the rand_selftest harness): its block function
against the two block vectors RFC 8439 publishes, byte for byte, and `draw`
on cases that can be checked by hand (with the block function replaced by a
transparent one where the point is which counters and words a draw uses)."""
import pytest

from tests import chacha_ref as R

# RFC 8439 appendix A.1, test vector #1: key, counter and nonce all zero
RFC_A1_1 = bytes.fromhex(
    "76b8e0ada0f13d90405d6ae55386bd28"
    "bdd219b8a08ded1aa836efcc8b770dc7"
    "da41597c5157488d7724e03fb8d84a37"
    "6a43b8f41518a11cc387b669b2ee6586")

# RFC 8439 §2.3.2: key 00..1f, block counter 1, nonce 00:00:00:09:00:00:00:4a:00:00:00:00
RFC_2_3_2 = bytes.fromhex(
    "10f1e7e4d13b5915500fdd1fa32071c4"
    "c7d1f4c733c068030422aa9ac3d46c4e"
    "d2826446079faa0914c2d705d98b02a2"
    "b5129cd1de164eb9cbd083e8a2503c4e")

SEED = bytes(range(1, 33))
NONCE = 0x0123456789ABCDEF


def test_block_rfc8439_a1_vector1():
    assert len(RFC_A1_1) == 64
    assert R.serialize(R.block([0] * 8, 0, 0, 0, 0)) == RFC_A1_1


def test_block_rfc8439_2_3_2():
    assert len(RFC_2_3_2) == 64
    key8 = R.key_words(bytes(range(32)))
    assert key8[0] == 0x03020100 and key8[7] == 0x1F1E1D1C
    out = R.block(key8, 1, 0x09000000, 0x4A000000, 0)
    assert R.serialize(out) == RFC_2_3_2
    assert out[0] == 0xE4E7F110 and out[15] == 0x4E3C50A2  # the RFC's state dump after the block operation


def test_quarter_round_rfc8439_2_1_1():
    x = [0x11111111, 0x01020304, 0x9B8D6F43, 0x01234567]
    R._quarter_round(x, 0, 1, 2, 3)
    assert x == [0xEA2A92F4, 0xCB1CF8CE, 0x4581472E, 0x5881C4BB]


def test_bits_1_is_always_one():
    """One bit: the candidate is the stream's first bit, so about half the
    elements redraw and every accepted value is 1."""
    got = [R.draw(SEED, NONCE, i, 4, 1) for i in range(200)]
    assert all(v == 1 and st == 0 for v, _, st in got)
    for i, (_, t, _) in enumerate(got):
        assert [R.candidate(SEED, NONCE, i, u, 4, 1) for u in range(t + 1)] == [0] * t + [1]
    assert 60 <= sum(t > 0 for _, t, _ in got) <= 140


@pytest.fixture
def clear_block(monkeypatch):
    """block() replaced by one whose word u is (counter low 16 bits) << 16 |
    (0xFF00 + u) (never zero), recording the state words 12-15 of every call."""
    calls = []

    def fake(key8, w12, w13, w14, w15):
        calls.append((w12, w13, w14, w15))
        return [((w12 & 0xFFFF) << 16) | (0xFF00 + u) for u in range(16)]

    monkeypatch.setattr(R, "block", fake)
    return calls


def test_mask_at_a_non_multiple_of_32(clear_block):
    # words 0, 1 whole, word 2 keeps its low 6 bits: 0xFF02 & 0x3F = 0x02
    v, t, st = R.draw(SEED, NONCE, 0, 3, 70)
    assert (t, st) == (0, 0)
    assert v == 0x0000FF00 | (0x0000FF01 << 32) | (0x02 << 64)
    assert v < 1 << 70
    # 64 bits in 2 words: nothing masked; 33 bits: one bit of word 1
    assert R.draw(SEED, NONCE, 0, 2, 64)[0] == 0x0000FF00 | (0x0000FF01 << 32)
    assert R.draw(SEED, NONCE, 0, 2, 33)[0] == 0x0000FF00 | (1 << 32)


def test_mask_real_stream():
    full = R.candidate(SEED, NONCE, 5, 0, 3, 96)
    assert R.candidate(SEED, NONCE, 5, 0, 3, 70) == full & ((1 << 70) - 1)
    assert full >> 70  # the mask removes something


def test_words_in_stream_order(clear_block):
    """40 words = 3 blocks: word k of the draw is word k % 16 of block k // 16,
    and the third block's last 8 words are unused."""
    v, t, st = R.draw(SEED, NONCE, 7, 40, 1280)
    base = 7 * 64 * 3
    assert clear_block == [(base + b, 0, NONCE & 0xFFFFFFFF, NONCE >> 32) for b in range(3)]
    ws = [(v >> (32 * k)) & 0xFFFFFFFF for k in range(40)]
    assert ws == [(((base + k // 16) & 0xFFFF) << 16) | (0xFF00 + k % 16) for k in range(40)]
    assert v >> 1280 == 0


def test_bound_one_rejects_everything(clear_block):
    assert R.draw(SEED, NONCE, 3, 2, 40, bound=1) == (None, 64, 2)
    # all 64 attempts were made, each at its own counter
    assert [c[0] for c in clear_block] == [3 * 64 + t for t in range(64)]


def test_bound_is_exclusive_and_whole_value_compared(clear_block):
    v = 0x0000FF00 | (0x0000FF01 << 32)  # attempt 0 of element 0; attempt t adds t << 16 to both words
    assert R.draw(SEED, NONCE, 0, 2, 64, bound=v + 1)[:2] == (v, 0)
    # attempt 0 == bound: rejected, and every later attempt is larger
    assert R.draw(SEED, NONCE, 0, 2, 64, bound=v + (1 << 48) + 1)[:2] == (v, 0)
    assert R.draw(SEED, NONCE, 0, 2, 64, bound=v - 0xFF00 + 1) == (None, 64, 2)  # top words equal, low word decides
    assert R.draw(SEED, NONCE, 0, 2, 64, bound=v) == (None, 64, 2)


def test_attempt_1_counter(monkeypatch):
    """Attempt 1 of element i starts at block counter (i*64 + 1)*blocks; the
    64-bit counter carries into word 13."""
    calls = []

    def fake(key8, w12, w13, w14, w15):
        calls.append((w13 << 32) | w12)
        return [0] * 16 if len(calls) <= 3 else [1] * 16  # attempt 0 (3 blocks) draws zero

    monkeypatch.setattr(R, "block", fake)
    i = 12345
    assert R.draw(SEED, NONCE, i, 40, 1280)[1:] == (1, 0)
    assert calls == [(i * 64) * 3 + b for b in range(3)] + [(i * 64 + 1) * 3 + b for b in range(3)]
    assert R.counter(i, 1, 40) == (i * 64 + 1) * 3
    del calls[:]
    i = 1 << 25  # 32 words, 2 blocks: i*64*2 = 2^32
    R.draw(SEED, NONCE, i, 32, 1024)
    assert calls[0] == 1 << 32 and calls[1] == (1 << 32) + 1
    assert R.counter(i, 1, 32) == (1 << 32) + 2
