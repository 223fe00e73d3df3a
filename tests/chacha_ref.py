"""Plain-Python reference of the obfuscation draw stream (DESIGN.md,
"Obfuscation draws: the stream contract"), written from that contract and
from RFC 8439 §2.1-2.3, with Python ints only. tests/test_chacha_ref.py pins
`block` to the RFC's published vectors; the GPU tests compare the kernels
with `draw` bit for bit.

Block function: ChaCha20, 20 rounds, original layout (64-bit counter in words
12-13, 64-bit nonce in words 14-15). Draw: element i (its position in the
stream), attempt t in 0..63, blocks = ceil(words/16) uses the counters
(i*64 + t)*blocks + b, b < blocks; the keystream words in order are the
little-endian words of the draw, the first `words` of them masked to `bits`.
The draw is the first attempt that is non-zero and, with a bound, < bound."""

M32 = 0xFFFFFFFF
SIGMA = tuple(int.from_bytes(b"expand 32-byte k"[4 * j:4 * j + 4], "little") for j in range(4))
ATTEMPTS = 64
ST_OK, ST_VALUE = 0, 2


def _rotl(v, c):
    return ((v << c) & M32) | (v >> (32 - c))


def _quarter_round(x, a, b, c, d):
    # RFC 8439 §2.1
    x[a] = (x[a] + x[b]) & M32
    x[d] = _rotl(x[d] ^ x[a], 16)
    x[c] = (x[c] + x[d]) & M32
    x[b] = _rotl(x[b] ^ x[c], 12)
    x[a] = (x[a] + x[b]) & M32
    x[d] = _rotl(x[d] ^ x[a], 8)
    x[c] = (x[c] + x[d]) & M32
    x[b] = _rotl(x[b] ^ x[c], 7)


def block(key8, w12, w13, w14, w15):
    """The 16 output words of one ChaCha20 block: state words 4-11 = key8,
    12-15 as given (RFC 8439 §2.3: ten double rounds, then the input state is
    added)."""
    init = list(SIGMA) + [int(k) & M32 for k in key8] + [w12 & M32, w13 & M32, w14 & M32, w15 & M32]
    assert len(init) == 16
    x = list(init)
    for _ in range(10):
        for col in range(4):  # column rounds
            _quarter_round(x, col, 4 + col, 8 + col, 12 + col)
        for dg in range(4):  # diagonal rounds
            _quarter_round(x, dg, 4 + (dg + 1) % 4, 8 + (dg + 2) % 4, 12 + (dg + 3) % 4)
    return [(a + b) & M32 for a, b in zip(x, init)]


def serialize(ws):
    """The block's words as the RFC prints them: little-endian bytes."""
    return b"".join(w.to_bytes(4, "little") for w in ws)


def key_words(seed32):
    assert len(seed32) == 32
    return [int.from_bytes(seed32[4 * j:4 * j + 4], "little") for j in range(8)]


def counter(i, attempt, words, b=0):
    """Block counter of keystream block b of attempt `attempt` of element i."""
    blocks = -(-words // 16)
    return (i * ATTEMPTS + attempt) * blocks + b


def candidate(seed32, nonce, i, attempt, words, bits):
    """Attempt `attempt` of element i before acceptance: an int < 2^bits."""
    key8 = key_words(seed32)
    blocks = -(-words // 16)
    stream = b""
    for b in range(blocks):
        ctr = counter(i, attempt, words, b)
        stream += serialize(block(key8, ctr & M32, ctr >> 32, nonce & M32, nonce >> 32))
    return int.from_bytes(stream[:4 * words], "little") & ((1 << bits) - 1)


def draw(seed32, nonce, i, words, bits, bound=None):
    """(value, attempt, 0) for the first attempt whose candidate is in
    [1, 2^bits) and, with a bound, in [1, bound); (None, 64, 2) when all 64
    attempts fail."""
    assert 0 < bits <= 32 * words
    for t in range(ATTEMPTS):
        v = candidate(seed32, nonce, i, t, words, bits)
        if v != 0 and (bound is None or v < bound):
            return v, t, ST_OK
    return None, ATTEMPTS, ST_VALUE
