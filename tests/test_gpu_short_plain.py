"""k_djn_pmd's short-plaintext entry (pdigit_dev.hpp "Short plaintexts") and
its exit through the digits: xhe_encrypt word for word against the oracle's
DJN-CRT encryption (oracle.paillier_oracle.encrypt_m on the same m and a).

A plaintext is short when m < B = 2^112 or 0 < n - m < B; a wave takes the
short entry only when every plaintext of its prologue lanes is short, so the
batch is laid out in runs of 64 elements (one wave at one lane per element,
four at four lanes, sixteen at sixteen):

  [0, 64)     short, signs alternating, with 0, 1, 2, B - 1, n - 1, n - 2 and
              n - B + 1 among them
  [64, 128)   short except element 81, a general one: a mixed wave at one lane
              per element, and at four lanes the wave of elements [80, 96)
  [128, 192)  the general boundary values B, n - B, n, n + 1, 2^2048 - 1, P, Q
              between short ones
  [192, 256)  all short positive
  [256, 320)  all short negative
  the rest    runs of 64, all short (random sign and length) or all general,
              three to one
  and the last element of each batch is short negative: the one-lane wave at
  the end of each batch takes the short path.

Keys: the golden 2048-bit DJN key and the structured keys `bottom` and
`mixed_swapped`, at window 16 and at 7 | XHE_WIN_SPLIT. Batches of 65, 2,113 and
16,449 elements (16, 4 and 1 lanes per element), each a prefix of the same (m,
a) list, so the three lane splits must agree on shared elements. The edge
elements' exponents cycle through a = 1, a = 2^rand_bits - 1 and an a with a
run of 40 zero bits. Compared with the oracle (computed once per key): every
element of [0, 320), each batch's last element and a seeded sample of 64 per
batch.
"""
import random

import numpy as np
import pytest

from tests import structured_keys as SK
from tests.conftest import hx, load_fixture

pytestmark = pytest.mark.gpu

SIZES = (65, 2113, 16449)  # 16, 4 and 1 lanes per element
KEYS = ("golden", "bottom", "mixed_swapped")
WINS = ("16", "7s")
B = 1 << 112
HEAD = 320


def _key(name):
    if name == "golden":
        k = load_fixture("paillier_2048_djn.json")["key"]
        return hx(k["p"]), hx(k["q"]), hx(k["h_pow_n"])
    k = SK.key(2048, name)
    return k.p, k.q, k.h


def _is_short(m, n):
    return m < B or 0 < n - m < B


def _short(rng, n, neg=None):
    """a short plaintext of random length (1..111 bits) and, unless given, random sign"""
    bits = rng.randrange(1, 112)
    s = rng.getrandbits(bits) | (1 << (bits - 1))
    neg = rng.random() < 0.5 if neg is None else neg
    return n - s if neg else s


_cases = {}


def _case(name):
    """m, a (integers), the checked elements per batch and the oracle's ciphertexts of all of them"""
    if name in _cases:
        return _cases[name]
    from oracle import paillier_oracle as O
    p, q, h = _key(name)
    n = p * q
    rb = n.bit_length() // 2
    rng = random.Random(f"short-plain-{name}")
    total = SIZES[-1]
    m = [0] * total
    a = [rng.randrange(1, 1 << rb) for _ in range(total)]
    # [0, 64): short, signs alternating, the short edge values among them
    for i in range(64):
        m[i] = _short(rng, n, neg=bool(i & 1))
    short_edges = [0, 1, 2, B - 1, n - 1, n - 2, n - B + 1]
    for j, v in enumerate(short_edges):
        m[3 + 8 * j] = v  # 3, 11, ..., 51
    # [64, 128): short except element 81
    for i in range(64, 128):
        m[i] = _short(rng, n)
    m[64] = n - (rng.getrandbits(27) | 1)  # the last element of the smallest batch: short negative
    m[81] = rng.getrandbits(2048)
    # [128, 192): the general boundary values between short ones
    general_edges = [B, n - B, n, n + 1, (1 << 2048) - 1, p, q]
    for i in range(128, 192):
        m[i] = _short(rng, n)
    for j, v in enumerate(general_edges):
        m[130 + 8 * j] = v
    for i in range(192, 256):
        m[i] = _short(rng, n, neg=False)
    for i in range(256, 320):
        m[i] = _short(rng, n, neg=True)
    # the rest: runs of 64, three short to one general
    for first in range(HEAD, total, 64):
        general = (first // 64) % 4 == 3
        for i in range(first, min(first + 64, total)):
            m[i] = rng.getrandbits(2048) if general else _short(rng, n)
    for s in SIZES:
        m[s - 1] = n - (rng.getrandbits(rng.randrange(1, 112)) | 1)
    assert all(_is_short(x, n) for x in m[:64]) and all(_is_short(m[i], n) == (i != 81) for i in range(64, 128))
    assert all(_is_short(x, n) for x in short_edges) and not any(_is_short(x, n) for x in general_edges)
    assert all(_is_short(m[i], n) != (i in range(130, 186, 8)) for i in range(128, 192))
    assert all(m[i] < B for i in range(192, 256)) and all(0 < n - m[i] < B for i in range(256, 320))
    assert all(0 < n - m[s - 1] < B for s in SIZES) and all(0 <= x < 1 << 2048 for x in m)
    # exponents of the edge elements
    zero = (rng.getrandbits(rb) | 1) & ~(((1 << 40) - 1) << 500)
    special = [1, (1 << rb) - 1, zero]
    edge_at = [3 + 8 * j for j in range(7)] + [64, 81] + [130 + 8 * j for j in range(7)] + [s - 1 for s in SIZES]
    for r, i in enumerate(edge_at):
        a[i] = special[r % 3]
    checked = {}
    for s in SIZES:
        sample = random.Random(f"short-sample-{name}-{s}").sample(range(s), 64)
        checked[s] = sorted(set(range(min(HEAD, s))) | {s - 1} | set(sample))
    okey = O.derive_private(p, q, h)
    want = {i: O.encrypt_m(okey, m[i], a[i]) for i in sorted(set().union(*checked.values()))}
    _cases[name] = (p, q, h, rb, m, a, checked, want)
    return _cases[name]


@pytest.mark.parametrize("win", WINS)
@pytest.mark.parametrize("name", KEYS)
def test_encrypt_matches_oracle(name, win):
    from xfl_amd import _native as nat
    p, q, h, rb, m, a, checked, want = _case(name)
    dk = nat.DeviceKey(2048, p * q, p, q, h, device=0, win_bits=nat.parse_win(win))
    assert dk.rand_bits == rb
    mw, aw = nat.ints_to_words(m, dk.nw), nat.ints_to_words(a, dk.rand_words)
    got = {s: dk.encrypt_words(mw[:s], aw[:s]) for s in SIZES}
    for s in SIZES:
        ints = nat.words_to_ints(got[s][checked[s]])
        bad = [i for i, c in zip(checked[s], ints) if c != want[i]]
        assert not bad, f"{name} win {win} n {s}: {len(bad)} of {len(checked[s])} checked ciphertexts differ, first {bad[:8]}"
    # the lane splits agree on the elements they share
    assert np.array_equal(got[65], got[2113][:65]) and np.array_equal(got[2113], got[16449][:2113])
