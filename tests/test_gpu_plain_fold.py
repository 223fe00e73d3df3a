"""k_djn_pmd with the plaintext folded into the log sum (pdigit_dev.hpp "The
plaintext as a logarithm"): xhe_encrypt word for word against the oracle's
DJN-CRT encryption (oracle.paillier_oracle.encrypt_m on the same m and a).

Keys: the golden 2048-bit DJN key and the structured keys `bottom` (an n of
2047 bits, the largest R/P) and `mixed_swapped` (p ~ q/2, p < q), each at
window 16 and at 7 | XHE_WIN_SPLIT (146 windows: the longest sum). Batches of
65, 2,113 and 16,449 elements, for which the library itself picks 16, 4 and 1
lanes per element (xhe.hip pmd_split); each is a prefix of the same 16,449 (m,
a) pairs, so the three must agree on their common elements.

Plaintexts: the edge list 0, 1, 2, n - 1, n - 2, P, Q, k P, k Q, 2^1024,
2^2048 - 1 and a random one, as runs of twelve that start at element 0, end at
element 63, start at element 64 and end at the last element of the two larger
batches - each run rotated by one, so elements 0, 63, 64 and the last carry
different edges; the rest seeded random below 2^2048. The edge elements'
exponents cycle through a = 1, a = 2^rand_bits - 1, an a with a run of 40 zero
bits (whole windows of both layouts) and a random one; the rest are random.
Every edge element and a seeded sample of 64 elements per batch are compared
with the oracle (computed once per key: the ciphertext does not depend on the
table layout).
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
NEDGE = 12


def _key(name):
    if name == "golden":
        k = load_fixture("paillier_2048_djn.json")["key"]
        return hx(k["p"]), hx(k["q"]), hx(k["h_pow_n"])
    k = SK.key(2048, name)
    return k.p, k.q, k.h


def _runs():
    """first elements of the edge runs: [0, 12), [52, 64), [64, 76) and the last twelve of the larger batches"""
    return [0, 64 - NEDGE, 64] + [s - NEDGE for s in SIZES[1:]]


_cases = {}


def _case(name):
    """m, a (integers), the checked elements per batch and the oracle's ciphertexts of all of them"""
    if name in _cases:
        return _cases[name]
    from oracle import paillier_oracle as O
    p, q, h = _key(name)
    n = p * q
    rb = n.bit_length() // 2
    rng = random.Random(f"plain-fold-{name}")
    total = SIZES[-1]
    m = [rng.getrandbits(2048) for _ in range(total)]
    a = [rng.randrange(1, 1 << rb) for _ in range(total)]
    edges = [0, 1, 2, n - 1, n - 2, p, q, rng.randrange(2, q) * p, rng.randrange(2, p) * q, 1 << 1024, (1 << 2048) - 1,
             rng.getrandbits(2048)]
    assert len(edges) == NEDGE and all(0 <= x < 1 << 2048 for x in edges)
    zero = (rng.getrandbits(rb) | 1) & ~(((1 << 40) - 1) << 500)
    special = [1, (1 << rb) - 1, zero]
    edge_at = set()
    for r, first in enumerate(_runs()):
        for j in range(NEDGE):
            m[first + j] = edges[(j + r) % NEDGE]
            if (j + r) % 4 < 3:
                a[first + j] = special[(j + r) % 4]
            edge_at.add(first + j)
    checked = {}
    for s in SIZES:
        sample = random.Random(f"sample-{name}-{s}").sample(range(s), 64)
        checked[s] = sorted({i for i in edge_at if i < s} | set(sample))
        assert {0, s - 1} <= set(checked[s]) and (s < 64 or 63 in checked[s])
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
