"""The log sum of k_djn_pmd as a carry chain (pdigit_dev.hpp PMD::lam_add: one
v_add_co / v_addc_co per word, the carry in vcc and, between the blocks of the
chain, in a scalar pair): xhe_encrypt word for word against the oracle's
DJN-CRT encryption (oracle.paillier_oracle.encrypt_m on the same m and a).

A carry chain only shows a fault when carries run long, and the log digits of
random rows rarely make them. Keys: the golden 2048-bit DJN key and the
structured key `bottom` (an n of 2047 bits, the largest R/P), each at window 16
and at 7 | XHE_WIN_SPLIT (146 windows: the longest sum). Batches of 65, 2,113
and 16,449 elements, for which the library itself picks 16, 4 and 1 lanes per
element (xhe.hip pmd_split: the lane-group tree adds whole sums through the same
chain); each is a prefix of the same 16,449 (m, a) pairs, so the three must
agree on their common elements.

Draws: exponents whose digits are all equal in a layout (digit 1, 2 and the
largest that fits every window of that layout, for both layouts: the sum is
then that of nwin rows of one index), a = 2^rand_bits - 1 and a = 1, each with
the plaintexts 0 and n - 1 - sixteen edge elements, as runs that start at
element 0, end at element 63 and end at the last element of the two larger
batches, each run rotated by one; the rest seeded random. Every edge element
and a seeded sample of 64 elements per batch are compared with the oracle
(computed once per key: the ciphertext does not depend on the table layout).
"""
import random

import numpy as np
import pytest

from tests import structured_keys as SK
from tests.conftest import hx, load_fixture

pytestmark = pytest.mark.gpu

SIZES = (65, 2113, 16449)  # 16, 4 and 1 lanes per element
KEYS = ("golden", "bottom")
WINS = ("16", "7s")
NEDGE = 16


def _key(name):
    if name == "golden":
        k = load_fixture("paillier_2048_djn.json")["key"]
        return hx(k["p"]), hx(k["q"]), hx(k["h_pow_n"])
    k = SK.key(2048, name)
    return k.p, k.q, k.h


def _equal_digits(rb, spec):
    """exponents below 2^rb whose digits in the layout `spec` are all d, for d = 1, 2 and the largest d that fits
    the narrowest window"""
    from xfl_amd import _native as nat
    wb = nat.parse_win(spec)
    w = wb & 0xFF
    nwin, nwide = nat.win_layout(rb, wb)
    bits, bit = [], 0
    for i in range(nwin):
        width = min(w + (1 if i < nwide else 0), rb - bit)
        bits.append((bit, width))
        bit += width
    assert bit == rb
    dmax = (1 << min(width for _, width in bits)) - 1
    out = [sum(d << b for b, _ in bits) for d in (1, 2, dmax)]
    assert all(0 < x < 1 << rb for x in out)
    return out


def _runs():
    """first elements of the edge runs: [0, 16), [48, 64) and the last sixteen of the larger batches"""
    return [0, 64 - NEDGE] + [s - NEDGE for s in SIZES[1:]]


_cases = {}


def _case(name):
    """m, a (integers), the checked elements per batch and the oracle's ciphertexts of all of them"""
    if name in _cases:
        return _cases[name]
    from oracle import paillier_oracle as O
    p, q, h = _key(name)
    n = p * q
    rb = n.bit_length() // 2
    rng = random.Random(f"lam-carry-{name}")
    total = SIZES[-1]
    m = [rng.randrange(n) for _ in range(total)]
    a = [rng.randrange(1, 1 << rb) for _ in range(total)]
    exps = [1, (1 << rb) - 1] + [x for spec in WINS for x in _equal_digits(rb, spec)]
    edges = [(x, mi) for x in exps for mi in (0, n - 1)]
    assert len(edges) == NEDGE
    edge_at = set()
    for r, first in enumerate(_runs()):
        for j in range(NEDGE):
            a[first + j], m[first + j] = edges[(j + r) % NEDGE]
            edge_at.add(first + j)
    checked = {}
    for s in SIZES:
        sample = random.Random(f"sample-{name}-{s}").sample(range(s), 64)
        checked[s] = sorted({i for i in edge_at if i < s} | set(sample))
    okey = O.derive_private(p, q, h)
    want = {i: O.encrypt_m(okey, m[i], a[i]) for i in sorted(set().union(*checked.values()))}
    _cases[name] = (p, q, h, rb, m, a, checked, want)
    return _cases[name]


@pytest.mark.parametrize("win", WINS)
@pytest.mark.parametrize("name", KEYS)
def test_long_carries_match_oracle(name, win):
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
