"""CPU: the operand sets of tests/wide_cases.py are what the GPU tests take them
for - not vacuous (most values at or above n^2, the largest one all ones,
q_max n^2 among them), every expected value different from what a kernel that
ignored an operand's top words would compute, and keys on both sides of the
number of subtractions an entry reduction needs."""
import math
import random

import pytest

from tests import wide_cases as W


def _sets(name):
    K, n, p, q, _ = W.key(name)
    n2w = 2 * K // 32
    d = W.DISTINCT[K]
    return K, n, p, q, n2w, d


@pytest.mark.parametrize("name", W.key_names())
def test_wide_is_not_vacuous(name):
    K, n, p, q, n2w, d = _sets(name)
    n2, top = n * n, 1 << (32 * n2w)
    qm = W.q_max(n, n2w)
    assert qm >= 1 and qm * n2 < top <= (qm + 1) * n2
    for dd in sorted({5, d}):
        ws = W.wide(n, n2w, dd, random.Random(name))
        assert len(ws) == len(set(ws)) == dd and all(0 <= x < top for x in ws)
        assert 4 * sum(x >= n2 for x in ws) >= 3 * dd
        assert max(ws) == top - 1 and qm * n2 in ws and n2 in ws
        assert any(x >= n2 and x not in W._fixed(n, n2w) for x in ws), "no random draw"
    ws = W.wide(n, n2w, d, random.Random(name))
    if d >= 16:  # the twins of 1, n + 1 and n^2 - 1 at the largest multiple that fits, and the values around it
        assert {u + qm * n2 for u in (1, n + 1) if u + qm * n2 < top} <= set(ws) and n2 - 1 + n2 in ws or qm == 1
        assert {x for x in (n2 + 1, qm * n2 - 1) if x >= n2} <= set(ws)
    us = W.units_wide(n, n2w, d, random.Random(name))
    assert len(set(us)) == d and all(math.gcd(c % n2, n) == 1 for c in us)
    assert 4 * sum(x >= n2 for x in us) >= 3 * d and max(us) < top
    assert max(us) >= top - 2 and any(x // n2 == qm for x in us)


@pytest.mark.parametrize("name", W.key_names())
def test_expected_differs_from_truncation(name):
    """a kernel that dropped the words above n^2's own, or took the operand as
    it stands, would not give the expected value for any wide operand"""
    K, n, p, q, n2w, d = _sets(name)
    n2 = n * n
    for x in W.wide(n, n2w, d, random.Random(name)) + W.units_wide(n, n2w, d, random.Random(name)):
        if x >= n2:
            assert x % n2 != W.truncated(x, n) and x % n2 != x, hex(x)


@pytest.mark.parametrize("name", W.key_names(private_only=True))
def test_non_units(name):
    K, n, p, q, n2w, d = _sets(name)
    n2 = n * n
    xs = W.non_units(n, p, q, n2w, d, random.Random(name))
    assert len(set(xs)) == d and all(x < 1 << (32 * n2w) for x in xs)
    assert all(math.gcd(x % n2, n) != 1 for x in xs)
    assert {0, n, n2} <= set(xs) and sum(x >= n2 for x in xs) >= d // 2 >= 2
    if d >= 16:
        assert {p, q, p * p, n2 - n} <= set(xs)


def test_keys_span_the_quotient():
    """computed from the keys: some need at most 4 subtractions of n^2, some 16 or more"""
    qs = {name: W.q_max(W.key(name)[1], 2 * W.key(name)[0] // 32) for name in W.key_names()}
    assert min(qs.values()) <= 4 and max(qs.values()) >= 16, qs
    assert any(4 < v < 16 for v in qs.values()), qs
    # every key size has a key of each kind it can have: full width (q_max <= 4) and one bit short
    for K in (2048, 3072, 4096):
        mine = [v for name, v in qs.items() if W.key(name)[0] == K]
        assert min(mine) <= 4 and max(mine) >= 5, (K, mine)


def test_mixed_interleaves():
    assert W.mixed([10, 11, 12], [1, 2]) == [10, 1, 11, 2, 12]
    assert W.mixed([10], [1, 2, 3]) == [10, 1, 2, 3]


@pytest.mark.parametrize("name", [name for name in W.key_names() if W.key(name)[0] == 2048])
def test_digit_model_takes_wide_operands(name):
    """the 2048-bit digit kernels' entry (k_ndig_in, pmdx_to_digits) in its
    integer model, tools/pdigit_model.py NDigits: x + ceil(R/n) n^2 reduces
    to t in [n, 2n + (x + n^2) / R] for x up to 2^4096 - 1 (the model asserts
    it, and that the digit t - n stays below 2n: R >= 2^13 n, so the excess is
    below n / 100 even at q_max = 63), the digits are those of x mod n^2, and
    a product of two wide operands comes out right and below n^2"""
    from tools.pdigit_model import Counter, NDigits
    K, n, p, q, n2w, d = _sets(name)
    n2 = n * n
    D = NDigits(n)
    assert D.R >= n << 13
    ws = W.wide(n, n2w, d, random.Random(name))
    ctr = Counter()
    for x, y in zip(ws, ws[1:] + ws[:1]):
        sx, sy = D.to_digits(x, ctr), D.to_digits(y, ctr)
        assert D.value(*sx) == x % n2
        assert D.from_digits(*D.mul(sx, sy, ctr), ctr) == x * y % n2
    assert ctr.max_col < 1 << 64
