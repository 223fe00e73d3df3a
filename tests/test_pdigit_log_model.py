"""The fixed-base row product with an additive second digit (pdigit_dev.hpp
"Additive second digit", k_djn_pmd; limb model tools/pdigit_model.py
LogDigits): state (a, c, Lhat) times row (e, lhat) is the 4 K^2 product on
(a, c) and Lhat + lhat, and the finish c_f = c + REDC(a Lhat) gives the pair
(a, c_f) of the same residue, R a + P c_f = x R^2 (mod P^2). Checked against
Python integers over chains of 44, 63 and 85 products (45, 64 and 86 windows:
windows 23, 16 and 12 of a 1024-bit exponent) for ten seeded 1024-bit moduli,
with the rows y = 1, y = P^2 - 1, e = 1 and e = P - 1 in every chain; the
columns stay below 2^63 and the unreduced sum below 2^1056. The rows' log
digits come without a per-row inversion from the chains of the inverse base
(k_tab_to_pmd): checked around the high/low split of the digit. CPU, pure
Python."""
import random

import pytest

from tools.pdigit_model import Counter, InverseBaseTable, LogDigits, random_prime_like, unit

K = 37
CHAINS = (44, 63, 85)


def _special_rows(D, rng):
    """units with the named first digits: y = 1, y = P^2 - 1, e = 1 (y = R^-1
    mod P), e = P - 1 (y = -R^-1 mod P), the last two with a random high digit"""
    P, P2 = D.P, D.P * D.P
    rinv = pow(D.R, -1, P)
    ys = [1, P2 - 1, rinv, rinv + P * rng.randrange(P), (P - rinv) + P * rng.randrange(P), P - rinv]
    for y, e in zip(ys[2:], (1, 1, P - 1, P - 1)):
        assert D.to_form(y)[0] == e
    return ys


@pytest.mark.parametrize("seed", range(10))
def test_row_product_chains(seed):
    rng = random.Random(1000 + seed)
    P = random_prime_like(1024, rng)
    D = LogDigits(P)
    assert D.k == K and D.LW == 33
    P2 = P * P
    ys = [unit(rng, P, P2) for _ in range(CHAINS[-1] + 1)]
    special = _special_rows(D, rng)
    # the named rows inside the shortest chain, one of them as the start value
    slots = rng.sample(range(1, CHAINS[0]), len(special) - 1)
    ys[0] = special[seed % len(special)]
    for s, y in zip(slots, special[:seed % len(special)] + special[seed % len(special) + 1:]):
        ys[s] = y
    st = D.start(D.row_direct(ys[0]))
    acc = ys[0]
    worst = 0
    for i, y in enumerate(ys[1:], 1):
        ctr = Counter()
        st = D.mul_row(st, D.row_direct(y), ctr)
        acc = acc * y % P2
        assert ctr.mads == 4 * K * K
        worst = max(worst, ctr.max_col)
        assert st[0] < P + (2 * P * P) // D.R + 1 and st[1] < D.R + 4 * P
        if i in CHAINS:
            fin = Counter()
            a, cf = D.finish(st, fin)
            assert (D.R * a + P * cf - acc * D.R * D.R) % P2 == 0
            assert cf < D.R + 7 * P and a == st[0]
            worst = max(worst, fin.max_col)
    assert worst < 1 << 63
    L = sum(w << (32 * j) for j, w in enumerate(st[2]))
    assert L < 86 * P < 1 << 1056 and L < D.R


def test_sum_bound_at_86_windows():
    """the worst case of the sum: 86 rows with the largest canonical log digit"""
    rng = random.Random(5)
    D = LogDigits(random_prime_like(1024, rng) | (((1 << 64) - 1) << 960))
    s = D.words(D.P - 1)
    for _ in range(85):
        s = D.lam_add(s, D.P - 1)
    L = sum(w << (32 * j) for j, w in enumerate(s))
    assert L == 86 * (D.P - 1) and L < 1 << 1056 and L < D.R


def test_lane_tree_join():
    """two partial products multiply by the general product on (a, c) and the
    sum of their log sums (k_djn_pmd, G > 1)"""
    rng = random.Random(11)
    P = random_prime_like(1024, rng)
    D = LogDigits(P)
    P2 = P * P
    ys = [unit(rng, P, P2) for _ in range(6)]
    ctr = Counter()
    left = D.start(D.row_direct(ys[0]))
    right = D.start(D.row_direct(ys[1]))
    for y in ys[2:4]:
        left = D.mul_row(left, D.row_direct(y), ctr)
    for y in ys[4:]:
        right = D.mul_row(right, D.row_direct(y), ctr)
    st = D.join(left, right, ctr)
    acc = 1
    for y in ys:
        acc = acc * y % P2
    assert D.log_value(st) == acc
    a, cf = D.finish(st, ctr)
    assert D.value(a, cf) == acc and ctr.max_col < 1 << 63


@pytest.mark.parametrize("win", [6, 7])
def test_rows_from_inverse_base_chains(win):
    """log digits from the inverse base's high and low chain entries, at the
    digits around the split d = hi 2^half + lo, equal the definition (one
    inversion per row) and are canonical; a chain over such rows is exact"""
    rng = random.Random(20 + win)
    P = random_prime_like(1024, rng)
    D = LogDigits(P)
    P2 = P * P
    T = InverseBaseTable(D, unit(rng, P, P2), win)
    half = win // 2
    digits = [0, 1, (1 << half) - 1, 1 << half, (1 << half) + 1, (1 << win) - 1]
    ctr = Counter()
    rows = []
    for d in digits:
        y, row = T.row(d, ctr)
        assert row == D.row_direct(y) and 0 <= row[1] < P
        rows.append((y, row))
    assert rows[0][0] == 1 and rows[0][1][0] == D.R % P
    assert ctr.max_col < 1 << 63
    st = D.start(rows[0][1])
    acc = 1
    for y, row in rows[1:]:
        st = D.mul_row(st, row, ctr)
        acc = acc * y % P2
    a, cf = D.finish(st, ctr)
    assert D.value(a, cf) == acc
