"""Table rows multiplied in pairs, in the limb model (tools/pdigit_model.py
LogDigits.pair / mul_lazy / chain_pairs; pdigit_dev.hpp "Rows in pairs").

Two rows (e1, lhat1), (e2, lhat2) become one two-digit operand by a Montgomery
product mod P whose quotient digits are kept: e1 e2 = R a12 - m P exactly, c12 =
(R - 1 - m) + E as lazy limbs, and the state takes it by the general product (7
K^2 mads per two windows against 8 K^2) while the log sum takes lhat1 + lhat2.

Chains of 44, 45, 63, 85 and 1,023 rows after the start row (an odd leftover
goes through mul_row), random rows with forced ones among them - y = P^2 - 1, e
= 1, e = P - 1, and y = 1, whose lhat is not zero - are compared against Python
integers and against the all-mul_row chain. Asserted: every 64-bit column below
2^63; a' < P (1 + 2P/R) and c' < R + 4P after every product (what pmd_exit
relies on); a12 < P (1 + P/R); the mad count of the chain.

Key: the golden 2048-bit key, both primes in the role of P. Exact integers, CPU."""
import random

import pytest

from tests.conftest import hx, load_fixture
from tools.pdigit_model import Counter, LogDigits

K = 37
CHAINS = (44, 45, 63, 85, 1023)


def _digits(role):
    k = load_fixture("paillier_2048_djn.json")["key"]
    P = hx(k["p"]) if role == "p" else hx(k["q"])
    D = LogDigits(P)
    assert D.k == K
    return D, P


def _forced(D, P):
    """units y mod P^2 with a forced first digit or value"""
    P2 = P * P
    Ri = pow(D.R, -1, P2)
    ys = [P2 - 1, Ri % P2, (P - 1) * Ri % P2, 1]
    rows = [D.row_direct(y) for y in ys]
    assert rows[1][0] == 1 and rows[2][0] == P - 1 and rows[3][1] != 0
    return ys


def _rows(D, P, n, rng):
    """n + 1 units: random, the forced ones at both parities of the chain"""
    P2 = P * P
    ys = []
    while len(ys) < n + 1:
        y = rng.randrange(1, P2)
        if y % P:
            ys.append(y)
    forced = _forced(D, P)
    for t, y in enumerate(forced):  # as the first and as the second row of a pair
        ys[1 + 2 * t + (t & 1)] = y
        ys[n - 2 * t - (t & 1)] = y
    ys[9], ys[10] = forced[0], forced[2]  # P^2 - 1 paired with e = P - 1
    ys[11], ys[12] = forced[1], forced[1]  # e = 1 with itself
    return ys


@pytest.mark.parametrize("role", ["p", "q"])
@pytest.mark.parametrize("n", CHAINS)
def test_pair_chain(n, role):
    D, P = _digits(role)
    P2, R = P * P, D.R
    rng = random.Random(f"pairs-{n}-{role}")
    ys = _rows(D, P, n, rng)
    rows = [D.row_direct(y) for y in ys]
    want = 1
    for y in ys:
        want = want * y % P2

    ctr, ranges = Counter(), {}
    st = D.chain_pairs(rows, ctr, ranges)
    assert D.log_value(st) == want, "pair chain differs from the integer product"
    assert D.exit_fused(st, Counter()) == want

    ref, rctr = D.start(rows[0]), Counter()
    for row in rows[1:]:
        ref = D.mul_row(ref, row, rctr)
        assert ref[0] < P * (1 + 2 * P / R) and ref[1] < R + 4 * P
    assert D.log_value(ref) == want
    assert st[2] == ref[2], "the log sums agree word for word"
    assert D.exit_fused(ref, Counter()) == want

    assert ctr.max_col < 1 << 63 and rctr.max_col < 1 << 63
    assert ranges["a_over_P"] < 1 + 2 * P / R
    assert ranges["c_minus_R_over_P"] < 4
    assert ranges["a12_over_P"] < 1 + P / R
    pairs, odd = n // 2, n % 2
    assert ctr.mads == pairs * 7 * K * K + odd * 4 * K * K
    assert rctr.mads == n * 4 * K * K
    print(f"n={n} role={role} mads {ctr.mads}/{rctr.mads} = {ctr.mads / rctr.mads:.4f} "
          f"max column 2^{ctr.max_col.bit_length()} ranges {ranges}")


@pytest.mark.parametrize("role", ["p", "q"])
def test_pair_forced_operands(role):
    """every forced row paired with every forced row, on a state at the top of its range"""
    D, P = _digits(role)
    P2, R = P * P, D.R
    rng = random.Random(f"pairs-forced-{role}")
    forced = _forced(D, P)
    y0 = rng.randrange(1, P2) | 1
    while y0 % P == 0:
        y0 += 2
    for s_a, s_c in ((0, 0), (P + 2 * P * P // R - 1, R + 4 * P - 1), (P - 1, R - 1), (1, 0)):
        for y1 in forced:
            for y2 in forced:
                ctr, ranges = Counter(), {}
                a12, fl, ls = D.pair(D.row_direct(y1), D.row_direct(y2), ctr, ranges)
                assert a12 < P * (1 + P / R)
                a, c = D.mul_lazy((s_a, s_c), (a12, fl), ctr, ranges)
                assert a < P * (1 + 2 * P / R) and c < R + 4 * P
                assert ctr.max_col < 1 << 63 and ctr.mads == 7 * K * K
                # against integers: the state's residue times y1 y2, the logs aside
                lam = ls * pow(R, -2, P) % P
                got = D.value(a, c) * (1 + P * lam) % P2
                assert got == D.value(s_a, s_c) * y1 * y2 % P2
