"""The plaintext folded into the log sum of k_djn_pmd (pdigit_dev.hpp "The
plaintext as a logarithm"; limb model tools/pdigit_model.py LogDigits): with
n = P Q, (1 + n m) = 1 + P (Q m) is the log digit muhat = Q m R^2 mod P, the
start value of the sum; after the row products and the finish, R a + P c_f =
(1 + n m) h^a R^2 (mod P^2), and one REDC on the 74 limbs of P^2 with a
reduce_once gives the canonical (1 + n m) h^a mod P^2 the kernel stores.

Checked against Python integers on the golden 2048-bit DJN key and on the
structured keys (top, bottom, mixed, mixed_swapped, pattern), both primes in
the role of P, over chains of 44, 63, 85 and 147 row products (45, 64, 86 and
148 windows of 23, 16, 12 and 7 bits over the key's own fixed-base rows
h^(d 2^(win w))), with the plaintexts 0, 1, 2, n - 1, n - 2, P, Q, k P, k Q,
2^1024, 2^2048 - 1 and a random one, and the exponents 1, 2^1024 - 1, one
with an all-zero window and a random one, in turn. Every column stays below
2^63, muhat below 2P, the sum below (nwin + 2) P < R, c_f below R + 7P and the
value handed to the last REDC below 2^15 P^2 with a top limb below 2^17. CPU,
pure Python."""
import random

import pytest

from tests import structured_keys as SK
from tests.conftest import hx, load_fixture
from tools.pdigit_model import Counter, LogDigits

K = 37
CHAINS = (44, 63, 85, 147)  # row products: one fewer than the windows
KEYS = ("golden", "top", "bottom", "mixed", "mixed_swapped", "pattern")
RAND_BITS = 1024


def _key(name):
    if name == "golden":
        k = load_fixture("paillier_2048_djn.json")["key"]
        return hx(k["p"]), hx(k["q"]), hx(k["h_pow_n"])
    k = SK.key(2048, name)
    return k.p, k.q, k.h


def _plaintexts(P, Q, rng):
    n = P * Q
    kp, kq = rng.randrange(2, Q), rng.randrange(2, P)
    return [0, 1, 2, n - 1, n - 2, P, Q, kp * P, kq * Q, 1 << 1024, (1 << 2048) - 1, rng.getrandbits(2048)]


def _exponents(win, nwin, rng):
    zero = rng.getrandbits(RAND_BITS) | 1
    zero &= ~(((1 << win) - 1) << (win * (nwin // 2)))  # an all-zero window in the middle
    return [1, (1 << RAND_BITS) - 1, zero, rng.getrandbits(RAND_BITS)]


@pytest.mark.parametrize("role", ["p", "q"])
@pytest.mark.parametrize("name", KEYS)
def test_fold_chains(name, role):
    p, q, h = _key(name)
    P, Q = (p, q) if role == "p" else (q, p)
    n, P2 = P * Q, P * P
    D = LogDigits(P)
    assert D.k == K and D.LW == 33
    rng = random.Random(f"fold-{name}-{role}")
    mu = D.mu_const(Q)
    assert mu == Q * pow(D.R, 4, P) % P
    ms = _plaintexts(P, Q, rng)
    # muhat of every plaintext once: it does not depend on the chain
    worst = 0
    mus = []
    for m in ms:
        ctr = Counter()
        w = D.plain_log(m, mu, ctr)
        assert ctr.mads == K * K + 2 * K * K
        muhat = sum(x << (32 * i) for i, x in enumerate(w))
        assert muhat < 2 * P and muhat % P == Q * m * D.R * D.R % P
        worst = max(worst, ctr.max_col)
        mus.append(w)
    hP = h % P2
    for ci, chain in enumerate(CHAINS):
        nwin = chain + 1
        win = -(-RAND_BITS // nwin)
        a_exp = _exponents(win, nwin, rng)[(ci + KEYS.index(name)) % 4]
        digits = [(a_exp >> (win * w)) & ((1 << win) - 1) for w in range(nwin)]
        ys = [pow(hP, d << (win * w), P2) for w, d in enumerate(digits)]
        rows = [D.row_direct(y) for y in ys]
        assert all(0 <= lh < P for _, lh in rows)
        # the (a, c) half of the state does not see the plaintext: one chain for every m
        st = D.start(rows[0])
        for row in rows[1:]:
            ctr = Counter()
            st = D.mul_row(st, row, ctr)
            worst = max(worst, ctr.max_col)
            assert st[0] < P + (2 * P * P) // D.R + 1 and st[1] < D.R + 4 * P
        ha = pow(hP, a_exp, P2)
        assert D.log_value(st) == ha
        for m, w in zip(ms, mus):
            # the sum as the kernel forms it: muhat first, then every row's log digit
            s = D.start_plain(rows[0], w)[2]
            for _, lh in rows[1:]:
                s = D.lam_add(s, lh)
            L = sum(x << (32 * i) for i, x in enumerate(s))
            assert L < (nwin + 2) * P and L < D.R
            ctr = Counter()
            a, cf = D.finish((st[0], st[1], s), ctr)
            assert cf < D.R + 7 * P
            X = D.to_mont2(a, cf, ctr)
            # R a + P c_f < 2 R P + 8 P^2 (a < P + 1, c_f < R + 7P) <= (2^14 + 8) P^2 for P >= 2^1023
            assert X[-1] < 1 << 17 and sum(x << (28 * i) for i, x in enumerate(X)) < 2 * D.R * P + 8 * P2 < P2 << 15
            out = D.redc_out(X, ctr)
            assert ctr.mads == (2 * K * K) + K * K + (2 * K) ** 2  # finish, to_mont2, the last REDC
            worst = max(worst, ctr.max_col)
            assert out == (1 + n * m) * ha % P2, (name, role, chain, hex(m)[:18])
    assert worst < 1 << 63


def test_sum_bound_with_plaintext():
    """the worst case of the sum at the most windows a 1024-bit exponent can
    have (window 1: 1024 rows of the largest canonical log digit) plus the
    largest muhat: below (nwin + 2) P, inside R = 2^12 * 2^1024 and the 33 words"""
    P = SK.key(2048, "top").p
    D = LogDigits(P)
    L = (2 * P - 1) + 1024 * (P - 1)
    assert L < (1024 + 2) * P < D.R <= 1 << (32 * D.LW)
    s = D.words(2 * P - 1)
    for _ in range(85):  # the carry chain itself, over the 86 rows of window 12
        s = D.lam_add(s, P - 1)
    assert sum(x << (32 * i) for i, x in enumerate(s)) == (2 * P - 1) + 85 * (P - 1)
