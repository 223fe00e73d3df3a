"""The ends of k_djn_pmd in the limb model (tools/pdigit_model.py LogDigits;
pdigit_dev.hpp "Short plaintexts", "The exit through the digits").

Short entry: a plaintext m with m < B = 2^112 (s = m) or 0 < n - m < B (s =
n - m) enters the log sum as muhat = +-s (Q R^2 B mod P) / B by a 4 x 37
product and four Montgomery steps; checked against Q m R^2 mod P for 0, 1, 2,
B - 1, n - 1, n - 2, n - B + 1 and random lengths of 0..111 bits in both signs.
B, n - B, n, n + 1, 2^2048 - 1, P and Q must be classified general.

Fused exit: from (a, c, Lhat) to the canonical (R a + P c)(1 + P L) R^-2 mod
P^2 through u = REDC(a), t = REDC(c + u Lhat), w = t + (R - 1 - m1) + E, z =
REDC(w), x = u + P z; checked on random states and on forced ones: a = 0, a =
P (u = P), a, c and Lhat at the tops of their ranges, and z landing on P - 1
before the u = P correction. Every quoted range (v < 2P, u <= P, t < 2P + 4,
w < 2R, z < P + 3) is asserted (in the model's methods and again here) and
every 64-bit column stays below 2^63.

Keys: the golden 2048-bit key and the structured keys `bottom` and
`mixed_swapped`, both primes in the role of P. Exact integers, CPU."""
import random

import pytest

from tests import structured_keys as SK
from tests.conftest import hx, load_fixture
from tools.pdigit_model import W, Counter, LogDigits

K = 37
L = 4
B = 1 << (W * L)
KEYS = ("golden", "bottom", "mixed_swapped")
N_RANDOM_STATES = 40


def _key(name):
    if name == "golden":
        k = load_fixture("paillier_2048_djn.json")["key"]
        return hx(k["p"]), hx(k["q"])
    k = SK.key(2048, name)
    return k.p, k.q


def _setup(name, role):
    p, q = _key(name)
    P, Q = (p, q) if role == "p" else (q, p)
    D = LogDigits(P)
    assert D.k == K and D.LW == 33 and D.SHORT_L == L
    return D, P, Q, P * Q


def _value(words):
    return sum(x << (32 * i) for i, x in enumerate(words))


@pytest.mark.parametrize("role", ["p", "q"])
@pytest.mark.parametrize("name", KEYS)
def test_short_entry(name, role):
    D, P, Q, n = _setup(name, role)
    rng = random.Random(f"ends-short-{name}-{role}")
    ms = D.ms_const(Q)
    assert ms == Q * pow(D.R, 2, P) * B % P and ms < P
    cases = [0, 1, 2, B - 1, n - 1, n - 2, n - B + 1]
    for bits in list(range(0, 112)) + [111] * 8:
        s = rng.getrandbits(bits) | (1 << (bits - 1)) if bits else 0
        cases += [s, n - s] if s else [s]
    worst = 0
    for m in cases:
        cl = D.classify_short(m, n)
        assert cl is not None, f"{m:#x} must be short"
        s, neg = cl
        assert s < B and (n - s if neg else s) == m and (s > 0 or not neg)
        ctr = Counter()
        words, v = D.short_log(s, neg, ms, ctr)
        assert ctr.mads == 2 * L * K
        assert v < 2 * P
        muhat = _value(words)
        assert 0 <= muhat <= 2 * P
        assert muhat % P == Q * m * D.R * D.R % P
        worst = max(worst, ctr.max_col)
    assert worst < 1 << 63


@pytest.mark.parametrize("name", KEYS)
def test_general_plaintexts_are_general(name):
    D, P, Q, n = _setup(name, "p")
    for m in (B, n - B, n, n + 1, (1 << 2048) - 1, P, Q):
        assert D.classify_short(m, n) is None, f"{m:#x} must be general"
    # the low words alone would pass: a difference of exactly 2^128, and m above n
    assert D.classify_short(n - (1 << 128) - 5, n) is None
    assert D.classify_short(n + 5, n) is None


def _want(D, a, c, Lh):
    P, R, P2 = D.P, D.R, D.P * D.P
    return (R * a + P * c) * (1 + P * (Lh * pow(R, -2, P) % P)) * pow(R, -2, P2) % P2


@pytest.mark.parametrize("role", ["p", "q"])
@pytest.mark.parametrize("name", KEYS)
def test_fused_exit(name, role):
    D, P, Q, n = _setup(name, role)
    R = D.R
    rng = random.Random(f"ends-exit-{name}-{role}")
    a_top, c_top, l_top = P + 2 * P * P // R, R + 4 * P - 1, R - 1  # a < P (1 + 2P/R), c < R + 4P, Lhat < R
    forced = [
        (0, rng.randrange(c_top), rng.randrange(R)),
        (P, rng.randrange(c_top), rng.randrange(R)),
        (a_top, c_top, l_top),
        (a_top, 0, 0),
        (0, 0, 0),
        (0, c_top, l_top),
        (P, c_top, l_top),
        # a = P: u = P = 0 (mod P), m1 = R - 1, z = c R^-2 - 1 + R^-1, so c = -R
        # (mod P) lands z on P - 1 before the u = P correction wraps it to 0
        (P, (-R) % P, rng.randrange(R)),
        (P, (-R) % P + P, l_top),
    ]
    states = forced + [(rng.randrange(a_top + 1), rng.randrange(c_top + 1), rng.randrange(R))
                       for _ in range(N_RANDOM_STATES)]
    worst = 0
    ranges = {}
    for i, (a, c, Lh) in enumerate(states):
        ctr = Counter()
        rg = {}
        x = D.exit_fused((a, c, D.words(Lh)), ctr, rg)
        assert x == _want(D, a, c, Lh), f"state {i}"
        assert x < P * P
        assert ctr.mads == 5 * K * K + K
        assert rg["u_over_P"] <= 1 and rg["t_minus_2P"] < 4 and rg["w_over_R"] < 2 and rg["z_minus_P"] < 3
        if a == P:
            assert rg["u_over_P"] == 1 and "z_at_u_fix" in rg
        if i in (7, 8):
            assert rg["z_at_u_fix"] == P - 1 and x % P == 0 and x // P == 0
        worst = max(worst, ctr.max_col)
        for k, v in rg.items():
            ranges[k] = max(ranges.get(k, v), v)
    assert worst < 1 << 63
    assert ranges["u_over_P"] == 1  # the forced a = P reached u = P


@pytest.mark.parametrize("name", KEYS)
def test_short_entry_through_exit(name):
    """entry and exit together: (1 + n m) y mod P^2 for a unit y held as a state
    with the short plaintext's muhat as its log sum"""
    D, P, Q, n = _setup(name, "p")
    rng = random.Random(f"ends-both-{name}")
    P2 = P * P
    ms = D.ms_const(Q)
    for m in (0, 1, B - 1, n - 1, n - B + 1, rng.getrandbits(60), n - rng.getrandbits(27)):
        s, neg = D.classify_short(m, n)
        words, _ = D.short_log(s, neg, ms, Counter())
        y = rng.randrange(1, P2)
        while y % P == 0:
            y = rng.randrange(1, P2)
        a, c = D.to_form(y)
        x = D.exit_fused((a, c, words), Counter())
        assert x == (1 + n * m) * y % P2
