"""The block-form Montgomery reductions at both ends of k_djn_pmd (bn_dev.hpp
Mont::red_rows; limb model tools/pdigit_model.py red_rows, LogDigits
redc_p_block / redc_out_block): the rows of step1_red, limb i of the high half
entering at the top of row i, against Python integers.

The exit REDC mod N = P^2 (74 limbs, zero high half) on v and v R^2 mod N for
v = 0, 1, N - 1, N, 2N - 1, on 2^15 N - 1 (the bound of what to_mont2 hands
over), on a low half of all-MASK limbs, on all-MASK limbs below a 17-bit top
limb and on seeded random values; the prologue's REDC by P (37 limbs, the high
37 limbs of m streamed in) on 0, 1, P - 1, P, R P - 1, 2^2048 - 1, R - 1 and
seeded random values. Moduli: both primes of the golden 2048-bit DJN key and of
the structured key `bottom`. Each result is the reduction's own value (X + q M)
/ R with q = -X / M mod R, equals the plain row-by-row model's, and every lazy
column stays below 2^63: a column holds a limb (or the unmasked top limb, below
2^32) plus at most L <= 74 products below 2^56 and a carry. CPU, pure Python."""
import random

import pytest

from tests import structured_keys as SK
from tests.conftest import hx, load_fixture
from tools.pdigit_model import MASK, Counter, LogDigits, W, limbs_loose

K = 37


def _primes():
    g = load_fixture("paillier_2048_djn.json")["key"]
    b = SK.key(2048, "bottom")
    return {"golden-p": hx(g["p"]), "golden-q": hx(g["q"]), "bottom-p": b.p, "bottom-q": b.q}


def _exact(X, M, R):
    """(X + q M) / R with q = -X M^-1 mod R: what a Montgomery reduction returns"""
    q = (-X * pow(M, -1, R)) % R
    assert (X + q * M) % R == 0
    return (X + q * M) // R


@pytest.mark.parametrize("name", sorted(_primes()))
def test_exit_redc_block_form(name):
    P = _primes()[name]
    D = LogDigits(P)
    assert D.k == K
    N, R2 = P * P, D.R * D.R
    rng = random.Random(f"redc-out-{name}")
    vs = [0, 1, N - 1, N, 2 * N - 1]
    X = vs + [v * R2 % N for v in vs] + [(N << 15) - 1, (1 << (W * K)) - 1, (1 << (W * (2 * K - 1) + 17)) - 1]
    X += [rng.randrange(N << 15) for _ in range(24)]
    worst = 0
    for x in X:
        xl = limbs_loose(x, 2 * K)
        ctr = Counter()
        out = D.redc_out_block(xl, ctr)
        assert ctr.mads == (2 * K) ** 2
        worst = max(worst, ctr.max_col)
        t = _exact(x, N, R2)
        assert t < 2 * N and out == (t - N if t >= N else t) == x * pow(R2, -1, N) % N
        assert out == D.redc_out(xl, Counter())  # the plain rows give the same value
    assert worst < 1 << 63


@pytest.mark.parametrize("name", sorted(_primes()))
def test_prologue_redc_block_form(name):
    P = _primes()[name]
    D = LogDigits(P)
    R = D.R
    rng = random.Random(f"redc-p-{name}")
    ms = [0, 1, P - 1, P, R * P - 1, (1 << 2048) - 1, R - 1]
    ms += [rng.getrandbits(2048) for _ in range(12)] + [rng.randrange(R * P) for _ in range(12)]
    worst = 0
    for m in ms:
        ctr = Counter()
        t = D.redc_p_block(m, ctr, nw=65)
        assert ctr.mads == K * K
        worst = max(worst, ctr.max_col)
        assert t == _exact(m, P, R) and t < 2 * P
        ml = [(m >> (W * j)) & MASK for j in range(2 * K)]
        assert t == D.redc_wide(ml, Counter())  # pmd_redc_wide's value
    assert worst < 1 << 63


def test_high_limb_enters_its_own_row():
    """limb i of the high half must be in the top column before row i + 1 runs: a value whose only set limb is
    high limb i reduces to 2^(W i) plus a multiple of P"""
    P = _primes()["golden-p"]
    D = LogDigits(P)
    for i in (0, 1, K - 2, K - 1):
        m = 1 << (W * (K + i))
        if m < D.R * P:
            assert D.redc_p_block(m, Counter(), nw=65) % P == (1 << (W * i)) % P
