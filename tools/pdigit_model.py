"""Limb-level model of arithmetic mod P^2 in base-P digits (DESIGN.md §4,
"Next: arithmetic mod p^2 in base-p digits"): x = x0 + P x1, 0 <= x0, x1 < P,

    (x0 + P x1)(y0 + P y1) = d0 + P ((d1 + x0 y1 + x1 y0) mod P)   (mod P^2)
    with x0 y0 = d0 + P d1, split by Barrett reduction (HAC 14.42) in
    radix b = 2^28 with a truncated quotient product.

It follows the schedule a kernel would run - 64-bit lazy column sums of 28-bit
limbs, one carry normalisation per product - checks every result against
Python integers, checks that no column sum reaches 2^64, and counts the
32x32->64 multiply-adds (v_mad_u64_u32) per product and per squaring next to
the current Montgomery product mod P^2 (2 S^2 + S, S = 74).

    python tools/pdigit_model.py [--bits 2048] [--trials 300]
"""
import argparse
import json
import random

W = 28
B = 1 << W
MASK = B - 1


def limbs(x, n):
    out = [(x >> (W * i)) & MASK for i in range(n)]
    assert x >> (W * n) == 0, "value does not fit"
    return out


def value(l):
    return sum(v << (W * i) for i, v in enumerate(l))


class Counter:
    def __init__(self):
        self.mads = 0
        self.max_col = 0


def cols_mul(a, b, ctr, lo=0, hi=None, acc=None):
    """lazy column sums of a*b for columns lo..hi-1 (hi default: all)"""
    n = len(a) + len(b) - 1
    hi = n if hi is None else hi
    acc = acc if acc is not None else [0] * (hi - lo)
    for i, ai in enumerate(a):
        for j, bj in enumerate(b):
            c = i + j
            if lo <= c < hi:
                acc[c - lo] += ai * bj
                ctr.mads += 1
    ctr.max_col = max(ctr.max_col, max(acc) if acc else 0)
    return acc


def normalize(cols, n, wrap=False):
    """carry-propagate lazy columns into n limbs (wrap: modulo b^n)"""
    out, carry = [], 0
    for i in range(n):
        x = (cols[i] if i < len(cols) else 0) + carry
        out.append(x & MASK)
        carry = x >> W
    assert wrap or carry == 0, "normalisation overflow"
    return out


class Digits:
    """Z/P^2 Z in base-P digits with Barrett reduction by P."""

    def __init__(self, P):
        self.P = P
        self.k = -(-P.bit_length() // W)          # limbs of P (37 at 1024 bits)
        self.Pl = limbs(P, self.k)
        self.mu = (1 << (W * 2 * self.k)) // P     # floor(b^2k / P)
        self.mul_ = limbs(self.mu, self.k + 1)

    def barrett(self, T, ctr, want_q):
        """(q, r) with T = q P + r, 0 <= r < P, for T < b^2k given as 2k limbs.
        q3 from the columns >= k-1 of q1*mu only (truncated): q - q3 <= 3."""
        k = self.k
        assert len(T) == 2 * k and value(T) < B ** (2 * k)
        q1 = T[k - 1:]                                     # floor(T / b^(k-1)): k+1 limbs
        top = cols_mul(q1, self.mul_, ctr, lo=k - 1)       # columns k-1 .. 2k+1
        # top[i] is column k-1+i: floor(q1 mu / b^(k+1)) = floor(v / b^2)
        v = sum(c << (W * i) for i, c in enumerate(top))
        q3 = v >> (2 * W)
        q3l = limbs(q3, k + 1)
        r2 = normalize(cols_mul(q3l, self.Pl, ctr, hi=k + 1), k + 1, wrap=True)  # (q3 P) mod b^(k+1)
        r = value(T[:k + 1]) - value(r2)
        if r < 0:
            r += B ** (k + 1)
        q, fix = q3, 0
        while r >= self.P:
            r -= self.P
            q += 1
            fix += 1
        assert fix <= 3, f"Barrett needed {fix} corrections"
        ctr.fix = max(getattr(ctr, "fix", 0), fix)
        return (q if want_q else None), r

    def split(self, x):
        return x % self.P, x // self.P

    def mul(self, x, y, ctr):
        (x0, x1), (y0, y1) = x, y
        k = self.k
        a0, a1, b0, b1 = (limbs(v, k) for v in (x0, x1, y0, y1))
        T = normalize(cols_mul(a0, b0, ctr), 2 * k)
        d1, d0 = self.barrett(T, ctr, True)
        U = cols_mul(a0, b1, ctr)
        U = cols_mul(a1, b0, ctr, acc=U)
        U = [u + dl for u, dl in zip(U, limbs(d1, k) + [0] * len(U))]
        ctr.max_col = max(ctr.max_col, max(U))
        U = normalize(U, 2 * k)
        _, z1 = self.barrett(U, ctr, False)
        return d0, z1

    def sqr(self, x, ctr):
        x0, x1 = x
        k = self.k
        a0, a1 = limbs(x0, k), limbs(x1, k)
        # x0^2 by product scanning: i < j pairs doubled, plus the squares
        cols = [0] * (2 * k - 1)
        for i in range(k):
            for j in range(i, k):
                cols[i + j] += a0[i] * a0[j] * (1 if i == j else 2)
                ctr.mads += 1
        ctr.max_col = max(ctr.max_col, max(cols))
        T = normalize(cols, 2 * k)
        d1, d0 = self.barrett(T, ctr, True)
        U = cols_mul(a0, a1, ctr)
        U = [2 * u + dl for u, dl in zip(U, limbs(d1, k) + [0] * len(U))]
        ctr.max_col = max(ctr.max_col, max(U))
        U = normalize(U, 2 * k)
        _, z1 = self.barrett(U, ctr, False)
        return d0, z1


class MontDigits:
    """Z/P^2 Z in MONTGOMERY digits - the form the device kernel runs
    (xfl_amd/csrc/pdigit_dev.hpp PMD): with R = b^k (b = 2^28, k limbs of P),
    a residue x is held as two k-limb integers (a, c) with

        x R^2 = R a + P c   (mod P^2)

    and the product of (a, c) and (e, f) is (a', c') with
        a' = REDC(a e)                  = (a e + m P) / R
        c' = REDC(a f + c e) + (R-1-m) + E,   E = (1 - R) mod P
    where m is the first REDC's quotient (a e = R a' - m P exactly), so that
    R a' + P c' = (R a + P c)(R e + P f) R^-2 (mod P^2). Both REDCs run as one
    operand-scanning loop over the limbs of (e, f) with lazy 64-bit
    accumulators; (R - 1 - m) + E enters limb by limb at the top of the second
    accumulator (limb i of m is known at step i and lands at weight b^i).
    Each step: k mads e_i*a + k mads m_i*P (first) and 3k mads e_i*c + f_i*a +
    m'_i*P (second): 5k^2 per product vs 2(2k)^2 for Montgomery mod P^2."""

    def __init__(self, P):
        self.P = P
        self.k = -(-P.bit_length() // W)
        self.R = 1 << (W * self.k)
        self.Pl = limbs(P, self.k)
        self.n0inv = (-pow(P, -1, B)) % B
        self.E = (1 - self.R) % P
        self.El = limbs(self.E, self.k)

    def to_form(self, x):
        """(a, c) with R a + P c = x R^2 mod P^2, a, c < P"""
        P, R = self.P, self.R
        X = x * R * R % (P * P)
        a = X * pow(R, -1, P) % P
        c = ((X - R * a) // P) % P  # exact: X = R a (mod P)
        return a, c

    def value(self, a, c):
        P2 = self.P * self.P
        return (self.R * a + self.P * c) * pow(self.R, -2, P2) % P2

    def mul(self, x, y, ctr):
        """one product, as the kernel's step schedule; returns (a', c')"""
        k, P = self.k, self.P
        (a, c), (e, f) = x, y
        al, cl = limbs_loose(a, k), limbs_loose(c, k)
        el, fl = limbs(e, k), limbs(f, k)
        T1 = [0] * k
        T2 = [0] * k
        for i in range(k):
            # position 0 first: the quotient digits
            x1 = T1[0] + el[i] * al[0]
            m1 = (x1 * self.n0inv) & MASK
            x1 += m1 * self.Pl[0]
            x2 = T2[0] + el[i] * cl[0] + fl[i] * al[0]
            m2 = (x2 * self.n0inv) & MASK
            x2 += m2 * self.Pl[0]
            assert x1 & MASK == 0 and x2 & MASK == 0
            ctr.mads += 5
            for j in range(1, k):
                T1[j - 1] = T1[j] + el[i] * al[j] + m1 * self.Pl[j]
                T2[j - 1] = T2[j] + el[i] * cl[j] + fl[i] * al[j] + m2 * self.Pl[j]
                ctr.mads += 5
            T1[k - 1] = 0
            T2[k - 1] = (MASK - m1) + self.El[i]
            T1[0] += x1 >> W
            T2[0] += x2 >> W
            ctr.max_col = max(ctr.max_col, max(T1), max(T2))
        a2 = _norm_value(T1)
        c2 = _norm_value(T2)
        return a2, c2


def limbs_loose(x, n):
    """limbs with the top one unmasked (values up to ~b^n * 2)"""
    out = [(x >> (W * i)) & MASK for i in range(n - 1)]
    out.append(x >> (W * (n - 1)))
    assert out[-1] < (1 << 32)
    return out


def _norm_value(T):
    return sum(t << (W * i) for i, t in enumerate(T))


def mont_digits_check(bits, trials, rng):
    worst, amax, cmax = 0, 0, 0
    for t in range(trials):
        P = random_prime_like(bits // 2, rng)
        D = MontDigits(P)
        P2 = P * P
        x = rng.randrange(P2)
        state = D.to_form(x)
        acc = x
        for s in range(6):  # a chain, as the fixed-base loop runs it
            y = rng.randrange(P2)
            ctr = Counter()
            state = D.mul(state, D.to_form(y), ctr)
            acc = acc * y % P2
            assert D.value(*state) == acc, "Montgomery-digit product wrong"
            worst = max(worst, ctr.max_col)
            amax = max(amax, state[0] / P)
            cmax = max(cmax, (state[1] - D.R) / P)
            assert state[1] < (1 << (W * D.k + 1)), "second digit outgrew its top limb"
    return {"mont_digit_mads_per_product": ctr.mads, "mont_digit_product_ratio": ctr.mads / (2 * (2 * D.k) ** 2),
            "mont_digit_max_column_log2": worst.bit_length(), "mont_digit_a_over_P": amax,
            "mont_digit_c_minus_R_over_P": cmax, "mont_digit_chain_trials": trials}


def random_prime_like(bits, rng):
    """an odd number with the top bit set (primality is irrelevant to the
    arithmetic being modelled)"""
    return rng.getrandbits(bits) | (1 << (bits - 1)) | 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bits", type=int, default=2048, help="key size; P has bits/2 bits")
    ap.add_argument("--trials", type=int, default=300)
    args = ap.parse_args()
    rng = random.Random(1)
    res = {"bits": args.bits}
    worst_col = 0
    fix = 0
    for t in range(args.trials):
        P = random_prime_like(args.bits // 2, rng)
        D = Digits(P)
        P2 = P * P
        edge = [0, 1, P2 - 1, P2 - P, P - 1, P]
        x = edge[t % len(edge)] if t < 12 else rng.randrange(P2)
        y = edge[(t // 2) % len(edge)] if t < 12 else rng.randrange(P2)
        cm, cs = Counter(), Counter()
        z = D.mul(D.split(x), D.split(y), cm)
        assert z[0] + P * z[1] == x * y % P2
        s = D.sqr(D.split(x), cs)
        assert s[0] + P * s[1] == x * x % P2
        worst_col = max(worst_col, cm.max_col, cs.max_col)
        fix = max(fix, getattr(cm, "fix", 0), getattr(cs, "fix", 0))
        res["mads_per_product"] = cm.mads
        res["mads_per_squaring"] = cs.mads
        res["k_limbs"] = D.k
    S = -(-args.bits // W)
    res["montgomery_mod_P2_mads"] = 2 * S * S + S
    res["montgomery_square_mads"] = S * (S + 1) // 2 + S * S + S
    res["product_ratio"] = res["mads_per_product"] / res["montgomery_mod_P2_mads"]
    res["squaring_ratio"] = res["mads_per_squaring"] / res["montgomery_square_mads"]
    res["max_column_sum_log2"] = worst_col.bit_length()
    res["max_barrett_corrections"] = fix
    res["trials_bit_exact"] = args.trials
    assert worst_col < (1 << 64)
    res.update(mont_digits_check(args.bits, max(4, args.trials // 10), rng))
    assert res["mont_digit_max_column_log2"] <= 64
    print(json.dumps(res))


if __name__ == "__main__":
    main()


# ---------------------------------------------------------------------------
# Montgomery digits mod n^2 (n = p q, public): the same product with the
# modulus n, W = 27-bit limbs and K = 80 (R = 2^2160 > 2^100 n at 2048 bits;
# 28-bit limbs would overflow the 64-bit lazy columns at K > 41), plus the
# conversions a kernel needs from and to plain residues mod n^2:
#   in:  X = x + ceil(R/n) n^2  (= x mod n^2, and REDC(X) = t lands in [n, 2n+))
#        REDC(X): X + m n = R t  ->  (t - n, R - m) are the digits of x R^-2
#        (R (t - n) + n (R - m) = X - R n ... = x + ceil(R/n) n^2 - R n + ...;
#        exactly: R(t-n) + n(R-m) = R t - n m = X == x (mod n^2)), then one
#        digit product by the digits of R^2 mod n^2 (a constant row) -> x
#   out: y0 = REDC(a) (quotient m_a, delta = [REDC(a) >= n]),
#        y1 = (REDC(REDC(c) - m_a + R n) + delta) mod n,   y = y0 + n y1
class NDigits(MontDigits):
    def __init__(self, n, W_=27, K=None):
        self.W = W_
        self.B = 1 << W_
        self.MASK = self.B - 1
        self.P = n
        self.k = K or -(-(n.bit_length() + 13) // W_)
        self.R = 1 << (W_ * self.k)
        self.n0inv = (-pow(n, -1, self.B)) % self.B
        self.E = (1 - self.R) % n
        self.Kn2 = -(-self.R // n) * n * n
        # digits of R^2 mod n^2 (the input conversion's constant row)
        X4 = pow(self.R, 4, n * n)
        e = X4 * pow(self.R, -1, n) % n
        self.w = (e, ((X4 - self.R * e) // n) % n)

    def limbs(self, x):
        out = [(x >> (self.W * i)) & self.MASK for i in range(self.k - 1)]
        out.append(x >> (self.W * (self.k - 1)))
        assert out[-1] < (1 << 32), "top limb overflows 32 bits"
        return out

    def redc(self, T, nlimbs, ctr):
        """operand-scanning REDC of an nlimbs-limb value (lazy columns):
        returns (t, m) with value + m n = R t"""
        n, W_ = self.P, self.W
        cols = [(T >> (W_ * i)) & self.MASK for i in range(nlimbs)]
        cols[-1] = T >> (W_ * (nlimbs - 1))
        cols += [0] * max(0, 2 * self.k - nlimbs)
        m = 0
        nl = [(n >> (W_ * j)) & self.MASK for j in range(self.k)]
        carry = 0
        for i in range(self.k):
            x = cols[i] + carry
            mi = (x * self.n0inv) & self.MASK
            m |= mi << (W_ * i)
            x += mi * nl[0]
            assert x & self.MASK == 0
            carry = x >> W_
            for j in range(1, self.k):
                cols[i + j] += mi * nl[j]
                ctr.max_col = max(ctr.max_col, cols[i + j])
            ctr.mads += self.k
        rest = sum(cols[i] << (W_ * (i - self.k)) for i in range(self.k, len(cols))) + carry
        assert (T + m * n) == rest * self.R
        return rest, m

    def mul(self, x, y, ctr):
        """MontDigits.mul with this W (limbs_loose for the state)"""
        k, n, W_ = self.k, self.P, self.W
        (a, c), (e, f) = x, y
        al, cl, el, fl = self.limbs(a), self.limbs(c), self.limbs(e), self.limbs(f)
        nl = [(n >> (W_ * j)) & self.MASK for j in range(k)]
        El = [(self.E >> (W_ * j)) & self.MASK for j in range(k)]
        T1, T2 = [0] * k, [0] * k
        for i in range(k):
            x1 = T1[0] + el[i] * al[0]
            m1 = (x1 * self.n0inv) & self.MASK
            x1 += m1 * nl[0]
            x2 = T2[0] + el[i] * cl[0] + fl[i] * al[0]
            m2 = (x2 * self.n0inv) & self.MASK
            x2 += m2 * nl[0]
            assert x1 & self.MASK == 0 and x2 & self.MASK == 0
            for j in range(1, k):
                T1[j - 1] = T1[j] + el[i] * al[j] + m1 * nl[j]
                T2[j - 1] = T2[j] + el[i] * cl[j] + fl[i] * al[j] + m2 * nl[j]
            ctr.mads += 5 * k
            T1[k - 1] = 0
            T2[k - 1] = (self.MASK - m1) + El[i]
            T1[0] += x1 >> W_
            T2[0] += x2 >> W_
            ctr.max_col = max(ctr.max_col, max(T1), max(T2))
        return (sum(t << (W_ * i) for i, t in enumerate(T1)), sum(t << (W_ * i) for i, t in enumerate(T2)))

    def to_digits(self, x, ctr):
        t, m = self.redc(x + self.Kn2, 2 * self.k + 1, ctr)
        # R t = x + Kn2 + m n with Kn2 < R n + n^2 and m < R: t < 2n + (x + n^2) / R. R >= 2^13 n, so for any x
        # the 2K words of a ciphertext hold (x < 64 n^2 on the sparsest modulus: (x + n^2) / R < 65 n / 2^13) the
        # first digit t - n stays below n + n / 100, inside the 2n of the state bound
        assert self.P <= t <= 2 * self.P + (x + self.P * self.P) // self.R, "REDC(x + Kn2) left [n, 2n + (x + n^2)/R]"
        assert t - self.P < 2 * self.P
        return self.mul((t - self.P, self.R - m), self.w, ctr)

    def from_digits(self, a, c, ctr):
        n = self.P
        ta, ma = self.redc(a, self.k, ctr)
        assert ta <= n
        delta = 1 if ta >= n else 0
        y0 = ta - delta * n
        u, _ = self.redc(c, self.k, ctr)
        tw, _ = self.redc(u - ma + self.R * n, 2 * self.k, ctr)
        y1 = (tw + delta) % n
        assert tw + delta < 3 * n
        return y0 + n * y1


def ndigits_check(bits, trials, rng):
    worst = 0
    for t in range(trials):
        n = random_prime_like(bits // 2, rng) * random_prime_like(bits // 2, rng)
        D = NDigits(n)
        n2 = n * n
        ctr = Counter()
        x = rng.randrange(n2) if t % 3 else rng.randrange(n)
        st = D.to_digits(x, ctr)
        assert D.value(*st) == x, "input conversion"
        acc = x
        for s in range(5):
            if s % 2:
                st = D.mul(st, st, ctr)  # squaring: the state as its own operand
                acc = acc * acc % n2
            else:
                y = rng.randrange(n2)
                st = D.mul(st, D.to_digits(y, ctr), ctr)
                acc = acc * y % n2
            assert D.value(*st) == acc
            assert st[0] < 2 * n and st[1] < D.R + 6 * n, "state bounds"
        assert D.from_digits(*st, ctr) == acc, "output conversion"
        worst = max(worst, ctr.max_col)
    return {"ndigit_K": D.k, "ndigit_W": D.W, "ndigit_max_column_log2": worst.bit_length(),
            "ndigit_trials": trials}


# ---------------------------------------------------------------------------
# The fixed-base row product with an additive second digit (pdigit_dev.hpp
# "Additive second digit"; k_djn_pmd). A table row y (a unit mod P) with the
# pair (e, f) is stored as (e, lhat), lhat = f y^-1 mod P, which is l R^2 for
# the l of  y R^2 = R e (1 + P l)  (mod P^2). The state is (a, c, Lhat) with
#
#     x R^2 = (R a + P c)(1 + P L),   Lhat = L R^2 (mod P), a plain sum
#
# and state x row is a' = REDC(a e), c' = REDC(c e) + (R-1-m) + E, Lhat' = Lhat
# + lhat: MontDigits.mul without the f a mads (4 k^2) and one multi-word
# addition. The finish folds the sum back: c_f = c + REDC(a Lhat), a Montgomery
# product mod P, and (a, c_f) is a pair again.
class LogDigits(MontDigits):
    LW = None  # 32-bit words of the log sum (a value below R)

    def __init__(self, P):
        super().__init__(P)
        self.LW = -(-W * self.k // 32)

    # -- rows
    def row_direct(self, y):
        """(e, lhat) of a unit y by one inversion (the definition)"""
        e, f = self.to_form(y)
        return e, f * pow(y, -1, self.P) % self.P

    def mont_mul(self, b, a, ctr):
        """b a R^-1 mod P (< b + P), operand scanning over the limbs of a with
        lazy 64-bit columns (Mont<K, 28, 1>::mul): 2 k^2 mads"""
        k = self.k
        bl, al = limbs_loose(b, k), limbs(a, k)
        T = [0] * k
        for i in range(k):
            x0 = T[0] + al[i] * bl[0]
            m = (x0 * self.n0inv) & MASK
            x0 += m * self.Pl[0]
            assert x0 & MASK == 0
            for j in range(1, k):
                T[j - 1] = T[j] + al[i] * bl[j] + m * self.Pl[j]
            T[k - 1] = 0
            T[0] += x0 >> W
            ctr.mads += 2 * k
            ctr.max_col = max(ctr.max_col, max(T))
        t = _norm_value(T)
        assert (t * self.R - a * b) % self.P == 0 and t < b + self.P
        return t

    def reduce_once(self, t):
        assert t < 2 * self.P
        return t - self.P if t >= self.P else t

    # -- the state
    def start(self, row):
        e, lhat = row
        return e, 0, self.words(lhat)

    def words(self, x):
        assert x >> (32 * self.LW) == 0
        return [(x >> (32 * i)) & 0xFFFFFFFF for i in range(self.LW)]

    def lam_add(self, s, lhat):
        """the LW-word add-with-carry of PMD::lam_add; the carry out must be 0"""
        out, cy = [], 0
        for sw, lw in zip(s, self.words(lhat)):
            x = sw + lw + cy
            out.append(x & 0xFFFFFFFF)
            cy = x >> 32
        assert cy == 0, "log sum left its words"
        return out

    def mul_row(self, state, row, ctr):
        """PMD::mul_row's step schedule on (a, c), and the sum"""
        k = self.k
        a, c, s = state
        e, lhat = row
        al, cl, el = limbs_loose(a, k), limbs_loose(c, k), limbs(e, k)
        T1, T2 = [0] * k, [0] * k
        for i in range(k):
            x1 = T1[0] + el[i] * al[0]
            m1 = (x1 * self.n0inv) & MASK
            x1 += m1 * self.Pl[0]
            x2 = T2[0] + el[i] * cl[0]
            m2 = (x2 * self.n0inv) & MASK
            x2 += m2 * self.Pl[0]
            assert x1 & MASK == 0 and x2 & MASK == 0
            for j in range(1, k):
                T1[j - 1] = T1[j] + el[i] * al[j] + m1 * self.Pl[j]
                T2[j - 1] = T2[j] + el[i] * cl[j] + m2 * self.Pl[j]
            ctr.mads += 4 * k
            T1[k - 1] = 0
            T2[k - 1] = (MASK - m1) + self.El[i]
            T1[0] += x1 >> W
            T2[0] += x2 >> W
            ctr.max_col = max(ctr.max_col, max(T1), max(T2))
        return _norm_value(T1), _norm_value(T2), self.lam_add(s, lhat)

    def join(self, x, y, ctr):
        """two states (the lane tree): the general product on (a, c), the sums added"""
        a, c = self.mul((x[0], x[1]), (y[0], y[1]), ctr)
        return a, c, self.lam_add(x[2], sum(w << (32 * i) for i, w in enumerate(y[2])))

    def finish(self, state, ctr):
        """(a, c_f): the pair form of the same residue"""
        a, c, s = state
        L = sum(w << (32 * i) for i, w in enumerate(s))
        assert L < self.R, "log sum outgrew K limbs"
        t = self.mont_mul(a, L, ctr)
        return a, c + t

    def log_value(self, state):
        a, c, s = state
        P, P2 = self.P, self.P * self.P
        L = sum(w << (32 * i) for i, w in enumerate(s)) * pow(self.R, -2, P) % P
        return self.value(a, c) * (1 + P * L) % P2

    # -- the plaintext as a logarithm (pdigit_dev.hpp "The plaintext as a
    # logarithm"; k_djn_pmd). With n = P Q, 1 + n m = 1 + P (Q m): the factor
    # (1 + n m) is the log digit muhat = Q m R^2 mod P, the start value of the
    # sum. After the finish R a + P c_f = (1 + n m) x R^2 (mod P^2), and one
    # REDC on the 2k limbs of P^2 leaves Montgomery form.
    def mu_const(self, Q):
        """Q R^4 mod P (KeyDev::mu_p / mu_q)"""
        return Q % self.P * pow(self.R, 4, self.P) % self.P

    def redc_wide(self, T, ctr):
        """pmd_redc_wide: 2k lazy columns (value < R P) -> t = value R^-1 mod P
        (< 2P), one row of k mads per quotient digit"""
        k = self.k
        T = list(T)
        assert len(T) == 2 * k and _norm_value(T) < self.R * self.P
        v = _norm_value(T)
        cy = 0
        for i in range(k):
            x = T[i] + cy
            m = (x * self.n0inv) & MASK
            x += m * self.Pl[0]
            assert x & MASK == 0
            cy = x >> W
            for j in range(1, k):
                T[i + j] += m * self.Pl[j]
            ctr.mads += k
            ctr.max_col = max(ctr.max_col, x, max(T[i + 1:i + k]))
        out = []
        for j in range(k):
            x = T[k + j] + cy
            out.append(x & MASK if j + 1 < k else x)
            cy = x >> W
            ctr.max_col = max(ctr.max_col, x)
        t = _norm_value(out)
        assert out[-1] < 1 << 32 and t < 2 * self.P and (t * self.R - v) % self.P == 0
        return t

    def plain_log(self, m, mu, ctr, nw=64):
        """pmd_lam_plain: the nw words of m as 2k limbs, REDC by P, the product
        by mu = Q R^4 mod P; returns muhat (< 2P) as the LW words of a sum"""
        k = self.k
        assert 0 <= m < 1 << (32 * nw) and 32 * nw <= W * 2 * k and 1 << (32 * nw) <= self.R * self.P
        t = self.redc_p_block(m, ctr, nw)
        muhat = self.mont_mul(t, mu, ctr)
        assert muhat < 2 * self.P and (muhat * self.R - t * mu) % self.P == 0
        return self.words(muhat)

    def start_plain(self, row, mu_words):
        """the first window's row on the lane that carries the plaintext: the
        row's log digit is added to muhat"""
        e, lhat = row
        return e, 0, self.lam_add(mu_words, lhat)

    def to_mont2(self, a, c, ctr):
        """PMD::to_mont2: X = R a + P c as 2k limbs (top limb unmasked) from lazy
        columns; k^2 mads"""
        k = self.k
        al, cl = limbs_loose(a, k), limbs_loose(c, k)
        T = [0] * k + al
        for i in range(k):
            for j in range(k):
                T[i + j] += cl[j] * self.Pl[i]
            ctr.mads += k
        ctr.max_col = max(ctr.max_col, max(T))
        out, cy = [], 0
        for j in range(2 * k):
            v = T[j] + cy
            out.append(v & MASK if j + 1 < 2 * k else v)
            cy = v >> W
            ctr.max_col = max(ctr.max_col, v)
        assert out[-1] < 1 << 32 and _norm_value(out) == self.R * a + self.P * c
        return out

    def redc_out(self, X, ctr):
        """Mont<2k, 28, 1>::redc_wide with a zero high half, then reduce_once:
        X R^-2 mod P^2, canonical. X: 2k limbs, value < R^2 P^2; (2k)^2 mads"""
        k2 = 2 * self.k
        P2 = self.P * self.P
        Nl = limbs(P2, k2)
        n0 = (-pow(P2, -1, B)) % B
        v = _norm_value(X)
        assert len(X) == k2 and v < self.R * self.R * P2
        T = list(X)
        for _ in range(k2):
            x0 = T[0]
            m = (x0 * n0) & MASK
            x0 += m * Nl[0]
            assert x0 & MASK == 0
            for j in range(1, k2):
                T[j - 1] = T[j] + m * Nl[j]
            T[k2 - 1] = 0
            T[0] += x0 >> W
            ctr.mads += k2
            ctr.max_col = max(ctr.max_col, x0, max(T))
        t = _norm_value(normalize(T, k2))
        assert t < 2 * P2 and (t * self.R * self.R - v) % P2 == 0
        return t - P2 if t >= P2 else t

    # -- the block-form reductions of k_djn_pmd (bn_dev.hpp Mont::red_rows:
    # the rows of step1_red, limb i of the high half entering at the top of
    # row i). `redc_out` above is the same row with a zero high half.
    def redc_p_block(self, m, ctr, nw=64):
        """pmd_redc_words: the nw words of m (below R P) as 2k limbs, the low k
        the start columns, the high k streamed into the rows: m R^-1 mod P (<
        2P), the value pmd_redc_wide returns"""
        k = self.k
        assert 0 <= m < 1 << (32 * nw) and 32 * nw <= W * 2 * k + 31 and m < self.R * self.P
        ml = limbs(m, 2 * k)
        t = _norm_value(normalize(red_rows(ml[:k], ml[k:], self.Pl, self.n0inv, ctr), k))
        assert t < 2 * self.P and (t * self.R - m) % self.P == 0
        return t

    def redc_out_block(self, X, ctr):
        """Mont<2k, 28, 1>::redc_wide(b, AZero) in block form, then reduce_once:
        X R^-2 mod P^2, canonical. X: 2k limbs (top limb unmasked)"""
        k2 = 2 * self.k
        P2 = self.P * self.P
        v = _norm_value(X)
        assert len(X) == k2 and v < self.R * self.R * P2
        T = red_rows(X, [0] * k2, limbs(P2, k2), (-pow(P2, -1, B)) % B, ctr)
        t = _norm_value(normalize(T, k2))
        assert t < 2 * P2 and (t * self.R * self.R - v) % P2 == 0
        return t - P2 if t >= P2 else t

    # -- the ends of k_djn_pmd (pdigit_dev.hpp "Short plaintexts", "The exit
    # through the digits"): the short-plaintext entry of the log sum and the
    # exit that folds the sum in on the way to the canonical residue.
    SHORT_L = 4  # limbs of a short plaintext's magnitude: s < 2^(28 * 4)

    def ms_const(self, Q):
        """Q R^2 2^(28 L) mod P (KeyDev::ms_p / ms_q)"""
        return Q % self.P * pow(self.R, 2, self.P) % self.P * (1 << (W * self.SHORT_L)) % self.P

    def classify_short(self, m, n, nw=64):
        """pmd_short_classify on the nw words of m: (s, negative) for a short
        plaintext - m = s < 2^(28 L), or 0 < n - m = s < 2^(28 L) - and None for
        a general one. Word by word as the kernel decides it: the words of m
        above the low four all zero, or the nw-word difference n - m (a borrow
        chain over every word) without a borrow out and zero above the low
        four; s is the low four words and must stay below 2^(28 L)."""
        assert 0 <= m < 1 << (32 * nw) and 0 < n < 1 << (32 * nw)
        Bs = 1 << (W * self.SHORT_L)
        lw = -(-W * self.SHORT_L // 32)  # the low words: 4
        lo_mask = (1 << (32 * lw)) - 1
        if m >> (32 * lw) == 0 and m & lo_mask < Bs:
            return m, False
        d, br = [], 0
        for k in range(nw):
            x = ((n >> (32 * k)) & 0xFFFFFFFF) - ((m >> (32 * k)) & 0xFFFFFFFF) - br
            d.append(x & 0xFFFFFFFF)
            br = 1 if x < 0 else 0
        s = sum(w << (32 * k) for k, w in enumerate(d[:lw]))
        if br == 0 and not any(d[lw:]) and 0 < s < Bs:
            return s, True
        return None

    def short_log(self, s, neg, ms, ctr):
        """pmd_lam_short: T = s ms on K + L lazy columns, L Montgomery steps by P
        (they divide by 2^(28 L)), v = s Q R^2 mod P < 2P; muhat = v or 2P - v.
        Returns (muhat words, v)."""
        k, L = self.k, self.SHORT_L
        assert 0 <= s < 1 << (W * L) and 0 <= ms < self.P
        sl, ml = limbs(s, L), limbs(ms, k)
        T = [0] * (k + L)
        for i in range(L):
            for j in range(k):
                T[i + j] += sl[i] * ml[j]
            ctr.mads += k
        ctr.max_col = max(ctr.max_col, max(T))
        for i in range(L):
            q = (T[i] * self.n0inv) & MASK
            for j in range(k):
                T[i + j] += q * self.Pl[j]
            ctr.mads += k
            assert T[i] & MASK == 0
            T[i + 1] += T[i] >> W
            ctr.max_col = max(ctr.max_col, max(T))
        v = _norm_value(T[L:])
        assert v < 2 * self.P and (v << (W * L)) % self.P == s * ms % self.P
        muhat = 2 * self.P - v if neg else v
        assert 0 <= muhat <= 2 * self.P
        return self.words(muhat), v

    def exit_fused(self, state, ctr, ranges=None):
        """pmd_exit: the canonical residue (R a + P c)(1 + P L) R^-2 mod P^2 from
        the state after the last product, 5 k^2 + k mads:
            u = REDC(a), quotient digits m1 kept          (u <= P)
            t = REDC(c + u Lhat)                          (t < 2P + 4)
            w = t + (R - 1 - m1) + E                      (w < 2R, top limb loose)
            z = REDC(w), reduced below P                  (z < P + 3 before)
            u = P: u <- 0, z <- (z + 1) mod P
            x = u + P z
        ranges: a dict that receives the largest u/P, t - 2P, w/R, z - P seen, and
        the reduced z of a state whose u reached P."""
        k, P, R = self.k, self.P, self.R
        a, c, s = state
        Lh = sum(w << (32 * i) for i, w in enumerate(s))
        assert Lh < R, "log sum outgrew K limbs"
        m1 = []
        u = _norm_value(normalize(red_rows(limbs_loose(a, k), [0] * k, self.Pl, self.n0inv, ctr, digits=m1), k))
        assert u <= P and u * R == a + value(m1) * P
        # operand scanning over the limbs of Lhat on the columns of c
        ul, ll = limbs(u, k), limbs(Lh, k)
        T = limbs_loose(c, k)
        for i in range(k):
            x0 = T[0] + ll[i] * ul[0]
            m = (x0 * self.n0inv) & MASK
            x0 += m * self.Pl[0]
            assert x0 & MASK == 0
            for j in range(1, k):
                T[j - 1] = T[j] + ll[i] * ul[j] + m * self.Pl[j]
            T[k - 1] = 0
            T[0] += x0 >> W
            ctr.mads += 2 * k + 1
            ctr.max_col = max(ctr.max_col, x0, max(T))
        t = _norm_value(T)
        assert t < 2 * P + 4 and (t * R - c - u * Lh) % P == 0
        # w = t + (MASK - m1_i + E_i) limb by limb, the top limb keeps the carry
        tl, wl, cy = limbs(t, k), [], 0
        for i in range(k):
            x = tl[i] + (MASK - m1[i]) + self.El[i] + cy
            wl.append(x & MASK if i + 1 < k else x)
            cy = x >> W
        w = _norm_value(wl)
        assert w < 2 * R and wl[-1] < 1 << 32
        z = _norm_value(normalize(red_rows(wl, [0] * k, self.Pl, self.n0inv, ctr), k))
        assert z < P + 3 and (z * R - w) % P == 0
        if ranges is not None:
            for key, val in (("u_over_P", u / P), ("t_minus_2P", t - 2 * P), ("w_over_R", w / R), ("z_minus_P", z - P)):
                ranges[key] = max(ranges.get(key, float("-inf")), val)
            if u >= P:
                ranges["z_at_u_fix"] = z % P  # what the u = P correction increments
        if z >= P:
            z -= P
        if u >= P:
            u -= P
            z = z + 1 - P if z + 1 >= P else z + 1
        # x = u + P z: k^2 mads on 2k lazy columns
        zl, T = limbs(z, k), limbs(u, k) + [0] * k
        for i in range(k):
            for j in range(k):
                T[i + j] += zl[j] * self.Pl[i]
            ctr.mads += k
        ctr.max_col = max(ctr.max_col, max(T))
        x = _norm_value(normalize(T, 2 * k))
        assert x == u + P * z and x < P * P
        return x

    # -- rows in pairs (pdigit_dev.hpp "Rows in pairs"; k_djn_pmd, one lane per
    # element). Two rows y1, y2 with y_i R^2 = R e_i (1 + P l_i): one Montgomery
    # product mod P with its quotient digits kept, e1 e2 = R a12 - m P exactly,
    # gives y1 y2 R^2 = (R a12 + P c12)(1 + P (l1 + l2)) with c12 = (R - 1 - m) +
    # E = -m (mod P): an ordinary two-digit operand of the general product.
    @staticmethod
    def _note(ranges, key, val):
        if ranges is not None:
            ranges[key] = max(ranges.get(key, float("-inf")), val)

    def pair(self, row1, row2, ctr, ranges=None):
        """PMD::mul_pair's step schedule: e1 in registers, e2 streamed. Returns
        a12 (< P (1 + P/R)), the lazy limbs (MASK - m_i) + E_i of c12 (each below
        2^29) and lhat1 + lhat2. 2 k^2 mads."""
        k, P = self.k, self.P
        (e1, l1), (e2, l2) = row1, row2
        al, el = limbs(e1, k), limbs(e2, k)
        T, cl, ml = [0] * k, [], []
        for i in range(k):
            x = T[0] + el[i] * al[0]
            m = (x * self.n0inv) & MASK
            x += m * self.Pl[0]
            assert x & MASK == 0
            for j in range(1, k):
                T[j - 1] = T[j] + el[i] * al[j] + m * self.Pl[j]
            T[k - 1] = 0
            T[0] += x >> W
            ctr.mads += 2 * k
            ctr.max_col = max(ctr.max_col, x, max(T))
            ml.append(m)
            cl.append((MASK - m) + self.El[i])
        a12 = _norm_value(T)
        assert a12 * self.R == e1 * e2 + value(ml) * P, "e1 e2 = R a12 - m P"
        assert max(cl) < 1 << 29 and (_norm_value(cl) + value(ml)) % P == 0
        self._note(ranges, "a12_over_P", a12 / P)
        self._note(ranges, "pair_col_log2", ctr.max_col.bit_length())
        return a12, cl, l1 + l2

    def mul_lazy(self, x, y, ctr, ranges=None):
        """MontDigits.mul with the operand's second digit given as lazy limbs (f_i
        below 2^29, value possibly above R: c12 of `pair`; `mul` would mask it)"""
        k = self.k
        (a, c), (e, fl) = x, y
        al, cl, el = limbs_loose(a, k), limbs_loose(c, k), limbs(e, k)
        assert len(fl) == k and max(fl) < 1 << 29
        T1, T2 = [0] * k, [0] * k
        for i in range(k):
            x1 = T1[0] + el[i] * al[0]
            m1 = (x1 * self.n0inv) & MASK
            x1 += m1 * self.Pl[0]
            x2 = T2[0] + el[i] * cl[0] + fl[i] * al[0]
            m2 = (x2 * self.n0inv) & MASK
            x2 += m2 * self.Pl[0]
            assert x1 & MASK == 0 and x2 & MASK == 0
            for j in range(1, k):
                T1[j - 1] = T1[j] + el[i] * al[j] + m1 * self.Pl[j]
                T2[j - 1] = T2[j] + el[i] * cl[j] + fl[i] * al[j] + m2 * self.Pl[j]
            ctr.mads += 5 * k
            T1[k - 1] = 0
            T2[k - 1] = (MASK - m1) + self.El[i]
            T1[0] += x1 >> W
            T2[0] += x2 >> W
            ctr.max_col = max(ctr.max_col, x1, x2, max(T1), max(T2))
        self._note(ranges, "mul_col_log2", ctr.max_col.bit_length())
        return _norm_value(T1), _norm_value(T2)

    def chain_pairs(self, rows, ctr, ranges=None):
        """k_djn_pmd's loop at one lane per element: the start row, then the rows
        two at a time (pair, general product, the sum takes lhat1 + lhat2), one
        mul_row for an odd leftover. Returns the state (a, c, sum words)."""
        P, R = self.P, self.R
        st = self.start(rows[0])
        i = 1
        while i < len(rows):
            if i + 1 < len(rows):
                a12, fl, ls = self.pair(rows[i], rows[i + 1], ctr, ranges)
                a, c = self.mul_lazy((st[0], st[1]), (a12, fl), ctr, ranges)
                st = (a, c, self.lam_add(st[2], ls))
                i += 2
            else:
                st = self.mul_row(st, rows[i], ctr)
                i += 1
            self._note(ranges, "a_over_P", st[0] / P)
            self._note(ranges, "c_minus_R_over_P", (st[1] - R) / P)
        return st


def red_rows(lo, hi, Nl, n0inv, ctr, digits=None):
    """Mont::red_rows: L rows T <- (T + m N) / 2^W on the lazy columns T = lo
    (L values, limbs or an unmasked top limb), limb i of `hi` written to the top
    column at the end of row i (step1_red: T[L-1] = hi_i after the row's blocks
    consumed the old top). Returns the L columns of (lo + hi 2^(W L) + q N) /
    2^(W L); every column is recorded in ctr.max_col (the kernel holds them in
    64 bits and adds products below 2^(2W): they must stay below 2^63).
    digits: a list that receives the L quotient digits (red_rows_q)."""
    L = len(lo)
    assert len(hi) == L and len(Nl) == L
    T = list(lo)
    x0 = T[0]
    m = (x0 * n0inv) & MASK
    for i in range(L):
        if digits is not None:
            digits.append(m)
        x0 += m * Nl[0]
        assert x0 & MASK == 0
        for j in range(1, L):
            T[j - 1] = T[j] + m * Nl[j]
        T[0] += x0 >> W
        T[L - 1] = hi[i]
        ctr.mads += L
        ctr.max_col = max(ctr.max_col, x0, max(T))
        x0 = T[0]  # the next row's digit, formed under this row's blocks
        m = (x0 * n0inv) & MASK
    return T


class InverseBaseTable:
    """One window of a fixed-base table for the base Bw mod P^2 with its rows'
    log digits formed as k_tab_to_pmd forms them: no inversion per row - y^-1
    mod P is the same entry for the base Bw^-1 mod P, the product of a high and
    a low chain entry (d = hi 2^half + lo; entries in Montgomery form mod P,
    entry 0 = R mod P), so lhat = MontMul(MontMul(f, hi'), lo')."""

    def __init__(self, D, Bw, win):
        self.D, self.Bw, self.win, self.half = D, Bw, win, win // 2
        P = D.P
        Binv = pow(Bw, -1, P)
        RP = D.R % P
        self.lo = [pow(Binv, d, P) * RP % P for d in range((1 << self.half) + 1)]
        self.hi = [pow(Binv, d << self.half, P) * RP % P for d in range(1 << (win - self.half))]

    def row(self, d, ctr):
        D = self.D
        y = pow(self.Bw, d, D.P * D.P)
        e, f = D.to_form(y)
        lo, hi = d & ((1 << self.half) - 1), d >> self.half
        t = D.reduce_once(D.mont_mul(f, self.hi[hi], ctr))
        t = D.reduce_once(D.mont_mul(t, self.lo[lo], ctr))
        return y, (e, t)


def unit(rng, P, bound):
    import math
    while True:
        y = rng.randrange(1, bound)
        if math.gcd(y, P) == 1:
            return y


def log_digits_check(bits, trials, rng, chain=44):
    """chains of row products against Python integers; returns the counters"""
    worst = amax = lmax = 0
    cmax = float("-inf")
    for t in range(trials):
        P = random_prime_like(bits // 2, rng)
        D = LogDigits(P)
        P2 = P * P
        ys = [unit(rng, P, P2) for _ in range(chain + 1)]
        st = D.start(D.row_direct(ys[0]))
        acc = ys[0]
        for y in ys[1:]:
            ctr = Counter()
            st = D.mul_row(st, D.row_direct(y), ctr)
            acc = acc * y % P2
            assert D.log_value(st) == acc, "row product wrong"
            assert ctr.mads == 4 * D.k * D.k
            worst = max(worst, ctr.max_col)
            amax = max(amax, st[0] / P)
            cmax = max(cmax, (st[1] - D.R) / P)
        fin = Counter()
        a, c = D.finish(st, fin)
        assert D.value(a, c) == acc, "finish wrong"
        worst = max(worst, fin.max_col)
        cmax = max(cmax, (c - D.R) / P)
        lmax = max(lmax, sum(w << (32 * i) for i, w in enumerate(st[2])).bit_length())
    return {"log_digit_mads_per_row_product": 4 * D.k * D.k, "log_digit_finish_mads": fin.mads,
            "log_digit_max_column_log2": worst.bit_length(), "log_digit_a_over_P": amax,
            "log_digit_c_minus_R_over_P": cmax, "log_digit_sum_bits": lmax, "log_digit_chain": chain,
            "log_digit_trials": trials}
