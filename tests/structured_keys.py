"""Named keys on structured primes (tests/golden/structured_primes.json, written
by tests/golden/gen_structured_primes.py): the primes nearest to the ends of
the K/2-bit range and two bit-pattern primes, paired so that the key-dependent
kernels meet what a random key never shows them.

    top            the largest prime and the next largest: close primes (ep, eq
                   of about K/2 + 8 bits), P - 1 nearly all ones, n and n^2 of
                   full width with a top limb of all ones
    bottom         the smallest prime and the next smallest: close primes, P - 1
                   a single long run of zeros, an n of K - 1 bits, the largest
                   ceil(R/M) and R - M
    mixed          the largest prime times one of the smallest: p ~ 2q, p > q
    mixed_swapped  the same primes with p < q
    pattern        (2048 only) two primes on repeated bit patterns: window digits

Within a family the first pair (in the order of the file) with gcd(p - 1,
q - 1) == 2 is taken, the reference's key-generation condition; `mixed` also
asks for an n of K bits, which at 3072 and 8192 bits passes over the very
smallest primes (their product with the largest falls just short of 2^(K-1)).

A plain module (no fixtures): key(K, name) -> Key, cached. The DJN base is
derived as tests/test_gpu_pmd_log.py does: a seeded x, h = (-x^2)^n mod n^2.
"""
import json
import math
import os
import random
from collections import namedtuple

HERE = os.path.dirname(os.path.abspath(__file__))
DATA = os.path.join(HERE, "golden", "structured_primes.json")

Key = namedtuple("Key", "name K p q n h")

SIZES = (2048, 3072, 4096, 8192)
N_BITS = {"top": 0, "bottom": -1, "mixed": 0, "mixed_swapped": 0}  # n.bit_length() - K


def names(K):
    return ("top", "bottom", "mixed", "mixed_swapped") + (("pattern",) if K == 2048 else ())


_data = None


def data():
    global _data
    if _data is None:
        with open(DATA) as f:
            _data = json.load(f)["widths"]
    return _data


def pattern_value(e):
    return int(e["unit"] * e["reps"] + e["tail"], 2)


def primes(H):
    """{'below': [...], 'above': [...], 'pattern': [...]} as integers, in the file's order"""
    d = data()[str(H)]
    return {"below": [(1 << H) - k for k in d["below"]],
            "above": [(1 << (H - 1)) + k for k in d["above"]],
            "pattern": [pattern_value(e) + e["offset"] for e in d.get("pattern", [])]}


def powmod(b, e, m):
    """pow(b, e, m) for b, e >= 0: on GMP when it is there (a 16384-bit modulus
    costs Python's pow seconds per call)"""
    from xfl_amd.paillier import _gmp
    return _gmp.powmod(b, e, m) if _gmp.available() else pow(b, e, m)


def _first_pair(ps, qs, ok=lambda p, q: True):
    for p in ps:
        for q in qs:
            if p != q and math.gcd(p - 1, q - 1) == 2 and ok(p, q):
                return p, q
    raise ValueError("no pair with gcd(p - 1, q - 1) == 2")


def pq(K, name):
    H = K // 2
    pr = primes(H)
    if name == "top":
        return _first_pair(pr["below"][:-1], pr["below"][1:], lambda p, q: p > q)
    if name == "bottom":
        return _first_pair(pr["above"][:-1], pr["above"][1:], lambda p, q: p < q)
    if name in ("mixed", "mixed_swapped"):
        p, q = _first_pair(pr["below"], pr["above"], lambda p, q: (p * q).bit_length() == K)
        return (p, q) if name == "mixed" else (q, p)
    if name == "pattern":
        return pr["pattern"][0], pr["pattern"][1]
    raise KeyError(name)


_keys = {}


def key(K, name):
    if (K, name) not in _keys:
        p, q = pq(K, name)
        n = p * q
        rng = random.Random(f"{K}-{name.replace('_swapped', '')}")  # the swapped key keeps its twin's h
        x = rng.getrandbits(n.bit_length()) | (1 << (n.bit_length() - 1))
        h = powmod(-(x * x) % (n * n), n, n * n)
        _keys[(K, name)] = Key(name, K, p, q, n, h)
    return _keys[(K, name)]


def zero_run(x):
    """the longest run of zero bits inside x"""
    return max(len(r) for r in bin(x)[2:].split("1"))
