"""Inputs shared by the obfuscator-pool tests (tests/test_obf_pool_host.py
states the identity on them in Python integers, tests/test_gpu_obf_pool.py
feeds them to xhe_encrypt_obf).

A plain module (no fixtures): edge_pairs(n, seed) -> [(m, X)] with m < n and
X < n^2, X not necessarily a unit.
"""
import math
import random


def edge_pairs(n, seed=0):
    """Every m in {0, 1, n - 1, n // 3} with every X in {1, n, n^2 - 1, n - 1,
    n (n - 1), a random unit, 0}, then random pairs. Among them: X = n^2 - 1
    with m = 1 (X + n t reaches n^2: the final subtraction fires), X = n and
    X = n (n - 1) (x0 = X mod n = 0), X = n - 1 (x0 = -1)."""
    n2 = n * n
    rnd = random.Random(f"obf-{n.bit_length()}-{seed}")
    unit = rnd.randrange(1, n2)
    while math.gcd(unit, n) != 1:
        unit = rnd.randrange(1, n2)
    ms = [0, 1, n - 1, n // 3]
    xs = [1, n, n2 - 1, n - 1, n * (n - 1), unit, 0]
    pairs = [(m, x) for m in ms for x in xs]
    pairs += [(rnd.randrange(n), rnd.randrange(n2)) for _ in range(12)]
    return pairs


def online(n, m, x):
    """what k_enc_obf computes, step by step -> (ct, whether n^2 was subtracted)"""
    x0 = x % n
    t = (m * x0) % n
    ct = x + n * t
    over = ct >= n * n
    return ct - (n * n if over else 0), over
