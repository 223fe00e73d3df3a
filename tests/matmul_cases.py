"""Shared inputs and the oracle fold of the 2-D encrypted matmul tests
(test_matmul_plan.py on the CPU, test_gpu_matmul2d.py on the GPU).

A case is (ciphertext shape, scalar shape, side): enc[M, B] @ X[B, D] (side
"left") or X[M, B] @ enc[B, D] ("right"). Ciphertexts are random residues mod
n^2 coprime to n with mixed exponents; X mixes magnitudes, signs and exact
zeros (0 * c: exponent -53, raw 1), as tests/test_gpu_matvec.py does.
"""
import random

import numpy as np

from oracle import paillier_oracle as O
from tests.conftest import FIXTURES, hx, load_fixture

# (cshape, xshape, side)
CASES = [((1, 1), (1, 1), "left"), ((1, 7), (7, 3), "left"), ((3, 5), (5, 2), "left"), ((5, 3), (2, 5), "right")]


def oracle_key():
    k = load_fixture(FIXTURES[0])["key"]
    return O.derive_private(hx(k["p"]), hx(k["q"]), hx(k["h_pow_n"]))


def make_case(ok, cshape, xshape, seed):
    """-> (raws, exps) flat over cshape (C order), X float32 [xshape]"""
    rng = random.Random(seed)
    n2 = ok["n_square"]
    size = int(np.prod(cshape))
    raws = []
    while len(raws) < size:
        c = rng.randrange(2, n2)
        if c % ok["p"] and c % ok["q"]:
            raws.append(c)
    exps = [rng.choice([-24, -53, -60, 0]) for _ in range(size)]
    nrng = np.random.default_rng(seed)
    X = (nrng.standard_normal(xshape) * np.exp2(nrng.integers(-12, 6, xshape))).astype(np.float32)
    X[nrng.random(xshape) < 0.15] = 0.0
    X.reshape(-1)[0] = -1.0
    if X.size > 2:
        X.reshape(-1)[X.size // 2] = 0.0
        X.reshape(-1)[-1] = 3.0
    return raws, exps, X


def oracle_matmul(ok, raws, exps, cshape, X, side):
    """[(raw, exponent)] flat over the [M, D] result: numpy's object-dtype dot
    product, a left fold of the reference's __mul__ and __add__"""
    if side == "left":
        (M, Bn), D = cshape, X.shape[1]
        term = lambda m, j, i: (m * Bn + i, X[i, j])  # noqa: E731
    else:
        (M, Bn), D = X.shape, cshape[1]
        term = lambda m, j, i: (i * D + j, X[m, i])  # noqa: E731
    out = []
    for m in range(M):
        for j in range(D):
            acc = None
            for i in range(Bn):
                c, x = term(m, j, i)
                t = O.mul_ct(ok, raws[c], exps[c], x.item())
                acc = t if acc is None else O.add_ct(ok, acc[0], acc[1], t[0], t[1])
            out.append(acc)
    return out
