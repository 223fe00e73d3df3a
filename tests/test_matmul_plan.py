"""CPU: the planner of the encrypted matmul (array._matmul_terms /
_matmul_plan: bases, idx, shifted exponents, emin), evaluated in Python
integers on the 2048-bit fixture key, equals the oracle's fold of the
reference's __mul__ / __add__ for enc[M, B] @ X[B, D] and X[M, B] @ enc[B, D]
(mixed signs, exact zeros, mixed ciphertext exponents)."""
import numpy as np
import pytest

from tests.matmul_cases import CASES, make_case, oracle_key, oracle_matmul


def _evaluate(ok, raws, exps, cshape, X, side):
    from xfl_amd.paillier.array import _encode_scalars_vec, _matmul_plan, _matmul_terms
    n2 = ok["n_square"]
    kabs, neg, e_k = (v.reshape(-1) for v in _encode_scalars_vec(X))
    bidx, sidx = _matmul_terms(cshape, X.shape, side == "left")
    need_inv, idx, shift, emin = _matmul_plan(np.array(exps), neg, e_k, bidx, sidx)
    bases = list(raws) + [pow(raws[i], -1, n2) for i in need_inv]
    out = []
    for o in range(idx.shape[0]):
        acc = 1
        for t in range(idx.shape[1]):
            acc = acc * pow(bases[idx[o, t]], int(kabs[sidx[o, t]]) << int(shift[o, t]), n2) % n2
        out.append((acc, int(emin[o])))
    return out, need_inv, idx


@pytest.mark.parametrize("cshape, xshape, side", CASES)
def test_plan_equals_oracle_fold(cshape, xshape, side):
    ok = oracle_key()
    raws, exps, X = make_case(ok, cshape, xshape, seed=100 * cshape[0] + 10 * cshape[1] + xshape[0])
    got, need_inv, idx = _evaluate(ok, raws, exps, cshape, X, side)
    assert got == oracle_matmul(ok, raws, exps, cshape, X, side)
    # one inverse per ciphertext a negative scalar multiplies, every index a base
    assert idx.dtype == np.int32 and idx.min() >= 0 and idx.max() < len(raws) + len(need_inv)
    assert list(need_inv) == sorted(set(need_inv))
    M, D = (cshape[0], xshape[1]) if side == "left" else (xshape[0], cshape[1])
    assert idx.shape == (M * D, cshape[1] if side == "left" else cshape[0])


def test_plan_of_a_row_matrix_is_the_vector_plan():
    """enc.reshape(1, B) @ X plans exactly what enc[B] @ X does (one row)."""
    from xfl_amd.paillier.array import _matmul_terms
    b2, s2 = _matmul_terms((1, 7), (7, 3), True)
    assert b2.tolist() == [list(range(7))] * 3
    assert s2.tolist() == [[3 * i + j for i in range(7)] for j in range(3)]
    bR, sR = _matmul_terms((7, 1), (3, 7), False)  # X[3, 7] @ enc[7] as a column
    assert bR.tolist() == b2.tolist()
    assert sR.tolist() == [[7 * m + i for i in range(7)] for m in range(3)]
