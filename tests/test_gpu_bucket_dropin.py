"""enc @ X and X.T @ enc over 8197 samples: the planner sends the dense product
to xhe_bucketexp, and the result is word for word what the Straus route
(base inversions + ops.multiexp_words on the same plan) gives, and on a 64-row
sample the object fold of PaillierCiphertext.__mul__ / __add__."""
import ctypes

import numpy as np
import pytest

from tests import cumsum_cases as CC

pytestmark = pytest.mark.gpu

B, D = 8192 + 5, 2


def _scalars(kind):
    rng = np.random.default_rng(77)
    if kind == "int":  # signed, exponent 0
        return rng.integers(-(1 << 20) + 1, 1 << 20, (B, D))
    x = rng.uniform(1.0, 2.0, (B, D)) * 2.0 ** rng.integers(-2, 3, (B, D))  # 53-bit mantissas, five exponents
    x[:, 0] *= -1.0
    x[:, 1] *= rng.choice([-1.0, 1.0], B)
    x[3, 1] = 0.0
    return x


def _straus(ctx, enc, X):
    """(words [D, n2w], exponents [D]) of enc[B] @ X[B, D] through ops.multiexp_words"""
    from xfl_amd.paillier import array as AR
    from xfl_amd.paillier import ops
    kabs, neg, e_k = AR._encode_scalars(ctx, X)
    bidx, sidx = AR._matmul_terms((1, X.shape[0]), X.shape, True)
    need_inv, idx, shift, emin = AR._matmul_plan(np.asarray(enc.exponents), neg, e_k, bidx, sidx)
    words = np.ascontiguousarray(np.asarray(enc.words), dtype=np.uint32)
    one = np.zeros((need_inv.size, 1), np.uint32)
    one[:, 0] = 1
    bases = np.concatenate([words, ops.powmod_words(ctx, words[need_inv], one, 1, invert_first=True)])
    kwords, kbits = AR._shifted_words(kabs[sidx], shift)
    return ops.multiexp_words(ctx, bases, idx, kwords, kbits), emin


def _launches(fn, names):
    """(fn(), launches the library timed under each name while it ran)"""
    import torch

    from xfl_amd import _native as nat
    L = nat.lib()
    L.xhe_profile(1)
    try:
        res = fn()
        torch.cuda.synchronize()
        counts = []
        for name in names:
            ms, n = ctypes.c_double(), ctypes.c_int64()
            L.xhe_profile_read(name, ctypes.byref(ms), ctypes.byref(n))
            counts.append(n.value)
    finally:
        L.xhe_profile(0)
    return res, counts


@pytest.mark.parametrize("kind", ["int", "float"])
def test_matmul_takes_the_bucket_route(kind, monkeypatch):
    from xfl_amd import _native as nat
    from xfl_amd.paillier import ops
    priv, pub = CC.keys()
    X = _scalars(kind)
    enc = CC.encrypt(pub, CC.plain(B, 11))
    assert enc.is_resident
    (left, right), (nbucket, ngather) = _launches(lambda: (enc @ X, X.T @ enc), [b"k_bucketexp", b"k_mexp_gather"])
    assert nbucket == 2 and ngather == 0
    words, emin = _straus(enc.context, enc, X)
    for res in (left, right):
        assert res.shape == (D,)
        assert np.array_equal(np.asarray(res.words), words)
        assert np.array_equal(np.asarray(res.exponents), emin)
    # the object fold on 64 rows, the bucket route forced for the small shape
    monkeypatch.setattr(nat, "BUCKET_MIN_TERMS", 1)
    monkeypatch.setattr(ops, "multiexp_route", lambda *a: True)
    small, (nbucket,) = _launches(lambda: enc[:64] @ X[:64], [b"k_bucketexp"])
    assert nbucket == 1
    obj = np.asarray(enc[:64])
    fold = []
    for j in range(D):
        acc = obj[0] * X[0, j].item()
        for i in range(1, 64):
            acc = acc + obj[i] * X[i, j].item()
        fold.append(acc)
    assert CC.ints(small) == ([c.raw_ciphertext for c in fold], [c.exponent for c in fold])


@pytest.mark.parametrize("form", ["enc[2,B]@X[B,3]", "X[3,B]@enc[B,2]"])
def test_bucket_route_over_ciphertext_rows(form, monkeypatch):
    """a 2-D ciphertext operand: one bucket call per ciphertext row, outputs in the order of the Straus route"""
    from xfl_amd import _native as nat
    from xfl_amd.paillier import ops
    priv, pub = CC.keys()
    Bs = 9
    X = np.random.default_rng(5).integers(-99, 100, (Bs, 3)) / 4.0
    enc = CC.encrypt(pub, CC.plain(2 * Bs, 12))
    run = (lambda: enc.reshape(2, Bs) @ X) if form.startswith("enc") else (lambda: X.T @ enc.reshape(Bs, 2))
    want = run()  # (9 terms: Straus)
    monkeypatch.setattr(nat, "BUCKET_MIN_TERMS", 1)
    monkeypatch.setattr(ops, "multiexp_route", lambda *a: True)
    got, (nbucket,) = _launches(run, [b"k_bucketexp"])
    assert nbucket == 2 and got.shape == want.shape
    assert CC.ints(got) == CC.ints(want)
