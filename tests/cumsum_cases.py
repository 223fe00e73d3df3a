"""np.cumsum / Series.cumsum / cumsum_segments over ciphertext arrays, shared by
tests/test_cumsum_host.py (CPU: the oracle stand-ins of tests/oracle_ops.py
plus a Python-integer ops.segscan_words) and tests/test_gpu_cumsum_dropin.py
(the real kernels). Each function takes `calls`, the list the installed
segscan records every call in: the device path is one call, a fallback none.

2048-bit golden key; precision=7, obfuscation=False arrays of 1, 5 and 70
elements and a 3 x 7 array. The plaintexts are multiples of 1/8, which encode
exactly, so the cumulative sums decrypt to np.cumsum of the plaintexts bit for
bit.
"""
import numpy as np
import pytest

from tests import dropin_cases as C
from tests.conftest import load_fixture

DJN = "paillier_2048_djn.json"
SIZES = (1, 5, 70)


def keys():
    return C.ctxs(load_fixture(DJN))


def plain(n, tag=0):
    return np.random.default_rng(100 + tag).integers(-4000, 4000, n) / 8.0


def encrypt(pub, vals, precision=7):
    from xfl_amd.paillier import Paillier
    return Paillier.encrypt(pub, np.asarray(vals, dtype=np.float64), precision=precision, obfuscation=False)


def ints(arr):
    """(residues, exponents) of a PaillierArray or object array, C order"""
    return C.raw(arr)


def prefix(raws, n2, lengths=None):
    """Python-integer inclusive prefix products, per run of `lengths`"""
    out, i = [], 0
    for ln in [len(raws)] if lengths is None else lengths:
        acc = 1
        for c in raws[i:i + ln]:
            acc = acc * c % n2
            out.append(acc)
        i += ln
    return out


def same_elements(got, want):
    """element for element: NaN where want has NaN, else equal residue and exponent"""
    got, want = list(got), list(want)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        if isinstance(w, float):
            assert isinstance(g, float) and np.isnan(g) and np.isnan(w), i
        else:
            assert (g.raw_ciphertext, g.exponent) == (w.raw_ciphertext, w.exponent), i


def scans(calls):
    """np.cumsum(arr), arr.cumsum() and both axes of the 3 x 7 array"""
    from xfl_amd.paillier import Paillier, PaillierArray
    priv, pub = keys()
    n2 = pub.n * pub.n
    for n in SIZES:
        vals = plain(n, n)
        arr = encrypt(pub, vals)
        raws, exps = ints(arr)
        assert len(set(exps)) == 1
        for res in (np.cumsum(arr), arr.cumsum()):
            assert isinstance(res, PaillierArray) and res.shape == (n,)
            assert ints(res) == (prefix(raws, n2), exps)
            assert res.is_resident == arr.is_resident
            assert np.array_equal(Paillier.decrypt(priv, res), np.cumsum(vals))
    vals = plain(21, 21).reshape(3, 7)
    a2d = encrypt(pub, vals)
    raws, exps = ints(a2d)
    grid = np.array(raws, dtype=object).reshape(3, 7)
    before = len(calls)
    for axis, lines in ((0, [list(grid[:, j]) for j in range(7)]), (1, [list(grid[i]) for i in range(3)])):
        res = np.cumsum(a2d, axis=axis)
        assert isinstance(res, PaillierArray) and res.shape == (3, 7)
        want = np.empty((3, 7), dtype=object)
        for t, line in enumerate(lines):
            if axis == 0:
                want[:, t] = prefix(line, n2)
            else:
                want[t] = prefix(line, n2)
        assert ints(res) == (list(want.reshape(-1)), exps), axis
        assert res.is_resident == a2d.is_resident
        assert np.array_equal(Paillier.decrypt(priv, res), np.cumsum(vals, axis=axis))
        assert ints(a2d.cumsum(axis=axis - 2)) == ints(res)  # negative axes, the method
    assert len(calls) == before + 4  # one segmented scan per call, whatever the number of lines
    flat = np.cumsum(a2d)  # axis=None: the flattened array, 1-D
    assert flat.shape == (21,) and ints(flat) == (prefix(raws, n2), exps)


def pandas_columns(calls):
    """Series.cumsum and DataFrame.cumsum give the same words"""
    import pandas as pd

    from xfl_amd.paillier import PaillierArray
    priv, pub = keys()
    n2 = pub.n * pub.n
    arr, arr2 = encrypt(pub, plain(70, 1)), encrypt(pub, plain(70, 2))
    before = len(calls)
    s = pd.Series(arr).cumsum()
    assert isinstance(s.array, PaillierArray) and len(calls) == before + 1
    assert ints(s.array) == (prefix(ints(arr)[0], n2), ints(arr)[1])
    df = pd.DataFrame({"a": arr, "b": arr2}).cumsum()
    for name, src in (("a", arr), ("b", arr2)):
        assert isinstance(df[name].array, PaillierArray)
        assert ints(df[name].array) == (prefix(ints(src)[0], n2), ints(src)[1]), name
    with pytest.raises((TypeError, NotImplementedError)):
        pd.Series(arr).cumprod()


def fallbacks(calls):
    """NA entries, two exponents in a line, dtype/out arguments: the reference's
    object fold, no segscan call. A column with NA entries gives what pandas
    gives for the object column: its elements, or its exception (see below
    which of the two each skipna value is today)."""
    import pandas as pd

    from xfl_amd.paillier import PaillierArray
    priv, pub = keys()
    arr = encrypt(pub, plain(5, 3))
    before = len(calls)
    holes = encrypt(pub, plain(8, 4)).take([0, 1, -1, 2, 3, -1, -1, 4, 5], allow_fill=True)
    assert holes._has_na()
    for skipna in (True, False):
        # whatever pandas makes of the object column: element for element, or the same error. Under pandas
        # 2.3.3: skipna=True is compared element for element (pandas masks the missing entries, folds the rest
        # and puts NaN back where they were); skipna=False takes the error branch - pandas hands NaN +
        # ciphertext to PaillierCiphertext.__radd__, which refuses to encrypt NaN, as the reference's does
        # (ValueError) - so there only the exception's type and message are compared
        try:
            want = pd.Series(np.asarray(holes), dtype=object).cumsum(skipna=skipna)
        except Exception as exc:  # noqa: BLE001
            with pytest.raises(type(exc)) as info:
                pd.Series(holes).cumsum(skipna=skipna)
            assert str(info.value) == str(exc)
            continue
        got = pd.Series(holes).cumsum(skipna=skipna)
        assert isinstance(got.array, PaillierArray)
        same_elements(np.asarray(got.array), want.to_numpy(dtype=object))
    mixed = PaillierArray._concat_same_type([encrypt(pub, plain(3, 5)), encrypt(pub, plain(3, 6), precision=5)])
    assert len(set(mixed.exponents.tolist())) == 2
    for got in (np.cumsum(mixed), mixed.cumsum()):
        same_elements(np.asarray(got), np.cumsum(np.asarray(mixed)))
    want = np.cumsum(np.asarray(arr))
    out = np.empty(5, dtype=object)
    same_elements(np.asarray(np.cumsum(arr, dtype=object, out=out)), want)
    same_elements(out, want)
    out2 = np.empty(5, dtype=object)
    same_elements(np.asarray(arr.cumsum(dtype=object, out=out2)), want)
    same_elements(out2, want)
    assert len(calls) == before


def lines_of_different_exponents(calls):
    """a 2 x 3 array whose rows have different exponents: axis=1 is one call, axis=0 the fallback"""
    from xfl_amd.paillier import PaillierArray
    priv, pub = keys()
    two = PaillierArray._concat_same_type([encrypt(pub, plain(3, 7)), encrypt(pub, plain(3, 8), precision=5)])
    two = two.reshape(2, 3)
    before = len(calls)
    res = np.cumsum(two, axis=1)
    assert len(calls) == before + 1 and isinstance(res, PaillierArray) and res.shape == (2, 3)
    same_elements(np.asarray(res).reshape(-1), np.cumsum(np.asarray(two), axis=1).reshape(-1))
    same_elements(np.asarray(np.cumsum(two, axis=0)).reshape(-1), np.cumsum(np.asarray(two), axis=0).reshape(-1))
    assert len(calls) == before + 1


def segments(calls):
    """cumsum_segments: lengths [3, 0, 5, 1] equal the four separate scans, in one call"""
    from xfl_amd.paillier import PaillierArray
    from xfl_amd.paillier_acceleration import cumsum_segments
    priv, pub = keys()
    n2 = pub.n * pub.n
    arr = encrypt(pub, plain(9, 9))
    lengths = [3, 0, 5, 1]
    parts = [np.cumsum(arr[lo:hi]) for lo, hi in ((0, 3), (3, 8), (8, 9))]
    before = len(calls)
    res = cumsum_segments(arr, lengths)
    assert len(calls) == before + 1
    assert isinstance(res, PaillierArray) and res.shape == (9,) and res.is_resident == arr.is_resident
    assert ints(res)[0] == [r for p in parts for r in ints(p)[0]] == prefix(ints(arr)[0], n2, lengths)
    assert ints(res)[1] == ints(arr)[1]
    # object arrays in; runs of different exponents are eligible, a run with two is the fallback
    assert ints(cumsum_segments(np.asarray(arr), lengths)) == ints(res)
    mixed = PaillierArray._concat_same_type([encrypt(pub, plain(3, 5)), encrypt(pub, plain(3, 6), precision=5)])
    before = len(calls)
    split = cumsum_segments(mixed, [3, 3])
    assert len(calls) == before + 1
    same_elements(np.asarray(split), list(np.cumsum(np.asarray(mixed)[:3])) + list(np.cumsum(np.asarray(mixed)[3:])))
    joined = cumsum_segments(mixed, [2, 4])
    assert len(calls) == before + 1
    same_elements(np.asarray(joined), list(np.cumsum(np.asarray(mixed)[:2])) + list(np.cumsum(np.asarray(mixed)[2:])))
    for bad in ([3, 5], [3, 0, 5, 2], [10, -1], []):
        with pytest.raises(ValueError):
            cumsum_segments(arr, bad)
    with pytest.raises(ValueError, match="1-D"):
        cumsum_segments(encrypt(pub, plain(6, 1)).reshape(2, 3), [6])
    with pytest.raises(TypeError):
        cumsum_segments(np.arange(4), [4])
