"""CPU: the cumulative sum's host logic (PaillierArray.cumsum, np.cumsum,
pandas' _accumulate, cumsum_segments) with the device entry points replaced:
tests/oracle_ops.py's stand-ins plus a Python-integer ops.segscan_words, the
ninth entry point, which records its calls. The same checks run on the real
kernel in tests/test_gpu_cumsum_dropin.py."""
import numpy as np
import pytest

from tests import cumsum_cases as CC
from tests import oracle_ops


@pytest.fixture
def calls(monkeypatch):
    from xfl_amd._native import ints_to_words, words_to_ints
    from xfl_amd.paillier import ops
    oracle_ops.install(monkeypatch)
    seen = []

    def segscan_words(ctx, cw, seg):
        seg = np.asarray(seg, dtype=np.int64)
        assert seg[0] == 0 and seg[-1] == cw.shape[0] and np.all(np.diff(seg) >= 0)
        seen.append(seg.tolist())
        raws = words_to_ints(np.ascontiguousarray(cw, dtype=np.uint32)) if cw.shape[0] else []
        out = CC.prefix(raws, ctx.n * ctx.n, np.diff(seg).tolist())
        return ints_to_words(out, cw.shape[1]) if out else np.zeros((0, cw.shape[1]), dtype=np.uint32)

    def segscan_dev(*a, **k):
        raise AssertionError("no device in this test")
    monkeypatch.setattr(ops, "segscan_words", segscan_words)
    monkeypatch.setattr(ops, "segscan_dev", segscan_dev)
    return seen


def test_scans(calls):
    CC.scans(calls)


def test_pandas_columns(calls):
    CC.pandas_columns(calls)


def test_fallbacks(calls):
    CC.fallbacks(calls)


def test_lines_of_different_exponents(calls):
    CC.lines_of_different_exponents(calls)


def test_cumsum_segments(calls):
    CC.segments(calls)
    assert [3, 0, 5, 1] in [np.diff(s).tolist() for s in calls]


def test_abi_has_segscan():
    """the header, the ctypes table and ops agree on the two new symbols"""
    import os

    from xfl_amd import _native as nat
    from xfl_amd.paillier import ops, resident
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "xhe.h")).read()
    for name in ("xhe_segscan", "xhe_segscan_host"):
        assert name in nat.SIGNATURES and f"int {name}(" in header
    assert callable(ops.segscan_words) and callable(ops.segscan_dev) and callable(resident.segscan)
