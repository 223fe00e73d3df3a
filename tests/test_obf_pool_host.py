"""CPU: the obfuscator pool's bookkeeping and the identity behind k_enc_obf.

resident.ObfPool is driven through a fake `ops` (numpy storage, recorded
calls) and a fake device key, so no GPU is touched: every filled row carries a
serial number, and the tests follow the numbers through reserve / take /
consume / drop. The identity X + n ((m (X mod n)) mod n) - [>= n^2] n^2 ==
(1 + n m) X mod n^2 is stated in Python integers on the inputs
tests/test_gpu_obf_pool.py feeds the kernel (tests/obf_cases.py).
"""
import ctypes
import os
import pickle

import numpy as np
import pytest

from tests import obf_cases
from tests import structured_keys as SK


class FakeOps:
    """numpy rows; fill writes a fresh serial number into word 0 of each row"""

    def __init__(self):
        self.calls = []
        self.serial = 0

    def alloc(self, cap, n2w):
        self.calls.append(("alloc", cap))
        return np.zeros((cap, n2w), dtype=np.int32)

    def fill(self, dk, rows):
        k = rows.shape[0]
        rows[:, 0] = np.arange(self.serial + 1, self.serial + 1 + k)
        rows[:, 1:] = -1
        self.serial += k
        self.calls.append(("fill", dk, k))

    def zero(self, rows):
        rows[:] = 0
        self.calls.append(("zero", rows.shape[0]))

    def copy(self, dst, src):
        dst[:] = src
        self.calls.append(("copy", src.shape[0]))


class FakeKey:
    device = 0
    n2w = 4


def _pool():
    from xfl_amd.paillier.resident import ObfPool
    ops = FakeOps()
    return ObfPool(0, FakeKey.n2w, ops), ops, FakeKey()


def _ids(views):
    return [int(r[0]) for v in views for r in v]


def test_reserve_then_take():
    pool, ops, dk = _pool()
    assert pool.reserve(dk, 10) == 10
    assert ops.calls == [("alloc", 10), ("fill", dk, 10)]
    assert (pool.cap, pool.head, pool.available) == (10, 0, 10)
    views = pool.take(4)
    assert len(views) == 1 and _ids(views) == [1, 2, 3, 4]
    assert (pool.head, pool.available) == (4, 6)
    assert pool.reserve(dk, 10) == 10  # tops up the four rows behind the head
    assert ops.calls[-1] == ("fill", dk, 4)
    assert pool.reserve(dk, 6) == 10 and ops.calls[-1] == ("fill", dk, 4)  # nothing to do


def test_wrap_around_take_and_fill():
    pool, ops, dk = _pool()
    pool.reserve(dk, 10)
    assert _ids(pool.take(4)) == [1, 2, 3, 4]
    pool.reserve(dk, 10)  # rows 0..3 <- 11..14
    views = pool.take(8)  # rows 4..9, then 0..1
    assert [v.shape[0] for v in views] == [6, 2]
    assert _ids(views) == [5, 6, 7, 8, 9, 10, 11, 12]
    assert (pool.head, pool.available) == (2, 2)
    n = len(ops.calls)
    assert pool.reserve(dk, 10) == 10  # the free rows wrap: 4..9, then 0..1
    assert ops.calls[n:] == [("fill", dk, 6), ("fill", dk, 2)]
    got = _ids(pool.take(10))
    assert got == [13, 14] + list(range(15, 23))
    assert pool.available == 0


def test_partial_and_empty_take():
    pool, ops, dk = _pool()
    assert pool.take(3) == []  # no storage yet
    pool.reserve(dk, 3)
    views = pool.take(5)
    assert _ids(views) == [1, 2, 3] and pool.available == 0
    assert pool.take(1) == [] and pool.consume(2, lambda v, off: pytest.fail("nothing to launch on")) == 0


def test_no_row_is_handed_out_twice():
    pool, ops, dk = _pool()
    rnd = np.random.default_rng(5)
    seen = []
    for _ in range(200):
        pool.reserve(dk, int(rnd.integers(1, 8)))
        seen += _ids(pool.take(int(rnd.integers(0, 9))))
    assert len(seen) == len(set(seen)) and seen == sorted(seen) and 0 not in seen


def test_head_advances_when_the_launch_raises():
    pool, ops, dk = _pool()
    pool.reserve(dk, 6)
    handed = []

    def launch(view, off):
        handed.extend(_ids([view]))
        raise RuntimeError("launch failed")

    with pytest.raises(RuntimeError):
        pool.consume(4, launch)
    assert handed == [1, 2, 3, 4]
    assert (pool.head, pool.available) == (4, 2)  # gone, although nothing ran on them
    offs = []
    assert pool.consume(5, lambda v, off: offs.append((off, _ids([v])))) == 2
    assert offs == [(0, [5, 6])]


def test_consume_offsets_at_the_wrap():
    pool, ops, dk = _pool()
    pool.reserve(dk, 5)
    pool.take(3)
    pool.reserve(dk, 5)
    got = []
    assert pool.consume(5, lambda v, off: got.append((off, v.shape[0]))) == 5
    assert got == [(0, 2), (2, 3)]


def test_growth_moves_live_rows_and_zeroes_the_old_ring():
    pool, ops, dk = _pool()
    pool.reserve(dk, 4)
    pool.take(3)
    pool.reserve(dk, 4)  # live: row 3 (4), rows 0..2 (5, 6, 7)
    old = pool.rows
    assert pool.reserve(dk, 6) == 6
    assert not old.any()
    assert (pool.cap, pool.head) == (6, 0)
    assert _ids(pool.take(6)) == [4, 5, 6, 7, 8, 9]


def test_capacity_clip():
    pool, ops, dk = _pool()
    assert pool.reserve(dk, 100, max_rows=7) == 7
    assert pool.cap == 7
    assert pool.reserve(dk, 100, max_rows=0) == 7  # a smaller budget later takes nothing away


def test_drop_zeroes_the_storage():
    pool, ops, dk = _pool()
    pool.reserve(dk, 5)
    rows = pool.rows
    assert rows.any()
    pool.drop()
    assert not rows.any() and ops.calls[-1] == ("zero", 5)
    assert (pool.rows, pool.cap, pool.head, pool.available) == (None, 0, 0, 0)
    assert pool.take(1) == []
    assert pool.reserve(dk, 2) == 2  # usable again


def test_context_methods_and_ownership(monkeypatch):
    from xfl_amd.paillier.context import PaillierContext
    for name in ("reserve_obfuscators", "obfuscators_available", "drop_obfuscators"):
        assert callable(getattr(PaillierContext, name))
    ctx = PaillierContext().init(p=104729, q=1299709)  # the 10,000th and the 100,000th prime
    monkeypatch.setenv("XHE_RESIDENT", "0")  # host-buffer mode: no pool, no device key
    assert ctx.reserve_obfuscators(100) == 0 and ctx.obfuscators_available() == 0
    assert ctx._dev == {}
    # a pool lives on the device key: dropped with it, never pickled or copied
    pool, ops, dk = _pool()
    pool.reserve(dk, 3)
    dk.obf_pool = pool
    rows = pool.rows
    ctx._dev[0] = dk
    assert ctx.obfuscators_available(0) == 3
    assert pickle.loads(pickle.dumps(ctx))._dev == {}
    assert ctx.to_public()._dev == {} and ctx.to_public().obfuscators_available(0) == 0
    ctx.drop_obfuscators()
    assert dk.obf_pool is None and not rows.any() and ctx.obfuscators_available(0) == 0


def test_env_pool_size_is_read_once(monkeypatch):
    from xfl_amd.paillier import resident
    monkeypatch.setattr(resident, "_OBF_AUTO", None)
    monkeypatch.setenv("XHE_OBF_POOL", "4096")
    assert resident.obf_auto() == 4096
    monkeypatch.setenv("XHE_OBF_POOL", "7")
    assert resident.obf_auto() == 4096
    monkeypatch.setattr(resident, "_OBF_AUTO", None)
    monkeypatch.delenv("XHE_OBF_POOL")
    assert resident.obf_auto() == 0
    resident.obf_top_up(None, None)  # unset: nothing is touched


@pytest.mark.parametrize("K,name", [(K, name) for K in SK.SIZES for name in SK.names(K)])
def test_online_identity(K, name):
    """ct = X + n ((m (X mod n)) mod n), less n^2 when it reaches it, is (1 + n m) X mod n^2"""
    p, q = SK.pq(K, name)
    n = p * q
    n2 = n * n
    fired = set()
    for m, x in obf_cases.edge_pairs(n):
        assert 0 <= m < n and 0 <= x < n2
        ct, over = obf_cases.online(n, m, x)
        assert 0 <= ct < n2 and ct == (1 + n * m) * x % n2, (m.bit_length(), x.bit_length())
        fired.add(over)
    assert fired == {False, True}
    assert obf_cases.online(n, 1, n2 - 1)[1]  # the case that must take the subtraction


def test_library_exports_the_entry_points():
    from xfl_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        pytest.skip("native library not built")
    L = ctypes.CDLL(_native.LIB_PATH)
    for name in ("xhe_obf_fill", "xhe_encrypt_obf"):
        assert hasattr(L, name) and name in _native.SIGNATURES, name
