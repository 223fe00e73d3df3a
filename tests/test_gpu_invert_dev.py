"""xhe_invert_dev: batch inversion mod n^2 whose root is inverted on the device
(k_modinv, csrc/modinv_dev.hpp) - no host copy, no synchronisation, failure in
a device status word - against Python's pow(c, -1, n^2), for every key size,
tree shapes with lone children, edge residues, operands at and above n^2
(tests/wide_cases.py) and non-units (return code XHE_OK, status 1)."""
import ctypes
import math
import random

import numpy as np
import pytest

from tests import wide_cases as W

pytestmark = pytest.mark.gpu

COUNTS = {"golden-2048-nodjn": (1, 2, 3, 5, 64, 257), "golden-3072": (1, 2, 3, 5, 64, 257),
          "golden-4096": (1, 2, 3, 5, 64, 257), "golden-8192": (1, 3, 5)}
_cache = {}


def _key(name):
    """(DeviceKey, n, p, q, operands, {operand: inverse}) - the reference computed once per key"""
    if name not in _cache:
        from xfl_amd import _native as nat
        K, n, p, q, _ = W.key(name)
        dk = nat.DeviceKey(K, n, None, None, None, device=0)
        n2 = n * n
        ops = [1, n2 - 1, 2, (n2 + 1) // 2, n + 1, pow(2, 64, n2), (1 << (32 * dk.n2w)) - 1]
        ops += W.units_wide(n, dk.n2w, W.DISTINCT[K], random.Random(K))
        assert all(math.gcd(x % n2, n) == 1 for x in ops)
        _cache[name] = (dk, n, p, q, ops, {x: pow(x, -1, n2) for x in ops})
    return _cache[name]


def _rows(dk, ints):
    import torch

    from xfl_amd import _native as nat
    return torch.from_numpy(nat.ints_to_words(ints, dk.n2w).view(np.int32).copy()).cuda()


def _ints(t):
    from xfl_amd import _native as nat
    return nat.words_to_ints(t.cpu().numpy().view(np.uint32))


@pytest.mark.parametrize("name,count", [(k, c) for k, cs in COUNTS.items() for c in cs])
def test_units_exact(name, count):
    import torch

    from xfl_amd.paillier import ops
    dk, _, _, _, vals, want = _key(name)
    cs = [vals[i % len(vals)] for i in range(count)]
    out, status = ops.invert_rows_dev(dk, _rows(dk, cs), stream=torch.cuda.current_stream())
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    assert _ints(out) == [want[c] for c in cs]


@pytest.mark.parametrize("name", list(COUNTS))
def test_non_units_set_status_not_return_code(name):
    """Each non-unit alone and among units at count 5: XHE_OK, status 1 after
    the caller's synchronisation; the next call on units in the same stream
    sets status 0 and is exact."""
    import torch

    from xfl_amd import _native as nat
    dk, n, p, q, vals, want = _key(name)
    L = nat.lib()
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    status = torch.full((1,), 7, dtype=torch.int32, device="cuda")

    def call(cs):
        dc = _rows(dk, cs)
        out = torch.empty_like(dc)
        rc = L.xhe_invert_dev(dk.handle, ctypes.c_void_p(dc.data_ptr()), len(cs), ctypes.c_void_p(out.data_ptr()),
                              ctypes.c_void_p(status.data_ptr()), s)
        assert rc == nat.XHE_OK
        torch.cuda.synchronize()
        return int(status.item()), out

    units = vals[7:11]
    for bad in (0, n, n * n, p, p * q + n * n):
        assert bad < 1 << (32 * dk.n2w)
        assert call([bad])[0] == 1, hex(bad)[:12]
        assert call(units[:2] + [bad] + units[2:])[0] == 1, hex(bad)[:12]
    st, out = call(units)
    assert st == 0 and _ints(out) == [want[c] for c in units]


def test_argument_checks():
    import torch

    from xfl_amd import _native as nat
    dk = _key("golden-2048-nodjn")[0]
    L = nat.lib()
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    dc = _rows(dk, [3])
    out, status = torch.empty_like(dc), torch.full((1,), 7, dtype=torch.int32, device="cuda")
    dp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    assert L.xhe_invert_dev(dk.handle, dp(dc), 1, dp(out), None, s) == nat.XHE_EINVAL
    assert L.xhe_invert_dev(dk.handle, dp(dc), -1, dp(out), dp(status), s) == nat.XHE_EINVAL
    assert L.xhe_invert_dev(dk.handle, None, 0, None, dp(status), s) == nat.XHE_OK  # count 0: status 0, nothing else
    torch.cuda.synchronize()
    assert int(status.item()) == 0
