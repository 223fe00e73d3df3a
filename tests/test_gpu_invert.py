"""Batch inversion mod n^2 (xhe_invert: PaillierCiphertext._raw_mul's
invert branch, paillier.py:173-187, utils.py:71-76) across the batch sizes
of its shapes - the whole-block product tree (2048-bit keys, up to 256
elements, k_wtree_*) and the level-by-level tree of larger batches - against
Python's pow(c, -1, n^2), with odd sizes (lone children at every level) and
edge residues; a non-invertible element fails with XHE_ENOINV, also one at
or above n^2 (a payload value is not reduced before it gets here)."""
import random

import numpy as np
import pytest

from tests.conftest import hx, load_fixture

pytestmark = pytest.mark.gpu


def _run(counts, seed=7):
    import torch

    from xfl_amd import _native as nat
    k = load_fixture("paillier_2048_djn.json")["key"]
    n, p = hx(k["n"]), hx(k["p"])
    n2 = n * n
    dk = nat.DeviceKey(2048, n, None, None, None, device=0)
    L = nat.lib()
    rng = random.Random(seed)
    s = torch.cuda.current_stream().cuda_stream
    for count in counts:
        cs = [rng.randrange(1, n2) for _ in range(count)]
        edges = [1, n2 - 1, n + 1, 2, (1 << 4095) % n2]
        cs[:min(count, len(edges))] = edges[:count]
        cs = [c if c % p and c % (n // p) else c + 1 for c in cs]
        dc = torch.from_numpy(nat.ints_to_words(cs, dk.n2w).view(np.int32).copy()).cuda()
        out = torch.empty_like(dc)
        nat.check(L.xhe_invert(dk.handle, dc.data_ptr(), count, out.data_ptr(), s), "invert")
        torch.cuda.synchronize()
        got = nat.words_to_ints(out.cpu().numpy().view(np.uint32))
        for i, (c, g) in enumerate(zip(cs, got)):
            assert g == pow(c, -1, n2), (count, i)
    # an element sharing the factor p has no inverse
    bad = torch.from_numpy(nat.ints_to_words([3, p * 5, 7], dk.n2w).view(np.int32).copy()).cuda()
    out = torch.empty_like(bad)
    assert L.xhe_invert(dk.handle, bad.data_ptr(), 3, out.data_ptr(), s) == nat.XHE_ENOINV


@pytest.mark.parametrize("counts", [[1, 2, 3, 7, 64], [129, 255, 256], [257, 1000]])
def test_invert_batch_sizes(counts):
    _run(counts)


def test_invert_no_inverse_level_tree():
    """The level-by-level tree's no-inverse return, in both of its shapes: 300
    elements (above the whole-block tree's kWtreeMax = 256: 16 lanes) and 4,100
    (above kN2RowMax = 4096: 4 lanes; both in csrc/paths.hpp), each with one multiple of p in the middle;
    the next valid batch in the same process still inverts."""
    import torch

    from xfl_amd import _native as nat
    k = load_fixture("paillier_2048_djn.json")["key"]
    n, p = hx(k["n"]), hx(k["p"])
    n2 = n * n
    dk = nat.DeviceKey(2048, n, None, None, None, device=0)
    L = nat.lib()
    rng = random.Random(11)
    s = torch.cuda.current_stream().cuda_stream

    def batch(count, bad):
        cs = [rng.randrange(1, n2) for _ in range(count)]
        cs = [c if c % p and c % (n // p) else c + 1 for c in cs]
        if bad:
            cs[count // 2] = p * 5
        dc = torch.from_numpy(nat.ints_to_words(cs, dk.n2w).view(np.int32).copy()).cuda()
        return cs, dc, torch.empty_like(dc)

    for count in (300, 4100):
        _, dc, out = batch(count, True)
        assert L.xhe_invert(dk.handle, dc.data_ptr(), count, out.data_ptr(), s) == nat.XHE_ENOINV, count
    cs, dc, out = batch(300, False)
    nat.check(L.xhe_invert(dk.handle, dc.data_ptr(), 300, out.data_ptr(), s), "invert")
    torch.cuda.synchronize()
    got = nat.words_to_ints(out.cpu().numpy().view(np.uint32))
    for i, (c, g) in enumerate(zip(cs, got)):
        assert g == pow(c, -1, n2), i


@pytest.mark.parametrize("count", [3, 300, 4200])
def test_invert_no_inverse_above_n_square(count):
    """A batch of units at and above n^2 (tests/wide_cases.py) with one operand
    in the middle whose residue mod n^2 has no inverse - a multiple of p plus
    q_max n^2, then q_max n^2 itself (residue 0), then n^2 + n: XHE_ENOINV in
    the whole-block tree and in both shapes of the level tree; the same batch
    without it inverts to pow(c mod n^2, -1, n^2)."""
    import torch

    from tests import wide_cases as W
    from xfl_amd import _native as nat
    k = load_fixture("paillier_2048_djn.json")["key"]
    n, p = hx(k["n"]), hx(k["p"])
    n2 = n * n
    dk = nat.DeviceKey(2048, n, None, None, None, device=0)
    L = nat.lib()
    s = torch.cuda.current_stream().cuda_stream
    qm = W.q_max(n, dk.n2w)
    assert qm >= 2
    units = W.units_wide(n, dk.n2w, 32, random.Random(13))
    cs = [units[(i + count) % 32] for i in range(count)]
    for bad in (5 * p + qm * n2, qm * n2, n2 + n):
        assert bad < 1 << (32 * dk.n2w)
        row = cs[:count // 2] + [bad] + cs[count // 2 + 1:]
        dc = torch.from_numpy(nat.ints_to_words(row, dk.n2w).view(np.int32).copy()).cuda()
        out = torch.empty_like(dc)
        assert L.xhe_invert(dk.handle, dc.data_ptr(), count, out.data_ptr(), s) == nat.XHE_ENOINV, (count, hex(bad)[:12])
    dc = torch.from_numpy(nat.ints_to_words(cs, dk.n2w).view(np.int32).copy()).cuda()
    out = torch.empty_like(dc)
    nat.check(L.xhe_invert(dk.handle, dc.data_ptr(), count, out.data_ptr(), s), "invert")
    torch.cuda.synchronize()
    got = nat.words_to_ints(out.cpu().numpy().view(np.uint32))
    want = {c: pow(c, -1, n2) for c in units}
    assert [want[c] for c in cs] == got
