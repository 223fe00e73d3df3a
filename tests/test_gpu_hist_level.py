"""xhe_hist_level on the GPU: every output word and count of the level-wise
histogram against Python integers (prod c[r] mod n^2 per (node, feature, bin),
np.bincount for the counts), through the C ABI in-process, and the drop-in's
level_histograms() against the loop of histograms(rows=...) it replaces."""
import ctypes
import random

import numpy as np
import pytest

from tests import cumsum_cases as CC
from tests.test_gpu_hist import DROP, _hist, _key

pytestmark = pytest.mark.gpu


def _case(bits, n_rows, nfeat, nbins, nnodes, layout):
    """(ciphertext ints, bins [nfeat, n_rows] uint16, node slots [n_rows] uint16) of a layout"""
    dk, n2 = _key(bits)
    rnd = random.Random(n_rows * 131 + nbins + 7 * nnodes)
    rng = np.random.default_rng(n_rows + 7 * nbins + 11 * nnodes)
    cs = [rnd.randrange(n2) for _ in range(n_rows)]
    bins = rng.integers(0, nbins, (nfeat, n_rows)).astype(np.uint16)
    node = rng.integers(0, nnodes, n_rows).astype(np.uint16)
    if layout == "ragged":  # node sizes 65 / 0 / 1 / 64 at tile 64: 2, 0, 1, 1 tiles
        node = rng.permutation(np.repeat([0, 2, 3], [65, 1, 64])).astype(np.uint16)
    elif layout == "inactive":
        node[::3] = nnodes
        node[1] = DROP
        node[node == 0] = nnodes
    elif layout == "onenode":
        node[:] = 2
    elif layout == "own":
        node = rng.permutation(n_rows).astype(np.uint16)
    elif layout == "big":  # 2,200 rows in node 0 (35 tiles of 64: two fold passes), 3 in node 1
        node = rng.permutation(np.repeat([0, 1], [n_rows - 3, 3])).astype(np.uint16)
    elif layout == "dropped":
        bins[0, :] = DROP
        bins[1, ::3] = DROP
        bins[1, 1] = nbins  # the first id past the bins drops too
    elif layout == "wide":
        top = 1 << (32 * dk.n2w)
        cs[0], cs[n_rows // 2], cs[-1] = n2, n2 + 1, top - 1
        node[0], node[n_rows // 2], node[-1] = 0, 1, 2
    return cs, bins, node


def _level(dk, cs, bins, nbins, node, nnodes, tile_rows, host=False):
    import torch

    from xfl_amd import _native as nat
    L = nat.lib()
    cw = nat.ints_to_words(cs, dk.n2w)
    nfeat, stride = bins.shape
    total = nnodes * nfeat * nbins
    out, cnt = np.empty((total, dk.n2w), np.uint32), np.empty(total, np.int32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    if host:
        nat.check(L.xhe_hist_level_host(dk.handle, vp(cw), len(cs), vp(bins), stride, nfeat, nbins, vp(node), nnodes,
                                        tile_rows, vp(out), vp(cnt)), "hist_level_host")
        return nat.words_to_ints(out), cnt
    dev = lambda a: torch.from_numpy(a.view(np.int16 if a.itemsize == 2 else np.int32)).cuda()  # noqa: E731
    cd, bd, nd = dev(cw), dev(bins), dev(node)
    od = torch.empty(out.shape, dtype=torch.int32, device="cuda")
    kd = torch.empty(cnt.shape, dtype=torch.int32, device="cuda")
    nat.check(L.xhe_hist_level(dk.handle, cd.data_ptr(), len(cs), bd.data_ptr(), stride, nfeat, nbins, nd.data_ptr(),
                               nnodes, tile_rows, od.data_ptr(), kd.data_ptr(),
                               torch.cuda.current_stream().cuda_stream), "hist_level")
    torch.cuda.synchronize()
    return nat.words_to_ints(od.cpu().numpy().view(np.uint32)), kd.cpu().numpy()


def _reference(cs, bins, nbins, node, nnodes, n2):
    nfeat = bins.shape[0]
    acc = [1] * (nnodes * nfeat * nbins)
    keys = []
    for f, fb in enumerate(bins):
        ok = (node < nnodes) & (fb < nbins)
        key = (node.astype(np.int64) * nfeat + f) * nbins + fb
        for r in np.flatnonzero(ok):
            acc[key[r]] = acc[key[r]] * cs[r] % n2
        keys.append(key[ok])
    return acc, np.bincount(np.concatenate(keys), minlength=len(acc))


# (n_rows, nfeat, nbins, nnodes, tile_rows, layout): the smallest shapes that reach each edge
EDGES = {
    "trivial": (1, 1, 1, 1, 64, "plain"),
    "one_node": (70, 2, 3, 1, 64, "plain"),
    "ragged": (130, 2, 3, 4, 64, "ragged"),
    "inactive": (100, 2, 3, 3, 64, "inactive"),
    "one_of_four": (100, 2, 3, 4, 64, "onenode"),
    "own_node": (100, 1, 2, 100, 64, "own"),  # the maximum padding
    "nodes_4096": (100, 1, 2, 4096, 64, "plain"),
    "fold_passes": (2203, 1, 2, 2, 64, "big"),
    "dropped": (70, 2, 4, 2, 64, "dropped"),
    "wide": (40, 2, 3, 3, 64, "wide"),
    "bins_4096": (100, 3, 4096, 3, 64, "plain"),
    "planner_tile": (3000, 4, 16, 8, 0, "plain"),
}
CASES = [(bits, *EDGES[e]) for bits in (2048, 3072) for e in EDGES]
CASES += [(bits, *EDGES["ragged"]) for bits in (4096, 8192)]


@pytest.mark.parametrize("bits,n_rows,nfeat,nbins,nnodes,tile_rows,layout", CASES)
def test_hist_level_abi(bits, n_rows, nfeat, nbins, nnodes, tile_rows, layout):
    dk, n2 = _key(bits)
    cs, bins, node = _case(bits, n_rows, nfeat, nbins, nnodes, layout)
    got, cnt = _level(dk, cs, bins, nbins, node, nnodes, tile_rows)
    want, want_cnt = _reference(cs, bins, nbins, node, nnodes, n2)
    assert np.array_equal(cnt, want_cnt)
    assert got == want
    if nnodes == 1:  # word for word xhe_hist on the same input
        hist, hist_cnt = _hist(dk, cs, bins, nbins, None, tile_rows)
        assert got == hist and np.array_equal(cnt, hist_cnt)


def test_hist_level_empty_call():
    """n_rows == 0 writes ones and zero counts"""
    dk, _ = _key(2048)
    got, cnt = _level(dk, [], np.zeros((2, 0), np.uint16), 3, np.zeros(0, np.uint16), 2, 0, host=True)
    assert got == [1] * 12 and not cnt.any()


def test_hist_level_host_equals_device():
    dk, n2 = _key(2048)
    cs, bins, node = _case(2048, 130, 2, 3, 4, "ragged")
    got, cnt = _level(dk, cs, bins, 3, node, 4, 64, host=True)
    dev, dev_cnt = _level(dk, cs, bins, 3, node, 4, 64)
    assert got == dev == _reference(cs, bins, 3, node, 4, n2)[0] and np.array_equal(cnt, dev_cnt)


@pytest.mark.parametrize("bad", [dict(nnodes=0), dict(nnodes=4097), dict(nbins=0), dict(nbins=4097), dict(nfeat=0),
                                 dict(n_rows=-1), dict(stride=9), dict(tile_rows=32), dict(tile_rows=96),
                                 dict(tile_rows=16384), dict(overlap=True)])
def test_hist_level_argument_errors(bad):
    import torch

    from xfl_amd import _native as nat
    dk, _ = _key(2048)
    a = dict(n_rows=10, stride=10, nfeat=2, nbins=4, nnodes=2, tile_rows=64, overlap=False)
    a.update(bad)
    c = torch.zeros((10, dk.n2w), dtype=torch.int32, device="cuda")
    b = torch.zeros((2, 10), dtype=torch.int16, device="cuda")
    nd = torch.zeros(10, dtype=torch.int16, device="cuda")
    out = torch.zeros(16, dtype=torch.int32, device="cuda")  # (never written: every call is refused)
    rc = nat.lib().xhe_hist_level(dk.handle, c.data_ptr(), a["n_rows"], b.data_ptr(), a["stride"], a["nfeat"],
                                  a["nbins"], nd.data_ptr(), a["nnodes"], a["tile_rows"],
                                  c.data_ptr() if a["overlap"] else out.data_ptr(), None,
                                  torch.cuda.current_stream().cuda_stream)
    assert rc == -1  # XHE_EINVAL


def _level_launches(fn):
    """(fn(), the number of xhe_hist_level calls the library timed while it ran)"""
    import torch

    from xfl_amd import _native as nat
    L = nat.lib()
    L.xhe_profile(1)
    try:
        res = fn()
        torch.cuda.synchronize()
        ms, launches = ctypes.c_double(), ctypes.c_int64()
        L.xhe_profile_read(b"k_hist_level", ctypes.byref(ms), ctypes.byref(launches))
    finally:
        L.xhe_profile(0)
    return res, launches.value


def test_level_histograms_dropin():
    """level_histograms() on a resident column: bit for bit the loop of histograms(rows=...) per node"""
    from xfl_amd.paillier_acceleration import histograms, level_histograms
    priv, pub = CC.keys()
    n, nfeat, nbins, nnodes = 300, 3, 5, 4
    arr = CC.encrypt(pub, CC.plain(n, 41))
    assert arr.is_resident
    rng = np.random.default_rng(6)
    bins = rng.integers(-1, nbins, (nfeat, n))
    nodes = rng.integers(-1, nnodes, n).astype(np.float64)
    nodes[nodes < 0] = np.nan  # a finished leaf
    (sums, counts), launches = _level_launches(lambda: level_histograms(arr, bins, nodes, nnodes, nbins))
    assert launches == 1
    assert sums.shape == (nnodes, nfeat, nbins) and sums.is_resident and counts.dtype == np.int64
    for v in range(nnodes):
        want, want_cnt = histograms(arr, bins, nbins=nbins, rows=np.flatnonzero(nodes == v))
        assert np.array_equal(np.asarray(sums[v].words), np.asarray(want.words))
        assert np.array_equal(counts[v], want_cnt)


def test_level_histograms_mixed_exponents_fall_back():
    """two exponents in the column: the per-node loop, the plaintext sums of the object fold"""
    from xfl_amd.paillier import Paillier, PaillierArray
    from xfl_amd.paillier_acceleration import level_histograms
    priv, pub = CC.keys()
    vals = CC.plain(40, 43)
    arr = PaillierArray._concat_same_type([CC.encrypt(pub, vals[:20]), CC.encrypt(pub, vals[20:], precision=3)])
    bins, nodes = np.arange(40).reshape(1, 40) % 4, np.arange(40) // 4 % 2
    (sums, counts), launches = _level_launches(lambda: level_histograms(arr, bins, nodes))
    assert launches == 0 and sums.shape == (2, 1, 4)
    obj = np.asarray(arr)
    for v in range(2):
        fold = np.array([obj[(bins[0] == b) & (nodes == v)].sum() for b in range(4)], dtype=object)
        assert np.array_equal(Paillier.decrypt(priv, sums[v][0]), Paillier.decrypt(priv, fold))
        assert counts[v][0].tolist() == [5] * 4
