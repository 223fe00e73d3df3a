"""xhe_hist_level_sparse on the GPU: every output word and count against Python
integers - the plain per-(node, feature, bin) product over ALL rows mod n^2
(the reference of tests/test_gpu_hist_level.py, which knows nothing of zero
bins) - through the C ABI in-process, and the drop-in's level_histograms(
default_bin=...) against its dense call."""
import ctypes

import numpy as np
import pytest

from tests import cumsum_cases as CC
from tests.conftest import hx, load_fixture
from tests.test_gpu_hist import DROP, _key
from tests.test_gpu_hist_level import _reference

pytestmark = pytest.mark.gpu

EINVAL, ENOINV = -1, -4


def _data(bits, n_rows, nfeat, nbins, nnodes, zero, layout):
    """(ciphertext ints, bins, node slots) of a layout; node 0 holds about 0.6 of the rows, half of a sparse
    feature's entries lie in its zero bin"""
    dk, n2 = _key(bits)
    top = 1 << (32 * dk.n2w)
    rng = np.random.default_rng(n_rows + 7 * nbins + 13 * nfeat + 17 * nnodes)
    cs = [int.from_bytes(rng.bytes(4 * dk.n2w), "little") % n2 for _ in range(n_rows)]
    bins = rng.integers(0, nbins, (nfeat, n_rows)).astype(np.uint16)
    for f, z in enumerate(zero):
        if z < nbins:
            bins[f, rng.random(n_rows) < 0.5] = z
    node = np.where(rng.random(n_rows) < 0.6, 0, rng.integers(0, nnodes, n_rows)).astype(np.uint16)
    z0, other = zero[0], (zero[0] + 1) % nbins
    if layout == "inactive":  # node 2 without a row; ids 0xFFFF and nnodes skip their rows
        node[node == 2] = 1
        node[::5] = nnodes
        node[1] = DROP
    elif layout == "nothing_outside":
        bins[0, node == 0] = z0
    elif layout == "empty_zero_bin":
        bins[0, (node == 0) & (bins[0] == z0)] = other
    elif layout == "dropped":  # ids 0xFFFF and nbins among a sparse feature's rows; one whole feature dropped
        bins[0, ::3] = DROP
        bins[0, 1] = nbins
        bins[1, :] = DROP
    elif layout == "spread":
        node = rng.permutation(n_rows).astype(np.uint16)
    elif layout == "wide":  # rows 0, 2 outside every zero bin, rows 1, 3 inside
        bins[:, [0, 2]] = (np.array(zero)[:, None] + 1) % nbins
        bins[:, [1, 3]] = np.array(zero)[:, None]
        node[:4] = 0, 0, 1, 1
        cs[0], cs[1], cs[2], cs[3] = top - 1, n2 + 1, n2 + 1, top - 1
    elif layout in ("nonunit_outside", "nonunit_inside", "nonunit_dense"):
        f = 1 if layout == "nonunit_dense" else 0
        cs[5] = hx(load_fixture(f"paillier_{bits}_djn.json")["key"]["n"])
        bins[:, 5] = np.array(zero) % nbins  # in every sparse feature's zero bin ...
        if layout != "nonunit_inside":
            bins[f, 5] = (zero[f] + 1) % nbins  # ... but this one's
    return cs, bins, node


def _nnz(bins, nbins, node, nnodes, zero):
    live = bins[:, node < nnodes]
    return sum(int((live[f] != z).sum()) if z < nbins else live.shape[1] for f, z in enumerate(zero))


def _totals(cs, node, nnodes, n2):
    t = [1] * nnodes
    for c, v in zip(cs, node):
        if v < nnodes:
            t[v] = t[v] * c % n2
    return t


def _sparse(dk, cs, bins, nbins, node, nnodes, zero, tile_rows=64, total=None, bound_off=0, host=False, overlap=False):
    """(return code, output ints, counts) of one xhe_hist_level_sparse call"""
    import torch

    from xfl_amd import _native as nat
    L = nat.lib()
    cw = nat.ints_to_words(cs, dk.n2w) if cs else np.zeros((0, dk.n2w), np.uint32)
    zb = np.asarray(zero, np.uint16)
    tw = None if total is None else nat.ints_to_words(total, dk.n2w)
    nfeat, stride = bins.shape
    nout = nnodes * nfeat * nbins
    out, cnt = np.empty((nout, dk.n2w), np.uint32), np.empty(nout, np.int32)
    vp = lambda a: None if a is None or not a.size else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    if host:
        rc = L.xhe_hist_level_sparse_host(dk.handle, vp(cw), len(cs), vp(bins), stride, nfeat, nbins, vp(zb), vp(node),
                                          nnodes, vp(tw), tile_rows, vp(out), vp(cnt))
        return rc, nat.words_to_ints(out), cnt
    dev = lambda a: None if a is None else torch.from_numpy(a.view(np.int16 if a.itemsize == 2 else np.int32)).cuda()  # noqa: E731
    cd, bd, zd, nd, td = dev(cw), dev(bins), dev(zb), dev(node), dev(tw)
    od = torch.empty(out.shape, dtype=torch.int32, device="cuda")
    kd = torch.empty(cnt.shape, dtype=torch.int32, device="cuda")
    rc = L.xhe_hist_level_sparse(dk.handle, cd.data_ptr(), len(cs), bd.data_ptr(), stride, nfeat, nbins, zd.data_ptr(),
                                 nd.data_ptr(), nnodes, _nnz(bins, nbins, node, nnodes, zero) + bound_off,
                                 None if td is None else td.data_ptr(), tile_rows,
                                 cd.data_ptr() if overlap else od.data_ptr(), kd.data_ptr(),
                                 torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, nat.words_to_ints(od.cpu().numpy().view(np.uint32)), kd.cpu().numpy()


# (n_rows, nfeat, nbins, nnodes, zero bins, tile_rows, layout): the smallest shapes that reach each edge
EDGES = {
    "ragged": (400, 3, 4, 3, (0, 3, 2), 64, "plain"),  # node 0's lists: a full slot and a short one; the others under one
    "inactive": (200, 2, 3, 4, (1, 0), 64, "inactive"),
    "nothing_outside": (100, 2, 3, 2, (1, 0), 64, "nothing_outside"),  # zero bin = total[0], the others 1
    "empty_zero_bin": (100, 2, 3, 2, (1, 0), 64, "empty_zero_bin"),  # 1 and count 0
    "mixed": (100, 3, 4, 2, (DROP, 1, DROP), 64, "plain"),
    "all_dense": (100, 2, 3, 2, (DROP, DROP), 64, "plain"),
    "dropped": (70, 3, 4, 2, (0, 1, 2), 64, "dropped"),
    "wide": (40, 2, 3, 2, (0, 2), 64, "wide"),
    "nonunit_inside": (40, 2, 3, 2, (1, DROP), 64, "nonunit_inside"),
    "nonunit_dense": (40, 2, 3, 2, (1, DROP), 64, "nonunit_dense"),
    "single_bin": (50, 1, 1, 2, (0,), 64, "plain"),
    "max_bins": (64, 1, 4095, 2, (7,), 64, "plain"),
    "one_node": (150, 2, 3, 1, (0, 2), 64, "plain"),
    "nodes_4096": (64, 1, 2, 4096, (0,), 64, "spread"),
    "planner_tile": (3000, 4, 16, 2, (0, 5, DROP, 15), 0, "plain"),  # node 0's dense feature: 38 slots, a fold pass
    "two_launch_groups": (16400, 1, 4095, 2, (DROP,), 64, "plain"),  # 257 or 258 slots, 255 to a launch group
}
CASES = [(2048, *EDGES[e]) for e in EDGES]
CASES += [(bits, 200, *EDGES["ragged"][1:]) for bits in (3072, 4096, 8192)]


@pytest.mark.parametrize("bits,n_rows,nfeat,nbins,nnodes,zero,tile_rows,layout", CASES)
def test_hist_level_sparse_abi(bits, n_rows, nfeat, nbins, nnodes, zero, tile_rows, layout):
    dk, n2 = _key(bits)
    cs, bins, node = _data(bits, n_rows, nfeat, nbins, nnodes, zero, layout)
    rc, got, cnt = _sparse(dk, cs, bins, nbins, node, nnodes, zero, tile_rows)
    want, want_cnt = _reference(cs, bins, nbins, node, nnodes, n2)
    assert rc == 0
    assert np.array_equal(cnt, want_cnt)
    assert got == want


def test_hist_level_sparse_totals_given_host_and_bound():
    """the ragged data: supplied totals (one above n^2) give the same words, so do host buffers; a bound one short fails"""
    dk, n2 = _key(2048)
    n_rows, nfeat, nbins, nnodes, zero, tile_rows, layout = EDGES["ragged"]
    cs, bins, node = _data(2048, n_rows, nfeat, nbins, nnodes, zero, layout)
    want, want_cnt = _reference(cs, bins, nbins, node, nnodes, n2)
    total = _totals(cs, node, nnodes, n2)
    raised = [total[0], total[1] + n2, total[2]]
    for kw in (dict(total=raised), dict(host=True), dict(host=True, total=total)):
        rc, got, cnt = _sparse(dk, cs, bins, nbins, node, nnodes, zero, tile_rows, **kw)
        assert rc == 0 and got == want and np.array_equal(cnt, want_cnt), kw
    assert _sparse(dk, cs, bins, nbins, node, nnodes, zero, tile_rows, bound_off=-1)[0] == EINVAL


def test_hist_level_sparse_error_codes():
    dk, n2 = _key(2048)
    n_rows, nfeat, nbins, nnodes, zero, tile_rows, _ = EDGES["nonunit_inside"]
    cs, bins, node = _data(2048, n_rows, nfeat, nbins, nnodes, zero, "nonunit_outside")
    assert _sparse(dk, cs, bins, nbins, node, nnodes, zero)[0] == ENOINV  # c = n multiplied under a sparse feature
    assert _sparse(dk, cs, bins, 4096, node, nnodes, zero)[0] == EINVAL
    assert _sparse(dk, cs, bins, nbins, node, nnodes, zero, overlap=True)[0] == EINVAL
    rc, got, cnt = _sparse(dk, [], np.zeros((2, 0), np.uint16), 3, np.zeros(0, np.uint16), 2, (0, DROP))  # n_rows == 0
    assert rc == 0 and got == [1] * 12 and not cnt.any()


def _columns():
    """a resident column and the same ciphertexts as a host column"""
    from xfl_amd.paillier import PaillierArray
    priv, pub = CC.keys()
    arr = CC.encrypt(pub, CC.plain(300, 47))
    assert arr.is_resident
    return pub, [arr, PaillierArray.from_buffers(pub, np.array(arr.words), arr.exponents.copy())]


def test_level_histograms_default_bin_dropin():
    """default_bin with sparse=True, False and None, and total=: bit for bit level_histograms() without it"""
    from xfl_amd.paillier import PaillierArray
    from xfl_amd.paillier_acceleration import level_histograms
    pub, cols = _columns()
    rng = np.random.default_rng(8)
    bins = rng.integers(-1, 5, (3, 300))
    bins[1, rng.random(300) < 0.9] = 2
    nodes = rng.integers(-1, 3, 300)
    obj = np.asarray(cols[0])
    total = PaillierArray(np.array([obj[nodes == v].sum() for v in range(3)], dtype=object))
    for arr in cols:
        want, want_cnt = level_histograms(arr, bins, nodes, nnodes=3, nbins=5)
        for kw in (dict(sparse=True), dict(sparse=False), dict(sparse=None), dict(sparse=True, total=total)):
            sums, counts = level_histograms(arr, bins, nodes, nnodes=3, nbins=5, default_bin=[None, 2, 0], **kw)
            assert np.array_equal(np.asarray(sums.words), np.asarray(want.words)), kw
            assert np.array_equal(counts, want_cnt) and sums.is_resident == want.is_resident
            assert np.array_equal(sums.exponents, want.exponents)


def test_level_histograms_default_bin_no_inverse():
    from xfl_amd.paillier import PaillierArray
    from xfl_amd.paillier_acceleration import level_histograms
    pub, cols = _columns()
    words = np.array(cols[0].words)
    words[3] = 0
    words[3, :words.shape[1] // 2] = np.frombuffer(pub.n.to_bytes(words.shape[1] * 2, "little"), np.uint32)
    bad = PaillierArray.from_buffers(pub, words, cols[0].exponents.copy())
    bins = np.zeros((1, 300), np.int64)
    bins[0, 3] = 1
    with pytest.raises(ZeroDivisionError):
        level_histograms(bad, bins, np.arange(300) % 2, nnodes=2, nbins=2, default_bin=0, sparse=True)
