"""xhe_hist_sparse on the GPU: every output word and count against Python
integers - the plain per-(feature, bin) product over ALL the call's elements
mod n^2 (the reference of tests/test_gpu_hist.py, which knows nothing of zero
bins) - through the C ABI in-process, and the drop-in's histograms(
default_bin=...) against its dense call."""
import ctypes

import numpy as np
import pytest

from tests import cumsum_cases as CC
from tests.conftest import hx, load_fixture
from tests.test_gpu_hist import DROP, _key, _reference

pytestmark = pytest.mark.gpu

EINVAL, ENOINV = -1, -4


def _data(bits, n_rows, nfeat, nbins, zero, layout):
    """(ciphertext ints, bins, row ids or None) of a layout; density about a half outside the zero bins"""
    dk, n2 = _key(bits)
    top = 1 << (32 * dk.n2w)
    rng = np.random.default_rng(n_rows + 7 * nbins + 13 * nfeat)
    cs = [int.from_bytes(rng.bytes(4 * dk.n2w), "little") % n2 for _ in range(n_rows)]
    bins = rng.integers(0, nbins, (nfeat, n_rows)).astype(np.uint16)
    for f, z in enumerate(zero):
        if z < nbins:
            bins[f, rng.random(n_rows) < 0.5] = z
    rows = None
    z0 = zero[0]
    if layout == "nothing_outside":
        bins[0, :] = z0
    elif layout == "empty_zero_bin":
        bins[0, bins[0] == z0] = (z0 + 1) % nbins
    elif layout == "dropped":  # ids 0xFFFF and nbins among a sparse feature's rows; one whole feature dropped
        bins[0, ::3] = DROP
        bins[0, 1] = nbins
        bins[1, :] = DROP
    elif layout == "rows":
        rows = rng.integers(0, n_rows, n_rows - 30).astype(np.int32)
    elif layout == "wide":  # rows 0, 2 outside every zero bin, rows 1, 3 inside
        bins[:, [0, 2]] = (np.array(zero)[:, None] + 1) % nbins
        bins[:, [1, 3]] = np.array(zero)[:, None]
        cs[0], cs[1], cs[2], cs[3] = top - 1, n2 + 1, n2 + 1, top - 1
    elif layout in ("nonunit_outside", "nonunit_inside"):
        n = hx(load_fixture(f"paillier_{bits}_djn.json")["key"]["n"])
        cs[5] = n
        bins[0, 5] = z0 if layout == "nonunit_inside" else (z0 + 1) % nbins
    return cs, bins, rows


def _nnz(bins, nbins, zero, rows):
    sel = bins if rows is None else bins[:, rows]
    return sum(int((sel[f] != z).sum()) if z < nbins else sel.shape[1] for f, z in enumerate(zero))


def _sparse(dk, cs, bins, nbins, zero, rows=None, tile_rows=64, total=None, bound_off=0, host=False, overlap=False):
    """(return code, output ints, counts) of one xhe_hist_sparse call"""
    import torch

    from xfl_amd import _native as nat
    L = nat.lib()
    cw = nat.ints_to_words(cs, dk.n2w) if cs else np.zeros((0, dk.n2w), np.uint32)
    zb = np.asarray(zero, np.uint16)
    tw = None if total is None else nat.ints_to_words([total], dk.n2w)
    nfeat, stride = bins.shape
    count = len(cs) if rows is None else len(rows)
    out, cnt = np.empty((nfeat * nbins, dk.n2w), np.uint32), np.empty(nfeat * nbins, np.int32)
    vp = lambda a: None if a is None or not a.size else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    if host:
        rc = L.xhe_hist_sparse_host(dk.handle, vp(cw), len(cs), vp(bins), stride, nfeat, nbins, vp(zb), vp(rows), count,
                                    vp(tw), tile_rows, vp(out), vp(cnt))
        return rc, nat.words_to_ints(out), cnt
    dev = lambda a: None if a is None else torch.from_numpy(a.view(np.int16 if a.itemsize == 2 else np.int32)).cuda()  # noqa: E731
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    cd, bd, zd, rd, td = dev(cw), dev(bins), dev(zb), dev(rows), dev(tw)
    od = torch.empty(out.shape, dtype=torch.int32, device="cuda")
    kd = torch.empty(cnt.shape, dtype=torch.int32, device="cuda")
    rc = L.xhe_hist_sparse(dk.handle, cd.data_ptr(), len(cs), bd.data_ptr(), stride, nfeat, nbins, zd.data_ptr(),
                           ptr(rd), count, _nnz(bins, nbins, zero, rows) + bound_off, ptr(td), tile_rows,
                           cd.data_ptr() if overlap else od.data_ptr(), kd.data_ptr(),
                           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, nat.words_to_ints(od.cpu().numpy().view(np.uint32)), kd.cpu().numpy()


# (n_rows, nfeat, nbins, zero bins, tile_rows, layout): the smallest shapes that reach each edge
EDGES = {
    "ragged_tiles": (400, 3, 4, (0, 3, 2), 64, "plain"),  # lists of about 150 ids: two full slots and a short one
    "nothing_outside": (100, 2, 3, (1, 0), 64, "nothing_outside"),  # zero bin = T, the others 1
    "empty_zero_bin": (100, 2, 3, (1, 0), 64, "empty_zero_bin"),  # 1 and count 0
    "mixed": (100, 3, 4, (DROP, 1, DROP), 64, "plain"),
    "all_dense": (100, 2, 3, (DROP, DROP), 64, "plain"),
    "dropped": (70, 3, 4, (0, 1, 2), 64, "dropped"),
    "row_list": (120, 2, 3, (2, 0), 64, "rows"),
    "wide": (40, 2, 3, (0, 2), 64, "wide"),
    "nonunit_inside": (40, 2, 3, (1, DROP), 64, "nonunit_inside"),
    "single_bin": (50, 1, 1, (0,), 64, "plain"),
    "max_bins": (64, 1, 4095, (7,), 64, "plain"),
    "planner_tile": (3000, 4, 16, (0, 5, DROP, 15), 0, "plain"),  # 47 slots of the dense feature: a fold pass
    "two_launch_groups": (16400, 1, 4095, (DROP,), 64, "plain"),  # 257 slots, 255 to a launch group at 4096 bins
}
CASES = [(2048, *EDGES[e]) for e in EDGES]
CASES += [(bits, 200, *EDGES["ragged_tiles"][1:]) for bits in (3072, 4096, 8192)]


@pytest.mark.parametrize("bits,n_rows,nfeat,nbins,zero,tile_rows,layout", CASES)
def test_hist_sparse_abi(bits, n_rows, nfeat, nbins, zero, tile_rows, layout):
    dk, n2 = _key(bits)
    cs, bins, rows = _data(bits, n_rows, nfeat, nbins, zero, layout)
    rc, got, cnt = _sparse(dk, cs, bins, nbins, zero, rows, tile_rows)
    want, want_cnt = _reference(cs, bins, nbins, rows, n2)
    assert rc == 0
    assert np.array_equal(cnt, want_cnt)
    assert got == want


def test_hist_sparse_total_given_host_and_bound():
    """the ragged data: a supplied total (above n^2) gives the same words, so do host buffers; a bound one short fails"""
    dk, n2 = _key(2048)
    n_rows, nfeat, nbins, zero, tile_rows, layout = EDGES["ragged_tiles"]
    cs, bins, rows = _data(2048, n_rows, nfeat, nbins, zero, layout)
    want, want_cnt = _reference(cs, bins, nbins, rows, n2)
    total = 1
    for c in cs:
        total = total * c % n2
    for kw in (dict(total=total + n2), dict(host=True), dict(host=True, total=total)):
        rc, got, cnt = _sparse(dk, cs, bins, nbins, zero, rows, tile_rows, **kw)
        assert rc == 0 and got == want and np.array_equal(cnt, want_cnt), kw
    assert _sparse(dk, cs, bins, nbins, zero, rows, tile_rows, bound_off=-1)[0] == EINVAL


def test_hist_sparse_error_codes():
    dk, n2 = _key(2048)
    n_rows, nfeat, nbins, zero, tile_rows, _ = EDGES["nonunit_inside"]
    cs, bins, rows = _data(2048, n_rows, nfeat, nbins, zero, "nonunit_outside")
    assert _sparse(dk, cs, bins, nbins, zero)[0] == ENOINV  # c = n multiplied under a sparse feature
    assert _sparse(dk, cs, bins, 4096, zero)[0] == EINVAL
    assert _sparse(dk, cs, bins, nbins, zero, overlap=True)[0] == EINVAL
    rc, got, cnt = _sparse(dk, [], np.zeros((2, 0), np.uint16), 3, (0, DROP))  # count == 0
    assert rc == 0 and got == [1] * 6 and not cnt.any()


def _columns():
    """a resident column and the same ciphertexts as a host column"""
    from xfl_amd.paillier import PaillierArray
    priv, pub = CC.keys()
    arr = CC.encrypt(pub, CC.plain(300, 47))
    assert arr.is_resident
    return pub, [arr, PaillierArray.from_buffers(pub, np.array(arr.words), arr.exponents.copy())]


def test_histograms_default_bin_dropin():
    """default_bin with sparse=True, False and None: bit for bit histograms() without it"""
    from xfl_amd.paillier_acceleration import histograms
    pub, cols = _columns()
    rng = np.random.default_rng(8)
    bins = rng.integers(-1, 5, (3, 300))
    bins[1, rng.random(300) < 0.9] = 2
    rows = rng.integers(0, 300, 170)
    total = np.asarray(cols[0])[rows].sum()
    for arr in cols:
        want, want_cnt = histograms(arr, bins, nbins=5, rows=rows)
        for kw in (dict(sparse=True), dict(sparse=False), dict(sparse=None), dict(sparse=True, total=total)):
            sums, counts = histograms(arr, bins, nbins=5, rows=rows, default_bin=[None, 2, 0], **kw)
            assert np.array_equal(np.asarray(sums.words), np.asarray(want.words)), kw
            assert np.array_equal(counts, want_cnt) and sums.is_resident == want.is_resident
            assert np.array_equal(sums.exponents, want.exponents)


def test_histograms_default_bin_no_inverse():
    from xfl_amd.paillier import PaillierArray
    from xfl_amd.paillier_acceleration import histograms
    pub, cols = _columns()
    words = np.array(cols[0].words)
    words[3] = 0
    words[3, :words.shape[1] // 2] = np.frombuffer(pub.n.to_bytes(words.shape[1] * 2, "little"), np.uint32)
    bad = PaillierArray.from_buffers(pub, words, cols[0].exponents.copy())
    bins = np.zeros((1, 300), np.int64)
    bins[0, 3] = 1
    with pytest.raises(ZeroDivisionError):
        histograms(bad, bins, nbins=2, default_bin=0, sparse=True)
