"""xhe_hist on the GPU: every output word and count of the fused multi-feature
histogram against Python integers (prod c[r] mod n^2 per (feature, bin),
np.bincount for the counts), through the C ABI in-process, and the drop-in's
histograms() against the per-feature groupby sums it replaces."""
import ctypes
import random

import numpy as np
import pytest

from tests import cumsum_cases as CC
from tests.conftest import hx, load_fixture

pytestmark = pytest.mark.gpu

DROP = 0xFFFF
_keys = {}


def _key(bits):
    """(public non-DJN device key, n^2) of the golden key of that size"""
    from xfl_amd._native import DeviceKey
    if bits not in _keys:
        n = hx(load_fixture(f"paillier_{bits}_djn.json")["key"]["n"])
        _keys[bits] = (DeviceKey(bits, n, None, None, None), n * n)
    return _keys[bits]


def _case(bits, count, nfeat, nbins, layout):
    """(ciphertext ints, bins [nfeat, stride] uint16, row ids or None) of a layout"""
    dk, n2 = _key(bits)
    rnd = random.Random(count * 131 + nbins)
    rng = np.random.default_rng(count + 7 * nbins)
    n_rows, rows = count, None
    if layout == "cyclic":  # 64 distinct ciphertexts taken cyclically
        n_rows, rows = 64, np.arange(count, dtype=np.int32) % 64
    elif layout == "subset":  # a shuffled subset with one repeated row
        n_rows = count + 9
        rows = rng.permutation(n_rows)[:count].astype(np.int32)
        rows[-1] = rows[0]
    cs = [rnd.randrange(n2) for _ in range(n_rows)]
    stride = n_rows + 3 if layout == "stride" else n_rows
    bins = np.full((nfeat, stride), 5, dtype=np.uint16)  # (the padding is never read: any id)
    bins[:, :n_rows] = rng.integers(0, nbins, (nfeat, n_rows))
    if layout in ("onebin", "cyclic"):
        bins[:, :n_rows] = nbins - 1
    elif layout == "dropped":
        bins[0, :] = DROP
        bins[1, :n_rows:3] = DROP
        bins[1, 1] = nbins  # the first id past the bins drops too
    elif layout == "wide":
        top = 1 << (32 * dk.n2w)
        cs[0], cs[count // 2], cs[-1] = n2, n2 + 1, top - 1
    return cs, bins, rows


def _hist(dk, cs, bins, nbins, rows, tile_rows, host=False):
    import torch

    from xfl_amd import _native as nat
    L = nat.lib()
    cw = nat.ints_to_words(cs, dk.n2w)
    nfeat, stride = bins.shape
    count = len(cs) if rows is None else len(rows)
    out = np.empty((nfeat * nbins, dk.n2w), np.uint32)
    cnt = np.empty(nfeat * nbins, np.int32)
    vp = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    if host:
        nat.check(L.xhe_hist_host(dk.handle, vp(cw), len(cs), vp(bins), stride, nfeat, nbins, vp(rows), count,
                                  tile_rows, vp(out), vp(cnt)), "hist_host")
        return nat.words_to_ints(out), cnt
    dev = lambda a: None if a is None else torch.from_numpy(a.view(np.int16 if a.itemsize == 2 else np.int32)).cuda()  # noqa: E731
    cd, bd, rd = dev(cw), dev(bins), dev(rows)
    od, nd = torch.empty(out.shape, dtype=torch.int32, device="cuda"), torch.empty(cnt.shape, dtype=torch.int32,
                                                                                 device="cuda")
    nat.check(L.xhe_hist(dk.handle, cd.data_ptr(), len(cs), bd.data_ptr(), stride, nfeat, nbins,
                         None if rd is None else rd.data_ptr(), count, tile_rows, od.data_ptr(), nd.data_ptr(),
                         torch.cuda.current_stream().cuda_stream), "hist")
    torch.cuda.synchronize()
    return nat.words_to_ints(od.cpu().numpy().view(np.uint32)), nd.cpu().numpy()


def _reference(cs, bins, nbins, rows, n2):
    sel = np.arange(len(cs)) if rows is None else rows
    prods, counts = [], []
    for fb in bins:
        ids = fb[sel].astype(np.int64)
        acc = [1] * nbins
        for r, b in zip(sel, ids):
            if b < nbins:
                acc[b] = acc[b] * cs[r] % n2
        prods += acc
        counts.append(np.bincount(ids[ids < nbins], minlength=nbins))
    return prods, np.concatenate(counts)


# (count, nfeat, nbins, tile_rows, layout): the smallest shapes that reach each edge
EDGES = {
    "trivial": (1, 1, 1, 64, "plain"),
    "tile_edge": (65, 2, 3, 64, "stride"),  # T = 2, one row in the last tile, stage B, empty (bin, tile)
    "two_slices": (64, 1, 2, 64, "onebin"),  # slices 32 + 32 combined in the block; bin 0 empty
    "dropped": (70, 2, 4, 64, "dropped"),
    "subset": (100, 2, 7, 64, "subset"),
    "wide": (40, 2, 3, 64, "wide"),
    "sparse_bins": (100, 3, 4096, 64, "plain"),
}
CASES = [(bits, *EDGES[e]) for bits in (2048, 3072) for e in EDGES]
CASES += [(bits, *EDGES["tile_edge"]) for bits in (4096, 8192)]
CASES += [(2048, 8192, 1, 2, 8192, "cyclic"),  # 256 slices: two combine passes
          (2048, 3000, 4, 16, 0, "plain")]  # the planner's tile


@pytest.mark.parametrize("bits,count,nfeat,nbins,tile_rows,layout", CASES)
def test_hist_abi(bits, count, nfeat, nbins, tile_rows, layout):
    dk, n2 = _key(bits)
    cs, bins, rows = _case(bits, count, nfeat, nbins, layout)
    got, cnt = _hist(dk, cs, bins, nbins, rows, tile_rows)
    want, want_cnt = _reference(cs, bins, nbins, rows, n2)
    assert np.array_equal(cnt, want_cnt)
    assert got == want


def test_hist_empty_call():
    """count == 0 writes ones and zero counts"""
    dk, n2 = _key(2048)
    got, cnt = _hist(dk, [], np.zeros((2, 0), np.uint16), 3, None, 0, host=True)
    assert got == [1] * 6 and not cnt.any()


def _hist_launches(fn):
    """(fn(), the number of xhe_hist calls the library timed while it ran)"""
    import torch

    from xfl_amd import _native as nat
    L = nat.lib()
    L.xhe_profile(1)
    try:
        res = fn()
        torch.cuda.synchronize()
        ms, launches = ctypes.c_double(), ctypes.c_int64()
        L.xhe_profile_read(b"k_hist", ctypes.byref(ms), ctypes.byref(launches))
    finally:
        L.xhe_profile(0)
    return res, launches.value


def test_hist_host_rejects_row_ids_out_of_range():
    from xfl_amd import _native as nat
    dk, _ = _key(2048)
    cw = np.zeros((4, dk.n2w), np.uint32)
    bins, out = np.zeros((1, 4), np.uint16), np.empty((2, dk.n2w), np.uint32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    for bad in (4, -1):
        rows = np.array([0, bad, 1], np.int32)
        assert nat.lib().xhe_hist_host(dk.handle, vp(cw), 4, vp(bins), 4, 1, 2, vp(rows), 3, 64, vp(out), None) == -1


def test_hist_host_equals_device():
    dk, n2 = _key(2048)
    cs, bins, rows = _case(2048, 100, 2, 7, "subset")
    got, cnt = _hist(dk, cs, bins, 7, rows, 64, host=True)
    dev, dev_cnt = _hist(dk, cs, bins, 7, rows, 64)
    assert got == dev == _reference(cs, bins, 7, rows, n2)[0] and np.array_equal(cnt, dev_cnt)


@pytest.mark.parametrize("bad", [dict(nbins=0), dict(nbins=4097), dict(nfeat=0), dict(count=-1, rows=True),
                                 dict(n_rows=-1), dict(stride=9), dict(tile_rows=32), dict(tile_rows=96),
                                 dict(tile_rows=16384), dict(count=9), dict(overlap=True)])
def test_hist_argument_errors(bad):
    import torch

    from xfl_amd import _native as nat
    dk, _ = _key(2048)
    a = dict(n_rows=10, stride=10, nfeat=2, nbins=4, count=10, tile_rows=64, rows=False, overlap=False)
    a.update(bad)
    c = torch.zeros((10, dk.n2w), dtype=torch.int32, device="cuda")
    b = torch.zeros((2, 10), dtype=torch.int16, device="cuda")
    r = torch.zeros(10, dtype=torch.int32, device="cuda")
    out = torch.zeros((2 * 4097, dk.n2w), dtype=torch.int32, device="cuda")
    rc = nat.lib().xhe_hist(dk.handle, c.data_ptr(), a["n_rows"], b.data_ptr(), a["stride"], a["nfeat"], a["nbins"],
                            r.data_ptr() if a["rows"] else None, a["count"], a["tile_rows"],
                            c.data_ptr() if a["overlap"] else out.data_ptr(), None,
                            torch.cuda.current_stream().cuda_stream)
    assert rc == -1  # XHE_EINVAL


def test_histograms_dropin():
    """histograms() on a resident column: bit for bit the per-feature groupby sums, and Python integers"""
    import pandas as pd

    from xfl_amd.paillier_acceleration import histograms
    priv, pub = CC.keys()
    n, nfeat, nbins = 300, 3, 5
    arr = CC.encrypt(pub, CC.plain(n, 41))
    assert arr.is_resident
    rng = np.random.default_rng(5)
    bins = rng.integers(-1, nbins, (nfeat, n))
    bins[:, :nbins] = np.arange(nbins)  # no empty bin
    (sums, counts), launches = _hist_launches(lambda: histograms(arr, bins))
    assert launches == 1  # one xhe_hist call served it, not the per-feature path
    assert sums.shape == (nfeat, nbins) and sums.is_resident and counts.dtype == np.int64
    raws, exps = CC.ints(arr)
    n2 = pub.n * pub.n
    for f in range(nfeat):
        data = pd.DataFrame(arr, columns=["ct"])
        data["bin"] = np.where(bins[f] < 0, np.nan, bins[f])
        res = data.groupby(["bin"])["ct"].agg(["count", "sum"])
        assert np.array_equal(np.asarray(sums[f].words), np.asarray(res["sum"].array.words))
        assert np.array_equal(counts[f], res["count"].to_numpy())
        want = [1] * nbins
        for c, b in zip(raws, bins[f]):
            if b >= 0:
                want[b] = want[b] * c % n2
        assert CC.ints(sums[f]) == (want, [exps[0]] * nbins)


def test_histograms_mixed_exponents_fall_back():
    """two exponents in the column: the per-feature groupby path, the plaintext sums of the object fold"""
    from xfl_amd.paillier import Paillier, PaillierArray
    from xfl_amd.paillier_acceleration import histograms
    priv, pub = CC.keys()
    vals = CC.plain(40, 43)
    arr = PaillierArray._concat_same_type([CC.encrypt(pub, vals[:20]), CC.encrypt(pub, vals[20:], precision=3)])
    assert len(set(arr.exponents.tolist())) == 2
    bins = np.arange(80).reshape(2, 40) % 4
    (sums, counts), launches = _hist_launches(lambda: histograms(arr, bins, nbins=4))
    assert launches == 0
    obj = np.asarray(arr)
    for f in range(2):
        fold = np.array([obj[bins[f] == b].sum() for b in range(4)], dtype=object)
        assert np.array_equal(Paillier.decrypt(priv, sums[f]), Paillier.decrypt(priv, fold))
        assert counts[f].tolist() == [10] * 4
