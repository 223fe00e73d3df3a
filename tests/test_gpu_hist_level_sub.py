"""xhe_hist_level_sub on the GPU: every output word and count of the level
histogram built by subtraction against Python integers over ALL rows (the
reference of tests/test_gpu_hist_level.py; the parent rows are that reference
on node >> 1), through the C ABI in-process, and the drop-in's
level_histograms(parent=...) against its direct call."""
import ctypes

import numpy as np
import pytest

from tests import cumsum_cases as CC
from tests.conftest import hx, load_fixture
from tests.test_gpu_hist import DROP, _key
from tests.test_gpu_hist_level import _level_launches, _reference

pytestmark = pytest.mark.gpu

CHUNK = 4  # paths.hpp kSibChunkMin: sib_chunk(M) for every M below 163,840


def _case(bits, n_rows, nfeat, nbins, nnodes, layout):
    """(ciphertext ints, bins, node slots, parent ints, parent counts) of a layout"""
    dk, n2 = _key(bits)
    top = 1 << (32 * dk.n2w)
    rng = np.random.default_rng(n_rows + 7 * nbins + 11 * nnodes)
    cs = [int.from_bytes(rng.bytes(4 * dk.n2w), "little") % n2 for _ in range(n_rows)]
    bins = rng.integers(0, nbins, (nfeat, n_rows)).astype(np.uint16)
    node = rng.integers(0, nnodes, n_rows).astype(np.uint16)
    sizes = {"right": [60, 40], "left": [40, 60], "tie": [50, 50], "ragged": [65, 0, 1, 64],
             "empty_pair": [30, 20, 0, 0], "wide": [26, 4, 4, 6]}.get(layout)
    if sizes:
        node = rng.permutation(np.repeat(np.arange(len(sizes)), sizes)).astype(np.uint16)
    if layout == "inactive":
        node[::3] = nnodes
        node[1] = DROP
    elif layout == "dropped":
        bins[0, :] = DROP
        bins[1, ::3] = DROP
        bins[1, 1] = nbins
    elif layout == "wide":  # n^2 (no unit: it must sit in a child that is not built), n^2 + 1 and the top value built
        cs[int(np.flatnonzero(node == 0)[0])] = n2
        cs[int(np.flatnonzero(node == 2)[0])] = n2 + 1
        cs[int(np.flatnonzero(node == 2)[1])] = top - 1
    par, par_cnt = _reference(cs, bins, nbins, node >> 1, nnodes // 2, n2)
    if layout == "empty_pair":  # a finished leaf's slots: what its parent holds does not matter
        for i in range(nfeat * nbins, 2 * nfeat * nbins):
            par[i], par_cnt[i] = int(rng.integers(2, 1 << 62)), 7
    elif layout == "wide":  # every parent row as far above n^2 as its words allow: 0 -> n^2, 1 -> n^2 + 1, ...
        par = [p + n2 if p < 2 else p + (top - 1 - p) // n2 * n2 for p in par]
    return cs, bins, node, par, par_cnt.astype(np.int32)


def _sub(dk, cs, bins, nbins, node, nnodes, par, par_cnt, tile_rows, host=False, overlap=None):
    """(return code, output ints, counts) of one xhe_hist_level_sub call"""
    import torch

    from xfl_amd import _native as nat
    L = nat.lib()
    cw, pw = nat.ints_to_words(cs, dk.n2w), nat.ints_to_words(par, dk.n2w)
    nfeat, stride = bins.shape
    total = nnodes * nfeat * nbins
    out, cnt = np.empty((total, dk.n2w), np.uint32), np.empty(total, np.int32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    if host:
        rc = L.xhe_hist_level_sub_host(dk.handle, vp(cw), len(cs), vp(bins), stride, nfeat, nbins, vp(node), nnodes,
                                       vp(pw), vp(par_cnt), tile_rows, vp(out), vp(cnt))
        return rc, nat.words_to_ints(out), cnt
    dev = lambda a: torch.from_numpy(a.view(np.int16 if a.itemsize == 2 else np.int32)).cuda()  # noqa: E731
    cd, bd, nd, pd, pc = dev(cw), dev(bins), dev(node), dev(pw), dev(par_cnt)
    od = torch.empty(out.shape, dtype=torch.int32, device="cuda")
    kd = torch.empty(cnt.shape, dtype=torch.int32, device="cuda")
    optr = {None: od, "parent": pd, "c": cd}[overlap].data_ptr()
    rc = L.xhe_hist_level_sub(dk.handle, cd.data_ptr(), len(cs), bd.data_ptr(), stride, nfeat, nbins, nd.data_ptr(),
                              nnodes, pd.data_ptr(), pc.data_ptr(), tile_rows, optr, kd.data_ptr(),
                              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, nat.words_to_ints(od.cpu().numpy().view(np.uint32)), kd.cpu().numpy()


# (n_rows, nfeat, nbins, nnodes, tile_rows, layout): the smallest shapes that reach each edge
EDGES = {
    "right_smaller": (100, 2, 3, 2, 64, "right"),
    "left_smaller": (100, 2, 3, 2, 64, "left"),
    "tie_builds_left": (100, 2, 3, 2, 64, "tie"),
    "ragged": (130, 2, 3, 4, 64, "ragged"),  # an empty built child: sibling = parent; a one-row child
    "empty_pair": (50, 2, 3, 4, 64, "empty_pair"),
    "inactive": (100, 2, 3, 4, 64, "inactive"),
    "dropped": (70, 2, 4, 2, 64, "dropped"),
    "wide": (40, 2, 3, 4, 64, "wide"),
    "one_row": (50, 1, 1, 2, 64, "plain"),
    "below_chunk": (50, 1, CHUNK - 1, 2, 64, "plain"),
    "one_chunk": (50, 1, CHUNK, 2, 64, "plain"),
    "chunk_plus_one": (50, 1, CHUNK + 1, 2, 64, "plain"),
    "bins_4096": (100, 3, 4096, 2, 64, "plain"),  # 3,072 chunk totals: a tree of 12 levels
    "nodes_4096": (100, 1, 2, 4096, 64, "plain"),
    "planner_tile": (3000, 4, 16, 8, 0, "plain"),
}
CASES = [(bits, *EDGES[e]) for bits in (2048, 3072) for e in EDGES]
CASES += [(bits, *EDGES["ragged"]) for bits in (4096, 8192)]


@pytest.mark.parametrize("bits,n_rows,nfeat,nbins,nnodes,tile_rows,layout", CASES)
def test_hist_level_sub_abi(bits, n_rows, nfeat, nbins, nnodes, tile_rows, layout):
    dk, n2 = _key(bits)
    cs, bins, node, par, par_cnt = _case(bits, n_rows, nfeat, nbins, nnodes, layout)
    rc, got, cnt = _sub(dk, cs, bins, nbins, node, nnodes, par, par_cnt, tile_rows)
    want, want_cnt = _reference(cs, bins, nbins, node, nnodes, n2)
    assert rc == 0
    assert np.array_equal(cnt, want_cnt)
    assert got == want


def test_hist_level_sub_host_equals_device():
    dk, n2 = _key(2048)
    cs, bins, node, par, par_cnt = _case(2048, 130, 2, 3, 4, "ragged")
    rc, got, cnt = _sub(dk, cs, bins, 3, node, 4, par, par_cnt, 64, host=True)
    rc_dev, dev, dev_cnt = _sub(dk, cs, bins, 3, node, 4, par, par_cnt, 64)
    assert rc == rc_dev == 0
    assert got == dev == _reference(cs, bins, 3, node, 4, n2)[0] and np.array_equal(cnt, dev_cnt)


def test_hist_level_sub_no_inverse():
    """a row of the built child equal to the key's p: XHE_ENOINV, as xhe_invert reports it"""
    dk, _ = _key(2048)
    cs, bins, node, par, par_cnt = _case(2048, 100, 2, 3, 2, "right")
    cs[int(np.flatnonzero(node == 1)[0])] = hx(load_fixture("paillier_2048_djn.json")["key"]["p"])
    assert _sub(dk, cs, bins, 3, node, 2, par, par_cnt, 64)[0] == -4  # XHE_ENOINV


@pytest.mark.parametrize("bad", [dict(nnodes=3), dict(overlap="parent"), dict(overlap="c")])
def test_hist_level_sub_argument_errors(bad):
    dk, _ = _key(2048)
    a = dict(nnodes=4, overlap=None)
    a.update(bad)
    cs, bins, node, par, par_cnt = _case(2048, 50, 2, 3, 4, "plain")
    assert _sub(dk, cs, bins, 3, node, a["nnodes"], par, par_cnt, 64, overlap=a["overlap"])[0] == -1  # XHE_EINVAL


def test_level_histograms_parent_dropin():
    """level 2 from level 1's histogram: bit for bit the direct call, in one k_hist_level_sub launch"""
    from xfl_amd.paillier_acceleration import level_histograms
    priv, pub = CC.keys()
    n, nfeat, nbins = 300, 3, 5
    arr = CC.encrypt(pub, CC.plain(n, 41))
    assert arr.is_resident
    rng = np.random.default_rng(6)
    bins = rng.integers(-1, nbins, (nfeat, n))
    nodes = rng.integers(-1, 4, n)
    level1 = level_histograms(arr, bins, np.where(nodes < 0, -1, nodes >> 1), 2, nbins)
    want, want_cnt = level_histograms(arr, bins, nodes, 4, nbins)

    def run(**kw):
        from xfl_amd import _native as nat
        L = nat.lib()
        n_sub = ctypes.c_int64()

        def call():
            import torch
            res = level_histograms(arr, bins, nodes, 4, nbins, **kw)
            torch.cuda.synchronize()
            L.xhe_profile_read(b"k_hist_level_sub", None, ctypes.byref(n_sub))
            return res
        (sums, counts), direct = _level_launches(call)
        assert np.array_equal(np.asarray(sums.words), np.asarray(want.words)) and np.array_equal(counts, want_cnt)
        assert sums.shape == (4, nfeat, nbins) and sums.is_resident and counts.dtype == np.int64
        return direct, n_sub.value

    assert run(parent=level1, subtract=True) == (0, 1)
    assert run(parent=level1, subtract=False) == (1, 0)
    other = level1[0]._view(0, level1[0].exponents + 1, level1[0].shape)  # the same rows at another exponent
    assert run(parent=(other, level1[1]), subtract=True) == (1, 0)
