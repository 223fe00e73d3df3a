"""xhe_hist_exp on the GPU: every output word, exponent and count of the fused
histogram over rows of mixed exponents against Python integers - cell (f, b) =
prod pow(c[r], 1 << (e[r] - emin), n^2) over its rows, emin their smallest
exponent - through the C ABI in-process, and the drop-in's histograms() on a
precision=None column against the per-feature groupby sums it replaces.

200 rows x 3 features x 5 bins in tiles of 64: four tiles, the last one of 8
rows. Feature 1 holds ids >= nbins (dropped), feature 2 never uses bin 4
(empty cells); five operands are at or above n^2."""
import ctypes
import random

import numpy as np
import pytest

from tests import cumsum_cases as CC
from tests import wide_cases as WC

pytestmark = pytest.mark.gpu

N_ROWS, NFEAT, NBINS, TILE = 200, 3, 5, 64
KEYS = ("golden-2048-nodjn", "golden-4096")
_state = {}


def _setup(name):
    """(public device key, n^2, ciphertext ints, bins [NFEAT, N_ROWS] uint16) of a key, made once"""
    from xfl_amd._native import DeviceKey
    if name not in _state:
        K, n, _, _, _ = WC.key(name)
        dk = DeviceKey(K, n, None, None, None)
        rnd, rng = random.Random(K), np.random.default_rng(K)
        cs = [rnd.randrange(n * n) for _ in range(N_ROWS)]
        cs[0:N_ROWS:45] = WC.wide(n, dk.n2w, 5, rnd)  # rows 0, 45, .., 180
        bins = rng.integers(0, NBINS, (NFEAT, N_ROWS)).astype(np.uint16)
        bins[1, ::7], bins[1, 3] = 0xFFFF, NBINS
        bins[2] %= NBINS - 1
        _state[name] = (dk, n * n, cs, bins)
    return _state[name]


def _exponents(pattern, n_bits):
    """(int32 exponent per row, the call's dmax) of a pattern"""
    rng, r = np.random.default_rng(len(pattern)), np.arange(N_ROWS)
    e, dmax = {
        "equal": (np.full(N_ROWS, 5), 0),
        "window9": (rng.integers(-4, 5, N_ROWS), 8),
        "gap_dmax": (np.where(r == 77, n_bits - 5, -3), n_bits - 2),  # one row emin + dmax above its cells' others
        "per_tile": (40 - 3 * (r // TILE), 9),  # every tile partial of a cell at another exponent
        "increasing": (r - 100, N_ROWS - 1),
        "decreasing": (100 - r, N_ROWS - 1),
        "signs": (rng.integers(-20, 21, N_ROWS), 40),
    }[pattern]
    return e.astype(np.int32), dmax


def _reference(cs, e, bins, rows, n2):
    sel = np.arange(N_ROWS) if rows is None else rows
    out, eout, cnt = [], [], []
    for fb in bins:
        for b in range(NBINS):
            S = [int(r) for r in sel if fb[r] == b]
            emin = min((int(e[r]) for r in S), default=0)
            acc = 1
            for r in S:
                acc = acc * pow(cs[r], 1 << (int(e[r]) - emin), n2) % n2
            out.append(acc)
            eout.append(emin)
            cnt.append(len(S))
    return out, eout, cnt


def _run(dk, cs, e, bins, rows, dmax, host=False, tile=TILE):
    import torch

    from xfl_amd import _native as nat
    L = nat.lib()
    cw = nat.ints_to_words(cs, dk.n2w)
    n_rows, count = len(cs), len(cs) if rows is None else len(rows)
    out = np.empty((NFEAT * NBINS, dk.n2w), np.uint32)
    eo, cnt = np.empty(NFEAT * NBINS, np.int32), np.empty(NFEAT * NBINS, np.int32)
    vp = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    if host:
        nat.check(L.xhe_hist_exp_host(dk.handle, vp(cw), vp(e), n_rows, vp(bins), n_rows, NFEAT, NBINS, vp(rows), count,
                                      dmax, tile, vp(out), vp(eo), vp(cnt)), "hist_exp_host")
        return nat.words_to_ints(out), eo.tolist(), cnt.tolist()
    dev = lambda a: None if a is None else torch.from_numpy(a.view(np.int16 if a.itemsize == 2 else np.int32)).cuda()  # noqa: E731
    dp = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    cd, ed, bd, rd = dev(cw), dev(e), dev(bins), dev(rows)
    od, xd, nd = (torch.empty(a.shape, dtype=torch.int32, device="cuda") for a in (out, eo, cnt))
    nat.check(L.xhe_hist_exp(dk.handle, dp(cd), dp(ed), n_rows, dp(bd), n_rows, NFEAT, NBINS, dp(rd), count, dmax, tile,
                             dp(od), dp(xd), dp(nd), torch.cuda.current_stream().cuda_stream), "hist_exp")
    torch.cuda.synchronize()
    return nat.words_to_ints(od.cpu().numpy().view(np.uint32)), xd.cpu().tolist(), nd.cpu().tolist()


@pytest.mark.parametrize("pattern", ["equal", "window9", "gap_dmax", "per_tile", "increasing", "decreasing", "signs"])
@pytest.mark.parametrize("name", KEYS)
def test_hist_exp_exact(name, pattern):
    dk, n2, cs, bins = _setup(name)
    e, dmax = _exponents(pattern, WC.key(name)[1].bit_length())
    got = _run(dk, cs, e, bins, None, dmax)
    assert got == _reference(cs, e, bins, None, n2)
    assert got[2][2 * NBINS + 4] == 0 and got[0][2 * NBINS + 4] == 1  # an empty cell: 1, 0, 0
    if pattern == "equal":  # the words xhe_hist gives for the same rows, with or without the exponent array
        from tests.test_gpu_hist import _hist
        words = _hist(dk, cs, bins, NBINS, None, TILE)[0]
        assert got[0] == words == _run(dk, cs, None, bins, None, 0)[0]


@pytest.mark.parametrize("pattern", ["window9", "per_tile"])
@pytest.mark.parametrize("name", KEYS)
def test_hist_exp_row_list(name, pattern):
    """70 of the 200 rows, some of them twice"""
    dk, n2, cs, bins = _setup(name)
    e, dmax = _exponents(pattern, 0)
    rows = np.random.default_rng(3).integers(0, N_ROWS, 70).astype(np.int32)
    rows[5], rows[69] = rows[4], 199
    assert _run(dk, cs, e, bins, rows, dmax) == _reference(cs, e, bins, rows, n2)


def test_hist_exp_host_equals_device_and_planner_tile():
    dk, n2, cs, bins = _setup(KEYS[0])
    e, dmax = _exponents("signs", 0)
    want = _reference(cs, e, bins, None, n2)
    assert _run(dk, cs, e, bins, None, dmax, host=True) == want == _run(dk, cs, e, bins, None, dmax, tile=0)


def test_hist_exp_empty_call():
    """count == 0 writes ones, zero exponents and zero counts"""
    dk, _, _, _ = _setup(KEYS[0])
    got = _run(dk, [], np.zeros(0, np.int32), np.zeros((NFEAT, 0), np.uint16), None, 3, host=True)
    assert got == ([1] * 15, [0] * 15, [0] * 15)


@pytest.mark.parametrize("bad", [dict(dmax=-1), dict(dmax="bitlen - 1"), dict(eout=False), dict(overlap=True),
                                 dict(count=9)])
def test_hist_exp_argument_errors(bad):
    import torch

    from xfl_amd import _native as nat
    dk, _, _, _ = _setup(KEYS[0])
    a = dict(dmax=4, eout=True, overlap=False, count=10)
    a.update(bad)
    if a["dmax"] == "bitlen - 1":
        a["dmax"] = WC.key(KEYS[0])[1].bit_length() - 1
    c = torch.zeros((10, dk.n2w), dtype=torch.int32, device="cuda")
    e = torch.zeros(10, dtype=torch.int32, device="cuda")
    b = torch.zeros((2, 10), dtype=torch.int16, device="cuda")
    out = torch.zeros((8, dk.n2w), dtype=torch.int32, device="cuda")
    eo = torch.zeros(8, dtype=torch.int32, device="cuda")
    rc = nat.lib().xhe_hist_exp(dk.handle, c.data_ptr(), e.data_ptr(), 10, b.data_ptr(), 10, 2, 4, None, a["count"],
                                a["dmax"], 64, c.data_ptr() if a["overlap"] else out.data_ptr(),
                                eo.data_ptr() if a["eout"] else None, None, torch.cuda.current_stream().cuda_stream)
    assert rc == -1  # XHE_EINVAL
    assert nat.lib().xhe_hist_exp(dk.handle, c.data_ptr(), e.data_ptr(), 10, b.data_ptr(), 10, 2, 4, None, 10,
                                  WC.key(KEYS[0])[1].bit_length() - 2, 64, out.data_ptr(), eo.data_ptr(), None,
                                  torch.cuda.current_stream().cuda_stream) == 0  # the largest dmax is served


def test_histograms_dropin_mixed_exponents():
    """a precision=None column: one xhe_hist_exp call, the groupby sums bit for bit, the plaintext bin sums"""
    from xfl_amd import _native as nat
    from xfl_amd.paillier import Paillier
    from xfl_amd.paillier_acceleration import histograms
    priv, pub = CC.keys()
    rng = np.random.default_rng(11)
    vals = rng.standard_normal(150) * 2.0 ** rng.integers(-6, 7, 150)
    arr = CC.encrypt(pub, vals, precision=None)
    assert len(set(arr.exponents.tolist())) > 4
    bins = rng.integers(0, 4, (2, 150))
    L = nat.lib()
    L.xhe_profile(1)
    try:
        sums, counts = histograms(arr, bins, nbins=4)
        launches = {}
        for k in (b"k_hist_exp", b"k_hist"):
            ms, n = ctypes.c_double(), ctypes.c_int64()
            L.xhe_profile_read(k, ctypes.byref(ms), ctypes.byref(n))
            launches[k] = n.value
    finally:
        L.xhe_profile(0)
    assert launches == {b"k_hist_exp": 1, b"k_hist": 0}
    for f in range(2):  # the path the same column took before: the groupby sum feature by feature
        want = arr._groupby_op(how="sum", has_dropped_na=True, min_count=0, ngroups=4, ids=bins[f])
        assert CC.ints(sums[f]) == CC.ints(want)
        assert counts[f].tolist() == np.bincount(bins[f], minlength=4).tolist()
        plain = np.array([vals[bins[f] == b].sum() for b in range(4)])
        assert np.all(np.abs(Paillier.decrypt(priv, sums[f]) - plain) < 1e-4)
