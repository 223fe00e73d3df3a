"""xhe_bucketexp on the GPU through the C ABI in-process: every output word of
out[j] = prod_t bases[t]^(+-k[j][t]) mod n^2 against Python's pow and %."""
import ctypes
import random

import numpy as np
import pytest

from tests.conftest import hx, load_fixture

pytestmark = pytest.mark.gpu

ENOINV, EINVAL = -4, -1
_keys = {}


def _key(bits):
    """(public non-DJN device key, n) of the golden key of that size"""
    from xfl_amd._native import DeviceKey
    if bits not in _keys:
        n = hx(load_fixture(f"paillier_{bits}_djn.json")["key"]["n"])
        _keys[bits] = (DeviceKey(bits, n, None, None, None), n)
    return _keys[bits]


def _case(bits, nterms, ncols, kbits, signs, extra):
    """(bases, k [ncols][nterms], neg uint8 [ncols, nterms] or None)"""
    dk, n = _key(bits)
    rnd = random.Random(nterms * 1009 + ncols * 31 + kbits)
    bases = [rnd.randrange(1, n * n) for _ in range(nterms)]
    ks = [[rnd.randrange(1 << kbits) for _ in range(nterms)] for _ in range(ncols)]
    ks[0][0] |= 1 << (kbits - 1)  # the top window is used
    neg = {"none": None, "neg": np.ones((ncols, nterms), np.uint8),
           "mixed": np.array([[rnd.randrange(2) for _ in range(nterms)] for _ in range(ncols)], np.uint8)}[signs]
    if extra == "wide":  # operands at and above n^2; n^2 itself (0 mod n^2) stays positive and counts in the
        # last of several columns only (k = 0 elsewhere), so every other output is a non-zero residue
        bases[1], bases[nterms // 2], bases[-1] = n * n, n * n + 1, (1 << (32 * dk.n2w)) - 1
        for col in ks[:-1] if ncols > 1 else ks:
            col[1] = 0
        if neg is not None:
            neg[:, 1] = 0
    elif extra == "zeros":  # a zero term under a set sign byte, and an all-zero column
        ks[0][1] = 0
        neg[0, 1] = 1
        ks[-1] = [0] * nterms
    return bases, ks, neg


def _run(dk, bases, ks, neg, kbits, win, host=False):
    """-> (rc, output ints)"""
    import torch

    from xfl_amd import _native as nat
    L = nat.lib()
    ncols, nterms, kw = len(ks), len(bases), (kbits + 31) // 32
    bw = nat.ints_to_words(bases, dk.n2w)
    kwords = nat.ints_to_words([k for col in ks for k in col], kw)
    vp = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    if host:
        out = np.empty((ncols, dk.n2w), np.uint32)
        rc = L.xhe_bucketexp_host(dk.handle, vp(bw), nterms, vp(kwords), vp(neg), kw, kbits, ncols, win, vp(out))
        return rc, nat.words_to_ints(out)
    bd, kd = torch.from_numpy(bw.view(np.int32)).cuda(), torch.from_numpy(kwords.view(np.int32)).cuda()
    nd = None if neg is None else torch.from_numpy(neg).cuda()
    od = torch.empty((ncols, dk.n2w), dtype=torch.int32, device="cuda")
    rc = L.xhe_bucketexp(dk.handle, bd.data_ptr(), nterms, kd.data_ptr(), None if nd is None else nd.data_ptr(), kw,
                         kbits, ncols, win, od.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, nat.words_to_ints(od.cpu().numpy().view(np.uint32))


def _reference(bases, ks, neg, n2):
    out = []
    for j, col in enumerate(ks):
        pos = den = 1
        for t, (b, k) in enumerate(zip(bases, col)):
            if neg is not None and neg[j, t]:
                den = den * pow(b, k, n2) % n2
            else:
                pos = pos * pow(b, k, n2) % n2
        out.append(pos * pow(den, -1, n2) % n2)
    return out


# (bits, nterms, ncols, kbits, win_bits, signs, extra, host)
CASES = [
    (2048, 1, 1, 1, 1, "none", None, False),        # one bucket, one term
    (2048, 300, 1, 24, 1, "mixed", None, False),    # 24 one-bit windows, 5 tiles
    (2048, 63, 3, 24, 3, "mixed", None, False),     # fewer buckets than lane groups
    (2048, 300, 3, 24, 8, "mixed", None, False),    # L = 4
    (2048, 63, 1, 24, 8, "neg", None, False),
    (2048, 63, 3, 24, 11, "none", None, False),     # L = 32, no Neg half
    (2048, 300, 1, 70, 11, "mixed", None, False),   # 4094 bins, windows straddling words, short top window
    (2048, 300, 3, 70, 0, "mixed", None, False),    # the planner's window
    (2048, 63, 3, 24, 8, "mixed", "wide", False),
    (2048, 63, 3, 24, 3, "mixed", "zeros", False),
    (2048, 63, 3, 24, 3, "mixed", None, True),
    (2048, 63, 1, 70, 0, "none", "wide", True),
    (3072, 1, 1, 1, 1, "neg", None, False),
    (3072, 63, 3, 24, 3, "mixed", "zeros", False),
    (3072, 300, 1, 70, 8, "mixed", None, False),
    (3072, 63, 1, 24, 11, "neg", None, False),
    (3072, 63, 3, 24, 8, "mixed", "wide", False),
    (3072, 300, 3, 24, 0, "none", None, True),
    (8192, 1, 1, 1, 1, "none", None, False),
    (8192, 63, 3, 24, 3, "mixed", "zeros", False),  # fewer buckets than the 16 lane groups
    (8192, 63, 1, 70, 8, "mixed", "wide", False),   # L = 16
    (8192, 63, 1, 24, 11, "neg", None, False),      # L = 128
    (8192, 63, 3, 24, 0, "none", None, True),
]


@pytest.mark.parametrize("bits,nterms,ncols,kbits,win,signs,extra,host", CASES)
def test_bucketexp_abi(bits, nterms, ncols, kbits, win, signs, extra, host):
    dk, n = _key(bits)
    bases, ks, neg = _case(bits, nterms, ncols, kbits, signs, extra)
    rc, got = _run(dk, bases, ks, neg, kbits, win, host)
    want = _reference(bases, ks, neg, n * n)
    assert rc == 0 and got == want
    assert all(want[:-1] if extra == "wide" and ncols > 1 else want)  # (no output is trivially 0)


@pytest.mark.parametrize("bits,host", [(2048, False), (2048, True), (8192, False)])
def test_bucketexp_non_unit_base(bits, host):
    """bases[t] = n: its power under a positive scalar, XHE_ENOINV under a negative one"""
    dk, n = _key(bits)
    bases, ks, neg = _case(bits, 63, 3, 24, "mixed", None)
    bases[5] = n
    neg[:, 5] = 0
    rc, got = _run(dk, bases, ks, neg, 24, 3, host)
    assert rc == 0 and got == _reference(bases, ks, neg, n * n)
    neg[1, 5] = 1
    assert _run(dk, bases, ks, neg, 24, 3, host)[0] == ENOINV


@pytest.mark.parametrize("bad", [dict(win=12), dict(win=-1), dict(nterms=0), dict(ncols=0), dict(kw=0),
                                 dict(kbits=33), dict(overlap=True)])
def test_bucketexp_argument_errors(bad):
    import torch

    from xfl_amd import _native as nat
    dk, _ = _key(2048)
    a = dict(nterms=4, ncols=2, kw=1, kbits=24, win=3, overlap=False)
    a.update(bad)
    b = torch.zeros((4, dk.n2w), dtype=torch.int32, device="cuda")
    k = torch.zeros((2, 4), dtype=torch.int32, device="cuda")
    out = torch.zeros((2, dk.n2w), dtype=torch.int32, device="cuda")
    rc = nat.lib().xhe_bucketexp(dk.handle, b.data_ptr(), a["nterms"], k.data_ptr(), None, a["kw"], a["kbits"],
                                 a["ncols"], a["win"], b.data_ptr() if a["overlap"] else out.data_ptr(),
                                 torch.cuda.current_stream().cuda_stream)
    assert rc == EINVAL
