"""k_djn_pmd with the table rows multiplied in pairs (pdigit_dev.hpp "Rows in
pairs"; one lane per element): xhe_encrypt word for word against the oracle's
DJN-CRT encryption (oracle.paillier_oracle.encrypt_m on the same m and a).

One child process with $XHE_PMD_SPLIT=1 (read once per process) builds one
seeded 2048-bit key (n of exactly 2048 bits: exponents up to 2^1024) at window
13 - 79 windows: the start row and 39 pairs, no leftover - and at window 12 - 86
windows: 42 pairs and one leftover row - and encrypts batches of 1, 63, 64, 65
and 129 elements: a partial wave, a whole wave, both waves of a block and a
second block. The 129 (m, a) pairs are fixed, so the oracle runs once; smaller
batches take slices of them.

Exponents: 0, 1, 2^1024 - 1, the top bit alone, and for both layouts exponents
whose only non-zero digit (1, and all ones) sits in the first or in the second
window of the first, a middle and the last pair - the other row of that pair,
and every other row, is then the row y = 1 of its window; the rest are seeded
random draws. Plaintexts: pairs [0, 64) are all short (+-s, s < 2^112, with 0, 1
and n - 1 among them), pairs [64, 129) all general, so the batches of 64 and 65
run wave-pure short and wave-pure general entries, the batch of 129 both, and
the batch of 63 (pairs [33, 96)) mixes them inside one wave.
"""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

RB = 1024
WINS = ("13", "12")
SIZES = (1, 63, 64, 65, 129)
OFFSETS = {1: 1, 63: 33, 64: 0, 65: 64, 129: 0}
SHORT = 1 << 112


def _windows(w):
    nwin = -(-RB // w)
    return [(i * w, min(w, RB - i * w)) for i in range(nwin)]


def _exponents():
    special = [0, 1, (1 << RB) - 1, 1 << (RB - 1)]
    for spec in WINS:
        wins = _windows(int(spec))
        npairs = (len(wins) - 1) // 2  # pair k: windows 1 + 2k, 2 + 2k
        for k in (0, npairs // 2, npairs - 1):
            for w in (1 + 2 * k, 2 + 2 * k):
                bit, width = wins[w]
                special += [1 << bit, ((1 << width) - 1) << bit]
    slots = list(range(0, 64, 4)) + list(range(64, 128, 4))  # among the short and among the general plaintexts
    assert len(special) <= len(slots) and all(x < 1 << RB for x in special)
    rng = random.Random(2413)
    a = [rng.randrange(1, 1 << RB) for _ in range(SIZES[-1])]
    for i, x in enumerate(special):
        a[slots[(i // 2) + (i % 2) * 16]] = x
    return a


def _plaintexts(n):
    rng = random.Random(1213)
    m = []
    for i in range(64):
        s = rng.randrange(1, 1 << rng.randrange(1, 113))
        assert s < SHORT
        m.append(s if i % 2 == 0 else n - s)
    m[0], m[1], m[2], m[3] = 0, n - 1, 1, SHORT - 1
    m += [rng.randrange(SHORT + 1, n - SHORT) for _ in range(SIZES[-1] - 64)]
    m[64], m[65] = SHORT, n - SHORT  # the first general values on both sides
    return m


def _key():
    """p, q and h = -x^2n mod n^2 (the reference's h_pow_n) from a fixed seed"""
    import math

    from xfl_amd.paillier.utils import getprimeover
    rng = random.Random(24)
    while True:
        p, q = getprimeover(1024, rng=rng), getprimeover(1024, rng=rng)
        if p != q and math.gcd(p - 1, q - 1) == 2 and (p * q).bit_length() == 2 * RB:
            break
    n = p * q
    x = rng.getrandbits(2 * RB) | (1 << (2 * RB - 1))
    return p, q, pow(-(x * x), n, n * n)


@pytest.fixture(scope="module")
def pairs(tmp_path_factory):
    """the (m, a) pairs and the oracle's ciphertexts, as words in one file"""
    from oracle import paillier_oracle as O
    from xfl_amd import _native as nat
    p, q, h = _key()
    n = p * q
    okey = O.derive_private(p, q, h)
    a, m = _exponents(), _plaintexts(n)
    want = [O.encrypt_m(okey, mi, ai) for mi, ai in zip(m, a)]
    path = str(tmp_path_factory.mktemp("pmd_pairs") / "pairs.npz")
    np.savez(path, p=nat.int_to_words(p, 32), q=nat.int_to_words(q, 32), h=nat.int_to_words(h, 128),
             m=nat.ints_to_words(m, 64), a=nat.ints_to_words(a, 32), want=nat.ints_to_words(want, 128))
    return path


_CHILD = r"""
import sys
sys.path.insert(0, {root!r})
import numpy as np
import torch
torch.cuda.init()
from xfl_amd import _native as nat

z = np.load({pairs!r})
p, q, h = (nat.words_to_ints(z[name][None, :])[0] for name in "pqh")
L = nat.lib()
stream = torch.cuda.current_stream().cuda_stream
for spec in {wins!r}:
    dk = nat.DeviceKey(2048, p * q, p, q, h, device=0, win_bits=nat.parse_win(spec))
    assert dk.rand_bits == {rb} and dk.rand_words == z["a"].shape[1]
    for count, off in {cases!r}:
        md = torch.from_numpy(z["m"][off:off + count].view(np.int32).copy()).cuda()
        ad = torch.from_numpy(z["a"][off:off + count].view(np.int32).copy()).cuda()
        ct = torch.zeros((count, dk.n2w), dtype=torch.int32, device="cuda")
        nat.check(L.xhe_encrypt(dk.handle, md.data_ptr(), ad.data_ptr(), count, ct.data_ptr(), stream), "encrypt")
        got = ct.cpu().numpy().view(np.uint32)
        bad = np.nonzero(np.any(got != z["want"][off:off + count], axis=1))[0]
        assert bad.size == 0, f"win {{spec}} n {{count}}: {{bad.size}} ciphertexts differ, first {{(bad[:8] + off).tolist()}}"
        print("ok", spec, count, flush=True)
    del dk
print("done", flush=True)
"""


def test_exponent_and_plaintext_cases():
    """the fixed pairs hold what the docstring says (CPU side of the fixture)"""
    a = _exponents()
    assert len(a) == SIZES[-1] and {0, 1, (1 << RB) - 1, 1 << (RB - 1)} <= set(a)
    for spec, npairs, left in (("13", 39, 0), ("12", 42, 1)):
        wins = _windows(int(spec))
        assert (len(wins) - 1) // 2 == npairs and (len(wins) - 1) % 2 == left
        for k in (0, npairs // 2, npairs - 1):
            for w in (1 + 2 * k, 2 + 2 * k):
                assert 1 << wins[w][0] in a


def test_encrypt_pairs_matches_oracle(pairs):
    env = dict(os.environ, XHE_PMD_SPLIT="1")
    code = _CHILD.format(root=ROOT, pairs=pairs, wins=WINS, rb=RB, cases=[(s, OFFSETS[s]) for s in SIZES])
    r = subprocess.run([sys.executable, "-u", "-c", code], capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0 and "done" in r.stdout, r.stdout[-3000:] + r.stderr[-4000:]
    assert r.stdout.count("ok ") == len(WINS) * len(SIZES)
