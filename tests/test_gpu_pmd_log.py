"""k_djn_pmd with the rows' second digit carried as a sum (pdigit_dev.hpp
"Additive second digit"): xhe_encrypt word for word against the oracle's
DJN-CRT encryption (oracle.paillier_oracle.encrypt_m on the same m and a).

One seeded 2048-bit key (n of exactly 2048 bits, so the exponents run to 2^1024
as the reference's djn_exp_bound), three table layouts - window 12 (86
windows: the longest log sum), window 16 and the split layout 13s (10 windows
of 14 bits, then 68 of 13) - each with the lanes per element pinned to 1, 4
and 16 ($XHE_PMD_SPLIT is read once per process: one fresh child process per
value, which builds the three keys), and batches of 1, 63, 64, 65 and 129
elements: a partial wave, a whole wave, both waves of a block and a second
block. The 129 (m, a) pairs are fixed, so the oracle runs once for all cases;
smaller batches take slices of them.

Exponents: 0, 1, 2^1024 - 1, the top bit alone (one set bit in the top window
of every layout), and for every layout exponents whose digits are all zero but
one, that one at the digits the row conversion splits on (1, 2^h - 1, 2^h, 2^w
- 1; k_tab_to_pmd forms a row's log digit from a high and a low entry of the
inverse base's chains) in the first, a middle, the first narrow and the last
window; then seeded random draws. A zero digit reads the row y = 1 of its
window, whose log digit is not zero (R = e + k P gives l = k / R). The rows
y = P^2 - 1, e = 1 and e = P - 1 of tests/test_pdigit_log_model.py cannot be
addressed by an exponent without a discrete logarithm; the model test covers
them. Plaintexts: 0, 1, n - 1 and random.
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
WINS = ("12", "16", "13s")
SIZES = (1, 63, 64, 65, 129)
# where each batch starts in the 129 pairs (every pair is used by the last)
OFFSETS = {1: 1, 63: 66, 64: 0, 65: 64, 129: 0}


def _layout(spec):
    """[(first bit, width)] of the windows of a layout (xhe win_layout / win_digit)"""
    w = int(spec.rstrip("s"))
    nwin, nhi = -(-RB // w), 0
    if spec.endswith("s") and RB % w and RB % w <= RB // w:
        nwin, nhi = RB // w, RB % w
    out, bit = [], 0
    for i in range(nwin):
        width = w + (1 if i < nhi else 0)
        out.append((bit, min(width, RB - bit)))
        bit += width
    assert bit >= RB
    return out, nhi


def _exponents():
    a = [0, 1, (1 << RB) - 1, 1 << (RB - 1)]
    for spec in WINS:
        wins, nhi = _layout(spec)
        for w in sorted({0, len(wins) // 2, nhi, len(wins) - 1}):
            bit, width = wins[w]
            half = width // 2
            for d in sorted({1, (1 << half) - 1, 1 << half, (1 << width) - 1}):
                a.append(d << bit)
    assert len(a) <= SIZES[-1] - 16 and all(x < 1 << RB for x in a)
    rng = random.Random(2048)
    return a + [rng.randrange(1, 1 << RB) for _ in range(SIZES[-1] - len(a))]


def _key():
    """p, q and h = -x^2n mod n^2 (the reference's h_pow_n) from a fixed seed"""
    import math

    from xfl_amd.paillier.utils import getprimeover
    rng = random.Random(22)
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
    a = _exponents()
    rng = random.Random(7)
    m = [0, 1, n - 1] + [rng.randrange(n) for _ in range(len(a) - 3)]
    rng.shuffle(m)  # the edge plaintexts meet different exponents
    m[0], m[1] = 0, n - 1
    want = [O.encrypt_m(okey, mi, ai) for mi, ai in zip(m, a)]
    path = str(tmp_path_factory.mktemp("pmd_log") / "pairs.npz")
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


@pytest.mark.parametrize("lanes", [1, 4, 16])
def test_encrypt_matches_oracle(pairs, lanes):
    env = dict(os.environ, XHE_PMD_SPLIT=str(lanes))
    code = _CHILD.format(root=ROOT, pairs=pairs, wins=WINS, rb=RB, cases=[(s, OFFSETS[s]) for s in SIZES])
    r = subprocess.run([sys.executable, "-u", "-c", code], capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0 and "done" in r.stdout, r.stdout[-3000:] + r.stderr[-4000:]
    assert r.stdout.count("ok ") == len(WINS) * len(SIZES)
