"""xhe_pack / xhe_pack_host against Python integers, every output compared
(tests/pack_cases.py holds the reference and the inputs: the raw ciphertext 1,
n^2 - 1 and a group of equal elements among random residues), on a handle made
from the public key alone.

Shapes: the default process takes one 16-lane row per output up to kPackRowMax
outputs (17 = one past a 256-thread block's 16) and the 4-lane digit kernels
beyond (4,097 groups; k = 3 and 8-bit slots keep the Python side short). The
pinned shapes run in child processes, one per switch setting - the switches
are read once per process - at 65 groups, one past a 4-lane block's 64. A
child that faults, aborts or runs into its timeout stops the module: no
further child is started.
"""
import ctypes
import json
import subprocess

import numpy as np
import pytest

from tests import pack_cases as PK

pytestmark = pytest.mark.gpu

K7, S = 7, 256
TIMEOUT = 300
_casualty = None


@pytest.fixture(scope="module")
def dk2048():
    return PK.public_key(2048)


def _check(dk, bits, count, k, s):
    cs, want = PK.case(bits, count, k, s)
    rc, got = PK.pack_dev(dk, cs, k, s)
    assert rc == 0
    assert len(got) == len(want) == -(-count // k)
    bad = [j for j in range(len(want)) if got[j] != want[j]]
    assert not bad, f"{len(bad)} of {len(want)} outputs differ, first {bad[:6]}"


# 1, a full group, one element into the second group, a short second group,
# and 17 groups (the last one short): one past a 16-lane block
@pytest.mark.parametrize("count", [1, 7, 8, 13, 17 * K7 - 3])
def test_pack_2048_default(dk2048, count):
    assert not dk2048.private
    _check(dk2048, 2048, count, K7, S)


def test_pack_above_row_max(dk2048):
    """4,097 groups: past kPackRowMax, the batch shape"""
    _check(dk2048, 2048, 4097 * 3 - 1, 3, 8)


@pytest.mark.parametrize("bits,k,count", [(3072, 11, 11 + 4), (4096, 15, 15 + 1), (8192, 31, 31 + 30)])
def test_pack_larger_keys(bits, k, count):
    """one full and one short group at the largest k of each key size"""
    from xfl_amd import _native as nat
    try:
        dk = PK.public_key(bits)
    except nat.XheError as e:
        if "(-5)" in str(e):  # XHE_ENOTSUP: a build without this key size
            pytest.skip(f"this build has no {bits}-bit shapes")
        raise
    _check(dk, bits, count, k, S)


@pytest.mark.parametrize("env", [{"XHE_N2_TPI": "4"}, {"XHE_N2_TPI": "16"}, {"XHE_NDIG": "0"},
                                 {"XHE_N2_TPI": "4", "XHE_NDIG": "0"}],
                         ids=["n2-tpi4", "n2-tpi16", "ndig0", "n2-tpi4-ndig0"])
def test_pack_pinned(env):
    """65 groups (the last one short) under each switch setting"""
    global _casualty
    from tests import pinned_cases as PC
    count = 65 * K7 - 2
    if _casualty:
        pytest.fail(f"not started: {_casualty}", pytrace=False)
    try:
        r = subprocess.run(PK.child_argv(2048, count, K7, S), env=PC.child_env({"env": env}), capture_output=True,
                           text=True, timeout=TIMEOUT)
    except subprocess.TimeoutExpired:
        _casualty = f"the child of {env} did not end within {TIMEOUT} s"
        pytest.fail(_casualty, pytrace=False)
    tail = r.stdout[-500:] + r.stderr[-3000:]
    faulted = any(s in r.stderr for s in ("illegal memory access", "Memory access fault", "HSA_STATUS_ERROR"))
    if r.returncode < 0 or r.returncode in (134, 139) or faulted:
        _casualty = f"the child of {env} ended with status {r.returncode}" + (" after a GPU fault" if faulted else "")
        pytest.fail(_casualty + "\n" + tail, pytrace=False)
    assert r.returncode == 0, tail
    lines = [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
    assert len(lines) == 1, tail
    assert lines[0]["rc"] == 0 and lines[0]["launches"] == 1
    _, want = PK.case(2048, count, K7, S)
    got = [int(v, 16) for v in lines[0]["out"]]
    assert len(got) == len(want) == 65
    bad = [j for j in range(65) if got[j] != want[j]]
    assert not bad, f"{len(bad)} of 65 outputs differ, first {bad[:6]}"


def test_pack_einval(dk2048):
    import torch

    from xfl_amd import _native as nat
    from xfl_amd.paillier import resident
    L, dk = nat.lib(), dk2048
    n = PK.modulus(2048)
    dev = dk.device
    with resident._On(dev):
        buf = torch.zeros((16, dk.n2w), dtype=torch.int32, device=f"cuda:{dev}")
    buf[:, 0] = 1
    c, out = buf[:8], buf[8:]
    s = resident._sp(dev)
    dp = resident._dp

    def rc(cp, count, k, shift, op):
        return L.xhe_pack(dk.handle, cp, count, k, shift, op, s)
    assert rc(dp(c), 8, 7, 256, dp(out)) == nat.XHE_OK
    # k * shift_bits = bitlen(n) - 1 is one bit too many; bitlen(n) - 2 is the limit
    nb = n.bit_length()
    assert rc(dp(c), 8, 1, nb - 1, dp(out)) == nat.XHE_EINVAL
    assert rc(dp(c), 8, 1, nb - 2, dp(out)) == nat.XHE_OK
    assert rc(dp(c), 8, 7, (nb - 2) // 7, dp(out)) == nat.XHE_OK
    assert rc(dp(c), 8, 7, (nb - 2) // 7 + 1, dp(out)) == nat.XHE_EINVAL
    k1 = next(k for k in range(2, 60) if (nb - 1) % k == 0)  # a product that is bitlen(n) - 1 exactly
    assert rc(dp(c), 8, k1, (nb - 1) // k1, dp(out)) == nat.XHE_EINVAL
    assert rc(dp(c), 8, 8, 256, dp(out)) == nat.XHE_EINVAL
    for k, shift in ((0, 256), (-1, 256), (7, 0), (7, -256)):
        assert rc(dp(c), 8, k, shift, dp(out)) == nat.XHE_EINVAL, (k, shift)
    assert rc(dp(c), -1, 7, 256, dp(out)) == nat.XHE_EINVAL
    assert rc(None, 8, 7, 256, dp(out)) == nat.XHE_EINVAL
    assert rc(dp(c), 0, 7, 256, dp(out)) == nat.XHE_OK
    # overlap: out inside c, out's end reaching into c, c's end reaching into out
    assert rc(dp(c), 8, 7, 256, dp(c)) == nat.XHE_EINVAL
    assert rc(dp(buf[1:9]), 8, 7, 256, dp(buf[:2])) == nat.XHE_EINVAL
    assert rc(dp(buf[:8]), 8, 7, 256, dp(buf[7:9])) == nat.XHE_EINVAL
    assert rc(dp(buf[2:10]), 8, 7, 256, dp(buf[:2])) == nat.XHE_OK  # adjacent is fine
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="xhe_pack"):
        nat.check(rc(dp(c), 8, 0, 256, dp(out)), "pack")


@pytest.mark.parametrize("count", [13, 17 * K7 - 3])
def test_pack_host_equals_device(dk2048, count):
    from xfl_amd import _native as nat
    dk = dk2048
    cs, want = PK.case(2048, count, K7, S)
    cw = np.ascontiguousarray(nat.ints_to_words(cs, dk.n2w))
    out = np.zeros((-(-count // K7), dk.n2w), dtype=np.uint32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    nat.check(nat.lib().xhe_pack_host(dk.handle, vp(cw), count, K7, S, vp(out)), "pack host")
    rc, dev = PK.pack_dev(dk, cs, K7, S)
    assert rc == 0 and nat.words_to_ints(out) == dev == want
    assert nat.lib().xhe_pack_host(dk.handle, vp(cw), count, 8, 256, vp(out)) == nat.XHE_EINVAL
    assert nat.lib().xhe_pack_host(dk.handle, vp(cw), count, 0, 256, vp(out)) == nat.XHE_EINVAL
