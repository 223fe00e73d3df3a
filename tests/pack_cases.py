"""Shared by the ciphertext-packing tests (tests/test_pack_host.py,
tests/test_gpu_pack.py, tests/test_gpu_pack_dropin.py): the Python-integer
statement of xhe_pack, its inputs, and the child process that runs one batch
under pinned $XHE_* switches (they are read once per process).

    out[j] = prod_{t<k} c[j k + t]^(2^(s (k-1-t))) mod n^2, missing elements 1
"""
import json
import random
import sys

from tests.conftest import ROOT, hx, load_fixture

FIXTURE = {2048: "paillier_2048_djn.json", 3072: "paillier_3072_djn.json", 4096: "paillier_4096_djn.json",
           8192: "paillier_8192_djn.json"}


def modulus(bits):
    return hx(load_fixture(FIXTURE[bits])["key"]["n"])


def _powmod():
    """libgmp's mpz_powm where the host has it (the 8192-bit chains take
    seconds in Python integers), else the built-in pow"""
    try:
        from xfl_amd.paillier import _gmp
        return _gmp.powmod if _gmp.available() else pow
    except Exception:  # noqa: BLE001
        return pow


def pack_ref(cs, k, s, n2):
    """Horner over every group of k: ((c0^(2^s) c1)^(2^s) c2 ...) mod n^2; an
    element past the end counts as 1"""
    pow = _powmod()  # noqa: A001
    out = []
    for j in range(0, len(cs), k):
        acc = cs[j] % n2
        for t in range(1, k):
            acc = pow(acc, 1 << s, n2)
            if j + t < len(cs):
                acc = acc * cs[j + t] % n2
        out.append(acc)
    return out


def inputs(bits, count, k, tag=""):
    """count residues below n^2: the raw ciphertext 1, n^2 - 1, n + 1, one
    group whose elements are all equal (when there are two groups), random
    ones elsewhere"""
    n = modulus(bits)
    n2 = n * n
    rng = random.Random(f"pack-{bits}-{count}-{k}-{tag}")
    cs = [rng.randrange(1, n2) for _ in range(count)]
    for i, v in enumerate((1, n2 - 1, n + 1)):
        if i < count:
            cs[(i * 5) % count] = v
    if count >= 2 * k:
        cs[k:2 * k] = [cs[k]] * k
    return cs


_cache = {}


def case(bits, count, k, s, tag=""):
    """(inputs, expected outputs), computed once per process"""
    key = (bits, count, k, s, tag)
    if key not in _cache:
        n = modulus(bits)
        cs = inputs(bits, count, k, tag)
        _cache[key] = (cs, pack_ref(cs, k, s, n * n))
    return _cache[key]


def public_key(bits):
    """a handle made from n alone (no tables to build)"""
    from xfl_amd import _native as nat
    return nat.DeviceKey(bits, modulus(bits), None, None, None)


def pack_dev(dk, cs, k, s):
    """xhe_pack on device buffers -> (return code, output ints)"""
    import numpy as np

    from xfl_amd import _native as nat
    from xfl_amd.paillier import resident
    import torch
    dev = dk.device
    c = resident.upload(np.ascontiguousarray(nat.ints_to_words(cs, dk.n2w)), dev)
    with resident._On(dev):
        out = torch.zeros((-(-len(cs) // k), dk.n2w), dtype=torch.int32, device=f"cuda:{dev}")
    rc = nat.lib().xhe_pack(dk.handle, resident._dp(c), len(cs), k, s, resident._dp(out), resident._sp(dev))
    if rc != nat.XHE_OK:
        return rc, None
    return rc, nat.words_to_ints(resident.download(out))


# ---------------------------------------------------------------- pinned children
_CHILD = r"""
import sys
sys.path.insert(0, {root!r})
import torch
torch.cuda.init()
from tests import pack_cases
pack_cases.run_child({bits}, {count}, {k}, {s})
"""


def child_argv(bits, count, k, s):
    return [sys.executable, "-c", _CHILD.format(root=ROOT, bits=bits, count=count, k=k, s=s)]


def run_child(bits, count, k, s):
    """one JSON line: the outputs of xhe_pack as hex, and the launches of k_pack"""
    import ctypes

    from xfl_amd import _native as nat
    L = nat.lib()
    dk = public_key(bits)
    L.xhe_profile(1)
    rc, out = pack_dev(dk, inputs(bits, count, k), k, s)
    tot, cnt = ctypes.c_double(), ctypes.c_int64()
    nat.check(L.xhe_profile_read(b"k_pack", ctypes.byref(tot), ctypes.byref(cnt)))
    L.xhe_profile(0)
    print(json.dumps({"rc": rc, "out": [hex(v) for v in out or []], "launches": cnt.value}), flush=True)
