"""k_djn_pmd's exit through the digits on the GPU (pdigit_dev.hpp pmd_exit;
tests/native/pmd_ends_selftest.hip, built on the CPU by
tests/native/build_pmd_ends.py from __graft_entry__.build()): the device
routine on states (a, c, Lhat) written by the host, one wave per launch, each
result checked exactly against host big integers - the forced states of
tests/test_pdigit_ends_model.py (a = 0, a = P, which forces u = P and which no
encryption can be steered to, the tops of the ranges, z on P - 1 before the u =
P correction) and 256 random states per prime of the golden 2048-bit DJN key.
One JSON line per check and prime with the number of wrong lanes; all must be
0."""
import json
import os
import subprocess

import pytest

from tests.conftest import hx, load_fixture

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "native", "_build", "pmd_ends_selftest")


def test_pmd_ends_selftest():
    # a missing harness fails the GPU suite (a skip would let it pass without it)
    assert os.path.exists(EXE), "pmd_ends_selftest not built (python tests/native/build_pmd_ends.py)"
    g = load_fixture("paillier_2048_djn.json")["key"]
    primes = [hx(g["p"]), hx(g["q"])]
    r = subprocess.run([EXE] + ["%x" % p for p in primes], capture_output=True, text=True, timeout=120)
    checks = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{") and '"bad"' in l]
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert sorted((c["check"], c["prime"]) for c in checks) == sorted(
        (name, i) for name in ("forced", "random") for i in range(len(primes)))
    assert all(c["bad"] == 0 for c in checks), checks
    assert all(c["of"] == 256 for c in checks if c["check"] == "random")
    assert all(c["of"] >= 9 for c in checks if c["check"] == "forced")
