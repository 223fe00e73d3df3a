"""k_djn_pmd's rows in pairs on the GPU (pdigit_dev.hpp PMD::mul_pair followed
by PMD::mul; tests/native/pmd_pair_selftest.hip, built on the CPU by
tests/native/build_pmd_pair.py from __graft_entry__.build()): the device
routines on row digits and states written by the host, one wave per launch,
each result checked exactly against host big integers - forced operands (e in
{1, P - 1, R mod P, 2^1023} paired with each other, and a pair whose product is
R), forced states (a = 0, the tops of the ranges of a and c), forced quotient
digits (the low 1..36 digits of m all zero, and all ones) and 256 random pairs
and states per prime of the golden 2048-bit DJN key. One JSON line per check
and prime with the number of wrong lanes; all must be 0."""
import json
import os
import subprocess

import pytest

from tests.conftest import hx, load_fixture

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "native", "_build", "pmd_pair_selftest")
CHECKS = ("pair_forced", "state_forced", "quotient_forced", "random")


def test_pmd_pair_selftest():
    # a missing harness fails the GPU suite (a skip would let it pass without it)
    assert os.path.exists(EXE), "pmd_pair_selftest not built (python tests/native/build_pmd_pair.py)"
    g = load_fixture("paillier_2048_djn.json")["key"]
    primes = [hx(g["p"]), hx(g["q"])]
    r = subprocess.run([EXE] + ["%x" % p for p in primes], capture_output=True, text=True, timeout=120)
    checks = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{") and '"bad"' in l]
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert sorted((c["check"], c["prime"]) for c in checks) == sorted(
        (name, i) for name in CHECKS for i in range(len(primes)))
    assert all(c["bad"] == 0 for c in checks), checks
    assert all(c["of"] == 256 for c in checks if c["check"] == "random")
    assert all(c["of"] >= 15 for c in checks if c["check"] != "random")
