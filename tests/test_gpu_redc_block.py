"""The block-form Montgomery reductions at both ends of k_djn_pmd on the GPU
(tests/native/redc_block_selftest.hip, built on the CPU by
tests/native/build_redc_block.py from __graft_entry__.build()):
Mont<74, 28, 1>::redc_wide(b, AZero{}) mod P^2 and the prologue's REDC by P
(pmd_redc_words) on host-chosen inputs, each result checked exactly against
host big integers. The moduli are the primes of the golden 2048-bit DJN key and
of the structured key `bottom` (the smallest primes: the largest R/P). One JSON
line per check and prime with the number of wrong lanes; all must be 0."""
import json
import os
import subprocess

import pytest

from tests import structured_keys as SK
from tests.conftest import hx, load_fixture

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "native", "_build", "redc_block_selftest")


def test_redc_block_selftest():
    # a missing harness fails the GPU suite (a skip would let it pass without it)
    assert os.path.exists(EXE), "redc_block_selftest not built (python tests/native/build_redc_block.py)"
    g = load_fixture("paillier_2048_djn.json")["key"]
    b = SK.key(2048, "bottom")
    primes = [hx(g["p"]), hx(g["q"]), b.p, b.q]
    r = subprocess.run([EXE] + ["%x" % p for p in primes], capture_output=True, text=True, timeout=120)
    checks = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{") and '"bad"' in l]
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert sorted((c["check"], c["prime"]) for c in checks) == sorted(
        (name, i) for name in ("redc_wide", "redc_p") for i in range(len(primes)))
    assert all(c["bad"] == 0 and c["of"] == 64 for c in checks), checks
