"""Every kernel path that only a $XHE_* switch reaches (INTEGRATION.md "Other
kernel switches"), bit for bit against Python integers.

tests/pinned_cases.py holds the table and what a child runs; the switches are
read once per process, so each case is one fresh child, started one after
another. tests/test_pinned_paths_host.py proves on the CPU that each case's
switches change the planner's decision to the path the case names; here the
child compares every produced row and reports one JSON line per (operation,
count), and the parent checks that the lines are the table's, complete and
clean. Launch labels are asserted only where the table lists them.

A child that dies by a signal, aborts, faults or runs into its timeout stops
the module: the GPU may be in a bad state, so every later case fails at once,
naming the first casualty, and starts no process.
"""
import subprocess

import pytest

from tests import pinned_cases as PC

pytestmark = pytest.mark.gpu

TIMEOUT = 300
_casualty = None  # the first child that ended abnormally


@pytest.mark.parametrize("case", PC.CASES, ids=[c["name"] for c in PC.CASES])
def test_pinned_path(case):
    global _casualty
    name = case["name"]
    if _casualty:
        pytest.fail(f"{name} not started: {_casualty}", pytrace=False)
    try:
        r = subprocess.run(PC.child_argv(name), env=PC.child_env(case), capture_output=True, text=True, timeout=TIMEOUT)
    except subprocess.TimeoutExpired:
        _casualty = f"the child of {name} did not end within {TIMEOUT} s"
        pytest.fail(_casualty, pytrace=False)
    tail = r.stdout[-2000:] + r.stderr[-3000:]
    faulted = any(s in r.stderr for s in ("illegal memory access", "Memory access fault", "HSA_STATUS_ERROR"))
    if r.returncode < 0 or r.returncode in (134, 139) or faulted:
        _casualty = f"the child of {name} ended with status {r.returncode}" + (" after a GPU fault" if faulted else "")
        pytest.fail(_casualty + "\n" + tail, pytrace=False)
    assert r.returncode == 0, tail
    report = PC.parse_report(r.stdout)
    assert all(line["case"] == name for line in report), tail
    assert sorted((line["op"], line["count"]) for line in report) == PC.expected_lines(case), tail
    wrong = [line for line in report if line["checked"] != line["count"] or line["bad"] != 0]
    assert not wrong, "\n".join(f"{w['op']} x {w['count']}: {w['checked']} rows checked, {w['bad']} differ, "
                                f"first {w['first_bad']}" for w in wrong)
