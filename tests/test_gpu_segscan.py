"""xhe_segscan on the GPU: every output row against Python integers, for every
key size, every level count the chunk length gives and both lane shapes.

tests/scan_cases.py holds the segment lists, the operands and what a child
runs. $XHE_N2_TPI is read once per process, so each setting (unset, 4, 16) is
one fresh child, started one after another; a child prints one JSON line per
(key, list, operands) and per entry-point check, and the parent asserts that
the lines are the table's, complete and clean.

A child that dies by a signal, aborts, faults or runs into its timeout stops
the module: the GPU may be in a bad state, so every later setting fails at
once, naming the first casualty, and starts no process.
"""
import subprocess

import pytest

from tests import scan_cases as SC

pytestmark = pytest.mark.gpu

TIMEOUT = 300
_casualty = None  # the first child that ended abnormally


@pytest.mark.parametrize("setting", SC.SETTINGS)
def test_segscan(setting):
    global _casualty
    if _casualty:
        pytest.fail(f"XHE_N2_TPI {setting} not started: {_casualty}", pytrace=False)
    try:
        r = subprocess.run(SC.child_argv(setting), env=SC.child_env(setting), capture_output=True, text=True,
                           timeout=TIMEOUT)
    except subprocess.TimeoutExpired:
        _casualty = f"the child of XHE_N2_TPI {setting} did not end within {TIMEOUT} s"
        pytest.fail(_casualty, pytrace=False)
    tail = r.stdout[-2000:] + r.stderr[-3000:]
    faulted = any(s in r.stderr for s in ("illegal memory access", "Memory access fault", "HSA_STATUS_ERROR"))
    if r.returncode < 0 or r.returncode in (134, 139) or faulted:
        _casualty = f"the child of XHE_N2_TPI {setting} ended with status {r.returncode}" + \
            (" after a GPU fault" if faulted else "")
        pytest.fail(_casualty + "\n" + tail, pytrace=False)
    assert r.returncode == 0, tail
    report = SC.parse_report(r.stdout)
    assert sorted((line["key"], line["list"], line["operands"]) for line in report) == \
        SC.expected_lines(SC.CHUNK_LENS[0]), tail
    lists = SC.segment_lists(SC.CHUNK_LENS[0])
    wrong = [line for line in report
             if line["bad"] != 0 or line["checked"] != line["count"]
             or (line["list"] in lists and line["count"] != sum(lists[line["list"]]))]
    assert not wrong, "\n".join(f"{w['key']} {w['list']} {w['operands']}: {w['checked']} of {w['count']} rows checked, "
                                f"{w['bad']} differ, first {w['first_bad']}" for w in wrong) + "\n" + r.stderr[-3000:]
