"""CPU: no case of tests/pinned_cases.py is vacuous.

The launch labels cannot tell most switch-only kernels from the default ones
(k_powmod_n2, k_dec_pow, k_nodjn_crt and k_djn_pub each label two kernels), so
what proves that a GPU case of tests/test_gpu_pinned_paths.py runs the path it
names is the planner itself: every `paths` line of a case goes through
tests/native/paths_check.cpp (the program and helpers of tests/test_paths.py,
which pins every rule) twice - with the case's switches, where the answer must
be the literal decision the case names, and without any, where it must be
another one. The switch names are held against parse_pins and INTEGRATION.md,
so a misspelt name (which the library would silently ignore) fails here.
"""
import math
import os
import re

import pytest

from tests import pinned_cases as PC
from tests.test_paths import ROOT, ask_paths_check, build_paths_check

# the one case whose pin names the default's own path (tests/pinned_cases.py docstring)
CONFIRMS_DEFAULT = {"dec-tpi16-8192"}


def _with_env(line, case):
    return " ".join([line] + [f"{k}={v}" for k, v in sorted(case["env"].items())])


def _lines(case):
    """(line with the switches, the default-side line, decision, default line given?)"""
    out = []
    for row in case["paths"]:
        line, want = row[0], row[1]
        out.append((_with_env(line, case), row[2] if len(row) > 2 else line, want, len(row) > 2))
    return out


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    exe = build_paths_check(tmp_path_factory.mktemp("pinned_paths"))
    lines = []
    for case in PC.CASES:
        for pinned, default, _, _ in _lines(case):
            lines += [pinned, default]
    return ask_paths_check(exe, sorted(set(lines)))


def _is(answer, want, line):
    """`pins` lines print every field: the decision is one of them"""
    return want in answer.split() if line.split()[0] == "pins" else answer == want


@pytest.mark.parametrize("case", PC.CASES, ids=[c["name"] for c in PC.CASES])
def test_case_reaches_its_path_only_by_its_switches(answers, case):
    assert case["paths"], "a case names the planner lines that describe it"
    assert all(k.startswith("XHE_") for k in case["env"]) and case["env"]
    n2 = {row[1] for row in case["paths"] if row[0].startswith("n2 ")}
    for pinned, default, want, given in _lines(case):
        # (a) with the case's environment: the literal path the case names
        assert _is(answers[pinned], want, pinned), f"{pinned}: chose {answers[pinned]}, the case names {want}"
        # (b) with no environment: another decision
        same = _is(answers[default], want, default)
        if case.get("confirms_default"):
            assert same, f"{default}: {answers[default]} - the case no longer confirms the default, drop its flag"
        else:
            assert not same, f"{default}: the default dispatch chooses {want} too - the case tests nothing new"
        if given:
            # the default-side line may differ only in what the switch itself changed
            a, b = pinned.split()[:len(default.split())], default.split()
            diff = {x.split("=")[0]: (x.split("=")[1], y.split("=")[1]) for x, y in zip(a, b) if x != y}
            assert len(a) == len(b) and set(diff) in ({"lanes"}, {"pub_nd"}), (pinned, default)
            if "lanes" in diff:
                assert {"4": "LANES4", "16": "ROW16"}[diff["lanes"][0]] in n2, f"{pinned}: no n2 line shows these lanes"
            else:
                assert any(row[0] == "pins" for row in case["paths"]), f"{pinned}: no pins line shows the flag"
    assert bool(case.get("confirms_default")) == (case["name"] in CONFIRMS_DEFAULT)


def test_confirming_case_has_a_differing_sibling():
    """the pin of a confirms_default case is tested for real by another case"""
    for name in CONFIRMS_DEFAULT:
        env = PC.BY_NAME[name]["env"]
        assert any(c["env"] == env and not c.get("confirms_default") for c in PC.CASES), name


def test_table_is_well_formed():
    for case in PC.CASES:
        lines = PC.expected_lines(case)
        assert lines and len(set(lines)) == len(lines), case["name"]
        for op, count in lines:
            assert op.partition(":")[0] in PC.OPS and count >= 1, (case["name"], op)
        for op, count, label, n in case.get("labels", ()):
            assert (op, count) in lines and label.startswith("k_") and (n == ">0" or n >= 0), (case["name"], op, count)
        assert case["key"][0] in PC.FIXTURE and case["key"][1] in ("priv_djn", "priv_nodjn", "pub_djn", "pub_nodjn")
        K = int(case["key"][0].split("-")[0])
        assert all(f"K={K}" in row[0] for row in case["paths"] if " K=" in row[0]), case["name"]
        if K == 8192:  # the golden vectors and the 5 wide units, tiled to at most 5
            assert all(op in ("decrypt_golden", "decrypt_arb_wide") and count <= 5 for op, count in lines), case["name"]


def test_every_narrow_operation_has_its_wide_twin():
    """a case that runs an operation on residues below n^2 runs it on operands
    at and above n^2 too, at the same counts; decrypt_arb_wide also where the
    2048-bit-only decrypt_arb is not: in every case that decrypts"""
    twins = set(PC.WIDE_TWIN.values())
    assert all(t.partition(":")[0] in PC.OPS and t.partition(":")[0].endswith("_wide") for t in twins)
    seen = set()
    for case in PC.CASES:
        ops = {}
        for op, counts in case["ops"]:
            ops.setdefault(op, set()).update(counts)
        for op, counts in ops.items():
            if op in PC.WIDE_TWIN:
                assert ops.get(PC.WIDE_TWIN[op]) == counts, (case["name"], op)
                seen.add(PC.WIDE_TWIN[op])
            elif op in twins:
                narrow = [k for k, v in PC.WIDE_TWIN.items() if v == op]
                assert any(ops.get(k) == counts for k in narrow) or op == "decrypt_arb_wide", (case["name"], op)
        if "decrypt_golden" in ops:
            assert ops.get("decrypt_arb_wide") == ops["decrypt_golden"], case["name"]
    assert seen == twins, twins - seen


@pytest.mark.parametrize("K", sorted(PC.DISTINCT))
def test_wide_rows_are_wide(K):
    """no (wide operation, count) of the table compares only residues below
    n^2: of the rows a count tiles (tests/pinned_cases.py _tile, start = count;
    segprod and multiexp roll the same way), one at least holds an operand at
    or above n^2 - a batch of one the largest value the words hold"""
    import random

    from tests import wide_cases as W
    fx = {2048: "golden-2048-nodjn", 3072: "golden-3072", 4096: "golden-4096", 8192: "golden-8192"}[K]
    _, n, _, _, _ = W.key(fx)
    n2, d = n * n, PC.DISTINCT[K]
    counts = set()
    for case in PC.CASES:
        if int(case["key"][0].split("-")[0]) == K:
            counts |= {c for op, cs in case["ops"] if op in PC.WIDE_TWIN.values() for c in cs}
    assert counts
    for units in (True, False):
        ops = PC.wide_operands(K, n, d, "host", units)
        assert len(ops) == d and 4 * sum(c >= n2 for c in ops) >= 3 * (d - d // 4)
        top = 1 << (2 * K)  # n2w = 2 K / 32 words
        assert all(c < top for c in ops) and ops[1] >= top - 2, "row 1: a batch of one"
        assert all(c % n2 != W.truncated(c, n) for c in ops if c >= n2)
        if units:
            assert all(math.gcd(c % n2, n) == 1 for c in ops)
        else:
            assert W.q_max(n, 2 * K // 32) * n2 in ops
        for count in sorted(counts):
            rows = [ops[(count + i) % d] for i in range(min(count, d))]
            assert any(c >= n2 for c in rows), (count, units)
    assert random.Random(f"pinned-{K}-x-wide").random() != random.Random(f"pinned-{K}-y-wide").random()


def test_add_operands_are_not_reduced():
    """the Barrett edge list of the narrow adds keeps its operands above n^2"""
    import inspect
    src = inspect.getsource(PC.Child._add_vectors)
    assert "% n2" not in src.split("want = []")[0]


def test_switch_names():
    """every name a case sets is a switch of parse_pins and documented; every
    switch of parse_pins is set by a case, or has no kernel to reach, or is
    pinned by the module named for it"""
    known = PC.parse_pins_names()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    used = PC.switches()
    for name in used:
        assert name in known, f"{name} is not read by parse_pins"
        assert re.search(rf"\${name}\b", doc), f"{name} is not in INTEGRATION.md"
    assert PC.NO_KERNEL == ("XHE_ENC_TPI",)
    for name in known:
        if name in PC.NO_KERNEL:
            assert name not in used
        elif name in PC.COVERED_ELSEWHERE:
            src = open(os.path.join(ROOT, PC.COVERED_ELSEWHERE[name])).read()
            assert re.search(rf'\b{name}\b', src) and "pytest.mark.gpu" in src, name
        else:
            assert name in used, f"no case sets {name}"


def test_child_environment_carries_only_the_case():
    """a switch set around the suite does not leak into a child"""
    case = PC.BY_NAME["enc-pubtpi4"]
    env = PC.child_env(case, {"PATH": "/bin", "XHE_DEC_TPI": "4", "XHE_PUB_TPI": "64", "XHE_LIB": "x"})
    assert env == {"PATH": "/bin", "XHE_LIB": "x", "XHE_PUB_TPI": "4"}
