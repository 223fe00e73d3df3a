"""Device arithmetic self-tests on the GPU (binaries built on the CPU by
tests/native/build.py, called from __graft_entry__.build()):

* mont_selftest - Mont<S, W, TPI>::mul / reduce_once / normalize for every
  limb shape of every key size against host big integers (hostbn.hpp);
* pdigit_selftest - the Montgomery-digit arithmetic mod P^2 (pdigit_dev.hpp
  PMD) against host big integers - product chains, the
  conversions to and from the 74-limb Montgomery form - plus its timing line
  against the production Montgomery product (row in LDS, as k_djn_pow_lds).

Each of these two prints one JSON line per check with the number of
mismatching elements; all must be 0.

* rand_selftest - k_rand_djn and k_rand_below launched with tiny `bits` and
  `bound`, where the zero-draw redraw and the 64-rejections exit run all the
  time. It prints what the kernels wrote; the comparison with the RFC-pinned
  reference (tests/chacha_ref.py) is made here."""
import json
import os
import subprocess

import pytest

from tests import chacha_ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BUILD = os.path.join(HERE, "native", "_build")


def _run(name):
    exe = os.path.join(BUILD, name)
    # a missing harness fails the GPU suite (it is built with the library by
    # __graft_entry__.build(); a skip would let the suite pass without it)
    assert os.path.exists(exe), f"{name} not built (python tests/native/build.py)"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    checks = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{") and '"bad"' in l]
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert checks and all(c["bad"] == 0 for c in checks), checks
    return checks, r.stdout


def test_montgomery_shapes_selftest():
    checks, _ = _run("mont_selftest")
    assert len(checks) >= 9


def test_montgomery_digit_selftest():
    checks, out = _run("pdigit_selftest")
    assert {c["check"] for c in checks} == {"mul", "sqr", "to_mont2", "from_mont2"}
    assert all(c.get("out_of_range", 0) == 0 for c in checks)
    assert "products_per_s" in out


FILL = "a5a5a5a5"
# words, bits, tpe. The last two: a whole top word (bits - 32 k = 32, the edge of the top-word mask); live words
# in lanes 1 and 2 of a group (every multi-lane case before it masks them to zero, so a wrong counter in those
# lanes would not show), the third lane's block half used (8 words) and a 22-bit top word
RAND_DJN = [(4, 1, 1), (4, 3, 1), (32, 2, 2), (32, 33, 2), (48, 2, 4), (128, 1, 8), (3, 70, 1), (4, 64, 1),
            (40, 1270, 4)]
# words, bits, bound; the last one again with a whole top word
RAND_BELOW = [(2, 40, (1 << 39) + 12345), (2, 33, (1 << 32) + (1 << 31)), (1, 1, 2), (2, 40, 1),
              (2, 64, (1 << 63) + (1 << 62) + 5)]


def _hexwords(s):
    assert len(s) % 8 == 0
    return [int(s[k:k + 8], 16) for k in range(0, len(s), 8)]


def test_rand_kernels_selftest():
    """Every word k_rand_djn / k_rand_below write at tiny `bits` / `bound`
    equals chacha_ref.draw: the redraw after a zero draw (half the elements
    at bits = 1), lanes that mask to zero or are idle, the scalar-store branch
    (words = 3), a bound whose top word ties in half the draws, and the
    ST_VALUE exit when nothing is acceptable. The reference itself must show
    the redraws, so the cases cannot quietly stop exercising them."""
    exe = os.path.join(BUILD, "rand_selftest")
    assert os.path.exists(exe), "rand_selftest not built (python tests/native/build.py)"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-500:] + r.stderr[-2000:]
    cases = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert [(c["words"], c["bits"], c["tpe"]) for c in cases if c["kernel"] == "djn"] == RAND_DJN
    assert [(c["words"], c["bits"], int(c["bound"], 16)) for c in cases if c["kernel"] == "below"] == RAND_BELOW
    assert len(cases) == len(RAND_DJN) + len(RAND_BELOW)
    bad = []
    for c in cases:
        words, bits, count, base = c["words"], c["bits"], c["count"], c["base"]
        assert count == 300
        seed, nonce = bytes.fromhex(c["key"]), int(c["nonce"], 16)
        bound = int(c["bound"], 16) if c["kernel"] == "below" else None
        name = (c["kernel"], words, bits, c["tpe"] if bound is None else bound)
        ref = [chacha_ref.draw(seed, nonce, base + i, words, bits, bound) for i in range(count)]
        redrawn = sum(t > 0 for _, t, _ in ref)
        if bound is None and bits <= 3:
            assert redrawn >= 20, (name, redrawn)  # a condition on the inputs: P(zero draw) >= 1/8
        got_st = _hexwords(c["status"])
        assert len(c["out"]) == 8 * count * words and len(got_st) == count
        if c["guard"] != FILL * words or c["status_guard"] != FILL:
            bad.append((name, "guard", c["guard"], c["status_guard"]))
        if got_st != [st for _, _, st in ref]:
            bad.append((name, "status", [i for i in range(count) if got_st[i] != ref[i][2]][:8]))
        if bound == 1:  # nothing acceptable: statuses only (the words are the last rejected candidate)
            assert all(st == chacha_ref.ST_VALUE for _, _, st in ref)
            continue
        assert all(st == 0 for _, _, st in ref), name
        # every word of the row, zeros above `bits` included
        want = ["".join("%08x" % ((v >> (32 * k)) & 0xFFFFFFFF) for k in range(words)) for v, _, _ in ref]
        got = [c["out"][8 * words * i:8 * words * (i + 1)] for i in range(count)]
        if got != want:
            rows = [i for i in range(count) if got[i] != want[i]]
            bad.append((name, "words", len(rows), rows[:8], [ref[i][1] for i in rows[:8]]))
    assert not bad, bad
