"""Segment lists, operands and the GPU child of the segmented scan's tests
(tests/test_scan_plan.py on the CPU, tests/test_gpu_segscan.py on the GPU).

xhe_segscan cuts every segment into chunks of C rows (xfl_amd/csrc/
scan_plan.hpp chunk_len: one fixed value, CHUNK_LENS below, asserted as a
literal by tests/test_scan_plan.py), scans the chunk totals the same way and
stops when every segment is one chunk: one level up to C rows a segment, two
up to C^2, three up to C^3, four from C^3 + 1. The lists below put a segment
on each side of every such edge; with C = 16 the longest, C^3 + 1, is 4,097
rows - one past kN2RowMax, so with $XHE_N2_TPI unset it also is the one list
that runs in the batch shape.

A plain module (no fixtures). run_child() is what a child process of
tests/test_gpu_segscan.py runs: one JSON line per (key, list, operands) with
the rows compared and how many differ; every row is compared with Python
integers (acc = acc * c % n^2).
"""
import ctypes
import json
import os
import random
import sys

import numpy as np

from tests.conftest import ROOT

CHUNK_LENS = (16,)
SETTINGS = ("unset", "4", "16")  # $XHE_N2_TPI of the three children
KEYS = ("golden-2048-djn", "golden-2048-nodjn", "golden-3072", "golden-4096", "golden-8192", "sparse_2046")


def segment_lists(C):
    """{name: segment lengths} of one chunk length"""
    lists = {"1": [1], "2": [2], "C": [C], "C+1": [C + 1], "C^2": [C * C], "C^2+1": [C * C + 1],
             "C^3+1": [C ** 3 + 1],
             "empties": [0, 1, C + 1, 0, C, C * C + 1, 0],  # empty segments first, inside and last
             "3x7": [7, 7, 7]}
    # one more than the lane groups of a 256-thread block (64 groups of 4 lanes, 16 of 16): as chunks
    # (the chunk pass, one group per chunk) and as rows of one segment (the apply pass, one per row)
    for g in (17, 65):
        lists[f"{g}x1"] = [1] * g
        lists[f"1x{g}"] = [g]
    return lists


def lists_for(key_name, C):
    """the lists a key runs: all of them, the three-level one only while it stays within 4,097 rows (else at
    2048 bits alone)"""
    out = dict(segment_lists(C))
    if C ** 3 + 1 > 4097 and not key_name.startswith("golden-2048"):
        del out["C^3+1"]
    return out


SPECIAL = ("empties", "3x7")  # the lists that also run with a 1 and a 0 among the operands


def offsets(lens):
    seg = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(np.asarray(lens, dtype=np.int64), out=seg[1:])
    return seg


def reference(cs, lens, n2):
    """the inclusive prefix products of every segment, as Python integers"""
    out, i = [], 0
    for ln in lens:
        acc = 1
        for c in cs[i:i + ln]:
            acc = acc * c % n2
            out.append(acc)
        i += ln
    return out


def wide_positions(lens, C):
    """rows that take an operand at or above n^2: the first, middle and last row of every segment and of its
    first two chunks, and the first row of the last chunk"""
    pos, lo = [], 0
    for ln in lens:
        rel = {0, ln // 2, ln - 1, C // 2, C - 1, C, C + C // 2, 2 * C - 1, (ln - 1) // C * C}
        pos += [lo + r for r in sorted(rel) if 0 <= r < ln]
        lo += ln
    return pos


def operands(kind, lens, n, n2w, C, rng):
    """the operand list of a run: `rand` residues below n^2; `wide` the same with tests/wide_cases.py's values
    at wide_positions; `special` with a 1 in the first non-empty segment and a 0 in the second chunk (or the
    middle) of the longest one"""
    from tests import wide_cases as W
    n2 = n * n
    count = sum(lens)
    cs = [rng.randrange(2, n2) for _ in range(count)]
    if kind == "wide":
        pos = wide_positions(lens, C)
        ws = W.wide(n, n2w, min(len(pos), 24), rng)
        for i, p in enumerate(pos):
            cs[p] = ws[i % len(ws)]
        assert any(c >= n2 for c in cs)
    elif kind == "special":
        seg = offsets(lens)
        nz = [s for s, ln in enumerate(lens) if ln > 1]
        longest = max(nz, key=lambda s: lens[s])
        one = [s for s in nz if s != longest][0]
        cs[int(seg[one]) + lens[one] // 2] = 1
        cs[int(seg[longest]) + min(C + 5, lens[longest] // 2)] = 0
    return cs


# ------------------------------------------------------------------ the parent's side
_CHILD = r"""
import sys
sys.path.insert(0, {root!r})
import torch
torch.cuda.init()
from tests import scan_cases
scan_cases.run_child({setting!r})
"""


def child_argv(setting):
    return [sys.executable, "-c", _CHILD.format(root=ROOT, setting=setting)]


def child_env(setting, environ=None):
    env = {k: v for k, v in (os.environ if environ is None else environ).items() if k != "XHE_N2_TPI"}
    if setting != "unset":
        env["XHE_N2_TPI"] = setting
    return env


def expected_lines(C):
    """the (key, list, operands) triples a child reports, and the entry-point checks"""
    out = []
    for key in KEYS:
        for name in lists_for(key, C):
            out += [(key, name, "rand"), (key, name, "wide")]
            if name in SPECIAL:
                out.append((key, name, "special"))
        out.append((key, "count0", "none"))
    out += [("golden-2048-nodjn", "host", "rand"), ("golden-2048-nodjn", "einval", "none"),
            ("golden-2048-nodjn", "profile", "none")]
    return sorted(out)


def parse_report(stdout):
    return [json.loads(line) for line in stdout.splitlines() if line.startswith("{")]


# ------------------------------------------------------------------- the child's side
def _report(key, name, kind, count, got, want, extra_bad=0):
    if got.shape != want.shape:
        checked, bad = 0, np.arange(max(len(got), len(want)))
    else:
        bad = np.nonzero(np.any(got != want, axis=1))[0]
        checked = len(want)
    print(json.dumps({"key": key, "list": name, "operands": kind, "count": count, "checked": checked,
                      "bad": int(bad.size) + extra_bad, "first_bad": bad[:6].tolist()}), flush=True)


def _call(nat, dk, c, count, seg, nseg, out):
    """xhe_segscan's return code on device tensors (or None pointers)"""
    from xfl_amd.paillier import resident
    return nat.lib().xhe_segscan(dk.handle, resident._dp(c), count, seg.ctypes.data_as(ctypes.c_void_p), nseg,
                                 resident._dp(out), resident._sp(dk.device))


def run_child(setting):
    import torch

    from tests import wide_cases as W
    from xfl_amd import _native as nat
    from xfl_amd.paillier import resident
    assert os.environ.get("XHE_N2_TPI") == (None if setting == "unset" else setting)
    C = CHUNK_LENS[0]
    L = nat.lib()
    for key in KEYS:
        K, n = W.key(key)[:2]
        n2 = n * n
        dk = nat.DeviceKey(K, n, None, None, None)
        assert not dk.private and not dk.djn
        dev = dk.device
        for name, lens in lists_for(key, C).items():
            seg = offsets(lens)
            for kind in ("rand", "wide") + (("special",) if name in SPECIAL else ()):
                cs = operands(kind, lens, n, dk.n2w, C, random.Random(f"segscan-{key}-{name}-{kind}"))
                want = reference(cs, lens, n2)
                assert all(w < n2 for w in want)
                if kind == "special":
                    assert want.count(0) >= 2 and 1 in cs  # everything behind the 0 in its segment is 0
                got = resident.download(resident.segscan(dk, resident.upload(nat.ints_to_words(cs, dk.n2w), dev), seg))
                # every output below n^2: equal words say so, a differing row is counted once more if it is not
                above = sum(int.from_bytes(r.tobytes(), "little") >= n2 for r in got) if kind == "wide" else 0
                _report(key, name, kind, len(cs), got, nat.ints_to_words(want, dk.n2w), above)
        # count = 0 with nseg = 1: XHE_OK, nothing written
        with resident._On(dev):
            canary = torch.full((1, dk.n2w), 0x5A5A5A5A, dtype=torch.int32, device=f"cuda:{dev}")
            src = torch.zeros((1, dk.n2w), dtype=torch.int32, device=f"cuda:{dev}")
        rc = _call(nat, dk, src, 0, np.zeros(2, dtype=np.int64), 1, canary)
        kept = resident.download(canary)
        _report(key, "count0", "none", 0, kept[:0], kept[:0], int(rc != 0) + int(np.any(kept != 0x5A5A5A5A)))
        if key != "golden-2048-nodjn":
            continue
        # ---- entry-point checks, on one key
        lens = segment_lists(C)["empties"]
        seg = offsets(lens)
        cs = operands("rand", lens, n, dk.n2w, C, random.Random("segscan-host"))
        cw = nat.ints_to_words(cs, dk.n2w)
        count = len(cs)
        L.xhe_profile(1)  # (resets the records)
        try:
            d_out = resident.download(resident.segscan(dk, resident.upload(cw, dev), seg))
            tot, all_n, own_n = ctypes.c_double(), ctypes.c_int64(), ctypes.c_int64()
            nat.check(L.xhe_profile_read(None, ctypes.byref(tot), ctypes.byref(all_n)))
            nat.check(L.xhe_profile_read(b"k_segscan", ctypes.byref(tot), ctypes.byref(own_n)))
        finally:
            L.xhe_profile(0)
        # k_segscan is the call's one label: no product or add kernel of another entry point was launched
        _report(key, "profile", "none", 0, d_out[:0], d_out[:0], int(own_n.value != 1) + int(all_n.value != 1))
        h_out = np.empty_like(cw)
        nat.check(L.xhe_segscan_host(dk.handle, cw.ctypes.data_as(ctypes.c_void_p), count,
                                     seg.ctypes.data_as(ctypes.c_void_p), len(lens), h_out.ctypes.data_as(ctypes.c_void_p)),
                  "segscan_host")
        _report(key, "host", "rand", count, h_out, d_out)
        # XHE_EINVAL: nothing is launched for any of these
        c = resident.upload(cw, dev)
        with resident._On(dev):
            big = torch.zeros((2 * count, dk.n2w), dtype=torch.int32, device=f"cuda:{dev}")
            big[:count].copy_(c)
        out = big[count:]
        i64 = lambda v: np.asarray(v, dtype=np.int64)  # noqa: E731
        nseg = len(lens)
        bad_first, bad_last, decreasing = seg.copy(), seg.copy(), seg.copy()
        bad_first[0] = 1
        bad_last[-1] = count - 1
        decreasing[2], decreasing[3] = seg[3], seg[2]
        assert decreasing[3] < decreasing[2]
        calls = {
            "ok": (_call(nat, dk, big[:count], count, seg, nseg, out), 0),
            "bad first offset": (_call(nat, dk, big[:count], count, bad_first, nseg, out), nat.XHE_EINVAL),
            "bad last offset": (_call(nat, dk, big[:count], count, bad_last, nseg, out), nat.XHE_EINVAL),
            "decreasing offsets": (_call(nat, dk, big[:count], count, decreasing, nseg, out), nat.XHE_EINVAL),
            "out == c": (_call(nat, dk, big[:count], count, seg, nseg, big[:count]), nat.XHE_EINVAL),
            "out overlaps c's tail": (_call(nat, dk, big[:count], count, seg, nseg, big[count - 1:2 * count - 1]),
                                      nat.XHE_EINVAL),
            "out overlaps c's head": (_call(nat, dk, big[1:count + 1], count, seg, nseg, big[:count]), nat.XHE_EINVAL),
            "nseg == 0": (_call(nat, dk, big[:count], count, i64([0]), 0, out), nat.XHE_EINVAL),
            "nseg < 0": (_call(nat, dk, big[:count], count, seg, -1, out), nat.XHE_EINVAL),
        }
        wrong = {k: v for k, v in calls.items() if v[0] != v[1]}
        if wrong:
            print(f"einval: (returned, expected) {wrong}", file=sys.stderr)
        resident.download(big)  # the stream is drained before the tensors go
        _report(key, "einval", "none", 0, d_out[:0], d_out[:0], len(wrong))
