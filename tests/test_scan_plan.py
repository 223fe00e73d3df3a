"""CPU: the plan of the segmented scan (xfl_amd/csrc/scan_plan.hpp).

tests/native/scan_plan_check.cpp (its own main, plain g++, started as a
separate process) prints the plan of each input line. The chunk-length rule and
the small plans are asserted as literals written from the header's comment;
the properties a plan must have are then checked on every segment list the GPU
test runs (tests/scan_cases.py), for every chunk length the rule returns.
"""
import os
import re
import subprocess

import pytest

from tests import scan_cases as SC

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# count -> chunk length: one fixed value, whatever the count
CHUNK_LEN = [(0, 16), (1, 16), (16, 16), (17, 16), (4096, 16), (4097, 16), (16384, 16), (1 << 20, 16),
             (1 << 31, 16), (1 << 40, 16)]

# segment lengths -> the printed plan: per level its rows, then first/len/total/carry of every chunk
PLANS = [
    ("1", "rows=1: 0/1/-1/-1"),
    ("16", "rows=16: 0/16/-1/-1"),
    ("17", "rows=17: 0/16/0/-1 16/1/1/0 | rows=2: 0/2/-1/-1"),
    ("0", "empty"),
    ("0,0,0", "empty"),
    ("7,7,7", "rows=21: 0/7/-1/-1 7/7/-1/-1 14/7/-1/-1"),
    ("0,1,17,0,16,33,0",
     "rows=67: 0/1/-1/-1 1/16/0/-1 17/1/1/0 18/16/-1/-1 34/16/2/-1 50/16/3/2 66/1/4/3 | rows=5: 0/2/-1/-1 2/3/-1/-1"),
    ("257", "rows=257: " + " ".join(f"{16 * t}/{16 if t < 16 else 1}/{t}/{t - 1}" for t in range(17))
     + " | rows=17: 0/16/0/-1 16/1/1/0 | rows=2: 0/2/-1/-1"),
]


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = os.path.join(str(tmp_path_factory.mktemp("scan_plan")), "scan_plan_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    os.path.join(HERE, "native", "scan_plan_check.cpp"), "-o", exe], check=True)

    def run(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr
        out = r.stdout.splitlines()
        assert len(out) == len(lines), r.stdout
        return out
    return run


def test_chunk_length_rule(ask):
    got = ask([f"chunk_len count={c}" for c, _ in CHUNK_LEN])
    assert [int(g) for g in got] == [want for _, want in CHUNK_LEN]
    # every value the rule returns is one the GPU test runs its lists at
    assert sorted(set(int(g) for g in got)) == sorted(SC.CHUNK_LENS)


def test_small_plans(ask):
    got = ask([f"plan {lens}" for lens, _ in PLANS])
    wrong = [(lens, g, want) for (lens, want), g in zip(PLANS, got) if g != want]
    assert not wrong, "\n".join(f"{lens}: planned {g}, expected {want}" for lens, g, want in wrong)


def _parse(text):
    """[(rows, [(first, len, total, carry)])] per level"""
    if text == "empty":
        return []
    levels = []
    for part in text.split(" | "):
        head, _, chunks = part.partition(":")
        levels.append((int(head[5:]), [tuple(int(v) for v in c.split("/")) for c in chunks.split()]))
    return levels


@pytest.mark.parametrize("C", SC.CHUNK_LENS)
def test_plan_properties(ask, C):
    lists = SC.segment_lists(C)
    lists["C^3"] = [C ** 3]
    lists["ragged"] = [C - 1, C + 1, 2 * C, 2 * C + 1, 0, 1, C * C - 1]
    got = ask([f"plan {','.join(str(v) for v in lens)}" for lens in lists.values()])
    for (name, lens), text in zip(lists.items(), got):
        levels = _parse(text)
        seg_lens = list(lens)  # the segments of the level in hand
        for depth, (rows, chunks) in enumerate(levels):
            where = f"{name}, level {depth}"
            assert rows == sum(seg_lens), where
            # the chunks partition [0, rows) in order
            assert [c[0] for c in chunks] == [sum(c[1] for c in chunks[:i]) for i in range(len(chunks))], where
            assert sum(c[1] for c in chunks) == rows, where
            assert all(1 <= c[1] <= C for c in chunks), where
            # no chunk crosses a segment boundary; an empty segment has no chunk; a chunk's carry is the chunk
            # before it in its own segment (the next level's row of that chunk), none for the first
            it = iter(chunks)
            lo, nxt_lens, nxt_rows = 0, [], 0
            for ln in seg_lens:
                mine = []
                while sum(c[1] for c in mine) < ln:
                    mine.append(next(it))
                assert sum(c[1] for c in mine) == ln and (not mine or mine[0][0] == lo), where
                assert len(mine) == -(-ln // C), where  # as few chunks as the length allows
                for t, (_, _, total, carry) in enumerate(mine):
                    if len(mine) == 1:
                        assert (total, carry) == (-1, -1), where
                    else:
                        assert total == nxt_rows + t and carry == (total - 1 if t else -1), where
                if len(mine) > 1:
                    nxt_lens.append(len(mine))
                    nxt_rows += len(mine)
                lo += ln
            assert next(it, None) is None, where
            seg_lens = nxt_lens
        # the levels end when every segment is one chunk, and not before
        assert seg_lens == [], name
        if levels:
            assert all(c[2] == -1 for c in levels[-1][1]), name
            nonempty = sum(1 for ln in lens if ln)
            assert len(levels[0][1]) >= nonempty and all(len(lv[1]) >= 1 for lv in levels), name
        want_levels = 0 if not sum(lens) else 1 + next(k for k in range(8) if max(lens) <= C ** (k + 1))
        assert len(levels) == want_levels, name


def test_header_is_host_only():
    """scan_plan.hpp: standard headers only and no HIP call"""
    src = open(os.path.join(ROOT, "xfl_amd", "csrc", "scan_plan.hpp")).read()
    assert re.findall(r'#include\s*"', src) == []
    assert not re.search(r"\bhip[A-Z_]|__global__|__device__|getenv", src)
