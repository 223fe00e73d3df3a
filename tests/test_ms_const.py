"""CPU: k_djn_pmd's short-plaintext factors KeyDev::ms_p = Q R^2 B mod P and
ms_q = P R^2 B mod Q (R = 2^(28 * 37), B = 2^(28 * 4); xfl_amd/csrc/keyconst.hpp
decrypt_constants) against Python integers.

tests/native/ms_const_check.cpp (its own main, built here with ASan + UBSan as
tests/test_mu_const.py builds its checker, started as a separate process)
derives the image of a key and prints the two fields through the bound KeyDev.
Checked on the golden 2048-bit DJN key (production window, split layout) and
the structured 2048-bit keys top, bottom, mixed, mixed_swapped and pattern as
private DJN keys: the value, canonical limbs (each below 2^28), and the place
in the blob - rows of 40 words right after mu_q, 16-byte aligned, before the
blob's last constant eq_words. Keys that do not run k_djn_pmd (public, non-DJN,
3072 bits) leave both fields null.
"""
import os
import subprocess

import pytest

from tests.conftest import hx, load_fixture

HERE = os.path.dirname(os.path.abspath(__file__))
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
XHE_WIN_SPLIT = 0x100
K, W = 37, 28
R = 1 << (W * K)
B = 1 << (W * 4)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("msconst") / "ms_const_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", *SAN, "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"),
                    os.path.join(HERE, "native", "ms_const_check.cpp"), "-o", exe], check=True)
    return exe


def _run(program, bits, priv, djn, win, n, p, q, h):
    line = " ".join([f"{bits:x}", f"{(1 if priv else 0) | (2 if djn else 0):x}", f"{win:x}", f"{n:x}",
                     f"{p:x}" if priv else "-", f"{q:x}" if priv else "-", f"{h:x}" if djn else "-"]) + "\n"
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=1"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1:halt_on_error=1"
    env.pop("LD_PRELOAD", None)  # the sanitizer runtime must come first in the child
    r = subprocess.run([program], input=line, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    out = {}
    for ln in r.stdout.splitlines():
        t = ln.split()
        if t[0] == "words":
            out["words"] = int(t[1])
        elif t[0] == "F":
            assert t[5:] != ["OUT-OF-BLOB"], ln[:80]
            out[t[1]] = None if int(t[2]) < 0 else (int(t[2]), [int(x, 16) for x in t[5:]])
    return out


def _golden():
    k = load_fixture("paillier_2048_djn.json")["key"]
    return hx(k["n"]), hx(k["p"]), hx(k["q"]), hx(k["h_pow_n"])


def _structured(name):
    from tests import structured_keys as SK
    k = SK.key(2048, name)
    return k.n, k.p, k.q, k.h


CASES = [("golden", 23 | XHE_WIN_SPLIT)] + [(s, 16) for s in ("top", "bottom", "mixed", "mixed_swapped", "pattern")]


@pytest.mark.parametrize("name,win", CASES, ids=[c[0] for c in CASES])
def test_ms_values(program, name, win):
    n, p, q, h = _golden() if name == "golden" else _structured(name)
    out = _run(program, 2048, True, True, win, n, p, q, h)
    for f, X, Y in (("ms_p", p, q), ("ms_q", q, p)):
        off, ls = out[f]
        assert len(ls) == K and all(x < (1 << W) for x in ls)
        assert sum(x << (W * i) for i, x in enumerate(ls)) == Y * pow(R, 2, X) * B % X, f
        assert off % 4 == 0
    # between mu_q and the blob's last constant, rows of 40 words
    assert out["ms_p"][0] == out["mu_q"][0] + 40 and out["ms_q"][0] == out["ms_p"][0] + 40
    last = out["eq_words"]
    assert out["ms_q"][0] + 40 <= last[0] and (last[0] + len(last[1]) + 3) & ~3 == out["words"]


def test_ms_absent_elsewhere(program):
    n, p, q, h = _golden()
    assert _run(program, 2048, False, True, 16, n, p, q, h)["ms_p"] is None  # public DJN
    k = load_fixture("paillier_2048_nodjn.json")["key"]
    out = _run(program, 2048, True, False, 16, hx(k["n"]), hx(k["p"]), hx(k["q"]), 0)
    assert out["ms_p"] is None and out["ms_q"] is None
    k = load_fixture("paillier_3072_djn.json")["key"]
    out = _run(program, 3072, True, True, 16, hx(k["n"]), hx(k["p"]), hx(k["q"]), hx(k["h_pow_n"]))
    assert out["ms_p"] is None and out["ms_q"] is None
