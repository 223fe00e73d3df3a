"""Build pmd_pair_selftest (k_djn_pmd's rows in pairs, PMD::mul_pair and PMD::mul,
against host big integers) the way tests/native/build.py builds its harnesses:
hipcc cross-compiles for gfx950 without a GPU, the binary lands in
tests/native/_build (git-ignored, shipped to the GPU box with the tree) and is
run by tests/test_gpu_pmd_pair.py. Called from __graft_entry__.build().

    python tests/native/build_pmd_pair.py
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "_build")
CSRC = os.path.join(ROOT, "xfl_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
NAME = "pmd_pair_selftest"
HEADERS = ["bn_dev.hpp", "hostbn.hpp", "pdigit_dev.hpp"]


def build(verbose=True):
    os.makedirs(OUT, exist_ok=True)
    src, exe = os.path.join(HERE, NAME + ".hip"), os.path.join(OUT, NAME)
    deps = [src] + [os.path.join(CSRC, h) for h in HEADERS]
    if os.path.exists(exe) and all(os.path.getmtime(d) <= os.path.getmtime(exe) for d in deps):
        return
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", src, "-o", exe + ".tmp"]
    if verbose:
        print("[tests/native]", " ".join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    os.replace(exe + ".tmp", exe)


if __name__ == "__main__":
    build()
    sys.exit(0)
