"""The sparse-aware histogram's planner (paths.hpp sparse_tile,
sparse_tiles_max, hist_sparse) on the CPU: tests/native/sparse_plan_check.cpp,
built with the address and undefined-behaviour sanitizers, in its own process."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_sparse_planner(tmp_path):
    exe = str(tmp_path / "sparse_plan_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(HERE, "native", "sparse_plan_check.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
