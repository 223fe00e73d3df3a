"""The planner of the subtraction on the sparse level histogram (paths.hpp
sub_sparse_list, level_sub_sparse) on the CPU:
tests/native/level_sub_sparse_plan_check.cpp, built with the address and
undefined-behaviour sanitizers, in its own process."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_level_sub_sparse_planner(tmp_path):
    exe = str(tmp_path / "level_sub_sparse_plan_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(HERE, "native", "level_sub_sparse_plan_check.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
