"""The bucket multi-exponentiation planner (paths.hpp bucket_window,
bucket_cost, multiexp_route) on the CPU: tests/native/bucket_plan_check.cpp,
built with the address and undefined-behaviour sanitizers, in its own process."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_bucket_planner(tmp_path):
    exe = str(tmp_path / "bucket_plan_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(HERE, "native", "bucket_plan_check.cpp"),
                    "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    from xfl_amd import _native as nat
    assert r.returncode == 0 and r.stdout.strip() == f"ok kBucketMinTerms={nat.BUCKET_MIN_TERMS}", r.stdout + r.stderr
