"""Graded level counts of lc_advect's launches (lagrangiancoherence_amd/csrc/launch_plan.h: lcplan::grading,
graded_slot, graded_range) as a plain C++ program under AddressSanitizer + UBSan on the CPU: exhaustively over small
cases every tile's ranges tile [0, total) in order, the longest range keeps its stated bound (chunk + depth), degenerate
parameters are today's uniform chunks, and the per-launch map of dispatch positions is a bijection that keeps the XCD.
The header is the one advect.hip's launcher and the two-seed kernel include."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "level_grading_test.cpp")


def test_level_grading_invariants_under_asan_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "level_grading_test")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600,
                       env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1", "UBSAN_OPTIONS": "print_stacktrace=1"})
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout


def test_advect_hip_takes_its_ranges_from_the_tested_header():
    """The launcher and the kernel call the header's functions (a copy of the arithmetic beside it would make the CPU
    test vacuous)."""
    src = open(os.path.join(ROOT, "lagrangiancoherence_amd", "csrc", "advect.hip")).read()
    for fn in ("lcplan::grading", "lcplan::graded_slot", "lcplan::graded_range"):
        assert fn in src, fn
