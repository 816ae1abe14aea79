"""Graded level counts of lc_advect's launches (lagrangiancoherence_amd/csrc/launch_plan.h: lcplan::grading,
graded_slot, graded_range) as a plain C++ program under AddressSanitizer + UBSan on the CPU: exhaustively over small
cases every tile's ranges tile [0, total) in order, the longest range keeps its stated bound (chunk + depth), degenerate
parameters are today's uniform chunks, and the per-launch map of dispatch positions is a bijection that keeps the XCD.
The header is the one advect.hip's launcher and the two-seed kernel include.

The program also states, by name, every plan tests/test_gpu_level_grading_matrix.py relies on (tile map and grid from the
header's xcd_chunk_tiles / xcd_grid / pole_rows) and checks the composition the kernel runs,
tile_of_block(graded_slot(...)): one workgroup per tile and launch, each tile's ranges [0, total) in order.  That these
checks can fail is shown here, on the CPU only: the program built against a perturbed copy of the header must fail."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "level_grading_test.cpp")
HEADER = os.path.join(ROOT, "lagrangiancoherence_amd", "csrc", "launch_plan.h")
# the plans tests/test_gpu_level_grading_matrix.py runs, as the program names them
CPU_PLANS = ["200 rows (14, 8, 14)", "rows [0, 128) of 328 (14, 8, 14)", "rows [64, 264) of 328 (14, 8, 14)",
             "rows [100, 300) of 328 (14, 8, 14)", "rows [128, 328) of 328 (14, 8, 14)", "328 rows (14, 24, 14): three eights",
             "200 rows (12, 8, 12): 4 launches", "200 rows (9, 8, 9): 5 launches", "200 rows (14, 8, 1)",
             "200 rows (14, 8, 20): depth capped", "200 rows (14, 1000, 14): zone capped", "rows [0, 128) (9, 8, 9): zeroed",
             "rows [100, 300) 34 levels (12, 8, 12)", "contiguous bands (14, 8, 14)", "contiguous bands (12, 8, 12)",
             "two tile rows per chunk (14, 8, 14)", "two tile rows per chunk (12, 8, 12)", "whole tile rows (14, 8, 14)",
             "whole tile rows (12, 8, 12)"]


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
    # the plans of the GPU matrix, each stated by name with the figures that file counts on, and the composition's sweep
    for what in CPU_PLANS:
        assert "plan " + what in r.stdout, what
    assert "composition tile_of_block(graded_slot)" in r.stdout and "xcd_chunk 0 / 3 / 5 / 17" in r.stdout


# (function, text in the header, what replaces it, what the program must then report)
MUTANTS = [
    ("graded_bound", "b -= graded_cut(g, graded_position(g, i - 1, slot));",
     "b -= graded_cut(g, graded_position(g, i - 1, slot)) + 1;", "FAIL"),
    ("graded_bound", "if (i == g.n - 1) b += graded_cut(g, graded_position(g, i, slot));",
     "if (i == g.n - 1) b += graded_cut(g, graded_position(g, i, slot)) + 1;", "FAIL"),
    ("graded_rotation", "return (launch < g.n - 1 ? launch : g.n + 1) * g.zone;",
     "return (launch < g.n - 1 ? launch : g.n + 1) * g.zone + (launch > 0);", "FAIL"),
    ("graded_rotation", "return (launch < g.n - 1 ? launch : g.n + 1) * g.zone;",
     "return (launch < g.n - 1 ? launch : g.n + 3) * g.zone;", "FAIL"),
    # the composition: a tile map that is wrong in one of its forms only, the plan's own arithmetic untouched
    ("tile_of_block", "if (xcd_chunk <= 0) return xcd * ((ntiles + XCDS - 1) / XCDS) + j;",
     "if (xcd_chunk <= 0) return xcd * ((ntiles + XCDS - 1) / XCDS) + (j ^ 1);", "composition, "),
    ("tile_of_block", "const int d = (cj * XCDS + xcd) * xcd_chunk + r;  // position in dispatch order",
     "const int d = (cj * XCDS + xcd) * xcd_chunk + (r == 4 ? 3 : r);", "composition, "),
]


@pytest.mark.parametrize("fn, old, new, says", MUTANTS, ids=[f"{m[0]}-{i}" for i, m in enumerate(MUTANTS)])
def test_a_perturbed_header_fails_the_program(tmp_path, fn, old, new, says):
    """Sensitivity, on the CPU alone (a graded range that is off by one reads past the last packed level: no such kernel is
    ever run): the same program against a copy of the header with one line of graded_bound, graded_rotation or
    tile_of_block changed must fail, and say where."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    text = open(HEADER).read()
    assert text.count(old) == 1, f"launch_plan.h no longer holds this line of {fn}: {old}"
    (tmp_path / "tests" / "c").mkdir(parents=True)
    (tmp_path / "lagrangiancoherence_amd" / "csrc").mkdir(parents=True)
    (tmp_path / "lagrangiancoherence_amd" / "csrc" / "launch_plan.h").write_text(text.replace(old, new))
    src = tmp_path / "tests" / "c" / "level_grading_test.cpp"
    shutil.copy(SRC, src)
    exe = str(tmp_path / "mutant")
    subprocess.run([gxx, "-std=c++17", "-O1", str(src), "-o", exe], check=True)   # (the program guards every index it takes from the header)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "all checks passed" not in r.stdout, f"{fn}: the perturbed header passes"
    assert says in r.stdout + r.stderr, r.stdout[-2000:] + r.stderr[-2000:]


def test_advect_hip_takes_its_ranges_from_the_tested_header():
    """The launcher and the kernel call the header's functions (a copy of the arithmetic beside it would make the CPU
    test vacuous)."""
    src = open(os.path.join(ROOT, "lagrangiancoherence_amd", "csrc", "advect.hip")).read()
    for fn in ("lcplan::grading", "lcplan::graded_slot", "lcplan::graded_range"):
        assert fn in src, fn
    # ... and the composition the program checks is the kernel's own expression
    assert "lcplan::tile_of_block(lcplan::graded_slot(A.grade, A.grade_launch, d), A.ntiles, A.ntx, A.xcd_chunk, A.tile_order)" in src
