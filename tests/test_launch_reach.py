"""What the deferred pack takes from lagrangiancoherence_amd/csrc/launch_plan.h, as a plain C++ program under
AddressSanitizer + UBSan on the CPU (tests/c/launch_reach_test.cpp): ``lcplan::launch_reach`` against every slot's range,
exhaustively over small plans (no range of launch i ends above it, some slot attains it), the block map of a launch that
carries pack workgroups (``pack_mix`` / ``pack_mix_block``: every advect position once on its own XCD, pack workgroups in
groups of 8) and the items of the pack workgroups (``pack_items``: every item once).  That the checks can fail is shown on
perturbed copies of the header."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "launch_reach_test.cpp")
HEADER = os.path.join(ROOT, "lagrangiancoherence_amd", "csrc", "launch_plan.h")


def test_launch_reach_and_block_map_under_asan_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "launch_reach_test")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600,
                       env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1", "UBSAN_OPTIONS": "print_stacktrace=1"})
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
    for what in ("launch_reach:", "pack_mix:", "pack_items:"):
        assert what in r.stdout, what


# (function, text in the header, what replaces it)
MUTANTS = [
    ("launch_reach", "return imin(g.total, (i + 1) * g.chunk + (i + 1 == g.n - 1 ? g.depth : 0));",
     "return imin(g.total, (i + 1) * g.chunk);"),                       # the last boundary's outward move forgotten
    ("launch_reach", "return imin(g.total, (i + 1) * g.chunk + (i + 1 == g.n - 1 ? g.depth : 0));",
     "return imin(g.total, (i + 1) * g.chunk + g.depth);"),             # every boundary moved outwards: not attained
    ("pack_mix_block", "idx = q * na + r;", "idx = q * na + (r ^ 1);"),  # an advect block off its XCD
    ("pack_mix", "m.pack_blocks = periods * pack_per_period;", "m.pack_blocks = periods * pack_per_period + 8;"),
]


@pytest.mark.parametrize("fn, old, new", MUTANTS, ids=[f"{m[0]}-{i}" for i, m in enumerate(MUTANTS)])
def test_a_perturbed_header_fails_the_program(tmp_path, fn, old, new):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not available")
    text = open(HEADER).read()
    assert text.count(old) == 1, f"launch_plan.h no longer holds this line of {fn}: {old}"
    (tmp_path / "tests" / "c").mkdir(parents=True)
    (tmp_path / "lagrangiancoherence_amd" / "csrc").mkdir(parents=True)
    (tmp_path / "lagrangiancoherence_amd" / "csrc" / "launch_plan.h").write_text(text.replace(old, new))
    src = tmp_path / "tests" / "c" / "launch_reach_test.cpp"
    shutil.copy(SRC, src)
    exe = str(tmp_path / "mutant")
    subprocess.run([gxx, "-std=c++17", "-O1", str(src), "-o", exe], check=True)   # (the program guards every index it takes from the header)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "all checks passed" not in r.stdout, f"{fn}: the perturbed header passes"
    assert "FAIL" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_the_library_takes_reach_and_block_map_from_the_tested_header():
    """The launcher and the kernel call the header's functions (a copy of the arithmetic beside it would make the CPU test
    vacuous), and both pack kernels write through the one shared node body."""
    csrc = os.path.join(ROOT, "lagrangiancoherence_amd", "csrc")
    adv, pack = open(os.path.join(csrc, "advect.hip")).read(), open(os.path.join(csrc, "pack.hip")).read()
    for fn in ("lcplan::launch_reach", "lcplan::pack_mix(", "lcplan::pack_mix_block(", "lcplan::pack_items("):
        assert fn in adv, fn
    for src in (adv, pack):
        assert '#include "pack_node.h"' in src and "pack_node_levels<" in src
    assert "mirror_index(int i, int n) {" not in pack and "__builtin_nontemporal_store" not in pack
