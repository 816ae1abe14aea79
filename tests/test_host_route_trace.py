"""What the one-call host routes ask of the HIP runtime, call by call, against the record of the commit before they shared one
device-side core (tests/golden/host_route_trace.txt, written by tests/golden/make_host_route_trace.py at the commit the file
names).

tests/c/host_route_trace.cpp drives ``lc_lcs_host`` (both dtypes, orders 1 to 3, the three x boundaries, SETTLS 0 and 4,
trajectories, smoothing, both float64 fidelity settings, plain and staged transfers, the pipelined form and its sub-ranges),
``lc_lcs_global_host`` and the positional ``lc_advect`` entry points against tests/c/fake_hip.c with its trace switched on:
every launch by kernel name with grid, block and stream, every copy and memset with kind, size, destination and source, every
event record, wait and synchronisation, and the sizes the call allocated -- no addresses, and nothing that depends on the
order of a call's allocations alone.  The full trace of the table is some 640 KB, so the record keeps per call the SHA-256 of
its trace and the count of each kind of line; the comparison is exact.  The library objects are compiled host-only (the
kernels become launch stubs): no GPU is involved."""
import hashlib
import os
import shutil
import subprocess
from collections import Counter

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lagrangiancoherence_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "host_route_trace.txt")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
UNITS = ["api", "pack", "advect", "sigma", "ridges", "halo", "preprocess"]
KINDS = ("launch", "memcpy", "memcpy_async", "memset_async", "event_record", "stream_wait", "event_sync", "stream_sync")
LC_PAD = 3          # csrc/lcs_common.h: lc_level_elems = (ny_f + LC_PAD) * (nx_f + LC_PAD) * 2

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")


def build_driver(workdir, driver="host_route_trace"):
    """tests/c/<driver>.cpp linked with the host side of csrc/ and the recording runtime; the program's path."""
    workdir = str(workdir)
    objs, procs = [], []
    for u in UNITS:
        o = os.path.join(workdir, f"{u}.o")
        procs.append(subprocess.Popen([HIPCC, "--cuda-host-only", "-std=c++17", "-fPIC", "-Wno-unused-function", "-O1",
                                       '-DLCS_BUILD_ID="trace"', "-c", os.path.join(CSRC, u + ".hip"), "-o", o],
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
        objs.append(o)
    for p in procs:
        out, _ = p.communicate()
        assert p.returncode == 0, out[-3000:]
    fake = os.path.join(workdir, "fake_hip.o")
    subprocess.run([HIPCC, "-x", "c", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-O1", "-c",
                    os.path.join(ROOT, "tests", "c", "fake_hip.c"), "-o", fake], check=True)
    clangxx = os.path.join(os.path.dirname(os.path.realpath(HIPCC)), "..", "lib", "llvm", "bin", "clang++")
    if not os.path.exists(clangxx):
        clangxx = "/opt/rocm/lib/llvm/bin/clang++"
    drv = os.path.join(workdir, driver + ".o")
    subprocess.run([clangxx, "-std=c++17", "-Wall", "-Wextra", "-O1", "-c", os.path.join(ROOT, "tests", "c", driver + ".cpp"), "-o", drv],
                   check=True)
    exe = os.path.join(workdir, driver)
    # (each host object refers to its own __hip_fatbin_<hash>, which only a device link defines: left unresolved, never read)
    r = subprocess.run([clangxx, drv, *objs, fake, "-o", exe, "-ldl", "-lm", "-lpthread", "-Wl,--unresolved-symbols=ignore-all"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def run_driver(exe):
    """``{label: [trace lines]}`` in the driver's order."""
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    calls, cur = {}, None
    for line in r.stdout.splitlines():
        if line.startswith("== "):
            assert line[3:] not in calls, line
            cur = calls[line[3:]] = []
        else:
            cur.append(line)
    return calls


def summary(lines):
    """One call's record: the digest of its trace and how many lines of each kind it has."""
    n = Counter(l.split(" ", 1)[0] for l in lines)
    assert set(n) <= set(KINDS) | {"allocs", "status"}, set(n)
    return hashlib.sha256("\n".join(lines).encode()).hexdigest() + "".join(f" {k}={n[k]}" for k in KINDS if n[k])


def read_golden():
    with open(GOLDEN) as f:
        rows = [l.rstrip("\n") for l in f if not l.startswith("#")]
    return dict(r.split(" | ") for r in rows)


@pytest.fixture(scope="module")
def calls(tmp_path_factory):
    return run_driver(build_driver(tmp_path_factory.mktemp("host_route_trace")))


def mismatches(calls, golden):
    return [(k, summary(calls[k]), golden[k]) for k in golden if summary(calls[k]) != golden[k]]


def test_the_record_covers_the_table():
    g = read_golden()
    host5 = [k for k in g if k.startswith("lcs_host nt=5 ")]
    assert len(host5) == 3 * 3 * 3 * 2 * 2 * 2 * 2 == 432       # (f32, f64 exact, f64 fast) x order x boundary x K x traj x smoothing x transfers
    assert len([k for k in g if k.startswith("lcs_host nt=41 ")]) == 6 and len([k for k in g if k.startswith("lcs_global_host")]) == 3
    assert len([k for k in g if k.startswith("lc_advect")]) == 3 and len(g) == 444
    with open(GOLDEN) as f:
        head = f.readline().split()
    assert head[:3] == ["#", "recorded", "at"] and len(head[3]) == 40


def test_every_call_asks_the_runtime_what_the_parent_asked(calls):
    golden = read_golden()
    assert list(calls) == list(golden)
    assert all(c[-1] == "status 0" for c in calls.values())
    bad = mismatches(calls, golden)
    assert not bad, (len(bad), bad[:3])


def test_the_comparison_tells_two_routes_apart(calls):
    """float64 at order 1, the reference's operation order against the fast form: the fast form owns and packs a fused-level
    image, the exact one packs nothing.  Their traces differ, and the comparison fails when one is taken for the other."""
    a = "lcs_host nt=5 f64 fid=exact order=1 cyclic=1 K=4 traj=0 gauss=0 pipe=1"
    b = a.replace("fid=exact", "fid=fast")
    golden = read_golden()
    assert calls[a] != calls[b] and summary(calls[a]) != summary(calls[b])
    swapped = dict(calls, **{a: calls[b], b: calls[a]})
    assert sorted(k for k, _, _ in mismatches(swapped, golden)) == sorted([a, b])
    one_byte = dict(calls, **{a: calls[a][:-2] + [calls[a][-2] + " 1"] + calls[a][-1:]})      # one more allocation of one byte
    assert [k for k, _, _ in mismatches(one_byte, golden)] == [a]


def images_of(label, lines):
    """The images an ``lc_lcs_host`` call of the 24 x 40 field allocated, from the sizes in its trace."""
    opt = dict(kv.split("=") for kv in label.split()[2:] if "=" in kv)
    nt, order, es = int(opt["nt"]) if "nt" in opt else int(label.split("nt=")[1].split()[0]), int(opt["order"]), 4 if " f32 " in label else 8
    level = (24 + LC_PAD) * (40 + LC_PAD) * 2 * es
    sizes = Counter(int(s) for s in [l for l in lines if l.startswith("allocs")][0].split()[1:])
    others = {nt * 24 * 40 * es, 33 * es, 47 * es, 33 * 47 * es, 33 * 47 * es * 5}        # planes, seeds, results, trajectories
    assert not {nt * level, (nt - 1) * level} & others
    assert sizes[nt * level] <= 1 and sizes[(nt - 1) * level] <= 1        # (lin and cub never exist together on these routes)
    return ({("lin" if order == 1 else "cub")} if sizes[nt * level] else set()) | ({"ext"} if sizes[(nt - 1) * level] else set())


def test_the_images_of_a_call_are_the_engines_plan(calls):
    """The C routes' image plan against ``engine.field_plan`` under the options the engine's reference-shaped call hands it
    (``Engine.f64_fuse_levels``, ``Engine._pack_options``): the same images for every case of the nt = 5 table."""
    from lagrangiancoherence_amd import engine as E
    n = 0
    for label, lines in calls.items():
        if not label.startswith("lcs_host nt=5 "):
            continue
        opt = dict(kv.split("=") for kv in label.split()[2:] if "=" in kv)
        dtype = np.dtype(np.float32 if " f32 " in label else np.float64)
        fuse = dtype == np.float32 or opt["fid"] == "fast"          # Engine.f64_fuse_levels
        fuse_levels, ext_image = E.Engine._pack_options(dtype, int(opt["K"]), fuse, None)
        plan = E.field_plan(dtype, False, int(opt["order"]), 5, fuse_levels, None, ext_image, E.Engine.EXT_IMAGE_F64, E.Engine.EXT_IMAGE_F64_O3)
        assert images_of(label, lines) == set(plan.images), (label, images_of(label, lines), plan.images)
        n += 1
    assert n == 432
