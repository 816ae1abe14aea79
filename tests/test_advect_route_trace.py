"""What the advect dispatcher asks of the HIP runtime, case by case, against the record of the commit before its launch
ladders were built by one helper (tests/golden/advect_route_trace.txt, written by tests/golden/make_advect_route_trace.py at
the commit the file names; never regenerated from later code).

tests/c/advect_route_trace.cpp drives ``lc_advect_ex`` (1 and 3 members), ``lc_advect_series``, ``lc_advect_series_dirs``,
``lc_tracer_sample`` and ``lc_sample_raw`` on fake device buffers of ``kernel_routes``' shapes against tests/c/fake_hip.c with
its trace switched on: the four dtype codes, orders 1 to 5, SETTLS_order 0 to 5, the three x boundaries, with and without
trajectories, six source presets (which of packed_lin, packed_ext, the raw planes and fuse_levels_raw are given), under
``lc_ctx_set_lds_tiles`` / ``lc_ctx_set_verify`` / ``lc_ctx_set_level_chunk`` settings and in contexts created under the
environments the route table uses.  Per case: every launch by kernel SYMBOL with grid, block and stream, every copy, memset
and synchronisation, the sizes allocated, and the status with the name ``lc_ctx_last_advect_kernel`` /
``lc_ctx_last_tracer_kernel`` reported and the launch count -- so a launch that runs one instance and reports another differs
from the record.  Calls the intake refuses are cases too (their status).  Some 227 000 cases and 70 MB of trace: the record
keeps, per group (environment, call, dtype, x boundary), the SHA-256 of the group's traces in the driver's order, the count of
each kind of line and the number of cases; the comparison is exact.  The library objects are compiled host-only (the kernels
become launch stubs): no GPU is involved."""
import os
from collections import defaultdict

import pytest

from tests import kernel_routes as KR
from tests import test_host_route_trace as H

GOLDEN = os.path.join(H.ROOT, "tests", "golden", "advect_route_trace.txt")

pytestmark = pytest.mark.skipif(not os.path.exists(H.HIPCC), reason="hipcc not found")

# Advect-side routes no CPU run can launch, each with the dispatcher line that makes it so.  The one admissible reason: the
# selection reads data a kernel wrote.
UNREACHED_ON_CPU = {
    "outer_substep_kernel": "advect_impl: `else if (moved[0])` -- the clamp flag the fused kernel sets, read back after a chunk",
    "outer_substep_batch_kernel": "advect_impl: `if (restarts[m] < 0 && moved[m])` -- the per-member clamp flags, likewise",
}


def group_of(label):
    return label.split(" | ")[0]


def record(cases):
    """``{group: digest of its cases' traces, line counts, number of cases}`` in the driver's order."""
    lines, n = defaultdict(list), defaultdict(int)
    for label, trace in cases.items():
        lines[group_of(label)] += trace
        n[group_of(label)] += 1
    return {g: f"{H.summary(lines[g])} cases={n[g]}" for g in lines}


def read_golden():
    with open(GOLDEN) as f:
        rows = [l.rstrip("\n") for l in f if not l.startswith("#")]
    return dict(r.split(" || ") for r in rows)


def mismatches(cases, golden):
    rec = record(cases)
    return [(g, rec.get(g), golden[g]) for g in golden if rec.get(g) != golden[g]]


def reported(cases):
    """``{reported kernel name: the symbols of the last launch of the cases that reported it}``."""
    out = defaultdict(set)
    for trace in cases.values():
        status = trace[-1].split(" ", 2)
        if len(status) == 3:
            launches = [l.split()[1] for l in trace if l.startswith("launch ")]
            out[status[2].rsplit(" launches=", 1)[0]].add(launches[-1])
    return out


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    return H.run_driver(H.build_driver(tmp_path_factory.mktemp("advect_route_trace"), "advect_route_trace"))


def test_the_record_covers_the_table():
    g = read_golden()
    envs = ("none", "LCS_PATCH_MODE=1", "LCS_PATCH_MODE=2", "LCS_F64_WG_TILE=1")
    table = [f"env={e} call={c} dtype={d} cyclic={x}" for e in envs for c in ("ex1", "ex3", "series", "dirs")
             for d in ("f32", "f64", "f64_wind_f32", "f64_wind_f32_lin32") for x in (0, 1, 2)]
    extra = [f"env=none call={c} dtype={d} cyclic=-" for c in ("tracer", "sample") for d in ("f32", "f64")] + ["env=none call=refusals dtype=f32 cyclic=-"]
    assert sorted(g) == sorted(table + extra) and len(g) == 197
    per_setting = 5 * 6 * 6           # orders x SETTLS orders x source presets (ex1: with and without trajectories)
    for k, v in g.items():
        n = int(v.rsplit("cases=", 1)[1])
        if k in table:
            assert n == per_setting * (12 if k.startswith("env=none ") else 3) * (2 if " call=ex1 " in k else 1), k
    with open(GOLDEN) as f:
        head = f.readline().split()
    assert head[:3] == ["#", "recorded", "at"] and len(head[3]) == 40


def test_every_group_asks_the_runtime_what_the_parent_asked(cases):
    golden = read_golden()
    assert list(record(cases)) == list(golden)
    bad = mismatches(cases, golden)
    assert not bad, (len(bad), bad[:3])


def test_the_sweep_launches_every_route_a_cpu_run_can(cases):
    """The sweep covers no less than the route table: every ``advect_`` name (112) and every ``tracer_kernel`` name (10) of
    ``kernel_routes.ROUTES`` is reported by some case, and the advect-side names it does not reach are the two of
    UNREACHED_ON_CPU."""
    wanted = [n for n in KR.ROUTES if n.startswith("advect_")]
    tracers = [n for n in KR.ROUTES if n.startswith("tracer_kernel")]
    assert len(wanted) == 112 and len(tracers) == 10
    seen = reported(cases)
    assert not [n for n in wanted + tracers if n not in seen]
    assert sorted(n for n in KR.ROUTES if not n.startswith("sigma") and n not in seen) == sorted(UNREACHED_ON_CPU)
    assert not [n for n in seen if n not in KR.ROUTES]
    # a reported name is one launched symbol, and a launched symbol has one name
    assert all(len(s) == 1 for s in seen.values()), {n: s for n, s in seen.items() if len(s) != 1}
    assert len({next(iter(s)) for s in seen.values()}) == len(seen)


def test_the_comparison_tells_two_boundaries_apart(cases):
    """Two cases that differ in ``cyclic_x`` only (the cyclic and the per-point instance of the one-seed LDS kernel): their
    traces differ, and taking one for the other fails the comparison for exactly their two groups."""
    a = "env=none call=ex1 dtype=f32 cyclic=0 | lds=2 verify=0 chunk=-1 order=1 K=4 traj=0 src=lin+ext"
    b = a.replace("cyclic=0", "cyclic=1")
    golden = read_golden()
    assert cases[a] != cases[b] and cases[a][-1] == "status 0 advect_lds_kernel<1, 4, false> launches=1"
    assert cases[b][-1] == "status 0 advect_lds_kernel<1, 4, true> launches=1"
    swapped = dict(cases)
    swapped[a], swapped[b] = cases[b], cases[a]
    assert sorted(g for g, _, _ in mismatches(swapped, golden)) == sorted([group_of(a), group_of(b)])
    renamed = dict(cases)                  # the right launches under another instance's name
    renamed[a] = cases[a][:-1] + [cases[b][-1]]
    assert [g for g, _, _ in mismatches(renamed, golden)] == [group_of(a)]
