"""What lc_advect_ex asks of the HIP runtime behind a deferred pack (lc_field_pack_deferred), on tests/c/fake_hip.c with its
trace switched on (tests/c/deferred_pack_trace.cpp; the library compiled host-only, no GPU): with a pack pending, an
eligible call launches no ``pack_fused_kernel`` and grows its launches by the pack workgroups of ``lcplan::pack_mix`` -- the
launches that carry nothing are today's --; every ineligible call launches ``pack_fused_kernel`` once, first, and then
exactly what it launches after a plain ``lc_field_pack``; with deferring switched off both the pack and the call are
today's.  A second deferred pack, a change of stream, ``lc_sync``, ``lc_sample`` and ``lc_ctx_destroy`` complete a pending
pack too."""
import os

import pytest

from tests import test_host_route_trace as H

pytestmark = pytest.mark.skipif(not os.path.exists(H.HIPCC), reason="hipcc not found")

PACK = "pack_fused_kernel"
NT, NY_F, FIRST = 72, 48, 32          # the driver's series and field rows; levels the deferred entry packs at once: [0, FIRST]
ADVECT_BLOCKS, POLE_BLOCKS, PACK_SHARE, PERIOD = 512, 8, 8, 64   # 512 x 512 seeds in tall patches of 8 x 64; two pole rows of 512 seeds; 8 pack blocks per 64


@pytest.fixture(scope="module")
def calls(tmp_path_factory):
    return H.run_driver(H.build_driver(tmp_path_factory.mktemp("deferred_pack_trace"), "deferred_pack_trace"))


def launches(trace):
    """``[(kernel symbol, grid.x, grid.z)]`` of a trace."""
    out = []
    for l in trace:
        if l.startswith("launch "):
            w = l.split()
            g = w[3].split(",")
            out.append((w[1], int(g[0]), int(g[2])))
    return out


def body(trace):
    return [l for l in trace if not l.startswith(("status", "allocs"))]


def pending(trace):
    return int(trace[-1].rsplit("pending=", 1)[1])


def pack_blocks(t_lo, upto, item_levels=8, items_per_wg=7):
    """Pack workgroups of a launch that carries the levels [t_lo, upto) of the driver's 48 x 96-node field among 512 advect
    workgroups: lcplan::pack_items and pack_mix_for_items (csrc/launch_plan.h), restated."""
    items = -(-(96 + H.LC_PAD) // 256) * (NY_F + H.LC_PAD) * -(-(upto - t_lo) // item_levels)
    want = max(items // items_per_wg, PACK_SHARE)
    mix = lambda shift: (ADVECT_BLOCKS // ((1 << shift) - PACK_SHARE)) * PACK_SHARE
    shift = 5
    while shift < 14 and mix(shift) > want and mix(shift + 1) > 0:
        shift += 1
    return mix(shift)


def cases_of(calls, kind):
    return sorted({k.split(" | ")[0] for k in calls if k.startswith(kind + " ")})


def test_the_deferred_entry_packs_the_first_levels_only(calls):
    for k, t in calls.items():
        if not k.startswith("pack ") or k.endswith("| twice"):
            continue
        (sym, gx, gz), = launches(t)
        nt = 41 if "nt=41" in k else NT
        assert PACK in sym and gx == 1
        if k.endswith("| deferred"):
            assert gz == (FIRST + 1 + 1) // 2 and pending(t) == FIRST + 1, k       # lin[0 .. 32], two levels per block
        else:                                                                      # today's, and the switch off
            assert gz == (nt + 1) // 2 and pending(t) == 0, k
    for name in cases_of(calls, "pack"):
        if "| " not in name and name + " | off" in calls:
            assert body(calls[name + " | off"]) == body(calls[name + " | today"]), name


def test_switched_off_every_call_is_todays(calls):
    names = cases_of(calls, "eligible") + cases_of(calls, "ineligible")
    assert len(names) == 14
    for name in names:
        assert calls[name + " | off"] == calls[name + " | today"], name
        assert not [s for s, _, _ in launches(calls[name + " | today"]) if PACK in s]
        assert body(calls["flush " + name + " | off"]) == [] == body(calls["flush " + name + " | today"])


def test_an_ineligible_call_completes_the_pack_first_and_is_todays(calls):
    names = cases_of(calls, "ineligible")
    assert sorted(n.split(" ", 1)[1].split(":")[0] for n in names) == sorted(
        ["nt=41", "K=0", "order=3", "traj_x", "two members", "outer clamp", "t0=10", "other images", "one launch"])
    for name in names:
        t, today = calls[name + " | deferred"], calls[name + " | today"]
        nt = 41 if "nt=41" in name else NT
        first = launches(t)[0]
        assert PACK in first[0] and first[2] == (nt - FIRST + 1) // 2, (name, first)    # the levels from 32 on, once
        assert body(t)[0].startswith("launch ") and body(t)[1:] == body(today), name
        assert t[-1] == today[-1] and pending(t) == 0, name
        assert body(calls["flush " + name + " | deferred"]) == [], name


def test_an_eligible_call_carries_the_pack_in_its_launches(calls):
    names = cases_of(calls, "eligible")
    assert len(names) == 5
    today_grid = ADVECT_BLOCKS + POLE_BLOCKS
    # Per launch: None, or the levels (t_lo, upto) it carries -- lin from t_lo + 1, ext from t_lo, both below upto.  Launch i packs up
    # to what launch i + 1 reaches (lcplan::launch_reach; levels count from t0): upto = min(nt, t0 + reach(i + 1) + 1).
    want = {
        "eligible nt=72": [(32, 72), None, None],          # graded: launch 1 of 3 reaches the series' end (64 + depth 32 > 71)
        "eligible nt=72 per-point": [(32, 72), None, None],
        "eligible nt=72 K=2 chunk=16": [None, (32, 49), (48, 65), (64, 72), None],    # launch 1 stays inside the 33 levels packed at once
        "eligible nt=72 uniform chunk=32": [(32, 65), (64, 72), None],
        "eligible nt=72 uniform chunk=8 t0=5": [None, None, (32, 38), (37, 46), (45, 54), (53, 62), (61, 70), (69, 72), None],
    }
    for name in names:
        t, today = calls[name + " | deferred"], calls[name + " | today"]
        got, was = launches(t), launches(today)
        assert not [s for s, _, _ in got if PACK in s], name
        assert [s for s, _, _ in got] == [s for s, _, _ in was] and len({s for s, _, _ in got}) == 1, name     # the same instance, launch by launch
        assert all(g == ADVECT_BLOCKS + POLE_BLOCKS for _, g, _ in was)
        assert [g for _, g, _ in got] == [today_grid + (pack_blocks(*c) if c else 0) for c in want[name]], (name, got)
        assert t[-1] == today[-1] and pending(t) == 0, name             # the same reported kernel and launch count; the pack is complete
        assert len(body(t)) == len(body(today))                         # no copy, event or synchronisation added
        assert body(calls["flush " + name + " | deferred"]) == [], name


def test_whatever_else_touches_the_context_completes_the_pack(calls):
    rest = (NT - FIRST + 1) // 2
    seq = {k.split(" | ")[0]: calls[k] for k in calls if k.endswith("| twice")}
    assert pending(seq["pack first"]) == FIRST + 1
    two = launches(seq["pack second"])
    assert [z for _, _, z in two] == [rest, (FIRST + 2) // 2] and pending(seq["pack second"]) == FIRST + 1    # the first one's rest, then its own first levels
    for what in ("set_stream", "sync", "sample", "tracer", "copy_to_host", "destroy"):
        first = launches(seq[what])[0]
        assert PACK in first[0] and first[2] == rest and pending(seq[what]) == 0, what
    # completed on the stream it began on; the stream the context turns to waits for it (the caller's own waits were recorded
    # before the rest of the pack was enqueued), and nothing else does
    assert body(seq["set_stream"])[0].endswith(" on s0") and body(seq["sync"])[0].endswith(" on s-null")
    kinds = [l.split()[0] for l in body(seq["set_stream"])]
    assert kinds == ["launch", "event_record", "stream_wait"], body(seq["set_stream"])
    rec, wait = body(seq["set_stream"])[1].split(), body(seq["set_stream"])[2].split()
    assert rec[1] == wait[-1] and rec[-1] == "s0" and wait[1] == "s-null", (rec, wait)      # event_record eN on s0; stream_wait s-null for eN
    for what in ("sync", "sample", "tracer", "destroy", "pack second"):
        assert "stream_wait" not in [l.split()[0] for l in body(seq[what])], what
    assert "tracer_kernel" in launches(seq["tracer"])[1][0]
