"""Diagnostic build (-DLCS_TIMELINE): when the workgroups of the two-seed order-1 kernel start and end, per launch of one
advect call -- how long a launch drains after its last workgroup was dispatched, how long the next one takes to fill the
chip, and the slot-time both leave unused.

    python -m lagrangiancoherence_amd.build --out build/ab/timeline.so -DLCS_TIMELINE
    LCS_LIB=build/ab/timeline.so python tools/launch_ends.py [--seeds 4096] [--nt 97] [--plan uniform:32] [--plan graded:32,3584,32] ...

A plan is `uniform:<level chunk>` (lc_ctx_set_level_chunk) or `graded:<chunk>,<zone>,<depth>` (lc_ctx_set_level_grading).
Stamps are the 100 MHz wall clock (one counter for the whole device; the shader clock differs between XCDs)."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from lagrangiancoherence_amd import flows  # noqa: E402
from lagrangiancoherence_amd.engine import Engine  # noqa: E402

TICK_US = 0.01


def read_timeline(lib, ctx):
    n, g = C.c_int(), C.c_int()
    lib.lc_debug_read_timeline.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    assert lib.lc_debug_read_timeline(ctx, None, 0, C.byref(n), C.byref(g)) == 0
    rec = np.zeros((n.value, g.value, 4), dtype=np.uint64)
    assert lib.lc_debug_read_timeline(ctx, rec.ctypes.data_as(C.c_void_p), rec.size // 4, C.byref(n), C.byref(g)) == 0
    return rec


def overlap(t0, t1, a, b):
    return np.clip(np.minimum(t1, b) - np.maximum(t0, a), 0, None).sum()


def analyse(rec, out):
    """Per launch: duration, drain (last dispatch -> end), ramp (start -> 95 % of the launch's level of residency), the
    slot-time unused in both (as microseconds of the whole chip: unused slot-time / that level), the gap to the next launch."""
    base = None
    rows, ends = [], []
    for li in range(rec.shape[0]):
        r = rec[li]
        ok = (r[:, 3] > 0) & (r[:, 1] > 0)
        t0 = r[ok, 0].astype(np.float64) * TICK_US
        t1 = r[ok, 1].astype(np.float64) * TICK_US
        if base is None:
            base = t0.min()
        t0, t1 = t0 - base, t1 - base
        start, last, end = t0.min(), t0.max(), t1.max()
        ev = np.concatenate([np.stack([t0, np.ones_like(t0)], 1), np.stack([t1, -np.ones_like(t1)], 1)])
        ev = ev[np.lexsort((ev[:, 1], ev[:, 0]))]
        res = np.cumsum(ev[:, 1])
        # the launch's own level of residency: the median over its middle half (single peaks lie 10-15 % above it)
        mid = (ev[:, 0] >= start + 0.25 * (end - start)) & (ev[:, 0] <= end - 0.25 * (end - start))
        peak = float(np.median(res[mid]))
        full = ev[np.argmax(res >= 0.95 * peak), 0]
        drain_lost = max(peak * (end - last) - overlap(t0, t1, last, end), 0.0) / peak
        ramp_lost = max(peak * (full - start) - overlap(t0, t1, start, full), 0.0) / peak
        # residency over the launch's last 300 microseconds, every 20
        at = np.searchsorted(ev[:, 0], end - np.arange(300.0, -1.0, -20.0), side="right") - 1
        prof = [int(res[i]) if i >= 0 else 0 for i in at]
        rows.append(dict(launch=li, wgs=int(ok.sum()), levels=int(r[ok, 3].sum()), start=start, end=end, dur=end - start, peak=int(peak),
                         drain=end - last, drain_lost=drain_lost, ramp=full - start, ramp_lost=ramp_lost, life=float(np.median(t1 - t0)),
                         life_max=float((t1 - t0).max()), prof=prof))
        ends.append(end)
    total = rows[-1]["end"] - rows[0]["start"]
    print("launch   wgs  levels/wg  start us   dur us level  median/max life us  drain us (unused)  ramp us (unused)  gap before us", file=out)
    for i, w in enumerate(rows):
        gap = w["start"] - rows[i - 1]["end"] if i else 0.0
        print(f"{w['launch']:6d} {w['wgs']:6d} {w['levels'] / w['wgs']:9.2f} {w['start']:9.1f} {w['dur']:8.1f} {w['peak']:5d} "
              f"{w['life']:8.1f} /{w['life_max']:7.1f} {w['drain']:9.1f} ({w['drain_lost']:6.1f}) {w['ramp']:8.1f} ({w['ramp_lost']:6.1f}) {gap:10.1f}", file=out)
        print("       resident workgroups 300 us .. 0 us before the launch's end, every 20 us: " + " ".join(str(p) for p in w["prof"]), file=out)
    lost = sum(w["drain_lost"] + w["ramp_lost"] for w in rows) + sum(rows[i]["start"] - rows[i - 1]["end"] for i in range(1, len(rows)))
    print(f"first start -> last end {total:.1f} us; drains + ramps + gaps leave {lost:.1f} chip-us unused = {100 * lost / total:.2f} % of it", file=out)
    return total, lost


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=4096)
    ap.add_argument("--nt", type=int, default=97)
    ap.add_argument("--plan", action="append", default=None)
    ap.add_argument("--out", default=None, help="also append the report to this file")
    a = ap.parse_args()
    plans = a.plan or ["uniform:32"]
    eng = Engine(0)
    lib = C.CDLL(os.environ["LCS_LIB"])
    u, v, lat, lon = flows.era5_like(nt=a.nt)
    slat, slon = flows.seed_grid(a.seeds, a.seeds, lat, lon)
    f = eng.prepare_field(u, v, lat, lon, 1)
    outs = [sys.stdout] + ([open(a.out, "a")] if a.out else [])
    for plan in plans:
        kind, _, val = plan.partition(":")
        if kind == "uniform":
            eng.set_level_chunk(int(val))
        else:
            eng.set_level_chunk(-1)
            eng.set_level_grading(*[int(s) for s in val.split(",")])
        ms = []
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(torch.cuda.current_stream())
            eng.advect(f, slat, slon, -900.0, 4, 1, True)
            e1.record(torch.cuda.current_stream())
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        rec = read_timeline(lib, eng.ctx)
        for o in outs:
            print(f"== plan {plan}: {a.seeds}^2 seeds, {a.nt - 1} levels, {eng.last_advect_kernel()}, {eng.last_advect_launches()} launches; "
                  f"advect call by events {ms[0]:.3f} {ms[1]:.3f} {ms[2]:.3f} ms (the records are the last one's)", file=o)
            analyse(rec, o)
    eng.close()


if __name__ == "__main__":
    main()
