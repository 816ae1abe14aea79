"""Time Engine.idw_interp: scattered parcel values gridded by inverse-distance weighting on the sphere.

    python tools/idw_timing.py [--warmup 3] [--reps 11] [--out profiles/idw/timing.txt] [--quick]

Two workloads, both float64, one plane, power 2, sources and values on the device already, the result left there:
  example   16 020 sources -> the 89 x 180 grid of the reference's example (latitudes -88 .. 88, longitudes -180 .. 178), without
            a bound: what the reference's xr_idx_interp does in its all-pairs numba loop.  63 workgroups of targets: the sources
            of each are split over 9 workgroups and combined (the kernels are printed).
  regional  51 493 sources -> a 221 x 233 grid over 60 W .. 2 W, 35 S .. 20 N at 0.25 degrees, with max_distance = 500 km and
            without.
The sources are seeded points uniform on the sphere (example) or on the region grown by 5 degrees (regional): the parcels of a
forward trajectory end up scattered, not on a grid.  A call is timed with a pair of device events on the current stream, after
`--warmup` calls: the median (and the smallest) of `--reps`, in ms per call -- the Engine's own host work (numpy cos / sin of the
coordinates, the sort by latitude with a bound, the uploads) is inside, as a user pays it.  `pairs`: the (target, source) pairs
the search kernel walks, counted on the host by the kernel's own rule (256 consecutive targets share one range of the sorted
sources); `within`: those within the bound, which pay the weight.  Before anything is reported, 300 seeded targets of each
result are compared with the numpy oracle of tests/idw.py within its tolerance.
Prints one JSON line per timing and a table; `--out` also writes both there.  Needs a GPU (there is no other path).
`--quick`: a tenth of the sources, to rehearse the script."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

THREADS = 256            # csrc/idw.hip: IDW_THREADS
BAND_MARGIN = 1e-12      # csrc/idw.hip: IDW_BAND_MARGIN


def pairs_walked(plan):
    """What idw_search_kernel walks and what is within reach: per workgroup of 256 consecutive targets, its targets times the
    sources of its range (idw_range_kernel's rule on the plan's own vectors)."""
    (sx, sy, sz), (tx, ty, tz) = plan["src"], plan["tgt"]
    chord2 = plan["max_chord2"]
    if not chord2 > 0:                      # without a bound every pair is walked and weighted
        return tx.size * sx.size, tx.size * sx.size
    walked = within = 0
    cs = np.sqrt(sx * sx + sy * sy)
    for p0 in range(0, tx.size, THREADS):
        t = slice(p0, min(p0 + THREADS, tx.size))
        if chord2 > 0:
            ct = np.sqrt(tx[t] * tx[t] + ty[t] * ty[t])
            lo, hi = np.argmin(tz[t]), np.argmax(tz[t])
            above = (sz >= tz[t][lo]) | ((ct[lo] - cs) ** 2 + (tz[t][lo] - sz) ** 2 <= chord2 + BAND_MARGIN)
            below = (sz <= tz[t][hi]) | ((ct[hi] - cs) ** 2 + (tz[t][hi] - sz) ** 2 <= chord2 + BAND_MARGIN)
            inside = np.flatnonzero(above & below)
            if inside.size == 0:
                continue
            r = slice(inside[0], inside[-1] + 1)
        else:
            r = slice(0, sx.size)
        dx, dy, dz = tx[t, None] - sx[None, r], ty[t, None] - sy[None, r], tz[t, None] - sz[None, r]
        cost = (dx * dx + dy * dy) + dz * dz
        walked += cost.size
        within += int((cost <= chord2).sum()) if chord2 > 0 else cost.size
    return walked, within


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    import torch
    from lagrangiancoherence_amd.dropin import get_engine
    from lagrangiancoherence_amd.engine import Engine
    from tests import idw as IDW
    eng = get_engine()
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    def series(fn):
        for _ in range(a.warmup):
            timed(fn)
        ms = [timed(fn)[0] for _ in range(a.reps)]
        return {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4)}
    shrink = 10 if a.quick else 1
    rng = np.random.default_rng(20261020)
    ex_lon, ex_lat = IDW.scattered(16020 // shrink, 20261020)
    rg_lon, rg_lat = rng.uniform(-65.0, 3.0, 51493 // shrink), rng.uniform(-40.0, 25.0, 51493 // shrink)
    workloads = [("example", ex_lon, ex_lat, np.linspace(-180.0, 178.0, 180), np.linspace(-88.0, 88.0, 89), (None,)),
                 ("regional", rg_lon, rg_lat, -60.0 + 0.25 * np.arange(233), -35.0 + 0.25 * np.arange(221), (500e3, None))]
    rows = []
    for name, x, y, lon, lat, bounds in workloads:
        z = IDW.values(None, x.size, 7)
        dev = [eng.to_device(v, np.float64) for v in (x, y, z)]
        for bound in bounds:
            fn = lambda: eng.idw_interp(dev[0], dev[1], dev[2], lon, lat, grid=True, max_distance=bound)
            _, u = timed(fn)
            kernels = eng.last_idw_kernel
            pick = np.random.default_rng(1).choice(lat.size * lon.size, 300, replace=False)
            Lon, Lat = np.meshgrid(lon, lat)
            o = IDW.oracle(x, y, z, Lon.ravel()[pick], Lat.ravel()[pick], max_distance=bound)
            got = u.cpu().numpy().ravel()[pick]
            assert np.array_equal(np.isnan(got), np.isnan(o["u64"])), f"{name}, max_distance {bound}: the NaN pattern differs from the oracle's"
            f = ~np.isnan(got)
            assert (np.abs(got - o["u64"])[f] <= IDW.bound_u(o, np.float64)[f]).all(), f"{name}, max_distance {bound}: beyond the tolerance of tests/idw.py"
            ms = series(fn)
            walked, within = pairs_walked(Engine.idw_plan(x, y, z.shape, lon, lat, True, 2, 6371000.0, bound))
            row = {"workload": name, "sources": int(x.size), "grid": f"{lat.size}x{lon.size}", "max_distance_km": None if bound is None else bound / 1e3,
                   "call_ms": ms, "kernels": kernels, "pairs_walked": walked, "pairs_within": within,
                   "gpairs_within_per_s": round(within / (ms["median"] * 1e-3) / 1e9, 2), "reps": a.reps,
                   "device": torch.cuda.get_device_name(0)}
            say(json.dumps(row))
            rows.append(row)
    say("| workload | sources -> grid | max_distance | kernels | pairs walked | pairs within | call ms (median / min) | 1e9 weighted pairs / s |")
    say("|---|---|---|---|---|---|---|---|")
    for r in rows:
        say(f"| {r['workload']} | {r['sources']} -> {r['grid']} | {r['max_distance_km'] or 'none'} km | {r['kernels']} | {r['pairs_walked']:.3e} | "
            f"{r['pairs_within']:.3e} | {r['call_ms']['median']} / {r['call_ms']['min']} | {r['gpairs_within_per_s']} |")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
