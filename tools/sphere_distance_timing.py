"""Time Engine.sphere_distance on the thinned Hessian ridge mask of a synthetic FTLE field, beside the index-metric transform.

    python tools/sphere_distance_timing.py [--warmup 3] [--reps 11] [--out profiles/sphere_distance/timing.txt] [--quick] [--once]

The field: lagrangiancoherence_amd.flows.era5_like on its 720 x 1440 grid (latitudes -89.875 .. 89.875, longitudes from -180),
97 levels of 900 s, advected backwards from its own grid (float32, order 1, SETTLS order 4, cyclic) by Engine.lcs; FTLE =
log(sigma) / 2; the mask is tools.find_ridges_spherical_hessian(sigma=1.2) thinned by tools.skeletonize_ridges -- the driver's
chain up to the distance transform.  One plane, float64, on the device already; the result stays there.

Three bounds: none, 330 km (what the driver's `dist < 12` stands for at 0.25 degrees) and 1500 km.  A call is timed with a pair
of device events on the current stream, after `--warmup` calls: the median (and the smallest) of `--reps`.  For scale,
Engine.distance_transform (the index metric, cyclic) on the same mask.  `pairs`: the (query pixel, candidate) pairs the search
kernel evaluates, counted on the host from the mask by the kernel's own rule (256 consecutive pixels share the union of their
rows' bands); `GFLOP/s of the call`: eight float64 operations per pair over the WHOLE call's time, so a lower bound of the search
kernel's own rate -- per-kernel times come from a kernel trace of `--once` (one call per bound and nothing else timed).
Before anything is reported, 1000 seeded pixels of each result are compared with the minimum over all ridge pixels, bit for bit.
Prints one JSON line per bound and a table; `--out` also writes both there.  Needs a GPU (there is no other path).
`--quick`: 180 x 360, 25 levels, to rehearse the script."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RADIUS = 6371000.0
BOUNDS = (None, 330e3, 1500e3)
THREADS = 256            # csrc/sphere_distance.hip: SD_THREADS
BAND_MARGIN = 1e-12      # csrc/sphere_distance.hip: SD_BAND_MARGIN
FP64_VECTOR_PEAK = 78.6e12   # MI355X, vector float64, FLOP/s (AMD's specification: an fma counts two)


def thinned_mask(eng, ny, nx, nt):
    from lagrangiancoherence_amd import flows
    from lagrangiancoherence_amd.tools import find_ridges_spherical_hessian, skeletonize_ridges
    from tests.labelled import DataArray
    u, v, lat, lon = flows.era5_like_on_device(eng.torch, eng.device, nt=nt, ny=ny, nx=nx)
    f = eng.prepare_field(u, v, lat, lon, 1)
    r = eng.lcs(f, lat, lon, -900.0, SETTLS_order=4, interp_order=1, cyclic_xboundary=True)
    ftle = np.log(r["sigma"].cpu().numpy().astype(np.float64)) / 2
    lat, lon = lat.astype(np.float64), lon.astype(np.float64)
    coords = {"latitude": lat, "longitude": lon}
    ridges, _ = find_ridges_spherical_hessian(DataArray(ftle, ("latitude", "longitude"), coords), sigma=1.2)
    thin = skeletonize_ridges(ridges, cyclic=True)
    return np.ascontiguousarray(thin.values, dtype=np.float64), lat, lon


def pairs_evaluated(mask, lat, lon, chord2):
    """What sd_search_kernel walks: per workgroup of 256 consecutive pixels, its pixels times the candidates of its band."""
    ny, nx = mask.shape
    row_start = np.concatenate([[0], np.cumsum(((mask != 0) & ~np.isnan(mask)).sum(axis=1))])
    lo, hi = np.zeros(ny, dtype=np.int64), np.full(ny, ny - 1, dtype=np.int64)
    if chord2 > 0:
        cl, sl = np.cos(lat * np.pi / 180), np.sin(lat * np.pi / 180)
        dc, ds = cl[:, None] - cl[None, :], sl[:, None] - sl[None, :]
        near = dc * dc + ds * ds <= chord2 + BAND_MARGIN
        lo, hi = near.argmax(axis=1), ny - 1 - near[:, ::-1].argmax(axis=1)
    p0 = np.arange(0, ny * nx, THREADS)
    p1 = np.minimum(p0 + THREADS, ny * nx) - 1
    pairs = 0
    for a, b in zip(p0, p1):
        r0, r1 = a // nx, b // nx
        pairs += int(b - a + 1) * int(row_start[hi[r0:r1 + 1].max() + 1] - row_start[lo[r0:r1 + 1].min()])
    return pairs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    import torch
    from lagrangiancoherence_amd.dropin import get_engine
    from lagrangiancoherence_amd.engine import Engine
    from tests import sphere_distance as SD
    eng = get_engine()
    ny, nx, nt = (180, 360, 25) if a.quick else (720, 1440, 97)
    mask_h, lat, lon = thinned_mask(eng, ny, nx, nt)
    mask = eng.to_device(mask_h, np.float64)
    count = int(np.count_nonzero(mask_h))
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
    X, Y, Z = SD.unit_vectors(lat, lon)
    idx = np.flatnonzero(mask_h)
    sample = np.random.default_rng(20261020).choice(mask_h.size, 1000, replace=False)
    costs = SD.cost_of((X[sample, None], Y[sample, None], Z[sample, None]), (X[idx][None, :], Y[idx][None, :], Z[idx][None, :]))
    want_c, want_n = costs.min(axis=1), idx[np.argmin(costs, axis=1)]
    rows = []
    for bound in BOUNDS:
        chord2 = Engine.sphere_tables(lat, lon, RADIUS, bound)[5]
        fn = lambda: eng.sphere_distance(mask, lat, lon, max_distance=bound, return_nearest=True, return_cost=True)
        _, (dist, nearest, cost) = timed(fn)
        got_c, got_n = cost.cpu().numpy().ravel()[sample], nearest.cpu().numpy().ravel()[sample]
        within = want_c <= chord2 if chord2 > 0 else np.ones_like(want_c, dtype=bool)
        assert np.array_equal(got_c, np.where(within, want_c, np.inf)) and np.array_equal(got_n, np.where(within, want_n, -1)), \
            f"max_distance {bound}: the device result differs from the minimum over all ridge pixels"
        if a.once:
            continue
        ms = series(lambda: eng.sphere_distance(mask, lat, lon, max_distance=bound))
        pairs = pairs_evaluated(mask_h, lat, lon, chord2)
        rate = 8 * pairs / (ms["median"] * 1e-3)
        row = {"shape": f"{ny}x{nx}", "ridge_pixels": count, "max_distance_km": None if bound is None else bound / 1e3,
               "within": round(float(np.isfinite(dist.cpu().numpy()).mean()), 4), "call_ms": ms, "pairs": pairs,
               "gflops_of_the_call": round(rate / 1e9, 1), "share_of_fp64_vector_peak": round(rate / FP64_VECTOR_PEAK, 4),
               "reps": a.reps, "device": torch.cuda.get_device_name(0)}
        say(json.dumps(row))
        rows.append(row)
    if not a.once:
        index_ms = series(lambda: eng.distance_transform(mask, cyclic=True))
        say(json.dumps({"shape": f"{ny}x{nx}", "index_metric_distance_transform_ms": index_ms}))
        say("| max_distance | points within | pairs | call ms (median / min) | GFLOP/s of the call | share of the float64 vector peak |")
        say("|---|---|---|---|---|---|")
        for r in rows:
            say(f"| {r['max_distance_km'] or 'none'} km | {r['within']} | {r['pairs']:.3e} | {r['call_ms']['median']} / {r['call_ms']['min']} | "
                f"{r['gflops_of_the_call']} | {r['share_of_fp64_vector_peak']} |")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
