"""Time the distance transform on the device beside scipy.ndimage.distance_transform_edt on one core of this host.

    python tools/bench_distance.py [--warmup 3] [--reps 11] [--slow-reps 3] [--scipy-reps 3] [--quick]

Two shapes: one 4096 x 4096 plane, and a stack of 8 planes of 1024 x 1024 in one call (scipy: the 8 planes one after the other).
Three masks, float64: `random` of density 0.02 (seed 20261019); `one-pixel` (a single pixel in a corner: the longest outward
search there is, O(nx) steps per pixel); `ridges`, what tools.find_ridges_spherical_hessian makes of a smooth synthetic
field, the realistic case.  Each is timed with max_distance unset and with max_distance 12.

The device time is Engine.distance_transform on a mask that already lies on the device, result left on the device: device
events around the call on the current stream, after `--warmup` calls, one event pair per repetition, median (and the
smallest) over `--reps` (`--slow-reps` where one call takes longer than 0.2 s).  scipy is timed with a host clock on the same
arrays, `--scipy-reps` times, median.  Before anything is reported the device result is compared with scipy's, bit for bit
(with max_distance: where scipy's is <= 12, +inf elsewhere).  Prints one JSON line per (shape, mask, bound) and a table;
needs a GPU (there is no other path).  `--quick`: 512 x 512 and 2 x 256 x 256, to rehearse the script."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SEED = 20261019
BOUND = 12.0


def smooth_field(ny, nx):
    """Waves a few hundred grid points long and a slow modulation, on a 60S-60N global grid."""
    lat, lon = np.linspace(-60.0, 60.0, ny), np.linspace(-180.0, 180.0, nx, endpoint=False)
    y, x = np.deg2rad(lat)[:, None], np.deg2rad(lon)[None, :]
    f = (np.sin(9 * x + 3 * np.sin(4 * y)) * np.cos(7 * y) + 0.6 * np.cos(14 * x - 11 * y) + 0.3 * np.sin(23 * x + 17 * y)
         + 0.5 * np.sin(5 * y + 2 * np.cos(3 * x)))
    return f, lat, lon


def ridge_mask(ny, nx):
    from lagrangiancoherence_amd.tools import find_ridges_spherical_hessian
    from tests.labelled import DataArray
    f, lat, lon = smooth_field(ny, nx)
    ridges, _ = find_ridges_spherical_hessian(DataArray(f, ("latitude", "longitude"), {"latitude": lat, "longitude": lon}),
                                              sigma=1.2, tolerance_threshold=0.0005e-3)
    return np.ascontiguousarray(ridges.values, dtype=np.float64)


def masks(shape):
    n, ny, nx = shape
    rng = np.random.default_rng(SEED)
    one = np.zeros(shape)
    one[:, 0, 0] = 1
    return {"random-0.02": (rng.random(shape) < 0.02).astype(np.float64),
            "one-pixel": one,
            "ridges": np.stack([np.roll(ridge_mask(ny, nx), 37 * i, axis=1) for i in range(n)])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--slow-reps", type=int, default=3)
    ap.add_argument("--scipy-reps", type=int, default=3)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    import torch
    from scipy import ndimage
    from lagrangiancoherence_amd.engine import Engine
    eng = Engine(0)
    rows = []
    for shape in ([(1, 512, 512), (2, 256, 256)] if a.quick else [(1, 4096, 4096), (8, 1024, 1024)]):
        for name, mask_h in masks(shape).items():
            mask = eng.to_device(mask_h, np.float64)
            t = []
            for _ in range(a.scipy_reps):
                t0 = time.perf_counter()
                ref = np.stack([ndimage.distance_transform_edt(p == 0) for p in mask_h])
                t.append((time.perf_counter() - t0) * 1e3)
            scipy_ms = statistics.median(t)
            for bound in (None, BOUND):
                def call():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    out = eng.distance_transform(mask, max_distance=bound)
                    e1.record()
                    torch.cuda.synchronize()
                    return e0.elapsed_time(e1), out
                first, out = call()
                want = ref if bound is None else np.where(ref <= bound, ref, np.inf)
                assert np.array_equal(out.cpu().numpy(), want), f"{shape} {name} {bound}: the device result differs from scipy's"
                slow = first > 200.0
                for _ in range(0 if slow else a.warmup):
                    call()
                ms = [call()[0] for _ in range(a.slow_reps if slow else a.reps)]
                row = {"shape": "x".join(map(str, shape)), "mask": name, "density": round(float((mask_h != 0).mean()), 5),
                       "max_distance": bound, "device_ms": {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3)},
                       "reps": len(ms), "scipy_ms": round(scipy_ms, 1), "scipy_over_device": round(scipy_ms / statistics.median(ms), 1),
                       "device": torch.cuda.get_device_name(0)}
                print(json.dumps(row), flush=True)
                rows.append(row)
    print("| shape | mask (density) | max_distance | device ms (median / min) | scipy ms, one core | scipy / device |")
    print("|---|---|---|---|---|---|")
    for r in rows:
        print(f"| {r['shape']} | {r['mask']} ({r['density']}) | {r['max_distance'] or 'none'} | {r['device_ms']['median']} / {r['device_ms']['min']} | "
              f"{r['scipy_ms']} | {r['scipy_over_device']} |")


if __name__ == "__main__":
    main()
