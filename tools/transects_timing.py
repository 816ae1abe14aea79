"""Time Engine.ridge_transects on the ridges of a synthetic FTLE field, beside the numpy restatement on one core of this host.

    python tools/transects_timing.py [--warmup 5] [--reps 21] [--out profiles/transects/timing.txt] [--quick]

The field: lagrangiancoherence_amd.flows.era5_like on the driver's 221 x 233 grid, 25 levels of 900 s, advected backwards from
its own grid (float32, order 1, SETTLS order 4, cyclic) by Engine.lcs; FTLE = log(sigma) / 2; the mask is what
tools.find_ridges_spherical_hessian(sigma=1.2) and tools.skeletonize_ridges make of it.  Two shapes: that one plane, and 30
planes in one call (the plane rolled along longitude by 7 columns per member).  Three float32 fields (the FTLE and the first
level of u and v), half_width 500 km, spacing 25 km (41 offsets), smooth 3, orient 'north', bilinear, cyclic.

A call is timed with the host's clock between two device synchronisations, the trace (Engine.trace_lines) and the fields lying
on the device already and the result staying there; the trace's own time is given beside it.  `--warmup` calls first, then the
median (and the smallest) of `--reps`.  The numpy restatement (tests/transects.py: oracle and composite) is timed once on the
single plane, after its values have been compared with the device's.  Prints one JSON line per shape; `--out` also writes them
there.  Needs a GPU (there is no other path).  `--quick`: 10 levels and 3 planes, to rehearse the script."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def thin_mask(eng, ny, nx, nt):
    from lagrangiancoherence_amd import flows
    from lagrangiancoherence_amd.tools import find_ridges_spherical_hessian, skeletonize_ridges
    from tests.labelled import DataArray
    u, v, lat, lon = flows.era5_like_on_device(eng.torch, eng.device, nt=nt, ny=ny, nx=nx)
    f = eng.prepare_field(u, v, lat, lon, 1)
    r = eng.lcs(f, lat, lon, -900.0, SETTLS_order=4, interp_order=1, cyclic_xboundary=True)
    ftle = np.log(r["sigma"].cpu().numpy().astype(np.float64)) / 2
    coords = {"latitude": lat.astype(np.float64), "longitude": lon.astype(np.float64)}
    ridges, _ = find_ridges_spherical_hessian(DataArray(ftle, ("latitude", "longitude"), coords), sigma=1.2)
    thin = skeletonize_ridges(ridges, cyclic=True)
    fields = np.stack([ftle, u[0].cpu().numpy(), v[0].cpu().numpy()]).astype(np.float32)
    return np.ascontiguousarray(thin.values, dtype=np.float64), fields, coords["latitude"], coords["longitude"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    import torch
    from lagrangiancoherence_amd.dropin import get_engine
    from tests import lines as L
    from tests import transects as T
    eng = get_engine()
    ny, nx, nt, members = (221, 233, 10, 3) if a.quick else (221, 233, 25, 30)
    plane, fields, lat, lon = thin_mask(eng, ny, nx, nt)
    opts = dict(half_width=500e3, spacing=25e3, smooth=3, orient="north", method="linear", cyclic=True)
    out = []

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r
    for n in (1, members):
        mask_h = plane if n == 1 else np.stack([np.roll(plane, 7 * i, axis=1) for i in range(n)])
        fields_h = fields if n == 1 else np.stack([np.stack([np.roll(f, 7 * i, axis=1) for i in range(n)]) for f in fields])
        mask, dev_fields = eng.to_device(mask_h, np.float64), eng.to_device(fields_h, np.float32)
        trace_ms = [timed(lambda: eng.trace_lines(mask, True, "sphere", lat, lon))[0] for _ in range(a.warmup + 5)][a.warmup:]
        trace = eng.trace_lines(mask, True, "sphere", lat, lon)

        def call():
            return eng.ridge_transects(trace, dev_fields, lat, lon, **opts)
        for _ in range(a.warmup):
            timed(call)
        ms = [timed(call)[0] for _ in range(a.reps)]
        got = {k: v.cpu().numpy() for k, v in call().items()}
        row = {"shape": f"{n}x{ny}x{nx}", "ridge_pixels": int(trace["pixel"].numel()), "lines": int(trace["count"].numel()),
               "offsets": int(got["offset"].size), "fields": int(fields.shape[0]), "kernels": eng.last_transects_kernel,
               "transects_ms": {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4)}, "reps": len(ms),
               "trace_lines_ms": round(statistics.median(trace_ms), 4), "device": torch.cuda.get_device_name(0)}
        if n == 1:
            t0 = time.perf_counter()
            want_trace = L.trace_planes(mask_h[None], True, metric="sphere", lat=lat, lon=lon)
            walk_ms = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            o = T.oracle(want_trace, fields_h[:, None], lat, lon, opts["half_width"], opts["spacing"], 3, "north", "linear", True)
            means = [T.composite(v, want_trace["offset"], want_trace["count"]) for v in o["values"]]
            row["numpy_one_plane_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            row["numpy_pixel_walk_ms"] = round(walk_ms, 1)
            assert np.array_equal(want_trace["pixel"], trace["pixel"].cpu().numpy())
            sep = T.separation(o["latitude"], o["longitude"], got["latitude"], got["longitude"])
            assert np.nanmax(sep) <= T.POSITION_BOUND, "the device's positions differ from the restatement's"
            same = np.isclose(got["values"], o["values"], rtol=1e-5, atol=1e-6, equal_nan=True)
            row["values_equal_to_float32_rounding"] = round(float(same.mean()), 6)      # the rest: samples whose cell is a matter of the last bit
            assert same.mean() > 0.999 and np.array_equal(got["line_count"].shape, np.stack([m[1] for m in means]).shape)
        print(json.dumps(row), flush=True)
        out.append(json.dumps(row))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
