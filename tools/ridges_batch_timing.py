#!/usr/bin/env python3
"""Time the ridge extraction of a whole FTLE series in its two forms, at the reference driver's shape
(LCS/area_of_influence.py:168-211: 29 windows of 541 x 781, sigma = 1.2, the six-tuple of return_eigvectors=True), device
tensors in and device tensors out:

  batched   one Engine.ridges_batch call on the stack, then the angle and the masking of the vectors over the whole batch
  loop      the 2-D route of tools.find_ridges_spherical_hessian (its device side, unchanged) plane after plane

Both run in one process after a warm-up, alternating, each timed with a host clock around `--inner` repetitions that end in a
device synchronise; the median over `--reps` windows and their extremes are reported, with the kernel launches one repetition
of each form makes (counted by torch's profiler; "not measured" where it cannot be) and whether the two forms returned the
same bits.  Writes the report to stdout and, with --out, to a file.

    python tools/ridges_batch_timing.py --out profiles/ridges_batch/timing.txt
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def series(n, ny, nx, seed=3):
    """A seeded stand-in for an FTLE record: meandering ridges over smooth noise, a different phase per plane."""
    rng = np.random.default_rng(seed)
    lat, lon = np.linspace(-67.5, 67.5, ny), -97.5 + 0.25 * np.arange(nx)
    LON, LAT = np.meshgrid(lon, lat)
    planes = []
    for m in range(n):
        ridge = np.exp(-((LAT - 10 * np.sin(np.deg2rad(3 * LON + 11 * m))) / 6.0) ** 2) + np.exp(-((LAT + 30 - 0.2 * LON - m) / 4.0) ** 2)
        planes.append(2.0 * ridge + 0.1 * rng.standard_normal((ny, nx)))
    return np.stack(planes), lat, lon


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--planes", type=int, default=29)
    ap.add_argument("--ny", type=int, default=541)
    ap.add_argument("--nx", type=int, default=781)
    ap.add_argument("--sigma", type=float, default=1.2)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--isglobal", type=int, default=0, help="the driver's domain is regional")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from lagrangiancoherence_amd import tools as T
    from lagrangiancoherence_amd.dropin import get_engine
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this tool measures on the device and has no other path")
    eng = get_engine()
    v, lat, lon = series(a.planes, a.ny, a.nx)
    stack = eng.to_device(v, np.float64)
    tol, g = 0.0005e-3, bool(a.isglobal)
    want = ("mask", "eigmin", "dt", "eigvec", "grad")

    def batched():
        r = eng.ridges_batch(stack, lat, lon, sigma=a.sigma, tolerance=tol, isglobal=g, want=want)
        angle, masked = T._angle_and_masked(torch, r["eigvec"], r["eigmin"])
        return r["mask"], r["eigmin"], r["dt"], masked, r["grad"], angle

    def loop():
        outs = []
        for m in range(a.planes):
            mask, eigmin, dt, vec, ddadx, ddady = T._hessian_ridges_plane(eng, stack[m], lat, lon, a.sigma, tol, g)
            angle, masked = T._angle_and_masked(torch, vec, eigmin)
            outs.append((mask, eigmin, dt, masked, torch.stack([ddadx, ddady]), angle))
        return outs

    def launches(fn):
        try:
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                fn()
                torch.cuda.synchronize()
            n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "emcpy" not in e.name and "emset" not in e.name)
            return str(n) if n else "not measured"
        except Exception as exc:      # the profiler is an optional part of torch builds
            return f"not measured ({type(exc).__name__})"

    def window(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.inner):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.inner * 1e3

    for _ in range(a.warmup):
        b, l = batched(), loop()
    torch.cuda.synchronize()
    same = all(torch.equal(torch.nan_to_num(b[k][m], nan=-7.0), torch.nan_to_num(l[m][k], nan=-7.0)) and
               torch.equal(torch.isnan(b[k][m]), torch.isnan(l[m][k])) for m in range(a.planes) for k in range(6))
    kernel = eng.last_ridges_kernel()
    n_ridge = int(b[0].sum())
    del b, l
    times = {"batched": [], "loop": []}
    for _ in range(a.reps):                   # alternating: what else the machine does falls on both forms alike
        times["batched"].append(window(batched))
        times["loop"].append(window(loop))
    counts = {"batched": launches(batched), "loop": launches(loop)}

    lines = [f"ridges of a series: {a.planes} planes of {a.ny} x {a.nx}, sigma {a.sigma}, six outputs, isglobal {g}, device tensors in and out",
             f"device: {torch.cuda.get_device_name(0)}; {a.warmup} warm-up calls of each form, then {a.reps} alternating windows of {a.inner} calls",
             f"batched kernels: {kernel}; ridge points {n_ridge} of {a.planes * a.ny * a.nx}; both forms return the same bits: {same}"]
    for k in ("batched", "loop"):
        t = times[k]
        lines.append(f"{k:8s} median {statistics.median(t):9.3f} ms per call   min {min(t):9.3f}   max {max(t):9.3f}   "
                     f"kernel launches per call: {counts[k]}")
    mb, ml = statistics.median(times["batched"]), statistics.median(times["loop"])
    spread = max(max(t) - min(t) for t in times.values())
    lines.append(f"loop / batched = {ml / mb:.2f}; largest min-to-max spread of a form {spread:.3f} ms")
    lines.append("windows, ms per call (batched, loop): " + "  ".join(f"({x:.3f}, {y:.3f})" for x, y in zip(times["batched"], times["loop"])))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
