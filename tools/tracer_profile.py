"""Timings of the tracer sampler (lc_tracer_sample) and of whole tracer calls.

    python tools/tracer_profile.py [--reps N] [--out FILE]

  * C3 size (4096^2 seeds, era5_like 0.25 degree flow, 97 levels, float32, order 1, SETTLS_order 4, timestep -900 s):
    the plain advect, the advect with trajectories, the sampler alone on those trajectories (mean only: the position
    stream rate = levels * seeds * 2 * 4 bytes / kernel time), and the mean-only Engine.advect_tracer call (scratch ring);
  * the reference example (89 x 180, 7 steps, float64, order 3, SETTLS_order 4): the drop-in's
    parcel_propagation(..., C=, return_traj=True) against what a user does on the host today -- the oracle's trajectories
    and one map_coordinates call per level (and the sampling loop alone).

Event timings (median of N after one warm-up); prints one JSON line and writes it to FILE.  For kernel times run it
under ``rocprofv3 --kernel-trace --stats -- python tools/tracer_profile.py --reps 3``."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from lagrangiancoherence_amd import dropin, flows
    from lagrangiancoherence_amd.engine import Engine
    from oracle import lcs_oracle as O
    from tests import labelled

    eng = Engine(0)
    dev = eng.device

    def timed(fn):
        fn()
        ts = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        return float(np.median(ts))

    out = {}
    # ---- C3
    nt = 97
    u, v, lat, lon = flows.era5_like_on_device(torch, dev, nt=nt)
    slat, slon = flows.seed_grid(4096, 4096, lat, lon)
    n = slat.size * slon.size
    field = eng.prepare_field(u, v, lat, lon, 1)
    tr = eng.prepare_tracer(torch.hypot(u, v), None, lat, lon, 1, dtype=field.dtype)
    kw = dict(SETTLS_order=4, interp_order=1, cyclic_xboundary=True)
    out["c3_advect_ms"] = timed(lambda: eng.advect(field, slat, slon, -900.0, **kw))
    out["c3_advect_kernel"] = eng.last_advect_kernel()
    res = {}
    out["c3_advect_traj_ms"] = timed(lambda: res.update(r=eng.advect(field, slat, slon, -900.0, return_traj=True, **kw)))
    tx, ty = res["r"][2], res["r"][3]
    del res["r"]
    out["c3_sampler_mean_only_ms"] = timed(lambda: eng.sample_tracer(tr, tx, ty, 0, 1, values=False, mean_count=nt))
    out["c3_sampler_values_ms"] = timed(lambda: eng.sample_tracer(tr, tx, ty, 0, 1, values=True, mean_count=nt))
    out["tracer_kernel"] = eng.last_tracer_kernel()
    out["c3_position_stream_TBps"] = nt * n * 2 * 4 / (out["c3_sampler_mean_only_ms"] * 1e-3) / 1e12
    del tx, ty
    torch.cuda.empty_cache()
    out["c3_advect_tracer_mean_only_ms"] = timed(lambda: eng.advect_tracer(field, tr, slat, slon, -900.0, **kw))
    del field, tr, u, v
    torch.cuda.empty_cache()

    # ---- the reference example
    u, v, lat, lon = flows.config1()
    c = np.hypot(u, v) + 20.0 * np.cos(np.deg2rad(lat))[None, :, None]
    times = np.datetime64("2000-01-01T00") + np.arange(u.shape[0]) * np.timedelta64(6, "h")
    coords = {"latitude": lat, "longitude": lon, "time": times}
    U = labelled.DataArray(u.transpose(1, 2, 0), ["latitude", "longitude", "time"], coords, name="u")
    V = labelled.DataArray(v.transpose(1, 2, 0), ["latitude", "longitude", "time"], coords, name="v")
    Cl = labelled.DataArray(c, ["time", "latitude", "longitude"], coords, name="c")
    call = dict(timestep=-6 * 3600, SETTLS_order=4, interp_order=3, cyclic_xboundary=True, verbose=False, return_traj=True)

    def wall(fn, reps):
        fn()
        ts = []
        for _ in range(reps):
            t = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t) * 1e3)
        return float(np.median(ts))

    out["example_dropin_C_ms"] = wall(lambda: dropin.parcel_propagation(U, V, C=Cl, **call), args.reps)
    out["example_dropin_noC_ms"] = wall(lambda: dropin.parcel_propagation(U, V, **call), args.reps)
    txo, tyo = O.parcel_propagation(u, v, lat, lon, timestep=-6 * 3600, SETTLS_order=4, interp_order=3,
                                    cyclic_xboundary=True, return_traj=True)
    loop = lambda: [O.xr_map_coordinates(c[i], lat, lon, txo[i], tyo[i], order=3) for i in range(txo.shape[0])]
    out["example_host_sampling_loop_ms"] = wall(loop, 3)
    out["example_host_oracle_traj_plus_loop_ms"] = wall(
        lambda: (O.parcel_propagation(u, v, lat, lon, timestep=-6 * 3600, SETTLS_order=4, interp_order=3,
                                      cyclic_xboundary=True, return_traj=True), loop()), 1)
    out["host_threads"] = os.environ.get("OMP_NUM_THREADS")
    line = json.dumps({k: (round(x, 4) if isinstance(x, float) else x) for k, x in out.items()})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    eng.close()


if __name__ == "__main__":
    main()
