"""Time a sliding-window FTLE series two ways under one build: the driver's per-window loop and LCS.series / Engine.lcs_series.

    python tools/series_profile.py [--reps N] [--out FILE] [--sigma-only]

  * driver-shaped (LCS/area_of_influence.py:168-181): a regional 0.25 degree box of 541 x 781, 36 six-hourly levels of a
    synthetic zonal jet strong enough to push parcels out of the box, window 8, stride 1 (29 windows), resample '3h', SETTLS
    order 4, interp order 3, a float32 record (float64 after the linear resampling, in both forms), timestep -6 h,
    non-cyclic (the reference's outer clamp).  Loop: ``LCS(...)(ds.isel(time=slice(w, w + 8)), ...)`` for every w; series:
    ``LCS(...).series(ds, window=8, stride=1, ...)``.  Both from the labelled record on the host to sigma on the host; the
    outputs are compared (both exceptions of INTEGRATION.md "Time series of FTLE" apply at this shape).
  * cyclic at C3 seed density (0.25 degree over the globe, 720 x 1440 = the era5_like field's own grid as seeds), 33
    levels, window 9, stride 4 (7 windows), float32, order 1, SETTLS order 4: Engine.lcs per window against one
    Engine.lcs_series on the same packed field (the pack is common to both and not timed).
  * ``--sigma-only``: the sigma stage alone at both shapes, lc_sigma per window against one lc_sigma_batch, for a
    ``rocprofv3 --kernel-trace --stats`` pass of its own.

Host wall clock around work that ends in a device synchronise; median of N after one warm-up; prints one JSON line and
writes it to FILE."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _driver_case():
    import pandas as pd
    from tests import labelled
    nt, ny, nx = 36, 541, 781
    lat = (-60.0 + 0.25 * np.arange(ny)).astype(np.float32)
    lon = (-150.0 + 0.25 * np.arange(nx)).astype(np.float32)
    t = np.arange(nt, dtype=np.float64)[:, None, None]
    yy = np.deg2rad(lat.astype(np.float64))[None, :, None]
    xx = np.deg2rad(lon.astype(np.float64))[None, None, :]
    # a westerly jet (35 m/s at its core, meandering with time) over a weaker background: parcels cross the box's edges
    core = np.deg2rad(20.0) + 0.15 * np.sin(0.35 * t + 2.0 * xx)
    u = 8.0 + 35.0 * np.exp(-((yy - core) / 0.2) ** 2) + 4.0 * np.cos(3.0 * xx - 0.5 * t) * np.cos(yy)
    v = 6.0 * np.sin(3.0 * xx - 0.5 * t) * np.cos(2.0 * yy) + 0.0 * t
    times = pd.date_range("2020-01-01", periods=nt, freq="6h").values
    coords = {"latitude": lat, "longitude": lon, "time": times}
    U = labelled.DataArray(u.astype(np.float32).transpose(1, 2, 0), ["latitude", "longitude", "time"], coords, name="u")
    V = labelled.DataArray(np.broadcast_to(v, u.shape).astype(np.float32).transpose(1, 2, 0), ["latitude", "longitude", "time"],
                           coords, name="v")
    return labelled.Dataset({"u": U, "v": V}), nt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sigma-only", action="store_true")
    args = ap.parse_args()
    import torch
    from lagrangiancoherence_amd import build, dropin, flows
    from LagrangianCoherence.LCS.LCS import LCS
    from tests import labelled

    eng = dropin.get_engine()
    sync = eng.synchronize

    def timed(fn, reps):
        fn()
        sync()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            r = fn()
            sync()
            ts.append(time.perf_counter() - t0)
        return float(np.median(ts)), ts, r

    out = {"build": build.csrc_hash(), "device": torch.cuda.get_device_name(0)}
    # ---------------------------------------------------------------- cyclic, C3 seed density
    u, v, lat, lon = flows.era5_like_on_device(torch, eng.device, nt=33)
    f = eng.prepare_field(u, v, lat, lon, 1)
    nsteps, n_win, stride, K, ts = 8, 7, 4, 4, -900.0
    kw = dict(SETTLS_order=K, interp_order=1, cyclic_xboundary=True)
    if args.sigma_only:
        res = eng.lcs_series(f, lat, lon, ts, nsteps, n_win, 0, stride, **kw)
        xs, ys = res["x_dep"], res["y_dep"]
        dlat, dlon = float(lat[1] - lat[0]), float(lon[1] - lon[0])
        for _ in range(args.reps):
            for m in range(n_win):
                eng.sigma(xs[m], ys[m], lat, dlat, dlon)
            eng.sigma_batch(xs, ys, lat, dlat, dlon)
        sync()
        out["cyclic_c3"] = {"sigma_kernels": [eng.last_sigma_kernel()]}
    else:
        t_loop, l_all, loop = timed(lambda: [eng.lcs(f, lat, lon, ts, t0=m * stride, nsteps=nsteps, **kw) for m in range(n_win)],
                                    args.reps)
        t_ser, s_all, ser = timed(lambda: eng.lcs_series(f, lat, lon, ts, nsteps, n_win, 0, stride, **kw), args.reps)
        same = all(torch.equal(ser[k][m], loop[m][k]) for m in range(n_win) for k in ("sigma", "x_dep", "y_dep"))
        out["cyclic_c3"] = {"shape": [int(lat.size), int(lon.size)], "levels": 33, "windows": n_win, "steps_per_window": nsteps,
                            "stride": stride, "K": K, "order": 1, "dtype": "float32", "loop_s": t_loop, "series_s": t_ser,
                            "loop_all_s": l_all, "series_all_s": s_all, "speedup": t_loop / t_ser, "bit_identical": bool(same),
                            "advect_kernel": eng.last_advect_kernel()}
    del f, u, v
    torch.cuda.empty_cache()
    # ---------------------------------------------------------------- driver-shaped, regional, non-cyclic
    ds, nt = _driver_case()
    window, stride = 8, 1
    ctor = dict(timestep=-6 * 3600, timedim="time", SETTLS_order=4)
    call = dict(s=1e5, resample="3h", verbose=False, traj_interp_order=3)

    def loop():
        return [LCS(**ctor)(labelled.Dataset({k: ds[k].isel(time=slice(w, w + window)) for k in ("u", "v")}), **call).values[0]
                for w in range(nt - window + 1)]

    def series():
        return LCS(**ctor).series(ds, window=window, stride=stride, **call).values

    if args.sigma_only:
        # the sigma stage alone at the driver's shape: positions of one series, lc_sigma per window vs lc_sigma_batch
        d = out.setdefault("driver", {})
        lat = ds.u.coords["latitude"]
        lon = ds.u.coords["longitude"]
        n = nt - window + 1
        rng = np.random.default_rng(0)
        xs = torch.as_tensor((lon[None, None, :] + 0.1 * rng.standard_normal((n, lat.size, lon.size))).astype(np.float32), device=eng.device)
        ys = torch.as_tensor((lat[None, :, None] + 0.1 * rng.standard_normal((n, lat.size, lon.size))).astype(np.float32), device=eng.device)
        for _ in range(args.reps):
            for m in range(n):
                eng.sigma(xs[m], ys[m], lat, 0.25, 0.25)
            eng.sigma_batch(xs, ys, lat, 0.25, 0.25)
        sync()
        d["sigma_kernels"] = [eng.last_sigma_kernel()]
    else:
        t_loop, l_all, a = timed(loop, args.reps)
        kern_loop = eng.last_advect_kernel()
        t_ser, s_all, b = timed(series, args.reps)
        kern_ser = eng.last_advect_kernel()
        out["driver"] = {"shape": [541, 781], "levels": nt, "window": window, "stride": stride, "windows": nt - window + 1,
                         "resample": "3h", "K": 4, "order": 3, "dtype": "float64 (float32 record, resampled)", "timestep_s": -21600, "cyclic": False,
                         "loop_s": t_loop, "series_s": t_ser, "loop_all_s": l_all, "series_all_s": s_all, "speedup": t_loop / t_ser,
                         "bit_identical": bool(all(np.array_equal(a[w], b[w]) for w in range(len(a)))),
                         "windows_bit_identical": int(sum(np.array_equal(a[w], b[w]) for w in range(len(a)))),
                         "sigma_max_rel_diff": float(max(np.max(np.abs(b[w] - a[w]) / np.maximum(np.abs(a[w]), 1e-30)) for w in range(len(a)))),
                         "sigma_frac_rel_diff_below_1e-3": float(np.mean([np.mean(np.abs(b[w] - a[w]) <= 1e-3 * np.abs(a[w]))
                                                                          for w in range(len(a))])),
                         "advect_kernel_loop_last": kern_loop, "advect_kernel_series": kern_ser}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
