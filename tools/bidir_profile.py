"""Time the attracting and the repelling field of one record two ways under one build: two single-direction calls and one
LCS.bidirectional / Engine.lcs_bidirectional.

    python tools/bidir_profile.py [--reps N] [--out FILE]

  * (a) the reference example's shape (examples/ideal_vortex.py:280-288): flows.config1() (89 x 180, 8 levels, float64),
    isglobal=True (0.5 degree regrid and T20), SETTLS order 4, interp order 3.  Two ``LCS(timestep=+-6 h)(ds, ...)`` against
    one ``LCS(...).bidirectional(ds, ...)``.
  * (b) the driver shape of tools/series_profile.py (541 x 781 regional box, 36 levels, window 8, stride 1, resample '3h',
    SETTLS order 4, interp order 3, non-cyclic): two ``series`` calls (-6 h and +6 h) against one
    ``bidirectional(window=8)``.
  * (c) C3 seed density (720 x 1440 seeds on the era5_like field's grid), 33 levels, window 9, stride 4 (7 windows),
    float32, order 1, SETTLS order 4, cyclic: two Engine.lcs_series against one Engine.lcs_bidirectional on the same packed
    field (the pack is common and not timed): the fused launches alone.

Both forms from the labelled record on the host to sigma on the host in (a) and (b).  Host wall clock around work that ends
in a device synchronise; median of N after one warm-up; the outputs are compared bit for bit.  Prints one JSON line and
writes it to FILE."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def _tuple(r):
    return r if isinstance(r, tuple) else (r,)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import pandas as pd
    import torch
    from lagrangiancoherence_amd import build, dropin, flows
    from LagrangianCoherence.LCS.LCS import LCS
    from series_profile import _driver_case
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

    def compare(two, one):
        """(all bit-identical, max relative sigma difference) of [backward, forward] outputs against bidirectional's."""
        same, rel = True, 0.0
        for a, b in zip(two, one):
            for x, y in zip(_tuple(a), _tuple(b)):
                same &= bool(np.array_equal(x.values, y.values))
            s0, s1 = _tuple(a)[0].values, _tuple(b)[0].values
            rel = max(rel, float(np.max(np.abs(s1 - s0) / np.maximum(np.abs(s0), 1e-30))))
        return same, rel

    out = {"build": build.csrc_hash(), "device": torch.cuda.get_device_name(0)}
    # ---------------------------------------------------------------- (a) the example's shape
    u, v, lat, lon = flows.config1()
    times = pd.date_range("2000-01-01", periods=u.shape[0], freq="6h").values
    coords = {"latitude": lat, "longitude": lon, "time": times}
    ds = labelled.Dataset({"u": labelled.DataArray(u.transpose(1, 2, 0), ["latitude", "longitude", "time"], coords, name="u"),
                           "v": labelled.DataArray(v.transpose(1, 2, 0), ["latitude", "longitude", "time"], coords, name="v")})
    ctor = dict(timedim="time", SETTLS_order=4)
    call = dict(isglobal=True, verbose=False)
    t_two, a_all, two = timed(lambda: [LCS(timestep=sg * 6 * 3600, **ctor)(ds, **call) for sg in (-1, 1)], args.reps)
    k_two = eng.last_advect_kernel()
    t_one, o_all, one = timed(lambda: LCS(timestep=6 * 3600, **ctor).bidirectional(ds, **call), args.reps)
    same, rel = compare(two, one)
    out["example"] = {"shape": [89, 180], "levels": int(u.shape[0]), "isglobal": True, "K": 4, "order": 3, "dtype": "float64",
                      "two_calls_s": t_two, "bidirectional_s": t_one, "two_calls_all_s": a_all, "bidirectional_all_s": o_all,
                      "speedup": t_two / t_one, "bit_identical": same, "sigma_max_rel_diff": rel,
                      "advect_kernel_two_calls": k_two, "advect_kernel_bidirectional": eng.last_advect_kernel(),
                      "advect_launches_bidirectional": eng.last_advect_launches()}
    # ---------------------------------------------------------------- (b) the driver shape
    ds, nt = _driver_case()
    ctor = dict(timedim="time", SETTLS_order=4)
    call = dict(s=1e5, resample="3h", verbose=False, traj_interp_order=3)
    t_two, a_all, two = timed(lambda: [LCS(timestep=sg * 6 * 3600, **ctor).series(ds, window=8, stride=1, **call)
                                       for sg in (-1, 1)], args.reps)
    k_two = eng.last_advect_kernel()
    t_one, o_all, one = timed(lambda: LCS(timestep=6 * 3600, **ctor).bidirectional(ds, window=8, stride=1, **call), args.reps)
    same, rel = compare(two, one)
    out["driver"] = {"shape": [541, 781], "levels": nt, "window": 8, "stride": 1, "windows": nt - 8 + 1, "resample": "3h", "K": 4,
                     "order": 3, "dtype": "float64 (float32 record, resampled)", "cyclic": False,
                     "two_series_s": t_two, "bidirectional_s": t_one, "two_series_all_s": a_all, "bidirectional_all_s": o_all,
                     "speedup": t_two / t_one, "bit_identical": same, "sigma_max_rel_diff": rel,
                     "advect_kernel_two_series": k_two, "advect_kernel_bidirectional": eng.last_advect_kernel()}
    del ds
    # ---------------------------------------------------------------- (c) C3 seed density, the fused launches
    u, v, lat, lon = flows.era5_like_on_device(torch, eng.device, nt=33)
    f = eng.prepare_field(u, v, lat, lon, 1)
    nsteps, n_win, stride, K = 8, 7, 4, 4
    kw = dict(SETTLS_order=K, interp_order=1, cyclic_xboundary=True)
    t_two, a_all, two = timed(lambda: [eng.lcs_series(f, lat, lon, sg * 900.0, nsteps, n_win, 0, stride, **kw) for sg in (-1, 1)],
                              args.reps)
    k_two = eng.last_advect_kernel()
    t_one, o_all, one = timed(lambda: eng.lcs_bidirectional(f, lat, lon, 900.0, nsteps, n_win, 0, stride, **kw), args.reps)
    same = all(torch.equal(one[k][d], two[d][k]) for d in (0, 1) for k in ("sigma", "x_dep", "y_dep"))
    out["cyclic_c3"] = {"shape": [int(lat.size), int(lon.size)], "levels": 33, "windows": n_win, "steps_per_window": nsteps,
                        "stride": stride, "K": K, "order": 1, "dtype": "float32", "two_series_s": t_two, "bidirectional_s": t_one,
                        "two_series_all_s": a_all, "bidirectional_all_s": o_all, "speedup": t_two / t_one, "bit_identical": bool(same),
                        "advect_kernel_two_series": k_two, "advect_kernel_bidirectional": eng.last_advect_kernel(),
                        "advect_launches_bidirectional": eng.last_advect_launches()}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
