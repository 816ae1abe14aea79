"""Time the footprint fold on the device: both kernel forms beside the path-length fold that reads the same planes.

    python tools/bench_footprint.py [--warmup 3] [--reps 9] [--seeds 4096] [--nt 97] [--chunk 16] [--quick]

The headline shape: `--seeds`^2 float32 seeds on the 720 x 1440 synthetic wind of bench.py (flows.era5_like), `--nt` - 1 steps of
-900 s, SETTLS order 4, interpolation order 1, blocks of `--chunk` steps; the target grid is the wind's grid, cyclic.

  fold      Engine.footprint_update on the first block's trajectories (level0 = 0, not final), for the direct and the tiled
            form, with hits alone, hits + mass (random weights with a quarter of zeros), and hits + mass + the value planes
            (c = the zonal wind sampled along the block).  Beside it Engine.lavd_update(c=None) on the same block: the
            path-length fold reads the same two position planes at the copy peak.  `left_window`: the share of the valid
            entries' half-weights that left the tiled form's LDS window (the census form's stats[2] over sum(hits)).
  pile-up   the same block with every position clamped into a regional box, target grid that box (not cyclic): what the
            regional clamp does to a run -- parcels pile into the edge cells, the worst contention there is.
  window    Engine.footprint over the whole window, without and with weights and tracer, under `auto` and under each forced
            form, beside Engine.lavd(tracer=None).

Device events around each call on the current stream, after `--warmup` calls; the median, the smallest and the largest of `--reps`
are printed.  Before anything is timed the two forms' integers are compared (equal, or the script stops).  One JSON line per
row, then a table; needs a GPU.  `--quick`: 512^2 seeds, 9 levels, to rehearse the script."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--seeds", type=int, default=4096)
    ap.add_argument("--nt", type=int, default=97)
    ap.add_argument("--chunk", type=int, default=16)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--skip-window", action="store_true")
    ap.add_argument("--skip-pile-up", action="store_true")
    a = ap.parse_args()
    if a.quick:
        a.seeds, a.nt, a.chunk = 512, 9, 4
    import torch
    from lagrangiancoherence_amd import flows
    from lagrangiancoherence_amd.engine import Engine
    eng = Engine(0)
    dt, kw = -900.0, dict(SETTLS_order=4, interp_order=1, cyclic_xboundary=True)
    u, v, lat, lon = flows.era5_like(nt=a.nt)
    slat, slon = flows.seed_grid(a.seeds, a.seeds, lat, lon)
    field = eng.prepare_field(u, v, lat, lon, 1)
    tracer = eng.prepare_tracer(u, None, lat, lon, 1, dtype=field.dtype)
    glat, glon = lat.astype(np.float64), lon.astype(np.float64)
    rng = np.random.default_rng(20261021)
    w = rng.random((a.seeds, a.seeds))
    w[rng.random(w.shape) < 0.25] = 0.0
    q, _ = eng.footprint_weights(w, w.shape)
    qd = eng.to_device(q, np.int32)
    c_scale = float(1 << 30) / float(np.abs(u).max())
    rows = []

    def timed(call):
        for _ in range(a.warmup):
            call()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}

    def emit(row):
        row["device"] = torch.cuda.get_device_name(0)
        print(json.dumps(row), flush=True)
        rows.append(row)

    # ---- the fold on one block
    _, _, tx, ty = eng.advect(field, slat, slon, dt, t0=0, nsteps=a.chunk, return_traj=True, **kw)
    c = eng.sample_tracer(tracer, tx, ty, level0=0, interp_order=1)[0][0]
    samples = int(tx.numel())
    yard = timed(lambda: eng.lavd_update(tx, ty, None, dt, 0))
    emit({"case": "fold", "what": "lavd_update(c=None)", "kernel": eng.last_lavd_kernel(), "samples": samples, "ms": yard,
          "read_TBps": round(2 * 4 * samples / yard["median"] / 1e9, 2)})

    def fold_cases(x, y, grid_lat, grid_lon, cyclic, case):
        variants = [("hits", dict(want=("hits",))), ("hits+mass", dict(q=qd)), ("hits+mass+c", dict(q=qd, c=c, c_scale=c_scale))]
        for name, extra in variants:
            got = {}
            for form in ("direct", "tiled"):
                eng.set_footprint_form(form)
                call = lambda: eng.footprint_update(x, y, grid_lat, grid_lon, 0, False, cyclic=cyclic, **extra)
                acc = call()
                got[form] = {k: t.clone() for k, t in acc.items() if t is not None}
                ms = timed(call)
                emit({"case": case, "what": name, "form": form, "kernel": eng.last_footprint_kernel(), "samples": samples, "ms": ms,
                      "over_lavd_update": round(ms["median"] / yard["median"], 2)})
            assert all(torch.equal(got["direct"][k], got["tiled"][k]) for k in got["direct"]), f"{case} {name}: the two forms differ"
            eng.set_footprint_form("census")
            acc = eng.footprint_update(x, y, grid_lat, grid_lon, 0, False, cyclic=cyclic, **extra)
            hits = int(got["direct"]["hits"].sum()) if "hits" in got["direct"] else 0
            stats = acc["stats"].tolist()
            emit({"case": case, "what": name, "form": "census", "left_window": round(stats[2] / max(hits, 1), 6),
                  "outside_grid": round(stats[0] / max(hits + stats[0], 1), 6)})
        eng.set_footprint_form("auto")

    fold_cases(tx, ty, glat, glon, True, "fold")
    # ---- the pile-up: positions clamped into a regional box, as the regional clamp leaves them
    if not a.skip_pile_up:
        box_lat, box_lon = glat[(glat > -30) & (glat < 30)], glon[(glon > -60) & (glon < 60)]
        px = tx.clamp(float(box_lon[0]), float(box_lon[-1]))
        py = ty.clamp(float(box_lat[0]), float(box_lat[-1]))
        fold_cases(px, py, box_lat, box_lon, False, "pile-up")
        del px, py
    del tx, ty, c
    torch.cuda.empty_cache()

    # ---- the whole window
    if not a.skip_window:
        nsteps = a.nt - 1
        ms = timed(lambda: eng.lavd(field, None, slat, slon, dt, nsteps=nsteps, level_chunk=a.chunk, **kw))
        lavd_ms = ms["median"]
        emit({"case": "window", "what": "Engine.lavd(tracer=None)", "ms": ms, "ms_per_step": round(ms["median"] / nsteps, 3)})
        for form in ("auto", "direct", "tiled"):
            eng.set_footprint_form(form)
            for name, extra in (("Engine.footprint()", {}), ("Engine.footprint(weights, tracer)", dict(weights=w, tracer=tracer))):
                ms = timed(lambda: eng.footprint(field, slat, slon, dt, glat, glon, nsteps=nsteps, level_chunk=a.chunk, **extra, **kw))
                emit({"case": "window", "what": name, "form": form, "kernel": eng.last_footprint_kernel(), "ms": ms,
                      "ms_per_step": round(ms["median"] / nsteps, 3), "over_lavd": round(ms["median"] / lavd_ms, 2)})
        eng.set_footprint_form("auto")

    print("| case | what | form | ms (median / min / max) | ratio | note |")
    print("|---|---|---|---|---|---|")
    for r in rows:
        ms = r.get("ms")
        ratio = r.get("over_lavd_update", r.get("over_lavd", ""))
        note = f"left the window {r['left_window']}, outside the grid {r['outside_grid']}" if "left_window" in r else r.get("kernel", "")
        print(f"| {r['case']} | {r['what']} | {r.get('form', '')} | {'' if ms is None else '%s / %s / %s' % (ms['median'], ms['min'], ms['max'])} | {ratio} | {note} |")
    eng.close()


if __name__ == "__main__":
    main()
