"""Time the component filter on one plane: label, sums and apply on the device, scipy.ndimage.label on this host.

    python tools/bench_components.py [--n 4096] [--density 0.41] [--connectivity 2] [--warmup 5] [--reps 20] [--no-scipy]

The mask is random (seed 20261018), float64; the intensity is uniform in [0, 1).  Every stage is timed with device events
on the current stream, after `--warmup` runs of the whole chain, one event pair per repetition; the figures are medians
(and the smallest) over `--reps`.  `filter` is Engine.filter_components as a user calls it, host clock around a device
synchronise: the three stages, the per-component arithmetic in torch and the one read-back of the counts in between.
`scipy_label` is scipy.ndimage.label of the same mask on this host, labelling only.  The device labels are compared with
scipy's before anything is reported.  Prints one JSON line; needs a GPU (there is no other path)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SEED = 20261018


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--density", type=float, default=0.41)
    ap.add_argument("--connectivity", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-scipy", action="store_true")
    a = ap.parse_args()
    import torch
    from lagrangiancoherence_amd.engine import Engine
    eng = Engine(0)
    rng = np.random.default_rng(SEED)
    mask_h = (rng.random((a.n, a.n)) < a.density).astype(np.float64)
    mask, inten = eng.to_device(mask_h, np.float64), eng.to_device(rng.random((a.n, a.n)), np.float64)

    def chain():
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        labels, counts = eng.label_components(mask, a.connectivity)
        ev[1].record()
        n_max = int(counts.max().item())
        ev_s = torch.cuda.Event(enable_timing=True)
        ev_s.record()
        sums = eng.component_sums(labels, counts, inten, n_max=n_max)
        ev[2].record()
        keep = (sums["area"] >= 4).to(torch.uint8)
        out = torch.empty_like(mask)
        ev_a = torch.cuda.Event(enable_timing=True)
        ev_a.record()
        eng._use_current_stream()
        eng.lib.lc_component_apply(eng.ctx, eng._ptr(labels), eng._ptr(mask), 1, a.n, a.n, 1, eng._ptr(keep), n_max, 0.0, eng._ptr(out))
        ev[3].record()
        torch.cuda.synchronize()
        return {"label": ev[0].elapsed_time(ev[1]), "sums": ev_s.elapsed_time(ev[2]), "apply": ev_a.elapsed_time(ev[3])}, labels, n_max

    for _ in range(a.warmup):
        _, labels, n_max = chain()
    runs = [chain()[0] for _ in range(a.reps)]
    whole = []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.filter_components(mask, inten, ["area", "mean_intensity"], [4, 0.5], a.connectivity)
        torch.cuda.synchronize()
        whole.append((time.perf_counter() - t0) * 1e3)
    res = {"n": a.n, "density": a.density, "connectivity": a.connectivity, "components": n_max, "warmup": a.warmup, "reps": a.reps,
           "device": torch.cuda.get_device_name(0)}
    for k in ("label", "sums", "apply"):
        v = [r[k] for r in runs]
        res[k + "_ms"] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    res["stages_ms_median"] = round(sum(res[k + "_ms"]["median"] for k in ("label", "sums", "apply")), 4)
    res["filter_ms"] = {"median": round(statistics.median(whole), 4), "min": round(min(whole), 4), "max": round(max(whole), 4)}
    if not a.no_scipy:
        from scipy import ndimage
        st = ndimage.generate_binary_structure(2, a.connectivity)
        t = []
        for _ in range(3):
            t0 = time.perf_counter()
            ref, n_ref = ndimage.label(mask_h != 0, structure=st)
            t.append((time.perf_counter() - t0) * 1e3)
        assert n_ref == n_max and np.array_equal(labels.cpu().numpy(), ref), "device labels differ from scipy's"
        res["scipy_label_ms"] = {"median": round(statistics.median(t), 2), "min": round(min(t), 2)}
        res["scipy_label_over_device_label"] = round(statistics.median(t) / res["label_ms"]["median"], 1)
        res["scipy_label_over_device_stages"] = round(statistics.median(t) / res["stages_ms_median"], 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
