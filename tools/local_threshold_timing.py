"""Time the local threshold of the driver's loop (LCS/area_of_influence.py:194-199: block 301, offset -0.8) on the device: the
one call behind tools.above_local_threshold against the route the package offered before it.

    python tools/local_threshold_timing.py [--warmup 3] [--reps 11] [--out profiles/local_threshold/timing.txt] [--quick]

Two shapes, float64: 1 x 541 x 781 (one window of the driver's domain) and 29 x 541 x 781 (its 29 windows).  The field is
seeded noise smoothed at sigma 1.5 about 1.5, made on the device; it lies there before the clock starts and the results stay
there.
    new     Engine.local_threshold(f, 50.0, offset=-0.8, want=("mask",)): two launches of gauss_line_kernel for all planes
    before  per plane Engine.gaussian_filter(plane, 50.0) (two launches of gauss_kernel, radius 200) and `plane > g + 0.8` in
            torch: what a caller had to write
A call is timed with the host's clock between two device synchronisations, the two routes alternating in one process after
`--warmup` calls of each; the median and the smallest of `--reps` are reported, and new / before of the medians.  Before
anything is timed the two masks are compared: both routes share the arithmetic of gauss_taps.h, so they are equal pixel for
pixel.  Prints one JSON line per shape and a table; `--out` also writes both there.  Needs a GPU (there is no other path).
`--quick`: 2 planes of 67 x 130 and one repeat, to rehearse the script."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIGMA, OFFSET = 50.0, -0.8       # (301 - 1) / 6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    import torch
    from lagrangiancoherence_amd.dropin import get_engine
    eng = get_engine()
    ny, nx = (67, 130) if a.quick else (541, 781)
    shapes = [(1, ny, nx), (2, ny, nx)] if a.quick else [(1, ny, nx), (29, ny, nx)]
    reps, warmup = (1, 1) if a.quick else (a.reps, a.warmup)
    lines, rows = [], []

    def say(text):
        print(text, flush=True)
        lines.append(text)
    for shape in shapes:
        gen = torch.Generator(device=eng.device).manual_seed(20261019)
        noise = torch.randn(shape, generator=gen, dtype=torch.float64, device=eng.device)
        f = torch.stack([1.5 + 5.0 * eng.gaussian_filter(p, 1.5) for p in noise]).contiguous()

        def new():
            return eng.local_threshold(f, SIGMA, offset=OFFSET, want=("mask",))["mask"]

        def before():
            return torch.stack([p > eng.gaussian_filter(p, SIGMA) + 0.8 for p in f])

        def timed(call):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = call()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, out
        (_, m_new), (_, m_before) = timed(new), timed(before)
        same = bool(torch.equal(m_new.bool(), m_before))
        assert same, f"{shape}: the two routes differ on {int((m_new.bool() != m_before).sum())} pixels"
        for _ in range(warmup):
            timed(new)
            timed(before)
        t_new, t_before = [], []
        for _ in range(reps):
            t_new.append(timed(new)[0])
            t_before.append(timed(before)[0])
        med_new, med_before = statistics.median(t_new), statistics.median(t_before)
        row = {"shape": "x".join(map(str, shape)), "dtype": "float64", "block_size": 301, "sigma": SIGMA, "offset": OFFSET,
               "kernels": eng.last_threshold_kernel, "mask_fraction": round(float(m_new.float().mean()), 4), "masks_equal": same,
               "new_ms": {"median": round(med_new, 4), "min": round(min(t_new), 4)},
               "before_ms": {"median": round(med_before, 4), "min": round(min(t_before), 4)},
               "new_over_before": round(med_new / med_before, 4), "reps": reps, "warmup": warmup,
               "device": torch.cuda.get_device_name(0)}
        say(json.dumps(row))
        rows.append(row)
    say("| shape | new ms (median / min) | before ms (median / min) | new / before | masks equal |")
    say("|---|---|---|---|---|")
    for r in rows:
        say(f"| {r['shape']} | {r['new_ms']['median']} / {r['new_ms']['min']} | {r['before_ms']['median']} / {r['before_ms']['min']} | "
            f"{r['new_over_before']} | {r['masks_equal']} |")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
