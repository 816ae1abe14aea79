"""Time lc_strain against lc_sigma on the same departure fields under one build, and record the host alternative.

    python tools/strain_profile.py [--reps N] [--out DIR] [--no-trace]

  * float32, 4096 x 4096: ``lc_strain`` (four planes out) against ``lc_sigma`` with the physical layout through the LDS-tile
    kernel (``set_sigma_march(0)``: the kernel of the same shape, the comparison the byte ratio 6 : 3 planes speaks of) and
    through the default marching kernel.
  * float64, 2048 x 2048, ``fd_fp32_cast`` on: ``lc_strain`` against ``lc_sigma``.
  * the route without the kernel, for scale: ``Engine.flowmap_gradient`` + copy to the host + ``numpy.linalg.svd`` of the
    3 x 2 matrices, on config 1's grid (89 x 180) and on 1024 x 1024, float64; wall clock, one run after one warm-up.

Kernel timings: HIP events around single launches on the engine's stream, ``--reps`` (default 30, at least 20) timed launches
per variant after 5 warm-up launches, the variants taking turns launch by launch; median, minimum and maximum.  Then one
``rocprofv3 --kernel-trace --stats`` child pass of this command (a process of its own, tracing only, no counters) for the
profiler's own per-kernel durations.  Writes ``DIR/strain_profile.json`` (default ``profiles/strain``), stamped with the
library's build id, and a short ``DIR/README.md`` (the table of the cases), and prints the JSON line."""
import argparse
import csv
import glob
import json
import os
import shutil
import signal
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def departure_fields(torch, device, ny, nx, dtype):
    """A smooth deformation of a global ny x nx seed grid, evaluated on the device: (x_dep, y_dep, lat, lon)."""
    lat = np.linspace(-89.5, 89.5, ny)
    lon = -180.0 + 360.0 / nx * np.arange(nx)
    yy = torch.as_tensor(np.deg2rad(lat), device=device)[:, None]
    xx = torch.as_tensor(np.deg2rad(lon), device=device)[None, :]
    x = torch.as_tensor(lon, device=device)[None, :] + 3.0 * torch.sin(3 * xx + 0.3) * torch.cos(2 * yy) + 1.5 * torch.sin(7 * xx) * torch.sin(5 * yy)
    y = torch.as_tensor(lat, device=device)[:, None] * 0.9 + 2.0 * torch.cos(2 * xx + 1.0) * torch.sin(3 * yy) * torch.cos(yy)
    td = getattr(torch, np.dtype(dtype).name)
    return x.to(td).contiguous(), y.to(td).contiguous(), lat.astype(dtype), lon.astype(dtype)


def timed_launches(torch, variants, reps, warmup=5):
    """variants: name -> callable enqueueing ONE launch.  Returns name -> {median_ms, min_ms, max_ms, launches}; the variants
    take turns, each timed launch between its own pair of events and behind an untimed launch of the same kernel, so that the
    device is busy while the host enqueues the events and the launch (an idle stream would add the host's enqueue time)."""
    for _ in range(warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    ev = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            fn()
            a.record()
            fn()
            b.record()
            ev[k].append((a, b))
        torch.cuda.synchronize()
    out = {}
    for k, pairs in ev.items():
        t = np.array([a.elapsed_time(b) for a, b in pairs])
        out[k] = {"median_ms": float(np.median(t)), "min_ms": float(t.min()), "max_ms": float(t.max()), "launches": int(t.size)}
    return out


def kernel_cases(eng, torch, reps):
    """The two timed comparisons: the C entry points on preallocated buffers, on torch's current stream."""
    from lagrangiancoherence_amd import _capi
    lib, ptr = eng.lib, eng._ptr
    out = {}
    for label, n, dtype in (("float32_4096", 4096, np.float32), ("float64_2048", 2048, np.float64)):
        x, y, lat, lon = departure_fields(torch, eng.device, n, n, dtype)
        dlat, dlon = float(lat[1] - lat[0]), float(lon[1] - lon[0])
        slat = eng.to_device(lat, dtype)
        lc = _capi.LC_F32 if dtype == np.float32 else _capi.LC_F64
        o = [torch.empty_like(x) for _ in range(4)]
        eng._use_current_stream()
        names = {}

        def strain():
            _capi.check(lib.lc_strain(eng.ctx, ptr(x), ptr(y), lc, n, n, ptr(slat), dlat, dlon, 1, 1, *(ptr(t) for t in o)), lib)

        def sigma():
            _capi.check(lib.lc_sigma(eng.ctx, ptr(x), ptr(y), lc, 0, n, n, n, ptr(slat), dlat, dlon, 1, _capi.LC_LAYOUT_PHYSICAL, 0, n,
                                     ptr(o[0])), lib)
        t = {}
        eng.set_sigma_march(0)
        t.update(timed_launches(torch, {"strain": strain, "sigma_tile": sigma}, reps))
        names["strain"], names["sigma_tile"] = eng.last_strain_kernel(), eng.last_sigma_kernel()
        eng.set_sigma_march(-1)
        if dtype == np.float32:     # the default route of a grid this size: the marching kernel
            t.update({"sigma_default": timed_launches(torch, {"sigma": sigma}, reps)["sigma"]})
            names["sigma_default"] = eng.last_sigma_kernel()
        cells = n * n
        item = np.dtype(dtype).itemsize
        for k, planes in (("strain", 6), ("sigma_tile", 3), ("sigma_default", 3)):
            if k in t:
                t[k]["kernel"] = names[k]
                t[k]["algorithmic_bytes"] = planes * cells * item            # planes read + planes written, once each
                t[k]["algorithmic_GBps"] = planes * cells * item / t[k]["median_ms"] / 1e6
                t[k]["Mcells_per_s"] = cells / t[k]["median_ms"] / 1e3
        t["time_ratio_strain_over_sigma_tile"] = t["strain"]["median_ms"] / t["sigma_tile"]["median_ms"]
        t["byte_ratio"] = 2.0
        t["shape"] = [n, n]
        out[label] = t
        del x, y, o
    return out


def host_alternative(eng, torch):
    """flowmap_gradient + copy to the host + numpy.linalg.svd, float64: what a caller had before lc_strain."""
    from lagrangiancoherence_amd import flows
    out = {}
    _, _, lat1, lon1 = flows.config1()
    for label, shape in (("config1_89x180", (lat1.size, lon1.size)), ("1024x1024", (1024, 1024))):
        x, y, lat, lon = departure_fields(torch, eng.device, *shape, np.float64)
        dlat, dlon = float(lat[1] - lat[0]), float(lon[1] - lon[0])

        def host():
            t = eng.to_host(eng.flowmap_gradient(x, y, lat, dlat, dlon))
            F = np.stack([np.stack([t[0], t[1]], -1), np.stack([t[2], t[3]], -1), np.stack([t[4], t[5]], -1)], -2)
            return np.linalg.svd(F, full_matrices=False)

        def device():
            r = eng.strain(x, y, lat, dlat, dlon)
            return {k: eng.to_host(v) for k, v in r.items()}
        res = {}
        for k, fn in (("flowmap_gradient_host_svd_s", host), ("strain_to_host_s", device)):
            fn()
            eng.synchronize()
            t0 = time.perf_counter()
            fn()
            eng.synchronize()
            res[k] = time.perf_counter() - t0
        res["Mcells_per_s_host_svd"] = shape[0] * shape[1] / res["flowmap_gradient_host_svd_s"] / 1e6
        out[label] = res
    return out


def short_kernel_name(name):
    name = name.replace("void ", "")
    return (name.split("(anonymous namespace)::", 1)[1] if "(anonymous namespace)::" in name else name).split("(")[0]


def kernel_trace_child(reps, timeout_s=240.0):
    """One ``rocprofv3 --kernel-trace --stats`` pass of ``--child`` (the kernel cases only) in a process of its own; tracing
    only.  Returns ({kernel: calls / avg_ms / min_ms / max_ms}, None) or ({}, why)."""
    exe = shutil.which("rocprofv3")
    if not exe:
        return {}, "rocprofv3 not on PATH"
    tmp = tempfile.mkdtemp(prefix="lcs_strain_kt_", dir="/tmp")
    try:
        cmd = [exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.join(tmp, "kt"), "--", sys.executable,
               os.path.abspath(__file__), "--child", "--reps", str(reps)]
        p = subprocess.Popen(cmd, cwd="/tmp", env={**os.environ, "TMPDIR": "/tmp"}, stdout=subprocess.DEVNULL,
                             stderr=subprocess.DEVNULL, start_new_session=True)
        try:
            rc = p.wait(timeout=timeout_s)
        except subprocess.TimeoutExpired:
            os.killpg(p.pid, signal.SIGKILL)
            p.wait()
            return {}, f"rocprofv3 --kernel-trace --stats pass exceeded {timeout_s:.0f} s"
        if rc != 0:
            return {}, f"rocprofv3 --kernel-trace --stats pass exited {rc}"
        out = {}
        for f in glob.glob(os.path.join(tmp, "kt", "**", "*_kernel_stats.csv"), recursive=True):
            for r in csv.DictReader(open(f)):
                k = short_kernel_name(r["Name"])
                if k.startswith(("strain_", "sigma_")):
                    out[k] = {"calls": int(r["Calls"]), "avg_ms": float(r["AverageNs"]) / 1e6, "min_ms": float(r["MinNs"]) / 1e6,
                              "max_ms": float(r["MaxNs"]) / 1e6}
        return (out, None) if out else ({}, "no strain / sigma kernel in the kernel-trace statistics")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def write_readme(out, path):
    """A short README beside the JSON line: the table of the measured cases and how to read it."""
    k32, k64, host = out["kernels"]["float32_4096"], out["kernels"]["float64_2048"], out["host_alternative"]
    kt = out.get("kernel_trace_stats", {})
    row = lambda name, d: (f"| `{d['kernel']}` | {name} | {d['median_ms']:.4f} | {d['min_ms']:.4f} – {d['max_ms']:.4f} | "
                           f"{d['algorithmic_GBps']:.0f} | {kt[d['kernel']]['avg_ms']:.4f} |" if d["kernel"] in kt else
                           f"| `{d['kernel']}` | {name} | {d['median_ms']:.4f} | {d['min_ms']:.4f} – {d['max_ms']:.4f} | "
                           f"{d['algorithmic_GBps']:.0f} | not measured |")
    kt_name = {k.split("<")[0]: k for k in kt}
    for d in (k32.get("sigma_default"),):       # the profiler spells the marching kernel with its template arguments
        if d and d["kernel"] not in kt and d["kernel"] in kt_name:
            kt[d["kernel"]] = kt[kt_name[d["kernel"]]]
    r32, r64 = k32["time_ratio_strain_over_sigma_tile"], k64["time_ratio_strain_over_sigma_tile"]
    verdict = ("inside" if r32 <= 2.0 * 1.04 else "OUTSIDE")
    lines = [
        "# Stretch factors and direction: `lc_strain` against `lc_sigma`",
        "",
        f"Written by `tools/strain_profile.py --reps {out['reps']}` on one MI355X, library build `{out['build_id']}`; "
        "`strain_profile.json` is the tool's output line. Both entry points run on the same departure fields (a smooth "
        "deformation of a global seed grid) with the physical tensor layout and `fd_fp32_cast` on. Times are HIP events around "
        f"single launches, each behind an untimed launch of the same kernel so that the stream is busy: median of {out['reps']} "
        f"after {out['warmup']} warm-up launches, the variants taking turns. The last column is the average of a "
        "`rocprofv3 --kernel-trace --stats` pass of the same launches in a process of its own (tracing only, no counters).",
        "",
        "| kernel | case | median ms | min – max ms | planes moved, GB/s | rocprofv3 avg ms |",
        "|---|---|---|---|---|---|",
        row("float32 4096², strain (6 planes)", k32["strain"]),
        row("float32 4096², σ, LDS-tile kernel (3 planes)", k32["sigma_tile"]),
        row("float32 4096², σ, default (marching) kernel", k32["sigma_default"]),
        row("float64 2048², strain", k64["strain"]),
        row("float64 2048², σ", k64["sigma_tile"]),
        "",
        f"* The comparison is `sigma_kernel_f32` at the same shape: the strain kernel moves six planes where σ moves three. "
        f"Time ratio {r32:.2f} at a byte ratio of 2.0: {verdict} the expectation of at most 2.0 within the ±4 % two boxes differ by.",
        f"* float64: time ratio {r64:.2f}. The two float64 kernels share the staging pass with its double-precision "
        "trigonometry; which unit bounds them was not measured (no counter pass was taken).",
        "* The eigen step is float64 for both dtypes (four square roots and three divisions per cell). At float32 the kernel "
        "runs at the tile σ kernel's rate per byte moved, so that arithmetic does not show in the time ratio.",
        "",
        "## The route without the kernel",
        "",
        "`Engine.flowmap_gradient` (nine planes), copy to the host, `numpy.linalg.svd` of the 3 × 2 matrices, float64; wall clock "
        "of one run after one warm-up, against `Engine.strain` + the copy of its four planes to the host.",
        "",
        "| grid | flowmap_gradient + host SVD | strain + copy to host | host route, Mcells/s |",
        "|---|---|---|---|",
    ]
    for label, d in host.items():
        lines.append(f"| {label} | {d['flowmap_gradient_host_svd_s'] * 1e3:.2f} ms | {d['strain_to_host_s'] * 1e3:.3f} ms | "
                     f"{d['Mcells_per_s_host_svd']:.2f} |")
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "strain"))
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--child", action="store_true", help="the kernel cases only (what the rocprofv3 pass runs)")
    args = ap.parse_args()
    reps = max(args.reps, 20)
    import torch
    from lagrangiancoherence_amd import _capi
    from lagrangiancoherence_amd.engine import Engine
    eng = Engine(0)
    if args.child:
        kernel_cases(eng, torch, reps)
        eng.synchronize()
        eng.close()
        return
    out = {"build_id": _capi.load().lc_build_id().decode(), "device": torch.cuda.get_device_name(0), "reps": reps, "warmup": 5,
           "kernels": kernel_cases(eng, torch, reps), "host_alternative": host_alternative(eng, torch)}
    eng.synchronize()
    eng.close()
    if not args.no_trace:
        stats, why = kernel_trace_child(reps)
        out["kernel_trace_stats"] = stats if stats else {"not_measured": why}
    line = json.dumps(out)
    print(line)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "strain_profile.json"), "w") as fh:
        fh.write(line + "\n")
    write_readme(out, os.path.join(args.out, "README.md"))


if __name__ == "__main__":
    main()
