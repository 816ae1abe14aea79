"""``LCS.series`` and its C entry points on the CPU: the symbols (``lc_advect_series``, ``lc_sigma_batch``), the drop-in's
argument checks, window count and time labels (forward / backward, with and without ``resample``), the claim that resampling
the record and slicing it gives what resampling each slice gives, the series against the per-window loop through a stand-in
engine answering with the CPU oracle (test_dropin_host_logic.py's), and the host orchestration of the batched outer clamp
against the recording fake HIP runtime under AddressSanitizer + UBSan.  The arithmetic on the GPU is tests/test_series_gpu.py's."""
import os
import shutil
import subprocess

import numpy as np
import pandas as pd
import pytest
import torch

from lagrangiancoherence_amd import _capi, build, dropin, flows
from lagrangiancoherence_amd.engine import Engine
from tests import labelled
from tests.test_capi_symbols import declared_symbols
from tests.test_dropin_host_logic import OracleEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lagrangiancoherence_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def lib():
    build.build_library(verbose=False)
    return _capi.load()


def test_new_symbols_in_header_prototypes_and_library(lib):
    for name in ("lc_advect_series", "lc_sigma_batch"):
        assert name in declared_symbols() and name in _capi.PROTOTYPES and hasattr(lib, name)
    assert declared_symbols() == sorted(_capi.PROTOTYPES)
    assert lib.lc_version() == 104 == _capi.LC_VERSION


def test_new_entry_points_check_arguments_before_any_hip_call(lib):
    import ctypes as C
    a = _capi.AdvectArgs(struct_size=C.sizeof(_capi.AdvectArgs))
    assert lib.lc_advect_series(None, C.byref(a)) == _capi.LC_EINVAL and b"null context" in lib.lc_last_error()
    a.struct_size -= 8
    assert lib.lc_advect_series(None, C.byref(a)) == _capi.LC_EINVAL and b"struct_size" in lib.lc_last_error()
    assert lib.lc_advect_series(None, None) == _capi.LC_EINVAL
    assert lib.lc_sigma_batch(None, None, None, _capi.LC_F32, 8, 8, None, 1.0, 1.0, 1, 0, 2, None) == _capi.LC_EINVAL
    assert b"null context" in lib.lc_last_error()


# ------------------------------------------------------------------ drop-in adapter through a stand-in engine
class OracleSeriesEngine(OracleEngine):
    """OracleEngine plus the calls LCS.series makes: the pack options, and lcs_series as a loop of lcs."""
    series_calls = []
    _pack_options = staticmethod(Engine._pack_options)

    def prepare_field(self, u, v, lat, lon, interp_order=1, dtype=None, fuse_levels=None, ext_image=None):
        return super().prepare_field(u, v, lat, lon, interp_order, dtype, fuse_levels)

    def lcs_series(self, f, slat, slon, timestep, nsteps, n_windows, t0=0, t0_stride=1, SETTLS_order=0, interp_order=1,
                   cyclic_xboundary=True, gauss_sigma=None, fd_fp32_cast=True, tensor_layout="reference", noncyclic_clamp=None):
        self.series_calls.append(dict(nt=f.nt, nsteps=nsteps, n_windows=n_windows, t0=t0, t0_stride=t0_stride, timestep=timestep))
        outs = [self.lcs(f, slat, slon, timestep, SETTLS_order, interp_order, cyclic_xboundary, t0 + m * t0_stride, nsteps,
                         gauss_sigma, fd_fp32_cast, tensor_layout) for m in range(n_windows)]
        return {k: torch.stack([o[k] for o in outs]) for k in ("sigma", "x_dep", "y_dep")}


@pytest.fixture(autouse=True)
def oracle_engine(monkeypatch):
    eng = OracleSeriesEngine()
    eng.series_calls = []
    monkeypatch.setattr(dropin, "_ENGINE", eng)
    return eng


def _dataset(nt=9, freq="6h", start="2000-01-01"):
    u, v, lat, lon = flows.config1()
    u, v = np.concatenate([u] * 2)[:nt], np.concatenate([v] * 2)[:nt]
    times = pd.date_range(start, periods=nt, freq=freq).values
    coords = {"latitude": lat, "longitude": lon, "time": times}
    U = labelled.DataArray(u.transpose(1, 2, 0), ["latitude", "longitude", "time"], coords, name="u")
    V = labelled.DataArray(v.transpose(1, 2, 0), ["latitude", "longitude", "time"], coords, name="v")
    return labelled.Dataset({"u": U, "v": V}), times, lat, lon


def _slice(ds, a, b):
    return labelled.Dataset({k: ds[k].isel(time=slice(a, b)) for k in ("u", "v")})


def test_the_shim_class_has_series():
    from LagrangianCoherence.LCS.LCS import LCS
    assert LCS is dropin.LCS and callable(getattr(LCS, "series"))


def test_argument_checks():
    from LagrangianCoherence.LCS.LCS import LCS
    ds, times, lat, lon = _dataset(nt=6)
    lcs = LCS(timestep=-6 * 3600, timedim="time", SETTLS_order=1)
    for bad in (None, 1, 0, -3, 2.5, True):
        with pytest.raises(ValueError, match="window"):
            lcs.series(ds, window=bad, verbose=False)
    for bad in (0, -1, 1.5, False):
        with pytest.raises(ValueError, match="stride"):
            lcs.series(ds, window=3, stride=bad, verbose=False)
    with pytest.raises(ValueError, match="longer than the record"):
        lcs.series(ds, window=7, verbose=False)
    with pytest.raises(TypeError):
        lcs.series(ds, window=3, return_traj=True, verbose=False)       # out of scope for a series
    # resampling a record whose own spacing is not uniform: the resampled axis does not hold every original level at i * r
    t = ds.u.coords["time"].copy()
    t[3:] = t[3:] + np.timedelta64(3, "h")
    bent = labelled.Dataset({k: labelled.DataArray(ds[k].values, ds[k].dims, {**ds[k].coords, "time": t}, k) for k in ("u", "v")})
    with pytest.raises(ValueError, match="resample"):
        lcs.series(bent, window=3, resample="3h", verbose=False)
    with pytest.raises(ValueError, match="resample"):
        dropin._resample_ratio(times, np.array([times[0], times[1], times[3]]))          # non-uniform resampled spacing
    with pytest.raises(ValueError, match="resample"):
        dropin._resample_ratio(times, times[:4] + np.timedelta64(1, "h"))               # original levels not on the axis
    assert dropin._resample_ratio(times, pd.date_range(times[0], times[-1], freq="2h").values) == 3


@pytest.mark.parametrize("timestep", [6 * 3600, -6 * 3600])
@pytest.mark.parametrize("resample", [None, "3h"])
def test_window_count_and_time_labels(oracle_engine, timestep, resample):
    from LagrangianCoherence.LCS.LCS import LCS
    nt, window, stride = 9, 4, 2
    ds, times, lat, lon = _dataset(nt=nt)
    lcs = LCS(timestep=timestep, timedim="time", SETTLS_order=1, return_dpts=True)
    sig, xd, yd = lcs.series(ds, window=window, stride=stride, resample=resample, verbose=False, traj_interp_order=1)
    n = (nt - window) // stride + 1
    first = np.arange(n) * stride
    want = times[first + window - 1] if timestep > 0 else times[first]      # LCS.py:158 per window
    assert sig.dims == xd.dims == yd.dims == ("time", "latitude", "longitude")
    assert sig.shape == (n, lat.size, lon.size) and xd.shape == yd.shape == sig.shape
    for a in (sig, xd, yd):
        assert np.array_equal(a.coords["time"], want)
    r = 2 if resample else 1
    call, = oracle_engine.series_calls
    assert call == dict(nt=(nt - 1) * r + 1, nsteps=(window - 1) * r, n_windows=n, t0=0, t0_stride=stride * r,
                        timestep=np.sign(timestep) * 6 * 3600 / r)
    # what each per-window call stamps
    for w in (0, n - 1):
        one = LCS(timestep=timestep, timedim="time", SETTLS_order=1, return_dpts=True)(
            _slice(ds, w * stride, w * stride + window), resample=resample, verbose=False, traj_interp_order=1)
        # (the per-window x_dep carries its label as times.tolist()[-1]: integer nanoseconds for datetime64[ns] times)
        assert one[0].coords["time"][0] == want[w] and np.datetime64(int(one[1].coords["time"]), "ns") == want[w]


def test_resampled_record_sliced_against_resampled_slices():
    """What LCS.series with ``resample`` rests on, measured: a window of the resampled record equals the resampled window
    bit for bit except at the window's FIRST level.  There interp1d (what xarray's resample().interpolate('linear')
    delegates to) returns the original level itself for the window, but for the whole record it evaluates the interval
    on the left, ``(y[k] - y[k-1]) / dx * dx + y[k-1]``, which can differ from ``y[k]`` in its last bit."""
    ds, times, lat, lon = _dataset(nt=9)
    # a float32 record (the meridional wind of tests/test_series_gpu.py's driver-shaped case)
    t = np.arange(9)[:, None, None]
    v32 = (6.0 * np.cos(0.25 * lon[None, None, :] - 0.4 * t) * np.sin(0.3 * lat[None, :, None])).astype(np.float32)
    v32 = labelled.DataArray(v32.transpose(1, 2, 0), ["latitude", "longitude", "time"], ds.u.coords, "v")
    first_differs = 0
    for da in (ds.u, v32):
        whole = dropin._resample_linear(da, "time", "3h")
        ax = whole.dims.index("time")
        r = 2
        for a, b in ((0, 4), (2, 6), (5, 9), (3, 5)):
            part = dropin._resample_linear(da.isel(time=slice(a, b)), "time", "3h")
            lv = np.take(whole.values, np.arange(a * r, (b - 1) * r + 1), axis=ax)
            assert np.array_equal(np.take(lv, np.arange(1, lv.shape[ax]), axis=ax),
                                  np.take(part.values, np.arange(1, lv.shape[ax]), axis=ax))
            assert np.array_equal(np.take(part.values, 0, axis=ax), np.take(da.values, a, axis=ax))   # the original level
            np.testing.assert_allclose(np.take(lv, 0, axis=ax), np.take(da.values, a, axis=ax), rtol=0, atol=2 * np.finfo(da.values.dtype).eps * np.abs(da.values).max())
            first_differs += not np.array_equal(np.take(lv, 0, axis=ax), np.take(part.values, 0, axis=ax))
            assert np.array_equal(whole.coords["time"][a * r:(b - 1) * r + 1], part.coords["time"])
    assert first_differs > 0        # (the left interval's value is not always the level itself)


@pytest.mark.parametrize("resample", [None, "3h"])
def test_series_equals_the_per_window_loop_through_the_oracle(resample):
    """The contract of LCS.series against the driver's loop (LCS/area_of_influence.py:168-181), with the oracle doing the
    arithmetic: regional (non-cyclic), SETTLS 4, backward, subdomain, return_dpts."""
    from LagrangianCoherence.LCS.LCS import LCS
    nt, window, stride = 8, 4, 1
    ds, times, lat, lon = _dataset(nt=nt)
    sub = {"latitude": slice(-40, 40), "longitude": slice(-100, 100)}
    kw = dict(timestep=-6 * 3600, timedim="time", SETTLS_order=4, subdomain=sub, return_dpts=True)
    sig, xd, yd = LCS(**kw).series(ds, window=window, stride=stride, resample=resample, verbose=False, traj_interp_order=1)
    assert sig.shape[0] == (nt - window) // stride + 1
    for w in range(sig.shape[0]):
        s1, x1, y1 = LCS(**kw)(_slice(ds, w * stride, w * stride + window), resample=resample, verbose=False, traj_interp_order=1)
        assert np.array_equal(sig.coords["latitude"], s1.coords["latitude"])
        if resample is None or w == 0:
            assert np.array_equal(sig.values[w], s1.values[0])
            assert np.array_equal(xd.values[w], x1.values) and np.array_equal(yd.values[w], y1.values)
        else:   # the window's first level differs in its last bits (test_resampled_record_sliced_against_resampled_slices)
            np.testing.assert_allclose(xd.values[w], x1.values, rtol=0, atol=1e-9)
            np.testing.assert_allclose(sig.values[w], s1.values[0], rtol=1e-7)


# ------------------------------------------------------------------ host orchestration under the sanitizers
UNITS = ["api", "pack", "advect", "sigma", "ridges", "halo", "preprocess"]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_series_host_orchestration_under_asan_and_ubsan(tmp_path):
    """tests/c/series_orchestration.cpp against the recording fake HIP runtime (tests/c/fake_hip.c): the batched outer
    clamp's flag read-backs and restarts with members firing in different chunks (or never), one launch per sub-step for
    every member, the refusals (lc_advect_series: row blocks, trajectories; lc_advect_batch / lc_advect_ex: the outer
    clamp), and a failure injected at every allocation and every copy -- no leak, no overrun, the context usable
    afterwards.  The library objects are compiled host-only (the kernels become launch stubs)."""
    objs, procs = [], []
    for u in UNITS:
        o = str(tmp_path / f"{u}.o")
        procs.append(subprocess.Popen([HIPCC, "--cuda-host-only", "-std=c++17", "-fPIC", "-Wno-unused-function", *SAN,
                                       '-DLCS_BUILD_ID="san"', "-c", os.path.join(CSRC, u + ".hip"), "-o", o],
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
        objs.append(o)
    for p in procs:
        out, _ = p.communicate()
        assert p.returncode == 0, out[-3000:]
    fake = str(tmp_path / "fake_hip.o")
    subprocess.run([HIPCC, "-x", "c", "-std=gnu11", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", *SAN,
                    "-c", os.path.join(ROOT, "tests", "c", "fake_hip.c"), "-o", fake], check=True)
    clangxx = os.path.join(os.path.dirname(os.path.realpath(HIPCC)), "..", "lib", "llvm", "bin", "clang++")
    if not os.path.exists(clangxx):
        clangxx = "/opt/rocm/lib/llvm/bin/clang++"
    drv = str(tmp_path / "series_orchestration.o")
    subprocess.run([clangxx, "-std=c++17", "-Wall", "-Wextra", *SAN, "-c", os.path.join(ROOT, "tests", "c", "series_orchestration.cpp"),
                    "-o", drv], check=True)
    exe = str(tmp_path / "series_orchestration")
    # (--wrap: the driver raises the clamp flags the stand-in's empty launches never raise, in the flag read-back)
    r = subprocess.run([clangxx, *SAN, drv, *objs, fake, "-o", exe, "-ldl", "-lm", "-lpthread", "-Wl,--wrap=hipMemcpyAsync",
                        "-Wl,--unresolved-symbols=ignore-all"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
                                UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1"))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    assert r.stdout.startswith("OK ") and int(r.stdout.split()[1]) > 60, r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
