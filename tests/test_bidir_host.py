"""``LCS.bidirectional`` and ``lc_advect_series_dirs`` on the CPU: the symbol, the entry point's argument checks, the
drop-in's refusals, shapes and time labels of both directions (with and without ``window``, ``resample``, ``return_dpts``,
``subdomain``, ``isglobal``), the result against the two single-direction calls through a stand-in engine answering with
the CPU oracle (test_dropin_host_logic.py's), and the host orchestration of the two-direction launches and the per-plane
outer clamp against the recording fake HIP runtime under AddressSanitizer + UBSan.  The arithmetic on the GPU is
tests/test_bidir_gpu.py's."""
import os
import subprocess

import numpy as np
import pytest
import torch

from lagrangiancoherence_amd import _capi, build, dropin
from tests.test_capi_symbols import declared_symbols
from tests.test_series_host import CSRC, HIPCC, ROOT, SAN, UNITS, OracleSeriesEngine, _dataset


@pytest.fixture(scope="module")
def lib():
    build.build_library(verbose=False)
    return _capi.load()


def test_new_symbol_in_header_prototypes_and_library(lib):
    assert "lc_advect_series_dirs" in declared_symbols() and "lc_advect_series_dirs" in _capi.PROTOTYPES
    assert hasattr(lib, "lc_advect_series_dirs")
    assert declared_symbols() == sorted(_capi.PROTOTYPES)
    assert lib.lc_version() == 104 == _capi.LC_VERSION


def test_entry_point_checks_arguments_before_any_hip_call(lib):
    import ctypes as C
    a = _capi.AdvectArgs(struct_size=C.sizeof(_capi.AdvectArgs))
    assert lib.lc_advect_series_dirs(None, C.byref(a), 2) == _capi.LC_EINVAL and b"null context" in lib.lc_last_error()
    for bad in (0, 3, -1):
        assert lib.lc_advect_series_dirs(None, C.byref(a), bad) == _capi.LC_EINVAL and b"n_dirs" in lib.lc_last_error()
    a.struct_size -= 8
    assert lib.lc_advect_series_dirs(None, C.byref(a), 2) == _capi.LC_EINVAL and b"struct_size" in lib.lc_last_error()
    assert lib.lc_advect_series_dirs(None, None, 2) == _capi.LC_EINVAL
    # (row blocks, trajectories and the level range need a context: tests/c/bidir_orchestration.cpp)


# ------------------------------------------------------------------ drop-in adapter through a stand-in engine
class OracleBidirEngine(OracleSeriesEngine):
    """OracleSeriesEngine plus lcs_bidirectional as a loop of lcs over both directions and every window."""
    bidir_calls = []

    def lcs_bidirectional(self, f, slat, slon, timestep, nsteps, n_windows=1, t0=0, t0_stride=1, SETTLS_order=0,
                          interp_order=1, cyclic_xboundary=True, gauss_sigma=None, fd_fp32_cast=True, tensor_layout="reference",
                          noncyclic_clamp=None):
        self.bidir_calls.append(dict(nt=f.nt, nsteps=nsteps, n_windows=n_windows, t0=t0, t0_stride=t0_stride, timestep=timestep,
                                     cyclic=cyclic_xboundary))
        outs = [[self.lcs(f, slat, slon, sign * abs(timestep), SETTLS_order, interp_order, cyclic_xboundary, t0 + m * t0_stride,
                          nsteps, gauss_sigma, fd_fp32_cast, tensor_layout) for m in range(n_windows)] for sign in (-1, 1)]
        return {k: torch.stack([torch.stack([o[k] for o in row]) for row in outs]) for k in ("sigma", "x_dep", "y_dep")}


@pytest.fixture(autouse=True)
def oracle_engine(monkeypatch):
    eng = OracleBidirEngine()
    eng.series_calls = []
    eng.bidir_calls = []
    monkeypatch.setattr(dropin, "_ENGINE", eng)
    return eng


def test_the_shim_class_has_bidirectional():
    from LagrangianCoherence.LCS.LCS import LCS
    assert LCS is dropin.LCS and callable(getattr(LCS, "bidirectional"))


def test_argument_checks():
    from LagrangianCoherence.LCS.LCS import LCS
    ds, times, lat, lon = _dataset(nt=6)
    with pytest.raises(ValueError, match="timestep"):
        LCS(timestep=0, timedim="time").bidirectional(ds, verbose=False)
    lcs = LCS(timestep=-6 * 3600, timedim="time", SETTLS_order=1)
    for bad in (1, 0, -3, 2.5, True):
        with pytest.raises(ValueError, match="window"):
            lcs.bidirectional(ds, window=bad, verbose=False)
    for bad in (0, -1, 1.5, False):
        with pytest.raises(ValueError, match="stride"):
            lcs.bidirectional(ds, window=3, stride=bad, verbose=False)
    with pytest.raises(ValueError, match="longer than the record"):
        lcs.bidirectional(ds, window=7, verbose=False)
    with pytest.raises(TypeError):
        lcs.bidirectional(ds, return_traj=True, verbose=False)          # out of scope, as in series


def _tuple(r):
    return r if isinstance(r, tuple) else (r,)


def _same_labelled(a, b):
    assert a.dims == b.dims and a.shape == b.shape
    assert np.array_equal(a.values, b.values)
    for k in b.coords:
        assert np.array_equal(np.asarray(a.coords[k]), np.asarray(b.coords[k])), k


@pytest.mark.parametrize("window,resample", [(None, None), (None, "3h"), (4, None), (4, "3h")])
@pytest.mark.parametrize("dpts", [False, True])
def test_labels_and_the_two_single_direction_calls(oracle_engine, window, resample, dpts):
    """Both directions against LCS(timestep=-+|dt|)(ds) (window None) or .series(ds, window) through the oracle: values, dims,
    time labels (first time backward, last forward: LCS.py:158), the subdomain crop and the return_dpts tuple."""
    from LagrangianCoherence.LCS.LCS import LCS
    nt, stride = 7, 2
    ds, times, lat, lon = _dataset(nt=nt)
    sub = {"latitude": slice(-40, 40), "longitude": slice(-100, 100)}
    ctor = dict(timestep=6 * 3600, timedim="time", SETTLS_order=1, subdomain=sub, return_dpts=dpts)
    call = dict(resample=resample, verbose=False, traj_interp_order=1)
    att, rep = LCS(**ctor).bidirectional(ds, window=window, stride=stride, **call)
    (calls,) = oracle_engine.bidir_calls
    r = 2 if resample else 1
    n = 1 if window is None else (nt - window) // stride + 1
    wlen = (nt - 1) * r + 1 if window is None else (window - 1) * r + 1
    assert calls == dict(nt=(nt - 1) * r + 1, nsteps=wlen - 1, n_windows=n, t0=0, t0_stride=1 if window is None else stride * r,
                         timestep=6 * 3600 / r, cyclic=False)
    first = np.arange(n) * (1 if window is None else stride)
    want_labels = {False: times[first], True: times[first + (nt - 1 if window is None else window - 1)]}
    for got, sign in ((att, -1), (rep, 1)):
        c = dict(ctor, timestep=sign * 6 * 3600)
        want = LCS(**c)(ds, **call) if window is None else LCS(**c).series(ds, window=window, stride=stride, **call)
        got, want = _tuple(got), _tuple(want)
        assert len(got) == len(want) == (3 if dpts else 1)
        for a, b in zip(got, want):
            _same_labelled(a, b)
        assert np.array_equal(np.asarray(got[0].coords["time"]), want_labels[sign > 0])
        assert got[0].shape == (n, int(((lat > -40) & (lat < 40)).sum()), int(((lon > -100) & (lon < 100)).sum()))


def test_isglobal_drops_the_subdomain_and_runs_cyclic(oracle_engine):
    from LagrangianCoherence.LCS.LCS import LCS
    ds, times, lat, lon = _dataset(nt=5)
    lcs = LCS(timestep=-6 * 3600, timedim="time", SETTLS_order=1, subdomain={"latitude": slice(-40, 40),
                                                                           "longitude": slice(-100, 100)})
    att, rep = lcs.bidirectional(ds, isglobal=True, interp_to_common_grid=False, truncation=None, verbose=False,
                                 traj_interp_order=1)
    assert lcs.subdomain is None and oracle_engine.bidir_calls[0]["cyclic"] is True
    assert att.shape == rep.shape == (1, lat.size, lon.size)
    assert att.coords["time"][0] == times[0] and rep.coords["time"][0] == times[-1]
    for got, sign in ((att, -1), (rep, 1)):
        want = LCS(timestep=sign * 6 * 3600, timedim="time", SETTLS_order=1)(ds, isglobal=True, interp_to_common_grid=False,
                                                                            truncation=None, verbose=False, traj_interp_order=1)
        _same_labelled(got, want)


# ------------------------------------------------------------------ host orchestration under the sanitizers
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")
def test_bidir_host_orchestration_under_asan_and_ubsan(tmp_path):
    """tests/c/bidir_orchestration.cpp against the recording fake HIP runtime (tests/c/fake_hip.c): two fused launches per
    level chunk, per-plane clamp flags that fire in different chunks for the two directions, the refusals (n_dirs, row
    blocks, trajectories, the level range), and a failure injected at every allocation and every copy -- no leak, no overrun,
    the context usable afterwards."""
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
    drv = str(tmp_path / "bidir_orchestration.o")
    subprocess.run([clangxx, "-std=c++17", "-Wall", "-Wextra", *SAN, "-c", os.path.join(ROOT, "tests", "c", "bidir_orchestration.cpp"),
                    "-o", drv], check=True)
    exe = str(tmp_path / "bidir_orchestration")
    r = subprocess.run([clangxx, *SAN, drv, *objs, fake, "-o", exe, "-ldl", "-lm", "-lpthread", "-Wl,--wrap=hipMemcpyAsync",
                        "-Wl,--unresolved-symbols=ignore-all"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
                                UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1"))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    assert r.stdout.startswith("OK ") and int(r.stdout.split()[1]) > 40, r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
