"""Scalar tracers along trajectories on the CPU: the C-ABI surface of lc_tracer_sample (symbols, argument checks, the
argument structure) and the drop-in's ``parcel_propagation(..., C=)`` adapter (dims, labels, return forms, the check of
``C`` against ``U``).  A stand-in engine answers the adapter's calls with the CPU oracle, as in
test_dropin_host_logic.py; the arithmetic on the GPU is tests/test_tracer_gpu.py's."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pandas as pd
import pytest
import torch

from lagrangiancoherence_amd import _capi, build, dropin, flows
from lagrangiancoherence_amd.engine import common_dtype
from oracle import lcs_oracle as O
from tests import labelled


@pytest.fixture(scope="module")
def lib():
    build.build_library(verbose=False)
    return _capi.load()


def test_library_exports_the_tracer_entry_points(lib):
    assert hasattr(lib, "lc_tracer_sample") and hasattr(lib, "lc_ctx_last_tracer_kernel")
    assert "lc_tracer_sample" in _capi.PROTOTYPES and "lc_ctx_last_tracer_kernel" in _capi.PROTOTYPES
    assert lib.lc_ctx_last_tracer_kernel(None) == b""


def test_tracer_args_are_checked_before_any_hip_call(lib):
    a = _capi.TracerArgs(struct_size=C.sizeof(_capi.TracerArgs))
    # the library accepts the ctypes mirror's size (it checks struct_size first) and stops at the null context
    assert lib.lc_tracer_sample(None, C.byref(a)) == _capi.LC_EINVAL and b"null context" in lib.lc_last_error()
    a.struct_size = C.sizeof(_capi.TracerArgs) - 8
    assert lib.lc_tracer_sample(None, C.byref(a)) == _capi.LC_EINVAL and b"struct_size" in lib.lc_last_error()
    assert lib.lc_tracer_sample(None, None) == _capi.LC_EINVAL
    with pytest.raises(ValueError, match="null context"):
        _capi.check(lib.lc_tracer_sample(None, C.byref(_capi.TracerArgs(struct_size=C.sizeof(_capi.TracerArgs)))), lib)


def test_tracer_args_mirror_has_the_header_layout():
    # size_t + 4 pointers, 4 ints, 4 doubles, 5 ints (+ pad), 2 pointers, 2 ints, 6 pointers, 1 int (+ pad) on LP64
    assert C.sizeof(_capi.TracerArgs) == 8 + 32 + 16 + 32 + 24 + 16 + 8 + 48 + 8
    names = [f[0] for f in _capi.TracerArgs._fields_]
    assert names[0] == "struct_size" and names[-1] == "mean_count"


# ------------------------------------------------------------------ drop-in adapter through a stand-in engine
class OracleTracerEngine:
    """Answers the calls ``dropin.parcel_propagation(..., C=)`` makes with oracle results as CPU tensors."""
    torch = torch
    device = "cpu (oracle stand-in)"

    def to_host(self, t):
        return t.detach().cpu().numpy()

    def f64_fuse_levels(self, dtype, n_seeds):
        return np.dtype(dtype) != np.dtype(np.float64) or n_seeds > (1 << 18)

    def pack_and_advect(self, u, v, lat, lon, slat, slon, timestep, SETTLS_order=0, interp_order=1, cyclic_xboundary=True,
                        fuse_levels=None, return_traj=False, **_):
        dt = common_dtype(u, v, lat, lon)
        f = SimpleNamespace(dtype=dt, nt=u.shape[0], lat=np.asarray(lat, dt), lon=np.asarray(lon, dt))
        tx, ty = O.parcel_propagation(np.asarray(u, dt), np.asarray(v, dt), f.lat, f.lon, timestep=timestep,
                                      SETTLS_order=SETTLS_order, interp_order=interp_order,
                                      cyclic_xboundary=cyclic_xboundary, return_traj=True)
        res = (tx[-1], ty[-1], tx, ty) if return_traj else (tx[-1], ty[-1])
        return (f, *(torch.as_tensor(np.ascontiguousarray(a)) for a in res))

    def prepare_tracer(self, c1, c2=None, lat_f=None, lon_f=None, interp_order=1, dtype=None):
        return SimpleNamespace(c=np.asarray(c1, dtype), lat=np.asarray(lat_f, dtype), lon=np.asarray(lon_f, dtype))

    def sample_tracer(self, tracer, traj_x, traj_y, level0=0, interp_order=1, **_):
        tx, ty = traj_x.numpy(), traj_y.numpy()
        c = np.stack([O.xr_map_coordinates(tracer.c[level0 + j], tracer.lat, tracer.lon, tx[j], ty[j], order=interp_order)
                      for j in range(tx.shape[0])])
        return (torch.as_tensor(c), None), (None, None)


@pytest.fixture
def oracle_engine(monkeypatch):
    monkeypatch.setattr(dropin, "_ENGINE", OracleTracerEngine())


def _fields():
    u, v, lat, lon = flows.config1()
    times = pd.date_range("2000-01-01", periods=u.shape[0], freq="6h").values
    coords = {"latitude": lat, "longitude": lon, "time": times}
    U = labelled.DataArray(u.transpose(1, 2, 0), ["latitude", "longitude", "time"], coords, name="u")
    V = labelled.DataArray(v.transpose(1, 2, 0), ["latitude", "longitude", "time"], coords, name="v")
    c = np.hypot(u, v) + np.cos(np.deg2rad(lat))[None, :, None]          # a smooth tracer on the wind's grid
    Cl = labelled.DataArray(c, ["time", "latitude", "longitude"], coords, name="tcwv")
    return U, V, Cl, c, times, lat, lon


@pytest.mark.parametrize("timestep", [-6 * 3600, 6 * 3600])
def test_parcel_propagation_with_tracer_returns_three_labelled_outputs(oracle_engine, timestep):
    U, V, Cl, c, times, lat, lon = _fields()
    kw = dict(timestep=timestep, propdim="time", SETTLS_order=2, cyclic_xboundary=True, verbose=False, interp_order=3)
    x, y, cs = dropin.parcel_propagation(U, V, return_traj=True, C=Cl, **kw)
    assert cs.dims == x.dims == ("time", "latitude", "longitude") and cs.shape == x.shape == (8, 89, 180)
    assert cs.name == "tcwv"
    for k in ("time", "latitude", "longitude"):
        assert np.array_equal(cs.coords[k], x.coords[k]), k
    labels = times[::-1] if timestep < 0 else times                      # labels reversed as the positions' are (Q6)
    assert np.array_equal(cs.coords["time"], labels)
    tx, ty = O.parcel_propagation(np.moveaxis(U.values, 2, 0), np.moveaxis(V.values, 2, 0), lat, lon, timestep=timestep,
                                  SETTLS_order=2, interp_order=3, cyclic_xboundary=True, return_traj=True)
    for i in (0, 3, 7):                                                  # entry i: level i (stored order) at entry i
        np.testing.assert_array_equal(cs.values[i], O.xr_map_coordinates(c[i], lat, lon, tx[i], ty[i], order=3))
    mean = cs.values.mean(axis=0)                                        # what cs.mean('time') gives the driver
    assert mean.shape == (89, 180) and np.isfinite(mean).all()

    x2, y2, c2 = dropin.parcel_propagation(U, V, return_traj=False, C=Cl, **kw)
    assert c2.dims == x2.dims == ("latitude", "longitude")
    assert c2.coords["time"] == x2.coords["time"] == labels.tolist()[-1]
    np.testing.assert_array_equal(c2.values, cs.values[-1])
    np.testing.assert_array_equal(x2.values, x.values[-1])


def test_tracer_is_sorted_like_the_wind(oracle_engine):
    U, V, Cl, c, times, lat, lon = _fields()
    # the tracer handed with descending latitudes and another dim order: sorted like U before sampling
    Cd = labelled.DataArray(c[:, ::-1, :].transpose(2, 1, 0), ["longitude", "latitude", "time"],
                            {"latitude": lat[::-1], "longitude": lon, "time": times}, name="tcwv")
    kw = dict(timestep=-3600, SETTLS_order=1, cyclic_xboundary=True, verbose=False, interp_order=1, return_traj=True)
    a = dropin.parcel_propagation(U, V, C=Cl, **kw)[2]
    b = dropin.parcel_propagation(U, V, C=Cd, **kw)[2]
    np.testing.assert_array_equal(a.values, b.values)


def test_mismatched_tracer_is_refused_before_an_engine_is_made(monkeypatch):
    made = []
    monkeypatch.setattr(dropin, "_ENGINE", None)
    monkeypatch.setattr(dropin, "Engine", lambda *a, **k: made.append(1))
    U, V, Cl, c, times, lat, lon = _fields()
    bad_lat = labelled.DataArray(c, ["time", "latitude", "longitude"],
                                 {"latitude": lat + 0.5, "longitude": lon, "time": times}, name="c")
    bad_time = labelled.DataArray(c[:-1], ["time", "latitude", "longitude"],
                                  {"latitude": lat, "longitude": lon, "time": times[:-1]}, name="c")
    bad_dims = labelled.DataArray(c, ["step", "latitude", "longitude"],
                                  {"latitude": lat, "longitude": lon, "step": times}, name="c")
    for bad, msg in ((bad_lat, "coordinates"), (bad_time, "coordinates"), (bad_dims, "dims")):
        with pytest.raises(AssertionError, match=msg):
            dropin.parcel_propagation(U, V, timestep=-3600, verbose=False, C=bad)
    assert made == [] and dropin._ENGINE is None


def test_without_tracer_the_call_still_returns_two(oracle_engine):
    U, V, Cl, c, times, lat, lon = _fields()
    r = dropin.parcel_propagation(U, V, timestep=-3600, SETTLS_order=1, cyclic_xboundary=True, verbose=False, interp_order=1)
    assert len(r) == 2 and r[0].dims == ("latitude", "longitude")
    r = dropin.parcel_propagation(U, V, timestep=-3600, SETTLS_order=1, cyclic_xboundary=True, verbose=False, interp_order=1,
                                  return_traj=True, C=None)
    assert len(r) == 2 and r[0].dims == ("time", "latitude", "longitude")
