"""The reference-shaped surfaces on a field that has the +-180 meridian in its interior: config 1's vortex evaluated on
0 ... 358 longitudes (``flows.ideal_vortex`` with ``lon_min=0, lon_max=360``).

The reference wraps at a hard-coded +-180 whatever the field's longitudes are (Q7, LCS/trajectory.py:93-94,119-120): a
parcel that passes 180 is rewritten to a negative longitude and its next sample goes through scipy's ``wrap`` map with an
index a period below zero.  Two vortex centres: config 1's own (-55, -20), whose far field alone reaches the grid, and
(180, -20), which puts the vortex core and its wake across the wrap.

- Drop-in (``LCS(...)(ds, isglobal=True, interp_to_common_grid=False, truncation=None)``, ``parcel_propagation(...,
  cyclic_xboundary=True, return_traj=True)``): float64 against the oracle at the tolerances tests/test_dropin_gpu.py uses
  for config 1 (1e-9 degrees, sigma to 1e-7), float32 inside the float32 oracle's band.
- ``lcs_host`` against ``Engine.prepare_field`` + ``Engine.lcs`` bit for bit, as tests/test_host_routes_gpu.py does.

The default ``isglobal=True`` form (regrid to -180 ... 179.5) is not covered here: the source range decides which targets
are NaN."""
import functools

import numpy as np
import pandas as pd
import pytest

from lagrangiancoherence_amd import flows
from tests import _seam as S
from tests import labelled
from tests._fullsize import band, lon_err, positions_check

pytestmark = pytest.mark.gpu
DT, K = -6 * 3600, 4
CENTRES = (-55, 180)
# float32 band floors (median, p99, max): 1, 2 and 16 ulp of a float32 longitude in [256, 512), where an unwrapped
# longitude of this grid lives (3.05e-5 degrees)
ULP = 2.0 ** -15
FLOORS = (ULP, 2 * ULP, 16 * ULP)


@functools.lru_cache(maxsize=None)
def _vortex(centre, dtype):
    cfg = dict(flows.vortex_config_subtropical, lon_min=0, lon_max=360, center=[centre, -20])
    u, v, lat, lon = flows.ideal_vortex(**cfg)
    assert lon[0] == 0 and lon[-1] == 358 and lon.size == 180
    return tuple(np.ascontiguousarray(a, dtype=dtype) for a in (u, v, lat, lon))


@functools.lru_cache(maxsize=None)
def _oracle(centre, order, arith):
    """(traj_x, traj_y, sigma, near-seam mask) of the oracle on the float32- or float64-valued inputs in `arith`."""
    from oracle import lcs_oracle as O
    a = _vortex(centre, np.float64 if arith == "exact" else np.float32)
    if arith == "float64":
        a = tuple(q.astype(np.float64) for q in a)
    u, v, lat, lon = a
    tx, ty = O.parcel_propagation(u, v, lat, lon, timestep=DT, SETTLS_order=K, interp_order=order, cyclic_xboundary=True,
                                  return_traj=True)
    sig = O.sigma_max(O.flowmap_gradient(tx[-1], ty[-1], lat, lon))
    near = None
    if arith == "float64":
        rx, ry, seam = S.propagate(u, v, lat, lon, lat, lon, DT, K, order, 0, u.shape[0] - 1)
        assert np.array_equal(rx, tx) and np.array_equal(ry, ty)
        near = seam < S.NEAR_SEAM
    return tx, ty, sig, near


def _dataset(centre, dtype):
    u, v, lat, lon = _vortex(centre, dtype)
    times = pd.date_range('2000-01-01', periods=u.shape[0], freq='6h').values
    coords = {'latitude': lat, 'longitude': lon, 'time': times}
    U = labelled.DataArray(u.transpose(1, 2, 0), ['latitude', 'longitude', 'time'], coords, name='u')
    V = labelled.DataArray(v.transpose(1, 2, 0), ['latitude', 'longitude', 'time'], coords, name='v')
    return labelled.Dataset({'u': U, 'v': V})


def _dropin(centre, order, dtype):
    from LagrangianCoherence.LCS import LCS, trajectory
    ds = _dataset(centre, dtype)
    tx, ty = trajectory.parcel_propagation(ds.u, ds.v, timestep=DT, propdim='time', SETTLS_order=K, interp_order=order,
                                           copy=True, return_traj=True, cyclic_xboundary=True, verbose=False)
    eig, xd, yd = LCS.LCS(timestep=DT, timedim='time', SETTLS_order=K, return_dpts=True)(
        ds.copy(), isglobal=True, interp_to_common_grid=False, truncation=None, verbose=False, traj_interp_order=order)
    assert tx.values.dtype == dtype and xd.values.dtype == dtype
    assert np.array_equal(tx.values[-1], xd.values) and np.array_equal(ty.values[-1], yd.values)
    return tx.values, ty.values, eig.values[0]


@pytest.mark.parametrize("order", [1, 3])
@pytest.mark.parametrize("centre", CENTRES)
def test_dropin_float64_on_0_360_longitudes(centre, order):
    tx, ty, sig = _dropin(centre, order, np.float64)
    ox, oy, osig, _ = _oracle(centre, order, "exact")
    if centre == 180:
        assert S.crossed(ox).mean() > 0.01                 # the vortex carries parcels across the wrap
    ex, ey = lon_err(tx, ox).max(), np.abs(ty - oy).max()
    print(f"drop-in 0..358 centre {centre} order {order}: max |dx| {ex:.2e} |dy| {ey:.2e} deg")
    assert ex <= 1e-9 and ey <= 1e-9
    np.testing.assert_allclose(sig, osig, rtol=1e-7)


@pytest.mark.parametrize("order", [1, 3])
@pytest.mark.parametrize("centre", CENTRES)
def test_dropin_float32_on_0_360_longitudes(centre, order):
    from lagrangiancoherence_amd import dropin
    tx, ty, _ = _dropin(centre, order, np.float32)
    o32, o64 = _oracle(centre, order, "float32"), _oracle(centre, order, "float64")
    near = o64[3]
    assert near.mean() <= 0.01, f"{near.sum()} seeds within {S.NEAR_SEAM} degrees of +-180"
    u, v, lat, lon = _vortex(centre, np.float32)
    eng = dropin.get_engine()
    field = eng.prepare_field(u, v, lat, lon, order)
    label = f"drop-in float32 0..358 centre {centre} order {order}"
    keep = positions_check(eng, field, lat, lon, np.arange(lat.size), np.arange(lon.size), tx[-1].astype(np.float64),
                           ty[-1].astype(np.float64), (o32[0][-1], o32[1][-1]), (o64[0][-1], o64[1][-1]), label, FLOORS,
                           interp_order=order, leave_out=near, K=K, timestep=float(DT), t0=0, nsteps=u.shape[0] - 1)
    eg = np.maximum(lon_err(tx, o64[0]), np.abs(ty.astype(np.float64) - o64[1]))[:, keep]
    eo = np.maximum(lon_err(o32[0], o64[0]), np.abs(o32[1].astype(np.float64) - o64[1]))[:, keep]
    band(eg, eo, f"{label} trajectories", *FLOORS)


@pytest.mark.parametrize("order", [1, 3])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_lcs_host_is_the_engine_route_on_0_360_longitudes(dtype, order):
    from lagrangiancoherence_amd.engine import Engine, lcs_host
    u, v, lat, lon = _vortex(180, dtype)
    kw = dict(SETTLS_order=K, interp_order=order, cyclic_xboundary=True)
    out = lcs_host(u, v, lat, lon, float(DT), **kw)
    eng = Engine(0)
    try:
        f = eng.prepare_field(u, v, lat, lon, order, fuse_levels=None if dtype == np.float32 else False)
        r = eng.lcs(f, lat, lon, float(DT), **kw)
        for k in ("x_dep", "y_dep", "sigma"):
            got, want = out[k], r[k].cpu().numpy()
            assert got.dtype == want.dtype == dtype and got.shape == want.shape
            assert np.array_equal(got, want, equal_nan=True), (k, int((got != want).sum()))
    finally:
        eng.close()
    assert np.isfinite(out["x_dep"]).all() and np.isfinite(out["sigma"]).any()
    # ... and both are the oracle's answer (float64), so agreeing is not agreeing on the wrong thing
    if dtype == np.float64:
        ox, oy, _, _ = _oracle(180, order, "exact")
        assert lon_err(out["x_dep"], ox[-1]).max() <= 1e-9 and np.abs(out["y_dep"] - oy[-1]).max() <= 1e-9
