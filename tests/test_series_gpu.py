"""FTLE over sliding windows on the GPU (``Engine.lcs_series``, ``lc_advect_series``, ``lc_sigma_batch``, ``LCS.series``):

  * every window of a series equals ``Engine.lcs`` at its own start level on the same packed field, bit for bit -- cyclic and
    the reference's outer clamp, float32 / float64, orders 1 / 3, K = 0 / 4, forward / backward, start strides 1 / 2,
    smoothing on / off, both tensor layouts;
  * the batched outer clamp with windows that diverge (never leave the box, leave in the first chunk, leave only in a
    later one): each equals its own lc_advect, the ones that never left keep the fused result, three sit within the parity
    suite's tolerance of the oracle;
  * lc_sigma_batch against lc_sigma plane by plane (marching and tile kernels, float32 and float64);
  * the drop-in contract: ``LCS(...).series(ds, window, stride)`` equals the driver's per-window loop bit for bit;
  * the memory-capped grouping gives the bits of one group."""
import numpy as np
import pandas as pd
import pytest

from tests import labelled

pytestmark = pytest.mark.gpu

POS_ATOL64 = 1e-9       # tests/test_gpu_parity.py


@pytest.fixture(scope="module")
def eng():
    from lagrangiancoherence_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _np(t):
    return t.detach().cpu().numpy()


def _field(seed, nt, ny=23, nx=31, dtype=np.float64, scale=20.0, regional=False):
    rng = np.random.default_rng(seed)
    if regional:
        lat = np.linspace(10.0, 30.0, ny).astype(dtype)
        lon = np.linspace(-70.0, -40.0, nx).astype(dtype)
    else:
        lat = np.linspace(-80, 80, ny).astype(dtype)
        lon = (-180 + 360.0 / nx * np.arange(nx)).astype(dtype)
    u = (scale * rng.standard_normal((nt, ny, nx))).astype(dtype)
    v = (0.5 * scale * rng.standard_normal((nt, ny, nx))).astype(dtype)
    return u, v, lat, lon


def _same(a, b):
    return np.array_equal(_np(a), _np(b), equal_nan=True)


CASES = [(cyc, dt, order, K, sign) for cyc in (True, False) for dt in (np.float32, np.float64) for order in (1, 3)
         for K in (0, 4) for sign in (1, -1)]


@pytest.mark.parametrize("cyclic,dtype,order,K,sign", CASES)
def test_series_members_equal_lcs_bit_for_bit(eng, cyclic, dtype, order, K, sign):
    i = CASES.index((cyclic, dtype, order, K, sign))
    stride, smooth, layout = 1 + i % 2, (i // 2) % 2 == 1, ("reference", "physical")[(i // 4) % 2]
    nt, nsteps, n = 24, 6, 5
    # the non-cyclic cases on a regional box with a strong wind: parcels leave it, so the sub-step phase runs
    u, v, lat, lon = _field(100 + i, nt, dtype=dtype, scale=40.0 if not cyclic else 20.0, regional=not cyclic)
    f = eng.prepare_field(u, v, lat, lon, order)
    kw = dict(SETTLS_order=K, interp_order=order, cyclic_xboundary=cyclic, gauss_sigma=1.5 if smooth else None,
              tensor_layout=layout)
    ts = sign * 3600.0
    res = eng.lcs_series(f, lat, lon, ts, nsteps, n, t0=1, t0_stride=stride, **kw)
    assert tuple(res["sigma"].shape) == (n, lat.size, lon.size)
    kern = eng.last_advect_kernel()
    left = False
    for m in range(n):
        one = eng.lcs(f, lat, lon, ts, t0=1 + m * stride, nsteps=nsteps, **kw)
        left |= eng.last_advect_kernel() == "outer_substep_kernel"
        for k in ("sigma", "x_dep", "y_dep"):
            assert _same(res[k][m], one[k]), (m, k)
    if not cyclic:
        assert left and kern == "outer_substep_batch_kernel"


def _diverging_wind(dtype, nt=48, ny=19, nx=61):
    """A regional box (0.5 degree columns), calm in longitude (u = 0: no parcel moves east or west) up to level 24, then a
    strong zonal flow that pushes the columns near the edges out."""
    u, v, lat, lon = _field(9, nt, ny, nx, dtype=dtype, scale=3.0, regional=True)
    u[:25] = 0
    u[25:] = u[25:] * 10 + 40.0
    return u, v, lat, lon


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("order,K", [(1, 1), (3, 4)])
def test_outer_clamp_members_diverge(eng, dtype, order, K):
    """Window m runs 20 steps (two chunks of the fused phase: 16 + 4) from level 2m: windows 0-2 never reach the strong levels,
    3-4 reach them only in their second chunk, 5-7 in their first.  Each equals its own lc_advect; the ones that never left
    keep the fused result (= the per-point clamp's, which coincides where nothing leaves).  At order 1 three windows (never
    left, left in the second chunk, left in the first) sit within the parity suite's tolerances of the oracle."""
    from oracle import lcs_oracle as O
    u, v, lat, lon = _diverging_wind(dtype)
    f = eng.prepare_field(u, v, lat, lon, order)
    n, nsteps, stride, ts = 8, 20, 2, 3600.0
    res = eng.lcs_series(f, lat, lon, ts, nsteps, n, t0=0, t0_stride=stride, SETTLS_order=K, interp_order=order,
                         cyclic_xboundary=False)
    assert eng.last_advect_kernel() == "outer_substep_batch_kernel"
    for m in range(n):
        x, y = eng.advect(f, lat, lon, ts, K, order, False, t0=m * stride, nsteps=nsteps)
        assert (eng.last_advect_kernel() == "outer_substep_kernel") == (m >= 3), m     # which windows left the box
        assert _same(res["x_dep"][m], x) and _same(res["y_dep"][m], y), m
        xp, yp = eng.advect(f, lat, lon, ts, K, order, False, t0=m * stride, nsteps=nsteps, noncyclic_clamp="pointwise")
        if m < 3:
            assert _same(res["x_dep"][m], xp) and _same(res["y_dep"][m], yp), m      # the fused result, kept
        elif m >= 5:
            assert np.abs(_np(res["x_dep"][m]).astype(np.float64) - _np(xp)).max() > 1e-3, m   # the two rules differ
    if order == 3:
        return   # (over these 20 clamped steps of the jet, lc_advect itself leaves the parity band at order 3, K = 4: bits only)
    if dtype == np.float64:
        # against the oracle in numpy's operation order (the two-sample form; the fused-level form differs by rounding)
        fe = eng.prepare_field(u, v, lat, lon, order, fuse_levels=False)
        re_ = eng.lcs_series(fe, lat, lon, ts, nsteps, n, t0=0, t0_stride=stride, SETTLS_order=K, interp_order=order,
                             cyclic_xboundary=False)
        assert eng.last_advect_kernel() == "outer_substep_batch_kernel"
        for m in (1, 3, 6):   # never left, left in the second chunk, left in the first
            xr_, yr_ = O.parcel_propagation(u, v, lat, lon, timestep=ts, SETTLS_order=K, interp_order=order, cyclic_xboundary=False,
                                            noncyclic_clamp="reference_outer", t0=m * stride, nsteps=nsteps)
            np.testing.assert_allclose(_np(re_["x_dep"][m]), xr_, rtol=0, atol=POS_ATOL64)
            np.testing.assert_allclose(_np(re_["y_dep"][m]), yr_, rtol=0, atol=POS_ATOL64)
    else:
        # float32 against the float64 oracle: the float32 oracle's own band, where both oracles agree on the clamp pattern
        u64, v64, lat64, lon64 = (a.astype(np.float64) for a in (u, v, lat, lon))
        for m in (1, 3, 6):
            kw = dict(timestep=ts, SETTLS_order=K, interp_order=order, cyclic_xboundary=False, noncyclic_clamp="reference_outer",
                      t0=m * stride, nsteps=nsteps)
            x32, _ = O.parcel_propagation(u, v, lat, lon, **kw)
            x64, _ = O.parcel_propagation(u64, v64, lat64, lon64, **kw)
            same = np.abs(x32 - x64) < 1e-2      # (a 1-ulp difference can switch a whole row x column cross product)
            eg = np.abs(_np(res["x_dep"][m]).astype(np.float64) - x64)[same]
            eo = np.abs(x32 - x64)[same]
            # the bounds of tests/test_gpu_parity.py::test_advect_noncyclic_reference_outer_float32_and_fast_path
            assert same.mean() > 0.9 and (eg < 1e-2).mean() > 0.97
            assert np.median(eg) <= max(4 * np.median(eo), 1e-5) and np.percentile(eg, 90) < 1e-3


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("nx", [64, 63])
def test_sigma_batch_equals_sigma_per_plane(eng, dtype, nx):
    rng = np.random.default_rng(nx)
    ny, n = 37, 4
    lat = np.linspace(-60, 60, ny).astype(dtype)
    lon = np.linspace(-100, 100, nx).astype(dtype)
    x = (lon[None, None, :] + rng.standard_normal((n, ny, nx))).astype(dtype)
    y = (lat[None, :, None] + rng.standard_normal((n, ny, nx))).astype(dtype)
    dlat, dlon = float(lat[1] - lat[0]), float(lon[1] - lon[0])
    eng.set_sigma_march(1)
    try:
        for cast in ((True, False) if dtype == np.float64 else (True,)):
            for layout in ("reference", "physical"):
                s = eng.sigma_batch(x, y, lat, dlat, dlon, fd_fp32_cast=cast, tensor_layout=layout)
                kb = eng.last_sigma_kernel()
                for m in range(n):
                    one = eng.sigma(x[m], y[m], lat, dlat, dlon, fd_fp32_cast=cast, tensor_layout=layout)
                    ks = eng.last_sigma_kernel()
                    assert _same(s[m], one), (m, cast, layout)
                if dtype == np.float32:
                    assert (kb, ks) == (("sigma_march_batch_kernel_f32", "sigma_march_kernel_f32") if nx % 2 == 0
                                        else ("sigma_batch_kernel_f32", "sigma_kernel_f32"))
                else:
                    tail = "float>" if cast else "double>"
                    assert kb == "sigma_batch_kernel<double, " + tail and ks == "sigma_kernel<double, " + tail
    finally:
        eng.set_sigma_march(-1)


@pytest.mark.parametrize("cyclic", [True, False])
def test_memory_capped_groups_give_the_bits_of_one_group(eng, cyclic):
    u, v, lat, lon = _diverging_wind(np.float32)
    f = eng.prepare_field(u, v, lat, lon, 3)
    kw = dict(SETTLS_order=2, interp_order=3, cyclic_xboundary=cyclic)
    whole = eng.lcs_series(f, lat, lon, 3600.0, 20, 9, t0=0, t0_stride=2, **kw)
    per = (5 if cyclic else 9) * lat.size * lon.size * 4
    assert eng.series_group(np.float32, lat.size * lon.size, 9, cyclic) == 9
    try:
        for g in (1, 2, 4):
            eng.SERIES_MEM_CAP = g * per
            assert eng.series_group(np.float32, lat.size * lon.size, 9, cyclic) == g
            part = eng.lcs_series(f, lat, lon, 3600.0, 20, 9, t0=0, t0_stride=2, **kw)
            for k in ("sigma", "x_dep", "y_dep"):
                assert _same(whole[k], part[k]), (g, k)
    finally:
        del eng.SERIES_MEM_CAP


# ------------------------------------------------------------------ the drop-in contract
def _labelled(u, v, lat, lon, times):
    coords = {"latitude": lat, "longitude": lon, "time": times}
    U = labelled.DataArray(u.transpose(1, 2, 0), ["latitude", "longitude", "time"], coords, name="u")
    V = labelled.DataArray(v.transpose(1, 2, 0), ["latitude", "longitude", "time"], coords, name="v")
    return labelled.Dataset({"u": U, "v": V})


def _slice(ds, a, b):
    return labelled.Dataset({k: ds[k].isel(time=slice(a, b)) for k in ("u", "v")})


def _check_contract(ds, nt, window, stride, ctor, call):
    from LagrangianCoherence.LCS.LCS import LCS
    out = LCS(**ctor).series(ds, window=window, stride=stride, verbose=False, **call)
    out = out if isinstance(out, tuple) else (out,)
    n = (nt - window) // stride + 1
    assert out[0].shape[0] == n
    for w in range(n):
        one = LCS(**ctor)(_slice(ds, w * stride, w * stride + window), verbose=False, **call)
        one = one if isinstance(one, tuple) else (one,)
        assert len(one) == len(out)
        assert np.array_equal(out[0].values[w], one[0].values[0]), w
        assert out[0].coords["time"][w] == one[0].coords["time"][0]
        for k in ("latitude", "longitude"):
            assert np.array_equal(out[0].coords[k], one[0].coords[k])
        for a, b in zip(out[1:], one[1:]):
            assert np.array_equal(a.values[w], b.values), w
    return out


def _driver_record(nt=12, ny=41, nx=61):
    lat = np.linspace(20.0, 30.0, ny).astype(np.float32)
    lon = np.linspace(-60.0, -45.0, nx).astype(np.float32)
    t = np.arange(nt)[:, None, None]
    yy = lat[None, :, None].astype(np.float64)
    xx = lon[None, None, :].astype(np.float64)
    u = (25.0 + 10.0 * np.sin(0.3 * yy + 0.5 * t) * np.cos(0.2 * xx)) * np.ones((nt, ny, nx))
    v = 6.0 * np.cos(0.25 * xx - 0.4 * t) * np.sin(0.3 * yy) * np.ones((nt, ny, nx))
    times = pd.date_range("2010-01-01", periods=nt, freq="6h").values
    return _labelled(u.astype(np.float32), v.astype(np.float32), lat, lon, times), nt


DRIVER_CTOR = dict(timestep=-6 * 3600, timedim="time", SETTLS_order=4,
                   subdomain={"latitude": slice(21.0, 29.0), "longitude": slice(-58.0, -47.0)}, return_dpts=True)


def test_dropin_series_equals_the_per_window_loop_driver_shape():
    """The driver's case (LCS/area_of_influence.py:168-181), shrunk: regional float32 box, SETTLS 4, -6 h, subdomain,
    order 3, non-cyclic (the outer clamp: a strong zonal jet pushes parcels out of the box), return_dpts -- bit for bit."""
    from lagrangiancoherence_amd.dropin import get_engine
    ds, nt = _driver_record()
    out = _check_contract(ds, nt, 8, 1, DRIVER_CTOR, dict(s=1e5, traj_interp_order=3))
    assert get_engine().last_advect_kernel() == "outer_substep_kernel"      # (the last per-window call left the box)
    assert out[0].values.dtype == np.float32 and out[1].shape == (5, 41, 61)


def test_dropin_series_with_resample_matches_the_loop_to_the_first_levels_rounding():
    """The same with resample='3h' (the driver's call).  Window 0 is bit-identical.  A later window's first level is the
    original level in the per-window call but the resampled record's interpolation from the left interval there, which
    differs in the last bit of the float32 input (tests/test_series_host.py::test_resampled_record_sliced_against_resampled_slices);
    everything else is the same arithmetic, so the windows agree to the response to that rounding."""
    from LagrangianCoherence.LCS.LCS import LCS
    ds, nt = _driver_record()
    call = dict(s=1e5, resample="3h", traj_interp_order=3, verbose=False)
    sig, xd, yd = LCS(**DRIVER_CTOR).series(ds, window=8, stride=1, **call)
    assert sig.shape[0] == 5
    for w in range(5):
        s1, x1, y1 = LCS(**DRIVER_CTOR)(_slice(ds, w, w + 8), **call)
        assert sig.coords["time"][w] == s1.coords["time"][0]
        if w == 0:
            assert np.array_equal(sig.values[0], s1.values[0]) and np.array_equal(xd.values[0], x1.values)
        else:
            np.testing.assert_allclose(xd.values[w], x1.values, rtol=0, atol=1e-5)
            np.testing.assert_allclose(yd.values[w], y1.values, rtol=0, atol=1e-5)
            rel = np.abs(sig.values[w] - s1.values[0]) / np.maximum(np.abs(s1.values[0]), 1e-30)
            assert (rel < 1e-3).mean() > 0.99


def test_dropin_series_equals_the_per_window_loop_global_regrid_t20():
    """isglobal=True: the 0.5 degree regrid and the T20 truncation run once on the whole record (level by level), cyclic;
    order 1 (float64 after the regrid: the order-3 pack of a 361-row grid is the documented exception)."""
    from lagrangiancoherence_amd import flows
    u, v, lat, lon = flows.config1()
    nt = 7
    u, v = np.concatenate([u] * 2)[:nt].astype(np.float32), np.concatenate([v] * 2)[:nt].astype(np.float32)
    times = pd.date_range("2000-01-01", periods=nt, freq="6h").values
    ds = _labelled(u, v, lat, lon, times)
    _check_contract(ds, nt, 3, 2, dict(timestep=6 * 3600, timedim="time", SETTLS_order=2),
                    dict(isglobal=True, traj_interp_order=1))
