"""Attracting and repelling FTLE in one call on the GPU (``Engine.lcs_bidirectional``, ``lc_advect_series_dirs``,
``LCS.bidirectional``):

  * entry ``[d, w]`` equals ``Engine.lcs`` at ``(-1, +1)[d] * |timestep|`` and start level ``t0 + w * stride`` on the same
    packed field, bit for bit, with the same dispatched kernel -- cyclic and the reference's outer clamp, float32 / float64,
    orders 1 / 3 (and one each of 2, 4, 5), K = 0 / 4, one or several windows, strides 1 / 2, smoothing on / off, both
    tensor layouts;
  * a C3-sized grid (2^23 seeds, float32, order 1, K = 4), where the member-pair kernel applies;
  * the outer clamp with one direction leaving the box in a late chunk and the other never leaving it;
  * the drop-in contract: ``bidirectional`` equals the two ``__call__``s (regional float32, the example's global
    ``isglobal=True`` configuration) and the two ``series`` calls;
  * parity with the CPU oracle in both directions, and the memory-capped grouping against one group."""
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


def _same(a, b):
    return np.array_equal(_np(a), _np(b), equal_nan=True)


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


def _check_against_lcs(eng, f, lat, lon, ts, nsteps, n, t0, stride, **kw):
    """Every [d, w] of lcs_bidirectional against its own Engine.lcs; returns (bidirectional's kernel, the single calls')."""
    res = eng.lcs_bidirectional(f, lat, lon, ts, nsteps, n, t0=t0, t0_stride=stride, **kw)
    kern = eng.last_advect_kernel()
    assert tuple(res["sigma"].shape) == (2, n, lat.size, lon.size)
    singles = set()
    for d, sign in ((0, -1.0), (1, 1.0)):
        for w in range(n):
            one = eng.lcs(f, lat, lon, sign * abs(ts), t0=t0 + w * stride, nsteps=nsteps, **kw)
            singles.add(eng.last_advect_kernel())
            for k in ("sigma", "x_dep", "y_dep"):
                assert _same(res[k][d, w], one[k]), (d, w, k)
    return kern, singles


CASES = [(cyc, dt, order, K, n) for cyc in (True, False) for dt in (np.float32, np.float64) for order in (1, 3)
         for K in (0, 4) for n in (1, 4)]


@pytest.mark.parametrize("cyclic,dtype,order,K,n", CASES)
def test_directions_equal_lcs_bit_for_bit(eng, cyclic, dtype, order, K, n):
    i = CASES.index((cyclic, dtype, order, K, n))
    stride, smooth, layout = 1 + (i // 2) % 2, (i // 4) % 2 == 1, ("reference", "physical")[(i // 8) % 2]
    nt, nsteps = 24, 6
    # the non-cyclic cases on a regional box with a strong wind: parcels leave it, so the sub-step phase runs
    u, v, lat, lon = _field(300 + i, nt, dtype=dtype, scale=40.0 if not cyclic else 20.0, regional=not cyclic)
    f = eng.prepare_field(u, v, lat, lon, order)
    kw = dict(SETTLS_order=K, interp_order=order, cyclic_xboundary=cyclic, gauss_sigma=1.5 if smooth else None,
              tensor_layout=layout)
    ts = (-1.0) ** i * 3600.0          # (the sign given does not matter: index 0 is backward, 1 forward)
    kern, singles = _check_against_lcs(eng, f, lat, lon, ts, nsteps, n, 1, stride, **kw)
    if cyclic:
        # the fused launches are lc_advect_series's kernel for the same windows (the single calls' for one window)
        eng.lcs_series(f, lat, lon, ts, nsteps, n, t0=1, t0_stride=stride, **kw)
        assert kern == eng.last_advect_kernel() and (n > 1 or singles == {kern}), (kern, singles)
    else:
        assert kern == "outer_substep_batch_kernel" and "outer_substep_kernel" in singles


@pytest.mark.parametrize("order", [2, 4, 5])
def test_general_orders(eng, order):
    u, v, lat, lon = _field(40 + order, 16, dtype=np.float64)
    f = eng.prepare_field(u, v, lat, lon, order)
    kern, singles = _check_against_lcs(eng, f, lat, lon, 3600.0, 5, 3, 0, 2, SETTLS_order=order - 1, interp_order=order,
                                       cyclic_xboundary=True)
    assert singles == {kern} and kern.startswith("advect_kernel"), kern


def test_large_grid_member_pairs(eng):
    """2^23 seeds (a 2048 x 4096 grid) of the 720 x 1440 float32 record of configs 3-5, order 1, K = 4, three windows: each direction's
    launch pairs windows t0_stride apart in one lane (PATCH_PAIR), as lc_advect_series does."""
    import torch
    from lagrangiancoherence_amd import flows
    nt = 12
    u, v, lat, lon = flows.era5_like(nt=nt)
    slat, slon = flows.seed_grid(2048, 4096, lat, lon, np.float32)
    assert slat.size * slon.size == 1 << 23
    f = eng.prepare_field(u, v, lat, lon, 1)
    kw = dict(SETTLS_order=4, interp_order=1, cyclic_xboundary=True)
    res = eng.lcs_bidirectional(f, slat, slon, 3600.0, 6, 3, t0=0, t0_stride=2, **kw)
    kern = eng.last_advect_kernel()
    assert "lds2" in kern and kern.endswith(", 3>"), kern      # the member-pair patch mode (PATCH_PAIR = 3)
    for d, sign in ((0, -1.0), (1, 1.0)):
        for w in range(3):
            x, y = eng.advect(f, slat, slon, sign * 3600.0, 4, 1, True, t0=2 * w, nsteps=6)
            assert _same(res["x_dep"][d, w], x) and _same(res["y_dep"][d, w], y), (d, w)
    del res, f
    torch.cuda.empty_cache()


def _one_way_wind(dtype, nt=40, ny=19, nx=61):
    """A regional box, calm up to level 20, then a 30 m/s eastward wind (about one degree per hour) in its eastern 8
    degrees only: going forward (timestep > 0) those parcels leave through the east edge in the second chunk of 16 levels;
    going backward they drift west into the calm part, 22 degrees from the west edge, and never leave."""
    lat = np.linspace(10.0, 19.0, ny).astype(dtype)
    lon = np.linspace(-70.0, -40.0, nx).astype(dtype)
    rng = np.random.default_rng(5)
    u = np.zeros((nt, ny, nx))
    v = 0.3 * rng.standard_normal((nt, ny, nx))
    east = lon > -48.0
    u[20:, :, east] = 30.0 + 2.0 * rng.standard_normal((nt - 20, ny, int(east.sum())))
    return u.astype(dtype), v.astype(dtype), lat, lon


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_outer_clamp_one_direction_leaves_late(eng, dtype):
    u, v, lat, lon = _one_way_wind(dtype)
    f = eng.prepare_field(u, v, lat, lon, 1)
    nsteps = 36          # chunks of 16 levels: the east columns leave in the second chunk going forward
    # (SETTLS_order = 0: Euler steps, displacement dt * u, so the two directions move every parcel the opposite ways; the
    # SETTLS bracket's extrapolation 2 u[t] - u[t + 1] would push the east columns out backward too at the calm/windy switch)
    res = eng.lcs_bidirectional(f, lat, lon, 3600.0, nsteps, 1, SETTLS_order=0, interp_order=1, cyclic_xboundary=False)
    assert eng.last_advect_kernel() == "outer_substep_batch_kernel"
    left = {}
    for d, sign in ((0, -1.0), (1, 1.0)):
        x, y = eng.advect(f, lat, lon, sign * 3600.0, 0, 1, False, t0=0, nsteps=nsteps)
        left[d] = eng.last_advect_kernel() == "outer_substep_kernel"
        assert _same(res["x_dep"][d, 0], x) and _same(res["y_dep"][d, 0], y), d
    assert left == {0: False, 1: True}, left


def test_parity_with_the_oracle_both_directions(eng):
    from oracle import lcs_oracle as O
    u, v, lat, lon = _field(11, 10, dtype=np.float64)
    f = eng.prepare_field(u, v, lat, lon, 1, fuse_levels=False)
    res = eng.lcs_bidirectional(f, lat, lon, 3600.0, 9, 1, SETTLS_order=2, interp_order=1, cyclic_xboundary=True)
    for d, sign in ((0, -1.0), (1, 1.0)):
        s, x, y = O.lcs(u, v, lat, lon, timestep=sign * 3600.0, SETTLS_order=2, interp_order=1, cyclic_xboundary=True)
        np.testing.assert_allclose(_np(res["x_dep"][d, 0]), x, rtol=0, atol=POS_ATOL64)
        np.testing.assert_allclose(_np(res["y_dep"][d, 0]), y, rtol=0, atol=POS_ATOL64)
        np.testing.assert_allclose(_np(res["sigma"][d, 0]), s, rtol=1e-7)


@pytest.mark.parametrize("cyclic", [True, False])
def test_memory_capped_groups_give_the_bits_of_one_group(eng, cyclic):
    u, v, lat, lon = _field(21, 30, dtype=np.float32, scale=40.0 if not cyclic else 20.0, regional=not cyclic)
    f = eng.prepare_field(u, v, lat, lon, 3)
    kw = dict(SETTLS_order=2, interp_order=3, cyclic_xboundary=cyclic)
    whole = eng.lcs_bidirectional(f, lat, lon, 3600.0, 18, 5, t0=0, t0_stride=2, **kw)
    per = (5 if cyclic else 9) * 2 * lat.size * lon.size * 4        # a window counts both directions' planes
    try:
        for g in (1, 2):
            eng.SERIES_MEM_CAP = g * per
            assert eng.series_group(np.float32, 2 * lat.size * lon.size, 5, cyclic) == g
            part = eng.lcs_bidirectional(f, lat, lon, 3600.0, 18, 5, t0=0, t0_stride=2, **kw)
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


def _tuple(r):
    return r if isinstance(r, tuple) else (r,)


def _check_calls(ds, ctor, call, window=None, stride=1):
    from LagrangianCoherence.LCS.LCS import LCS
    att, rep = LCS(**ctor).bidirectional(ds, window=window, stride=stride, verbose=False, **call)
    for got, sign in ((att, -1), (rep, 1)):
        c = dict(ctor, timestep=sign * abs(ctor["timestep"]))
        if window is None:
            want = LCS(**c)(ds, verbose=False, **call)
        else:
            want = LCS(**c).series(ds, window=window, stride=stride, verbose=False, **call)
        got, want = _tuple(got), _tuple(want)
        assert len(got) == len(want)
        for a, b in zip(got, want):
            assert a.dims == b.dims and np.array_equal(a.values, b.values), sign
            for k in b.coords:
                assert np.array_equal(np.asarray(a.coords[k]), np.asarray(b.coords[k])), (sign, k)
    return att, rep


def _regional_record(nt=12, ny=41, nx=61):
    lat = np.linspace(20.0, 30.0, ny).astype(np.float32)
    lon = np.linspace(-60.0, -45.0, nx).astype(np.float32)
    t = np.arange(nt)[:, None, None]
    yy = lat[None, :, None].astype(np.float64)
    xx = lon[None, None, :].astype(np.float64)
    u = (25.0 + 10.0 * np.sin(0.3 * yy + 0.5 * t) * np.cos(0.2 * xx)) * np.ones((nt, ny, nx))
    v = 6.0 * np.cos(0.25 * xx - 0.4 * t) * np.sin(0.3 * yy) * np.ones((nt, ny, nx))
    times = pd.date_range("2010-01-01", periods=nt, freq="6h").values
    return _labelled(u.astype(np.float32), v.astype(np.float32), lat, lon, times)


REGIONAL_CTOR = dict(timestep=-6 * 3600, timedim="time", SETTLS_order=4,
                     subdomain={"latitude": slice(21.0, 29.0), "longitude": slice(-58.0, -47.0)}, return_dpts=True)


def test_dropin_regional_float32_equals_the_two_calls():
    """Regional float32 record, SETTLS 4, order 3, non-cyclic (the outer clamp: the jet pushes parcels out of the box going
    forward), subdomain, return_dpts: bit for bit against the two __call__s."""
    att, rep = _check_calls(_regional_record(), REGIONAL_CTOR, dict(s=1e5, traj_interp_order=3))
    assert att[0].values.dtype == np.float32 and att[1].dims == ("latitude", "longitude")


def test_dropin_window_form_equals_the_two_series_calls():
    ds = _regional_record()
    att, rep = _check_calls(ds, REGIONAL_CTOR, dict(s=1e5, traj_interp_order=3), window=8, stride=2)
    assert att[0].shape[0] == rep[0].shape[0] == 3


def test_dropin_example_global_config_equals_the_two_calls():
    """The reference example's pair (examples/ideal_vortex.py:280-288): config 1, isglobal=True (0.5 degree regrid and
    T20), SETTLS 4, order 3, float64."""
    from lagrangiancoherence_amd import flows
    u, v, lat, lon = flows.config1()
    times = pd.date_range("2000-01-01", periods=u.shape[0], freq="6h").values
    ds = _labelled(u, v, lat, lon, times)
    att, rep = _check_calls(ds, dict(timestep=6 * 3600, timedim="time", SETTLS_order=4), dict(isglobal=True))
    assert att.coords["time"][0] == times[0] and rep.coords["time"][0] == times[-1]
