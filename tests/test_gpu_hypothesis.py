"""Randomised parity: hypothesis draws grid shapes, seed grids, K, interpolation order, time-step sign,
boundary mode and a start window; the float64 HIP path must agree with the CPU oracle on every draw."""
import numpy as np
import pytest
from hypothesis import HealthCheck, given, settings
from hypothesis import strategies as st

pytestmark = pytest.mark.gpu

# Deterministic draws by default (the same examples on every run); LCS_HYP_RANDOM=1 LCS_HYP_SCALE=10 explores.
import os
_DERAND = not os.environ.get("LCS_HYP_RANDOM")
_SCALE = int(os.environ.get("LCS_HYP_SCALE", "1"))

_ENG = {}


def _engine():
    if "e" not in _ENG:
        from lagrangiancoherence_amd.engine import Engine
        _ENG["e"] = Engine(0)
    return _ENG["e"]


@settings(max_examples=60 * _SCALE, deadline=None, derandomize=_DERAND, suppress_health_check=[HealthCheck.too_slow, HealthCheck.data_too_large])
@given(ny=st.integers(8, 30), nx=st.integers(8, 40), nt=st.integers(2, 5), K=st.integers(0, 4),
       order=st.sampled_from([1, 3]), dt=st.sampled_from([-5400.0, -600.0, 900.0, 7200.0]),
       cyclic=st.booleans(), seeds_on_nodes=st.booleans(), seed=st.integers(0, 2 ** 31 - 1),
       lat_hi=st.sampled_from([60.0, 85.0, 88.0]), scale=st.sampled_from([5.0, 25.0, 80.0]))
def test_float64_advect_and_sigma_match_oracle(ny, nx, nt, K, order, dt, cyclic, seeds_on_nodes, seed, lat_hi, scale):
    from oracle import lcs_oracle as O
    eng = _engine()
    rng = np.random.default_rng(seed)
    lat = np.linspace(-lat_hi, lat_hi, ny)
    lon = -180 + 360.0 / nx * np.arange(nx)
    u = scale * rng.standard_normal((nt, ny, nx))
    v = 0.5 * scale * rng.standard_normal((nt, ny, nx))
    if seeds_on_nodes:
        slat, slon = lat, lon
    else:
        slat = np.linspace(lat[0], lat[-1], int(rng.integers(7, 40)))
        slon = np.linspace(lon[0], lon[-1], int(rng.integers(7, 50)))
    t0 = int(rng.integers(0, nt - 1))
    nsteps = int(rng.integers(1, nt - t0))
    f = eng.prepare_field(u, v, lat, lon, order)
    x, y = eng.advect(f, slat, slon, dt, SETTLS_order=K, interp_order=order, cyclic_xboundary=cyclic, t0=t0,
                      nsteps=nsteps)
    xr_, yr_ = O.parcel_propagation(u, v, lat, lon, timestep=dt, SETTLS_order=K, interp_order=order,
                                    cyclic_xboundary=cyclic, seed_lat=slat, seed_lon=slon, t0=t0, nsteps=nsteps)
    xg, yg = x.cpu().numpy(), y.cpu().numpy()
    # 1e-9 degrees -- or, where this white-noise flow amplifies more than that, what the oracle itself makes of seeds moved
    # by a few ulp of the coordinates (1.4e-14 degrees at 100; measured through a 1e-12 degree shift): the fused-level default
    # rounds differently from numpy (fuse_levels=False does not: tools/repro_hyp_fp64.py, 6e-14 where this form shows 7e-9
    # at a point that a 1e-12 degree shift of the seeds moves by 8e-6)
    xs_, ys_ = O.parcel_propagation(u, v, lat, lon, timestep=dt, SETTLS_order=K, interp_order=order, cyclic_xboundary=cyclic,
                                    seed_lat=slat + 1e-12, seed_lon=slon + 1e-12, t0=t0, nsteps=nsteps)
    sx = np.abs(xs_ - xr_)
    from scipy.ndimage import maximum_filter
    sens = maximum_filter(np.maximum(np.minimum(sx, np.abs(sx - 360.0)), np.abs(ys_ - yr_)), size=3, mode="nearest") * 0.1   # ~7 ulp
    dxg = np.abs(xg - xr_)
    dxg = np.minimum(dxg, np.abs(dxg - 360.0)) if cyclic else dxg
    assert (np.abs(yg - yr_) <= 1e-9 + sens).all(), float(np.abs(yg - yr_).max())
    assert (dxg <= 1e-9 + sens).all(), float(dxg.max())
    if slat.size >= 5 and slon.size >= 5:
        # sigma from the ORACLE's departure points on both sides: isolates the gradient/eigen kernel
        ref = O.sigma_max(O.flowmap_gradient(xr_, yr_, slat, slon))
        sig = eng.sigma(xr_, yr_, slat, slat[1] - slat[0], slon[1] - slon[0]).cpu().numpy()
        ok = np.isfinite(ref)
        np.testing.assert_allclose(sig[ok], ref[ok], rtol=1e-7)


@settings(max_examples=40 * _SCALE, deadline=None, derandomize=_DERAND, suppress_health_check=[HealthCheck.too_slow, HealthCheck.data_too_large])
@given(fny=st.integers(12, 60), fnx=st.integers(20, 120), nt=st.integers(2, 6), K=st.integers(0, 5),
       order=st.sampled_from([1, 3]), dt=st.sampled_from([-3600.0, -900.0, 900.0, 5400.0]), cyclic=st.booleans(),
       sny=st.integers(7, 90), snx=st.integers(7, 130), seed=st.integers(0, 2 ** 31 - 1),
       wind=st.sampled_from([0.5, 1.0, 3.0]))
def test_float32_kernels_agree_with_each_other_and_the_oracle(fny, fnx, nt, K, order, dt, cyclic, sny, snx, seed, wind):
    """float32: the default LDS-tile kernel (common case unconditional + exact redo for flagged lanes, lanes
    without a seed shadowing a neighbour) and the direct-gather kernel share the arithmetic, so on any grid
    shape, seed density, K, boundary mode and wind strength they must agree to float32 rounding, and both must
    sit at float32 distance from the float64 oracle on the same (float32-valued) inputs."""
    import os
    from oracle import lcs_oracle as O
    from lagrangiancoherence_amd import flows
    eng = _engine()
    u, v, lat, lon = flows.era5_like(nt=nt, ny=fny, nx=fnx, seed=seed)
    u, v = (u * np.float32(wind)), (v * np.float32(wind))
    slat, slon = flows.seed_grid(sny, snx, lat, lon)
    f = eng.prepare_field(u, v, lat, lon, order)
    out = {}
    try:
        for flag in ("0", "1", "2"):     # direct gathers, LDS tiles forced to two seeds per lane at order 1, one seed per lane
            eng.set_lds_tiles(int(flag))
            x, y = eng.advect(f, slat, slon, dt, SETTLS_order=K, interp_order=order, cyclic_xboundary=cyclic,
                              noncyclic_clamp="pointwise")     # the fused kernels' own per-point clamp
            out[flag] = (x.cpu().numpy().astype(np.float64), y.cpu().numpy().astype(np.float64))
    finally:
        eng.set_lds_tiles(-1)
    xo, yo = O.parcel_propagation(u.astype(np.float64), v.astype(np.float64), lat.astype(np.float64),
                                  lon.astype(np.float64), timestep=dt, SETTLS_order=K, interp_order=order,
                                  cyclic_xboundary=cyclic, seed_lat=slat.astype(np.float64),
                                  seed_lon=slon.astype(np.float64), noncyclic_clamp="pointwise")

    def dist(a, b, periodic):
        d = np.abs(a - b)
        return np.minimum(d, np.abs(d - 360)) if periodic else d
    assert np.isfinite(out["1"][0]).all() and np.isfinite(out["1"][1]).all()
    # The reference's index map (scale n, 'wrap' with period n-1: Q2/Q3b) jumps at c = n-1.  A seed row or
    # column that starts exactly there (c is rational in the grid sizes) lands on either side depending on
    # the precision of c, in the float32 ORACLE too -- leave those out of the float32-vs-float64 comparison.
    cy0 = fny * (slat.astype(np.float64) - lat[0]) / (lat[-1] - lat[0])
    cx0 = fnx * (slon.astype(np.float64) - lon[0]) / (lon[-1] - lon[0])
    ok = (np.abs(cy0 - (fny - 1)) > 1e-3)[:, None] & (np.abs(cx0 - (fnx - 1)) > 1e-3)[None, :]
    # kernel vs kernel: rounding only (a different contraction here and there), amplified by the flow at worst
    dxk, dyk = dist(out["0"][0], out["1"][0], cyclic)[ok], np.abs(out["0"][1] - out["1"][1])[ok]
    assert np.percentile(dxk, 99) < 2e-4 and np.percentile(dyk, 99) < 2e-4 and dxk.max() < 0.1 and dyk.max() < 0.1
    # kernel vs float64 oracle: float32 distance (the 'order' seed rows at each end use the constant-mode
    # order-1 rule on both sides and are included)
    # the two LDS-tile kernels and the direct kernel share one arithmetic: bit-identical
    assert np.array_equal(out["1"][0], out["2"][0]) and np.array_equal(out["1"][1], out["2"][1])
    for flag in ("0", "1"):
        dx, dy = dist(out[flag][0], xo, cyclic)[ok], np.abs(out[flag][1] - yo)[ok]
        assert np.percentile(dx, 99) < 2e-3 and np.percentile(dy, 99) < 2e-3, (flag, dx.max(), dy.max())
        assert np.median(dx) < 1e-4 and np.median(dy) < 1e-4


@settings(max_examples=30, deadline=None, derandomize=True, suppress_health_check=[HealthCheck.too_slow, HealthCheck.data_too_large, HealthCheck.filter_too_much])
@given(fny=st.integers(12, 60), fnx=st.integers(20, 120), nt=st.integers(2, 6), K=st.integers(0, 5),
       order=st.sampled_from([1, 3]), dt=st.sampled_from([-3600.0, -900.0, 900.0, 5400.0]),
       offset=st.sampled_from([0.0, 90.0, 180.0, 262.5]), sny=st.integers(7, 90), snx=st.integers(7, 130),
       seed=st.integers(0, 2 ** 31 - 1), wind=st.sampled_from([0.5, 1.0, 3.0]))
def test_float32_cyclic_kernels_on_longitudes_that_start_anywhere(fny, fnx, nt, K, order, dt, offset, sny, snx, seed, wind):
    """float32, cyclic, the field's longitudes shifted by `offset` (the wind arrays unchanged: the flow is periodic): the
    reference wraps at a hard-coded +-180 (Q7), which lies inside the field unless it starts at -180.  Whatever kernel a
    lc_ctx_set_lds_tiles setting reaches there, the three settings must agree as on the flow's own longitudes (1 and 2 bit
    for bit, 0 to float32 rounding) and sit at float32 distance from the float64 oracle.  Seeds whose float64 position
    comes within 1e-2 degrees of +-180 at any update are left out (float32 and float64 may wrap them on different
    iterations and then sample two cells apart); a draw that leaves out more than 2 % is discarded."""
    from hypothesis import assume
    from lagrangiancoherence_amd import flows
    from tests import _seam as S
    eng = _engine()
    u, v, lat, lon = flows.era5_like(nt=nt, ny=fny, nx=fnx, seed=seed)
    u, v = (u * np.float32(wind)), (v * np.float32(wind))
    lon = (lon.astype(np.float64) + offset).astype(np.float32)
    slat, slon = flows.seed_grid(sny, snx, lat, lon)
    f64 = [a.astype(np.float64) for a in (u, v, lat, lon, slat, slon)]
    tx, ty, seam = S.propagate(*f64, dt, K, order, 0, nt - 1)     # the float64 oracle, restated to see inside a level
    xo, yo = tx[-1], ty[-1]
    near = seam < S.NEAR_SEAM
    assume(near.mean() <= 0.02)
    f = eng.prepare_field(u, v, lat, lon, order)
    out = {}
    try:
        for flag in (0, 1, 2):
            eng.set_lds_tiles(flag)
            x, y = eng.advect(f, slat, slon, dt, SETTLS_order=K, interp_order=order, cyclic_xboundary=True)
            out[flag] = (x.cpu().numpy().astype(np.float64), y.cpu().numpy().astype(np.float64))
    finally:
        eng.set_lds_tiles(-1)

    def dist(a, b):
        d = np.abs(a - b)
        return np.minimum(d, np.abs(d - 360))
    assert np.isfinite(out[1][0]).all() and np.isfinite(out[1][1]).all()
    # seeds that start exactly on the index map's jump at c = n - 1 are left out, as in the test above
    cy0 = fny * (f64[4] - f64[2][0]) / (f64[2][-1] - f64[2][0])
    cx0 = fnx * (f64[5] - f64[3][0]) / (f64[3][-1] - f64[3][0])
    ok = (np.abs(cy0 - (fny - 1)) > 1e-3)[:, None] & (np.abs(cx0 - (fnx - 1)) > 1e-3)[None, :] & ~near
    assert np.array_equal(out[1][0], out[2][0]) and np.array_equal(out[1][1], out[2][1])
    dxk, dyk = dist(out[0][0], out[1][0])[ok], np.abs(out[0][1] - out[1][1])[ok]
    assert np.percentile(dxk, 99) < 2e-4 and np.percentile(dyk, 99) < 2e-4 and dxk.max() < 0.1 and dyk.max() < 0.1
    for flag in (0, 1):
        dx, dy = dist(out[flag][0], xo)[ok], np.abs(out[flag][1] - yo)[ok]
        assert np.percentile(dx, 99) < 2e-3 and np.percentile(dy, 99) < 2e-3, (flag, offset, dx.max(), dy.max())
        assert np.median(dx) < 1e-4 and np.median(dy) < 1e-4, (flag, offset)


@settings(max_examples=30 * _SCALE, deadline=None, derandomize=_DERAND, suppress_health_check=[HealthCheck.too_slow, HealthCheck.data_too_large])
@given(dtype=st.sampled_from(["float32", "float64"]), order=st.sampled_from([1, 3]), K=st.integers(0, 4),
       lds=st.sampled_from([-1, 0, 1, 2]), sny=st.integers(9, 140), snx=st.integers(9, 150), nt=st.integers(4, 9),
       split=st.integers(1, 7), chunk=st.integers(1, 5), members=st.integers(1, 3), traj=st.booleans(),
       cyclic=st.booleans(), seed=st.integers(0, 2 ** 31 - 1))
def test_continuation_chunks_and_batches_never_change_a_bit(dtype, order, K, lds, sny, snx, nt, split, chunk, members, traj,
                                                              cyclic, seed):
    """lc_advect_from / lc_ctx_set_level_chunk / lc_advect_batch on random grids, kernels, orders, K, boundary modes and
    split points: a series advected in two pieces, in level chunks, or as one member of a batch equals the single call,
    bit for bit, trajectories included (the loop of LCS/trajectory.py:80-126 carries only positions between levels)."""
    from lagrangiancoherence_amd import flows
    eng = _engine()
    u, v, lat, lon = flows.era5_like(nt=nt, ny=36, nx=72, seed=seed)
    slat, slon = flows.seed_grid(sny, snx, lat, lon)
    u, v, lat, lon, slat, slon = (a.astype(dtype) for a in (u * np.float32(1.5), v, lat, lon, slat, slon))
    f = eng.prepare_field(u, v, lat, lon, order)
    nsteps = nt - members                       # member m starts at level m
    split = min(split, nsteps - 1) if nsteps > 1 else 0
    kw = dict(SETTLS_order=K, interp_order=order, cyclic_xboundary=cyclic, noncyclic_clamp="pointwise")
    try:
        eng.set_lds_tiles(lds)
        eng.set_level_chunk(0)
        ref = eng.advect(f, slat, slon, -1800.0, t0=0, nsteps=nsteps, return_traj=traj, **kw)
        if split:
            a = eng.advect(f, slat, slon, -1800.0, t0=0, nsteps=split, return_traj=traj, **kw)
            b = eng.advect(f, slat, slon, -1800.0, t0=split, nsteps=nsteps - split, return_traj=traj, start=(a[0], a[1]), **kw)
            assert bool((b[0] == ref[0]).all()) and bool((b[1] == ref[1]).all())
            if traj:
                assert bool((a[2] == ref[2][:split + 1]).all()) and bool((b[3] == ref[3][split:]).all())
        eng.set_level_chunk(chunk)
        got = eng.advect(f, slat, slon, -1800.0, t0=0, nsteps=nsteps, return_traj=traj, **kw)
        assert all(bool((g == r).all()) for g, r in zip(got, ref))
        if cyclic and members > 1:
            xb, yb = eng.advect_batch(f, slat, slon, -1800.0, members, nsteps, SETTLS_order=K, interp_order=order)
            assert bool((xb[0] == ref[0]).all()) and bool((yb[0] == ref[1]).all())
            eng.set_level_chunk(0)
            xm, ym = eng.advect(f, slat, slon, -1800.0, t0=members - 1, nsteps=nsteps, **kw)
            assert bool((xb[members - 1] == xm).all()) and bool((yb[members - 1] == ym).all())
    finally:
        eng.set_level_chunk(-1)
        eng.set_lds_tiles(-1)


@settings(max_examples=25 * _SCALE, deadline=None, derandomize=_DERAND, suppress_health_check=[HealthCheck.too_slow, HealthCheck.data_too_large])
@given(ny=st.integers(8, 260), nx=st.integers(8, 300), nt=st.integers(1, 3), seed=st.integers(0, 2 ** 31 - 1),
       scale=st.sampled_from([1.0, 37.5, 1e-3]))
def test_float64_cubic_prefilter_matches_scipy_at_any_size(ny, nx, nt, seed, scale):
    """float64 order-3 pack on random grid sizes (both sweeps below / at / above the 64-node limit of the streaming form,
    ragged chunks and row blocks) against scipy.ndimage.spline_filter(mode='mirror') itself: a few last bits of the
    field's scale; pads mirror the coefficients exactly; ext = 2 img[t] - img[t+1] exactly."""
    from scipy.ndimage import spline_filter
    eng = _engine()
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((nt, ny, nx)) * scale
    v = rng.standard_normal((nt, ny, nx)) * scale
    lat = np.linspace(-80.0, 80.0, ny)
    lon = np.linspace(-180.0, 179.0, nx)
    f = eng.prepare_field(u, v, lat, lon, 3)
    img = f.cub.cpu().numpy().reshape(nt, ny + 3, nx + 3, 2)
    assert np.array_equal(eng.prepare_field(u, v, lat, lon, 3, ext_image=False).cub.cpu().numpy().reshape(img.shape), img)   # (no ext image: pads_only_kernel)
    tol = 2e-14 * scale * 6.0
    for t in range(nt):
        for c, w in ((0, u), (1, v)):
            ref = spline_filter(w[t], order=3, mode="mirror")
            assert np.abs(img[t, 1:ny + 1, 1:nx + 1, c] - ref).max() <= tol
    assert np.array_equal(img[:, 0], img[:, 2]) and np.array_equal(img[:, ny + 1], img[:, ny - 1]) and np.array_equal(img[:, ny + 2], img[:, ny - 2])
    assert np.array_equal(img[:, :, 0], img[:, :, 2]) and np.array_equal(img[:, :, nx + 1], img[:, :, nx - 1])
    if nt >= 2:
        ext = f.ext.cpu().numpy().reshape(nt - 1, ny + 3, nx + 3, 2)
        assert np.array_equal(ext, 2.0 * img[:-1] - img[1:])


@settings(max_examples=40 * _SCALE, deadline=None, derandomize=_DERAND, suppress_health_check=[HealthCheck.too_slow, HealthCheck.data_too_large])
@given(ny=st.integers(64, 420), nx=st.integers(64, 900), nt=st.integers(2, 4), seed=st.integers(0, 2 ** 31 - 1),
       scale=st.sampled_from([1e-3, 1.0, 40.0]), wind_f32=st.booleans())
def test_float64_one_pass_prefilter_matches_scipy_on_any_shape(ny, nx, nt, seed, scale, wind_f32):
    """float64 order 3, both axes of 64 nodes or more: the one-pass prefilter (pack.hip: prefilter_fused_stream_kernel -- the
    longitude recursion as a scan across the lanes of a workgroup, 4..12 waves by the line length, halo waves, mirrored halo
    columns, row pieces on an idle chip) against scipy's recursion on every node, pads and the fused-level image included;
    float32 planes in (numpy's promotion of a float32 wind on float64 coordinates) take the same kernel."""
    from oracle import lcs_oracle as O
    eng = _engine()
    rng = np.random.default_rng(seed)
    lat = np.linspace(-80.0, 80.0, ny)
    lon = -180 + 360.0 / nx * np.arange(nx)
    u = scale * rng.standard_normal((nt, ny, nx))
    v = scale * (0.3 + rng.standard_normal((nt, ny, nx)))
    if wind_f32:
        u, v = u.astype(np.float32), v.astype(np.float32)
    f = eng.prepare_field(u, v, lat, lon, 3)
    img = f.cub.cpu().numpy().reshape(nt, ny + 3, nx + 3, 2)
    tol = 2e-14 * float(np.abs(u).max())
    for t in range(nt):
        for k, w in enumerate((u, v)):
            want = O.spline_prefilter_mirror(w[t].astype(np.float64))
            got = img[t, 1:ny + 1, 1:nx + 1, k]
            assert np.abs(got - want).max() <= tol, (t, k, float(np.abs(got - want).max()), tol)
    assert np.array_equal(img[:, 0, 1:nx + 1], img[:, 2, 1:nx + 1]) and np.array_equal(img[:, ny + 2, 1:nx + 1], img[:, ny - 2, 1:nx + 1])
    assert np.array_equal(img[:, :, 0], img[:, :, 2]) and np.array_equal(img[:, :, nx + 2], img[:, :, nx - 2])
    if f.ext is not None:
        ext = f.ext.cpu().numpy().reshape(nt - 1, ny + 3, nx + 3, 2)
        assert np.array_equal(ext, 2.0 * img[:-1] - img[1:])
