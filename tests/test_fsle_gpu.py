"""Finite-size Lyapunov exponents on the GPU (``lc_fsle_update``, ``Engine.fsle_update``, ``Engine.fsle``, ``LCS.fsle``).

The expected value never comes from the engine.  The kernel is judged by the numpy restatement of the definition in
``np.longdouble`` (tests/fsle.py), run on the very float32 / float64 positions the kernel is given; cells are left out where a
separation comes within E of the threshold at some level (E = 8 x the error of the numpy restatement in the kernel's dtype on
the same record), and tau / fsle are held to the bound that E implies (``fsle.bounds``).  The pipeline is judged by the CPU
oracle's ``parcel_propagation(return_traj=True)`` fed to the same restatement.

Measured on an MI355X (this file's own prints): see the docstrings of the float64, float32 and end-to-end tests."""
import numpy as np
import pandas as pd
import pytest

from tests import fsle as F
from tests import labelled

pytestmark = pytest.mark.gpu

SHAPES = list(F.GRIDS)                      # (7, 5) smaller than a patch, (37, 64) / (33, 130) odd remainders and several patches, the lines
KERNEL = {np.float32: "fsle_update_kernel<float, 8>", np.float64: "fsle_update_kernel<double, 8>"}


@pytest.fixture(scope="module")
def eng():
    from lagrangiancoherence_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _np(t):
    return t.detach().cpu().numpy()


_JUDGED = {}


def _judged(shape, dtype, mode, cyclic):
    """The record, the judge's result and the bounds of one case; computed once."""
    key = (shape, dtype, mode, cyclic)
    if key not in _JUDGED:
        tx, ty, lat, lon, thr = F.case(shape, dtype, mode)
        err = F.distance_error(tx, ty, lat, lon, dtype, cyclic)
        J = F.definition(tx, ty, lat, lon, thr, mode, F.TIMESTEP, np.longdouble, cyclic)
        _JUDGED[key] = (tx, ty, lat, lon, thr, err, J, F.bounds(J, 8 * err, np.finfo(dtype).eps, F.TIMESTEP))
    return _JUDGED[key]


def _against_the_judge(eng, shape, dtype, mode, cyclic, max_left_out):
    tx, ty, lat, lon, thr, err, J, B = _judged(shape, dtype, mode, cyclic)
    tau, fs = eng.fsle_update(tx, ty, lat, lon, thr, mode, F.TIMESTEP, 0, cyclic=cyclic)
    assert eng.last_fsle_kernel() == KERNEL[dtype]
    tau, fs = _np(tau), _np(fs)
    assert tau.dtype == dtype and fs.dtype == dtype and tau.shape == (3, *shape) == fs.shape
    assert B["left_out"].mean() <= max_left_out
    R = F.check_against_judge(tau, fs, J, B, F.TIMESTEP)
    print(f"fsle {np.dtype(dtype).name} {shape} {mode} cyclic={cyclic}: numpy distance error {err:.2e}, left out {R['left_out']:.4f}, "
          f"{R['cells']} crossings compared ({R['ambiguous']} with two candidate pairs), tau rel {R['tau_rel']:.2e} "
          f"(bound up to {R['tau_rel_bound']:.2e}), fsle rel {R['fsle_rel']:.2e}")
    return tau, fs, J, B


@pytest.mark.parametrize("cyclic", [True, False])
@pytest.mark.parametrize("mode", ["ratio", "distance"])
@pytest.mark.parametrize("shape", SHAPES)
def test_float64_against_longdouble(eng, shape, mode, cyclic):
    """No cell is left out: the NaN pattern is the judge's everywhere, every crossing lies in the judge's interval and within
    the bound of 8 x numpy's float64 distance error.  Measured on an MI355X over the 20 cases: numpy's distance error 7.9e-16 to
    4.7e-14, no cell left out, no cell with two candidate pairs, tau within 1.4e-13 relative (bounds up to 4.6e-11), fsle 1.4e-13."""
    tau, fs, J, B = _against_the_judge(eng, shape, np.float64, mode, cyclic, 0.0)
    assert np.array_equal(np.isnan(tau), J["pair"] < 0) and np.array_equal(np.isnan(fs), J["pair"] < 0)
    assert B["relevant"].sum(axis=1).max() <= 1               # one candidate pair everywhere: the judge's pair, exactly


@pytest.mark.parametrize("cyclic", [True, False])
@pytest.mark.parametrize("mode", ["ratio", "distance"])
@pytest.mark.parametrize("shape", SHAPES)
def test_float32_against_longdouble(eng, shape, mode, cyclic):
    """The same with the margin 8 x numpy's float32 distance error (the factor covers a kernel that orders the half-angle
    arithmetic differently from numpy); at most 1 % of the cells are left out (tests/test_fsle.py holds the records to that,
    and to between 10 % and 90 % of crossings per threshold, without a device).  Measured on an MI355X over the 20 cases:
    numpy's distance error 4.7e-7 to 2.1e-5 (the pairs whose raw longitude difference is near 360 degrees), 0 to 0.56 % of the
    cells left out, up to 131 of 4620 compared crossings with two candidate pairs, tau within 1.1e-5 relative (bounds up to
    2.3e-2, where d(j) - d(j-1) is small), fsle 1.6e-5."""
    _against_the_judge(eng, shape, np.float32, mode, cyclic, 0.01)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_hand_worked_records(eng, dtype):
    """The hand-worked records of tests/test_fsle.py through the kernel; the tie goes to the E pair."""
    for tx, ty, lat, lon, thr, mode, cyclic in F.hand_cases():
        tx, ty, lat, lon = (a.astype(dtype) for a in (tx, ty, lat, lon))
        thr = F.in_dtype(thr, dtype)
        err = max(F.distance_error(tx, ty, lat, lon, dtype, cyclic), float(np.finfo(dtype).eps))
        J = F.definition(tx, ty, lat, lon, thr, mode, F.TIMESTEP, np.longdouble, cyclic)
        B = F.bounds(J, 8 * err, np.finfo(dtype).eps, F.TIMESTEP)
        tau, fs = (_np(t) for t in eng.fsle_update(tx, ty, lat, lon, thr, mode, F.TIMESTEP, 0, cyclic=cyclic))
        assert not B["left_out"].any()
        F.check_against_judge(tau, fs, J, B, F.TIMESTEP)
    tx, ty, lat, lon, thr = F.tie_case()
    tx, ty, lat, lon = (a.astype(dtype) for a in (tx, ty, lat, lon))
    thr, = F.in_dtype([thr], dtype)
    tau, fs = (_np(t) for t in eng.fsle_update(tx, ty, lat, lon, [thr], "distance", F.TIMESTEP, 0))
    J = F.definition(tx, ty, lat, lon, [thr], "distance", F.TIMESTEP, np.longdouble)
    e_value, n_value = (float(J["pairs"]["fsle"][0, p, 0, 0]) for p in (0, 2))
    assert abs(e_value / n_value - 1) > 0.1
    assert abs(float(fs[0, 0, 0]) / e_value - 1) < 64 * np.finfo(dtype).eps


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_nan_reaches_its_own_cell_and_its_four_neighbours_only(eng, dtype):
    """The NaN is put at the crossing level of cells in the last column, so that it undoes a crossing, and one of the four
    neighbours lies across the seam."""
    tx, ty, lat, lon, thr, err, J0, _ = _judged((37, 64), dtype, "ratio", True)
    clean = [_np(t) for t in eng.fsle_update(tx, ty, lat, lon, thr, "ratio", F.TIMESTEP, 0, cyclic=True)]
    rows = [r for r in range(1, 36) if J0["pair"][0, r, 63] >= 0][:3]
    assert len(rows) == 3
    for r in rows:
        allowed = np.zeros((37, 64), bool)
        for rr, cc in ((r, 63), (r - 1, 63), (r + 1, 63), (r, 62), (r, 0)):
            allowed[rr, cc] = True
        bad = ty.copy()
        bad[int(J0["level"][0, r, 63]), r, 63] = np.nan
        got = [_np(t) for t in eng.fsle_update(tx, bad, lat, lon, thr, "ratio", F.TIMESTEP, 0, cyclic=True)]
        for g, c in zip(got, clean):
            changed = ~((g == c) | (np.isnan(g) & np.isnan(c)))
            assert not changed[:, ~allowed].any() and changed[0, r, 63]
        # and what it gives is the judge's for the record with the NaN in it (NaN pattern included)
        J = F.definition(tx, bad, lat, lon, thr, "ratio", F.TIMESTEP, np.longdouble, True)
        B = F.bounds(J, 8 * F.distance_error(tx, bad, lat, lon, dtype, True), np.finfo(dtype).eps, F.TIMESTEP)
        F.check_against_judge(got[0], got[1], J, B, F.TIMESTEP)


@pytest.mark.parametrize("mode", ["ratio", "distance"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_any_split_into_blocks_gives_the_bits_of_one_block(eng, dtype, mode):
    tx, ty, lat, lon, thr = F.case((33, 130), dtype, mode)
    dev = [eng.to_device(a, dtype) for a in (tx, ty)]
    whole = [_np(t) for t in eng.fsle_update(*dev, lat, lon, thr, mode, F.TIMESTEP, 0, cyclic=True)]
    assert np.isfinite(whole[0]).mean() > 0.1
    for block in (1, 3, 5):
        tau = fs = None
        for lo in range(0, F.N_LEVELS - 1, block):
            hi = min(lo + block, F.N_LEVELS - 1)
            tau, fs = eng.fsle_update(dev[0][lo:hi + 1], dev[1][lo:hi + 1], lat, lon, thr, mode, F.TIMESTEP, lo, tau, fs, cyclic=True)
        assert np.array_equal(_np(tau), whole[0], equal_nan=True) and np.array_equal(_np(fs), whole[1], equal_nan=True), block
    # level0 == 0 overwrites whatever the tensors held
    tau.fill_(1.0), fs.fill_(1.0)
    again = eng.fsle_update(*dev, lat, lon, thr, mode, F.TIMESTEP, 0, tau, fs, cyclic=True)
    assert again[0] is tau and np.array_equal(_np(tau), whole[0], equal_nan=True) and np.array_equal(_np(fs), whole[1], equal_nan=True)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_engine_fsle_streams_the_record_in_any_chunking(eng, dtype):
    """Engine.fsle on a packed field: level_chunk 1, 4 and all steps give the same bits, which are fsle_update's on the
    trajectory of one advect call; entry 0 of a trajectory is the seed grid, of a continued one its start."""
    from lagrangiancoherence_amd import flows
    u, v, lat, lon = (a.astype(dtype) for a in flows.config1())
    f = eng.prepare_field(u, v, lat, lon, 1)
    kw = dict(SETTLS_order=2, interp_order=1, cyclic_xboundary=True)
    ts, thr = -21600.0, [1.2, 1.5, 2.0]
    x, y, tx, ty = eng.advect(f, lat, lon, ts, return_traj=True, **kw)
    assert np.array_equal(_np(tx[0]), np.broadcast_to(lon, (lat.size, lon.size))) and np.array_equal(_np(ty[0]), np.broadcast_to(lat[:, None], (lat.size, lon.size)))
    x3, y3 = eng.advect(f, lat, lon, ts, nsteps=3, **kw)
    _, _, cx, cy = eng.advect(f, lat, lon, ts, t0=3, nsteps=2, start=(x3, y3), return_traj=True, **kw)
    assert np.array_equal(_np(cx[0]), _np(x3)) and np.array_equal(_np(cy[0]), _np(y3)) and np.array_equal(_np(cx[2]), _np(tx[5]))
    ref = [_np(t) for t in eng.fsle_update(tx, ty, lat, lon, thr, "ratio", ts, 0, cyclic=True)]
    assert 0.03 < np.isfinite(ref[0]).mean() < 0.5          # (the oracle's record: 18 %, 9 % and 6 % of the cells cross)
    for chunk in (1, 4, 7, 16):
        got = eng.fsle(f, lat, lon, ts, thr, level_chunk=chunk, **kw)
        assert np.array_equal(_np(got["tau"]), ref[0], equal_nan=True) and np.array_equal(_np(got["fsle"]), ref[1], equal_nan=True), chunk
        assert np.array_equal(_np(got["x_dep"]), _np(x)) and np.array_equal(_np(got["y_dep"]), _np(y)), chunk
    # a window inside the record, final separations, the per-point clamp of a regional run (which streams too)
    d = F.spacing(lat, lon)
    a = eng.fsle(f, lat, lon, ts, [1.3 * d], "distance", t0=2, nsteps=4, level_chunk=3, SETTLS_order=2, cyclic_xboundary=False,
                 noncyclic_clamp="pointwise")
    _, _, wx, wy = eng.advect(f, lat, lon, ts, t0=2, nsteps=4, return_traj=True, SETTLS_order=2, cyclic_xboundary=False,
                              noncyclic_clamp="pointwise")
    b = eng.fsle_update(wx, wy, lat, lon, [1.3 * d], "distance", ts, 0, cyclic=False)
    assert np.array_equal(_np(a["tau"]), _np(b[0]), equal_nan=True) and np.array_equal(_np(a["fsle"]), _np(b[1]), equal_nan=True)


# ------------------------------------------------------------------ end to end against the oracle
def _dataset(u, v, lat, lon):
    times = pd.date_range("2010-01-01", periods=u.shape[0], freq="6h").values
    coords = {"latitude": lat, "longitude": lon, "time": times}
    U = labelled.DataArray(u.transpose(1, 2, 0), ["latitude", "longitude", "time"], coords, name="u")
    V = labelled.DataArray(v.transpose(1, 2, 0), ["latitude", "longitude", "time"], coords, name="v")
    return labelled.Dataset({"u": U, "v": V}), times


def _e2e_check(tau, fs, u, v, lat, lon, thr, mode, order, cyclic, t0, nsteps, what):
    """One window of LCS.fsle against the oracle's record fed to the judge; cells whose margin is below what a position error of
    POS_ATOL64 can move a pair's separation by (plus 8 x numpy's float64 error) are left out, at most 1 %."""
    from oracle import lcs_oracle as O
    tx, ty = O.parcel_propagation(u, v, lat, lon, interp_order=order, cyclic_xboundary=cyclic, return_traj=True, t0=t0, nsteps=nsteps, **F.E2E)
    J = F.definition(tx, ty, lat, lon, thr, mode, F.E2E["timestep"], np.longdouble, cyclic)
    E = F.position_error_margin(J["D"]) + 8 * F.distance_error(tx, ty, lat, lon, np.float64, cyclic)
    B = F.bounds(J, E, np.finfo(np.float64).eps, F.E2E["timestep"])
    assert B["left_out"].mean() <= 0.01 and (J["pair"] >= 0).mean() > 0.1
    R = F.check_against_judge(tau, fs, J, B, F.E2E["timestep"])
    print(f"end to end {what}: E {E:.2e}, left out {R['left_out']:.4f}, {R['cells']} crossings compared, tau rel {R['tau_rel']:.2e} "
          f"(bound up to {R['tau_rel_bound']:.2e}), fsle rel {R['fsle_rel']:.2e}")
    return tx, ty


@pytest.mark.parametrize("order", [1, 3])
def test_end_to_end_global_windows_against_the_oracle(order):
    """LCS.fsle on a global 24 x 48 vortex, 9 levels, float64, three windows of 5 levels, against the oracle's trajectories.
    Measured on an MI355X: E 3.9e-7 to 7.2e-7, no cell left out, 1284 to 1350 crossings per window, tau within 4.8e-14 relative
    (bounds up to 1.9e-4), fsle 4.8e-14."""
    from LagrangianCoherence.LCS.LCS import LCS
    u, v, lat, lon = F.vortex_record()
    ds, times = _dataset(u, v, lat, lon)
    ratios = [1.1, 1.3, 1.6]
    out = LCS(return_dpts=True, **F.E2E).fsle(ds, ratio=ratios, window=5, stride=2, isglobal=True, interp_to_common_grid=False,
                                               truncation=None, traj_interp_order=order, level_chunk=3, verbose=False)
    assert len(out) == 4
    fs, tau, x_dep, y_dep = out
    for a, name in ((fs, "fsle"), (tau, "tau")):
        assert a.dims == ("threshold", "time", "latitude", "longitude") and a.name == name and a.shape == (3, 3, 24, 48)
        assert a.values.dtype == np.float64
        assert np.array_equal(np.asarray(a.coords["threshold"]), ratios) and np.array_equal(np.asarray(a.coords["latitude"]), lat)
        assert np.array_equal(np.asarray(a.coords["longitude"]), lon)
        assert np.array_equal(np.asarray(a.coords["time"]), times[[0, 2, 4]])           # backward: a window's first time
    assert x_dep.dims == ("time", "latitude", "longitude") and x_dep.shape == (3, 24, 48)
    for w in range(3):
        tx, ty = _e2e_check(tau.values[:, w], fs.values[:, w], u, v, lat, lon, ratios, "ratio", order, True, 2 * w, 4,
                            f"global order {order} window {w}")
        np.testing.assert_allclose(x_dep.values[w], tx[-1], rtol=0, atol=F.POS_ATOL64)
        np.testing.assert_allclose(y_dep.values[w], ty[-1], rtol=0, atol=F.POS_ATOL64)
    # final separations, the whole record as one window, forward: the last time labels it
    d = F.spacing(lat, lon)
    fwd = dict(F.E2E, timestep=-F.E2E["timestep"])
    fs, tau = LCS(**fwd).fsle(ds, final_separation=1.3 * d, isglobal=True, interp_to_common_grid=False, truncation=None,
                              traj_interp_order=order, verbose=False)
    assert fs.shape == (1, 1, 24, 48) and np.array_equal(np.asarray(fs.coords["time"]), times[[-1]])
    assert np.array_equal(np.asarray(fs.coords["threshold"]), [1.3 * d])
    assert np.all(tau.values[np.isfinite(tau.values)] > 0)


def test_end_to_end_regional_one_block_and_the_subdomain_crop():
    """A regional record (cyclic_xboundary=False: the reference's outer clamp, which cannot be continued, so Engine.fsle makes one
    advect over all levels and one update), with the strict subdomain crop on fsle and tau and none on the departure points.
    Measured on an MI355X: E 4.9e-5 (parcels clamped at the box's edge come close together), 0.43 % of the cells left out, 3167
    crossings, tau within 1.0e-14 relative."""
    from LagrangianCoherence.LCS.LCS import LCS
    u, v, lat, lon = F.regional_record()
    ds, times = _dataset(u, v, lat, lon)
    ratios = [1.05, 1.15, 1.3]
    sub = {"latitude": slice(7.0, 13.0), "longitude": slice(-55.0, -41.0)}
    whole = LCS(**F.E2E).fsle(ds, ratio=ratios, traj_interp_order=1, verbose=False)
    fs, tau, x_dep, y_dep = LCS(subdomain=sub, return_dpts=True, **F.E2E).fsle(ds, ratio=ratios, traj_interp_order=1, level_chunk=2, verbose=False)
    assert whole[0].shape == (3, 1, 24, 48) and np.array_equal(np.asarray(whole[0].coords["time"]), times[[0]])
    _e2e_check(whole[1].values[:, 0], whole[0].values[:, 0], u, v, lat, lon, ratios, "ratio", 1, False, 0, 8, "regional order 1")
    mlat, mlon = (lat > 7.0) & (lat < 13.0), (lon > -55.0) & (lon < -41.0)
    assert np.array_equal(np.asarray(fs.coords["latitude"]), lat[mlat]) and np.array_equal(np.asarray(fs.coords["longitude"]), lon[mlon])
    assert np.array_equal(fs.values, whole[0].values[:, :, mlat][..., mlon], equal_nan=True)
    assert np.array_equal(tau.values, whole[1].values[:, :, mlat][..., mlon], equal_nan=True)
    assert x_dep.shape == (1, 24, 48) and y_dep.shape == (1, 24, 48)
