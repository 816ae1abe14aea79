"""Vorticity, LAVD, rotation and path length on the GPU (``lc_vorticity``, ``lc_lavd_update``, ``Engine.vorticity``,
``Engine.lavd_update``, ``Engine.lavd``, ``LCS.lavd``, ``tools.relative_vorticity``).

The expected value never comes from the engine.  The kernels are judged by the numpy restatements of the two definitions in
``np.longdouble`` (tests/lavd.py), run on the very float32 / float64 inputs the kernels are given, within E = 8 x the largest
difference between the restatement in the kernel's dtype and in longdouble on the same inputs (4 eps x the output's scale where
that difference is 0).  ``level_mean`` is the mean of omega as it is rounded to the dtype -- it is what is subtracted from that
omega --, so its bound, 8 eps64 x sum |w omega| / sum w, is held against the longdouble mean of the omega the call returns with
``deviation='none'``; the other modes must return the same bits.  The pipeline is judged by the CPU chain: the oracle's
trajectories, the numpy vorticity, the oracle's ``xr_map_coordinates`` and the numpy fold.

Measured on an MI355X (this file's own prints): the docstrings of the tests have the figures."""
import numpy as np
import pandas as pd
import pytest

from tests import fsle as F
from tests import labelled
from tests import lavd as L

pytestmark = pytest.mark.gpu

# (4, 4) the minimum, (5, 7) smaller than a workgroup, (33, 130) several workgroups with remainders both ways, (19, 36) on
# -90 .. 90: both pole rows
GRIDS = [((4, 4), False), ((5, 7), False), ((33, 130), False), ((19, 36), True)]
GIVEN = {1: [3e-7], 3: [3e-7, -1e-6, 0.0]}
NAMES = {np.float32: "float", np.float64: "double"}


@pytest.fixture(scope="module")
def eng():
    from lagrangiancoherence_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _np(t):
    return t.detach().cpu().numpy()


def _vort_name(dtype, deviation):
    T = NAMES[dtype]
    return f"vorticity_kernel<{T}>+vorticity_finish_kernel<{T}>" + ("" if deviation == "none" else f"+vorticity_subtract_kernel<{T}>")


_WINDS = {}


def _wind(grid, poles, nt, dtype):
    key = (grid, poles, nt, dtype)
    if key not in _WINDS:
        _WINDS[key] = L.wind_case(*grid, nt, dtype, poles)
    return _WINDS[key]


def _check_vorticity(eng, u, v, lat, lon, dtype, cyclic, deviation, what):
    """One call against the judge: the NaN pattern, every node within E, the kernel's name.  Returns the engine's arrays."""
    box = (lat[0], lat[-1], lon[0], lon[-1])
    mine = L.vorticity(u, v, *box, dtype, cyclic, deviation)
    judge = L.vorticity(u, v, *box, np.longdouble, cyclic, deviation)
    E = L.error_measure(mine["omega"], judge["omega"], dtype, L.vorticity_scale(u, v, *box))
    res = eng.vorticity(u, v, lat, lon, cyclic=cyclic, deviation=deviation, dtype=dtype)
    assert eng.last_vorticity_kernel() == _vort_name(dtype, deviation if isinstance(deviation, str) else "given")
    om, mean = _np(res["omega"]), _np(res["level_mean"])
    assert om.dtype == dtype and om.shape == u.shape and mean.dtype == np.float64 and mean.shape == (u.shape[0],)
    assert np.array_equal(np.isnan(om), np.isnan(judge["omega"])), what
    err = np.nanmax(np.abs(om.astype(np.longdouble) - judge["omega"])) if np.isfinite(om).any() else 0.0
    print(f"vorticity {what}: E {E:.2e}, largest error {float(err):.2e} ({float(err) / E:.3f} E)")
    assert err <= E, (what, float(err), E)
    return om, mean


@pytest.mark.parametrize("grid,poles", GRIDS)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_vorticity_against_longdouble(eng, dtype, grid, poles):
    """nt 1 and 3, cyclic and not, the three deviation modes: every node within E, the judge's NaN pattern (none here),
    ``level_mean`` within 8 eps64 x sum |w omega| / sum w of the longdouble mean of the returned omega and the same bits in every
    mode, the kernels' names, two runs bit for bit.  Measured on an MI355X over the 96 calls: E 1.2e-11 to 7.8e-11 1/s in float32
    and 3.6e-20 to 2.0e-19 in float64; the largest error 0.125 E to 0.166 E (at the worst node of nearly every case the kernel
    gives the bits of the numpy restatement in its dtype); ``level_mean`` off by at most 0.091 of its bound."""
    for nt in (1, 3):
        u, v, lat, lon = _wind(grid, poles, nt, dtype)
        box = (lat[0], lat[-1], lon[0], lon[-1])
        for cyclic in (True, False):
            what = f"{np.dtype(dtype).name} {grid} nt={nt} cyclic={cyclic}"
            om, mean = _check_vorticity(eng, u, v, lat, lon, dtype, cyclic, "none", what + " none")
            # the mean of the omega the call returned, in longdouble
            pole_rows = L.vorticity(u, v, *box, dtype, cyclic, "none")["pole_rows"]
            w = np.broadcast_to(np.cos(np.longdouble(L.K) * L.row_latitudes(lat[0], lat[-1], grid[0])[0].astype(np.longdouble))[None, :, None], om.shape).copy()
            w[:, pole_rows, :] = 0
            counted = np.isfinite(om) & (w != 0)
            prod = np.where(counted, w * om.astype(np.longdouble), 0)
            s1 = np.where(counted, w, 0).sum(axis=(1, 2))
            bound = 8 * np.finfo(np.float64).eps * np.abs(prod).sum(axis=(1, 2)) / s1
            off = np.abs(mean.astype(np.longdouble) - prod.sum(axis=(1, 2)) / s1)
            print(f"level_mean {what}: off by {float((off / bound).max()):.3f} of the bound")
            assert np.all(off <= bound), (what, off, bound)
            kept = {}
            for deviation in ("domain", GIVEN[nt]):
                om_d, mean_d = _check_vorticity(eng, u, v, lat, lon, dtype, cyclic, deviation, what + f" {deviation}")
                assert np.array_equal(mean_d, mean)
                sub = mean if isinstance(deviation, str) else np.asarray(deviation)
                assert np.array_equal(om_d, (om.astype(np.float64) - sub[:, None, None]).astype(dtype))
                kept[str(deviation)] = om_d
            again = eng.vorticity(u, v, lat, lon, cyclic=cyclic, deviation="domain", dtype=dtype)
            assert np.array_equal(_np(again["omega"]), kept["domain"]) and np.array_equal(_np(again["level_mean"]), mean)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_vorticity_nan_pattern_is_the_judges(eng, dtype):
    """One NaN in u at a corner, one on the seam column, one beside a pole row (and one in v on the seam column, whose stencil
    crosses the seam): NaN at the nodes whose stencil holds one and nowhere else, every other node within E, the pole row's mean
    over the finite nodes.  Measured on an MI355X: the judge's pattern in all 16 calls, the largest error 0.125 E to 0.126 E."""
    for grid, poles in (((19, 36), True), ((33, 130), False)):
        u, v, lat, lon = (a.copy() for a in _wind(grid, poles, 3, dtype))
        ny, nx = grid
        u[0, 0, 0] = np.nan                   # a corner
        u[1, ny // 2, nx - 1] = np.nan        # the seam column
        u[2, 2, 5] = np.nan                   # beside the row beside the pole row: reaches that row
        u[2, ny - 2, 9] = np.inf              # beside the last (pole) row
        v[1, 3, 0] = np.nan                   # the seam column: reaches column nx - 1 on a cyclic grid
        for cyclic in (True, False):
            for deviation in ("none", "domain"):
                om, mean = _check_vorticity(eng, u, v, lat, lon, dtype, cyclic, deviation, f"NaN {np.dtype(dtype).name} {grid} cyclic={cyclic} {deviation}")
                assert np.isnan(om).sum() >= 7 and np.all(np.isfinite(mean))
                assert np.isnan(om[1, 3, nx - 1]) == cyclic and np.isnan(om[1, 3, 1])
                if poles:
                    assert np.all(np.isfinite(om[:, [0, ny - 1], :]))
    nothing = eng.vorticity(u * np.nan, v, lat, lon, dtype=dtype)
    assert np.isnan(_np(nothing["level_mean"])).all() and np.isnan(_np(nothing["omega"])).all()


def test_relative_vorticity_tool_sorts_and_labels(eng):
    from LagrangianCoherence.LCS import tools
    u, v, lat, lon = _wind((33, 130), False, 3, np.float64)
    times = pd.date_range("2010-01-01", periods=3, freq="6h").values
    coords = {"latitude": lat[::-1], "longitude": lon, "time": times}
    U = labelled.DataArray(u[:, ::-1].transpose(1, 2, 0), ["latitude", "longitude", "time"], coords, name="u")
    V = labelled.DataArray(v[:, ::-1].transpose(1, 2, 0), ["latitude", "longitude", "time"], coords, name="v")
    out = tools.relative_vorticity(U, V, cyclic=True)
    assert out.dims == ("time", "latitude", "longitude") and out.name == "vorticity" and isinstance(out, labelled.DataArray)
    assert np.array_equal(np.asarray(out.coords["latitude"]), lat) and np.array_equal(np.asarray(out.coords["time"]), times)
    assert np.array_equal(out.values, _np(eng.vorticity(u, v, lat, lon, cyclic=True, deviation="none")["omega"]))
    plane = tools.relative_vorticity(U.isel(time=1), V.isel(time=1), cyclic=True, deviation="domain")
    assert plane.dims == ("latitude", "longitude")
    assert np.array_equal(plane.values, _np(eng.vorticity(u[1:2], v[1:2], lat, lon, cyclic=True)["omega"])[0])


# ------------------------------------------------------------------ the fold
FOLD_SHAPES = [(1, 1), (7, 5), (33, 130), (1, 257)]
TS = -900.0


def _fold_errors(got, tx, ty, c, dtype):
    """The three outputs against the judge, each within its own E; returns the errors in units of E."""
    mine = L.fold(tx, ty, c, TS, dtype)
    judge = L.fold(tx, ty, c, TS, np.longdouble)
    out = []
    for k, name in ((1, "lavd"), (2, "rotation"), (3, "length")):
        E = L.error_measure(mine[k], judge[k], dtype, np.abs(judge[k]).max())
        err = float(np.abs(got[name].astype(np.longdouble) - judge[k]).max())
        assert err <= E, (name, err, E)
        out.append(err / E)
    return out


@pytest.mark.parametrize("shape", FOLD_SHAPES)
@pytest.mark.parametrize("n_levels", [2, 5, 17])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_fold_against_longdouble(eng, dtype, n_levels, shape):
    """Random walks that cross the seam and pass within a degree of a pole: lavd, rotation and length within E of the longdouble
    restatement; without c the same length bits and nothing else.  Measured on an MI355X over the 24 cases: every output's
    largest error between 0.123 E and 0.125 E (float32's short sine and arcsine included)."""
    tx, ty, c = L.walk_case(n_levels, shape, dtype)
    res = eng.lavd_update(tx, ty, c, TS, 0, final=True)
    assert eng.last_lavd_kernel() == f"lavd_update_kernel<{NAMES[dtype]}, true>"
    got = {k: _np(res[k]) for k in ("lavd", "rotation", "length")}
    assert all(a.dtype == dtype and a.shape == shape for a in got.values()) and tuple(res["acc"].shape) == (3, *shape)
    rel = _fold_errors(got, tx, ty, c, dtype)
    print(f"fold {np.dtype(dtype).name} {n_levels} levels {shape}: errors {rel[0]:.3f} E, {rel[1]:.3f} E, {rel[2]:.3f} E")
    acc = _np(res["acc"])
    assert all(np.array_equal(acc[k].astype(dtype), got[n]) for k, n in enumerate(("lavd", "rotation", "length")))
    only = eng.lavd_update(tx, ty, None, TS, 0, final=True)
    assert eng.last_lavd_kernel() == f"lavd_update_kernel<{NAMES[dtype]}, false>"
    assert only["lavd"] is None and only["rotation"] is None and np.array_equal(_np(only["length"]), got["length"])
    assert np.array_equal(_np(only["acc"])[:2], np.zeros((2, *shape)))
    assert "lavd" not in eng.lavd_update(tx, ty, c, TS, 0)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_fold_hand_worked_records(eng, dtype):
    for tx, ty, c, dt, (lavd, rot, length) in L.hand_cases():
        res = eng.lavd_update(tx.astype(dtype), ty.astype(dtype), c.astype(dtype), dt, 0, final=True)
        tol = 64 * np.finfo(dtype).eps
        assert abs(float(_np(res["lavd"])[0, 0]) - lavd) <= tol * lavd and abs(float(_np(res["rotation"])[0, 0]) - rot) <= tol * lavd
        # (the seam step: the argument of the sine is near pi, where one rounding of it is eps pi against a sine of k / 2)
        assert abs(float(_np(res["length"])[0, 0]) - length) <= 8 * np.finfo(dtype).eps * np.pi / (L.K / 2) * length


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_fold_nan_stays_in_its_parcel_and_any_split_gives_the_same_bits(eng, dtype):
    tx, ty, c = L.walk_case(17, (33, 130), dtype)
    dev = [eng.to_device(a, dtype) for a in (tx, ty, c)]
    whole = eng.lavd_update(*dev, TS, 0, final=True)
    clean = {k: _np(whole[k]) for k in ("lavd", "rotation", "length")}
    for block in (1, 3, 5):
        acc = res = None
        for lo in range(0, 16, block):
            hi = min(lo + block, 16)
            res = eng.lavd_update(dev[0][lo:hi + 1], dev[1][lo:hi + 1], dev[2][lo:hi + 1], TS, lo, acc, final=hi == 16)
            acc = res["acc"]
        assert all(np.array_equal(_np(res[k]), clean[k]) for k in clean), block
    assert np.array_equal(_np(acc), _np(whole["acc"]))
    # level0 == 0 overwrites whatever acc held
    acc.fill_(1.0)
    again = eng.lavd_update(*dev, TS, 0, acc, final=True)
    assert again["acc"] is acc and all(np.array_equal(_np(again[k]), clean[k]) for k in clean)
    for where, level, (r, col) in (("c", 4, (2, 3)), ("x", 9, (32, 129)), ("y", 16, (0, 64))):
        bad = {"x": tx, "y": ty, "c": c}
        bad[where] = bad[where].copy()
        bad[where][level, r, col] = np.nan
        res = eng.lavd_update(bad["x"], bad["y"], bad["c"], TS, 0, final=True)
        got = {k: _np(res[k]) for k in clean}
        hit = np.zeros((33, 130), bool)
        hit[r, col] = True
        for k in clean:
            touched = (k != "length") if where == "c" else (k == "length")
            assert np.array_equal(np.isnan(got[k]), hit if touched else np.zeros_like(hit)), (where, k)
            assert np.array_equal(got[k][~hit], clean[k][~hit]) and (touched or np.array_equal(got[k], clean[k])), (where, k)


# ------------------------------------------------------------------ streaming
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_engine_lavd_streams_the_record_in_any_chunking(eng, dtype):
    """A 16-step record on a (24, 48) seed grid: level_chunk 1, 3 and 16 give the same bits in all five outputs, and they are the
    bits of advect_tracer's whole record folded by one lavd_update call."""
    u, v, lat, lon = (a.astype(dtype) for a in F.vortex_record(nt=17))
    assert (lat.size, lon.size) == (24, 48)
    f = eng.prepare_field(u, v, lat, lon, 1)
    om = eng.vorticity(u, v, lat, lon, cyclic=True)["omega"]
    tr = eng.prepare_tracer(om, None, lat, lon, 1, dtype=f.dtype)
    kw = dict(SETTLS_order=2, interp_order=1, cyclic_xboundary=True)
    ts = -21600.0
    rec = eng.advect_tracer(f, tr, lat, lon, ts, return_traj=True, tracer_traj=True, **kw)
    assert tuple(rec["traj_x"].shape) == (17, 24, 48) == tuple(rec["c"].shape)
    ref = eng.lavd_update(rec["traj_x"], rec["traj_y"], rec["c"], ts, 0, final=True)
    ref = {**{k: _np(ref[k]) for k in ("lavd", "rotation", "length")}, "x_dep": _np(rec["x"]), "y_dep": _np(rec["y"])}
    assert np.all(np.isfinite(ref["lavd"])) and ref["lavd"].max() > 0 and ref["length"].max() > 0
    for chunk in (1, 3, 16):
        got = eng.lavd(f, tr, lat, lon, ts, level_chunk=chunk, **kw)
        assert all(np.array_equal(_np(got[k]), ref[k]) for k in ref), chunk
    # a window inside the record, the path length alone, the per-point clamp of a regional run (which streams too)
    a = eng.lavd(f, None, lat, lon, ts, t0=2, nsteps=5, level_chunk=2, SETTLS_order=2, cyclic_xboundary=False, noncyclic_clamp="pointwise")
    _, _, wx, wy = eng.advect(f, lat, lon, ts, t0=2, nsteps=5, return_traj=True, SETTLS_order=2, cyclic_xboundary=False, noncyclic_clamp="pointwise")
    b = eng.lavd_update(wx, wy, None, ts, 0, final=True)
    assert a["lavd"] is None and a["rotation"] is None and np.array_equal(_np(a["length"]), _np(b["length"]))


# ------------------------------------------------------------------ end to end against the oracle chain
E2E_BOUND = 8 * 2.7e-16   # of each output's largest value: 8 x the distance measured (test_end_to_end_against_the_oracle_chain)


def _dataset(u, v, lat, lon, times=None):
    times = pd.date_range("2010-01-01", periods=u.shape[0], freq="15min").values if times is None else times
    coords = {"latitude": lat, "longitude": lon, "time": times}
    U = labelled.DataArray(u.transpose(1, 2, 0), ["latitude", "longitude", "time"], coords, name="u")
    V = labelled.DataArray(v.transpose(1, 2, 0), ["latitude", "longitude", "time"], coords, name="v")
    return labelled.Dataset({"u": U, "v": V}), times


def test_end_to_end_against_the_oracle_chain():
    """LCS.lavd on the moving vortex of tests/test_lavd.py at 1 degree (41 x 51 nodes, 9 levels, float64, interpolation order 1)
    against the CPU chain: the oracle's trajectories, the numpy vorticity, the oracle's xr_map_coordinates, the numpy fold.  The
    bound is relative to max(lavd) (and to the largest rotation and length for those).  Measured on an MI355X: lavd 7.0e-18,
    rotation 7.0e-18, length 2.7e-16 of the largest value; the bound is 8 x the largest of the three, 2.2e-15 (the issue's
    ceiling is 1e-6).  The engine's maximum: 1.978 at (-20, -55) against a median of 0.0272, the oracle chain's to 12 digits."""
    from LagrangianCoherence.LCS.LCS import LCS
    u, v, lat, lon = L.vortex_record(1.0, 9)
    assert (lat.size, lon.size) == (41, 51)
    ds, times = _dataset(u, v, lat, lon)
    lavd, rot, length, x_dep, y_dep = LCS(return_dpts=True, **L.PHYSICAL).lavd(ds, traj_interp_order=1, level_chunk=3, verbose=False)
    for a, name in ((lavd, "lavd"), (rot, "rotation"), (length, "path_length")):
        assert a.dims == ("time", "latitude", "longitude") and a.name == name and a.shape == (1, 41, 51) and a.values.dtype == np.float64
        assert np.array_equal(np.asarray(a.coords["time"]), times[[-1]])                    # forward: the window's last time
        assert a.attrs == {"integration_time": 8 * 900.0}
    o_lavd, o_rot, o_len, tx, ty = L.oracle_chain(u, v, lat, lon, order=1, noncyclic_clamp="reference_outer")
    worst = 0.0
    for got, want, what in ((lavd, o_lavd, "lavd"), (rot, o_rot, "rotation"), (length, o_len, "length")):
        rel = float(np.abs(got.values[0] - want).max() / np.abs(want).max())
        print(f"end to end {what}: {rel:.2e} of the largest value")
        worst = max(worst, rel)
        assert rel <= E2E_BOUND, (what, rel)
    np.testing.assert_allclose(x_dep.values[0], tx[-1], rtol=0, atol=F.POS_ATOL64)
    np.testing.assert_allclose(y_dep.values[0], ty[-1], rtol=0, atol=F.POS_ATOL64)
    where, top, median = L.physical_assertions(lavd.values[0], lat, lon)
    print(f"engine LAVD maximum {top:.3f} at {where}, median {median:.4f}; oracle chain {L.physical_assertions(o_lavd, lat, lon)}")
    assert np.all(lavd.values >= np.abs(rot.values))


def test_windows_labels_and_a_backward_run():
    """window=5, stride=2 on the 9 levels: three entries, each bit for bit the one-window call on that slice, labelled as strain
    labels its windows; a backward run is labelled with each window's first time; the subdomain crop is strain's."""
    from LagrangianCoherence.LCS.LCS import LCS
    u, v, lat, lon = L.vortex_record(1.0, 9)
    ds, times = _dataset(u, v, lat, lon)
    lcs = LCS(**L.PHYSICAL)
    out = lcs.lavd(ds, window=5, stride=2, traj_interp_order=1, verbose=False)
    s1 = lcs.strain(ds, window=5, stride=2, traj_interp_order=1, verbose=False)[0]
    assert len(out) == 3
    for a in out:
        assert a.shape == (3, 41, 51) and np.array_equal(np.asarray(a.coords["time"]), np.asarray(s1.coords["time"]))
        assert np.array_equal(np.asarray(a.coords["time"]), times[[4, 6, 8]]) and a.attrs == {"integration_time": 4 * 900.0}
    for w in range(3):
        sl = slice(2 * w, 2 * w + 5)
        one = lcs.lavd(_dataset(u[sl], v[sl], lat, lon, times[sl])[0], traj_interp_order=1, level_chunk=2, verbose=False)
        for a, b in zip(out, one):
            assert np.array_equal(a.values[w], b.values[0]), w
        L.physical_assertions(out[0].values[w], lat, lon)
    sub = {"latitude": slice(-30.0, -10.0), "longitude": slice(-65.0, -45.0)}
    back = LCS(timestep=-900.0, SETTLS_order=2, subdomain=sub, return_dpts=True).lavd(ds, window=5, stride=2, traj_interp_order=1, verbose=False)
    assert len(back) == 5 and np.array_equal(np.asarray(back[0].coords["time"]), times[[0, 2, 4]])
    mlat, mlon = (lat > -30.0) & (lat < -10.0), (lon > -65.0) & (lon < -45.0)
    assert back[0].shape == (3, mlat.sum(), mlon.sum()) and back[3].shape == (3, 41, 51)
    assert np.array_equal(np.asarray(back[2].coords["latitude"]), lat[mlat])
    with pytest.raises(ValueError, match="deviation"):
        lcs.lavd(ds, deviation=[0.0] * 8, verbose=False)
    none = lcs.lavd(ds, deviation="none", traj_interp_order=1, verbose=False)
    given = lcs.lavd(ds, deviation=[0.0] * 9, traj_interp_order=1, verbose=False)
    assert np.array_equal(none[0].values, given[0].values) and not np.array_equal(none[0].values, lcs.lavd(ds, traj_interp_order=1, verbose=False)[0].values)
