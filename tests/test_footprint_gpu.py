"""Footprints on the GPU (``lc_footprint_update``, ``Engine.footprint_update``, ``Engine.footprint``, ``LCS.footprint``,
``tools.trajectory_density``).

The expected value never comes from the engine: it is the numpy restatement of tests/footprint.py (float64 index map,
``np.rint``, ``np.add.at`` into int64) on the very arrays the kernel is given.  Every output is an integer sum, so everything
is compared with ``np.array_equal``, for both kernel forms forced through ``set_footprint_form``, with the kernel's name
asserted.  The float64 maps are the same integers under the same float64 scaling, and are compared as equal too."""
import numpy as np
import pandas as pd
import pytest

from tests import footprint as P
from tests import fsle as F
from tests import labelled
from tests import lavd as L

pytestmark = pytest.mark.gpu

NAMES = {np.float32: "float", np.float64: "double"}
FORMS = {0: "direct", 1: "tile"}
# (1, 1) one parcel, (4, 4) and (5, 7) smaller than a patch, (33, 130) several workgroups with remainders both ways
SHAPES = [(1, 1), (4, 4), (5, 7), (33, 130)]


@pytest.fixture(scope="module")
def eng():
    from lagrangiancoherence_amd.engine import Engine
    e = Engine(0)
    yield e
    e.set_footprint_form(-1)
    e.close()


def _np(t):
    return t if t is None or isinstance(t, np.ndarray) else t.detach().cpu().numpy()


def _host(acc):
    return {k: _np(acc[k]) for k in P.PLANES + ("stats",)}


def _name(form, dtype, has_c):
    return f"footprint_{FORMS[form]}_kernel<{NAMES[dtype]}, {'true' if has_c else 'false'}>"


def _both_forms(eng, dtype, has_c, call):
    """``call()`` under each forced form: the kernel's name, and the host copy of what it returned."""
    out = []
    for form in (0, 1):
        eng.set_footprint_form(form)
        out.append(_host(call()))
        assert eng.last_footprint_kernel() == _name(form, dtype, has_c)
    eng.set_footprint_form(-1)
    return out


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("n_levels", [2, 3, 17])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_kernel_against_the_restatement(eng, dtype, n_levels, shape):
    """The three target grids; the mixed record (cell edges, the seam, other turns of the circle, outside, NaN, +-inf, 1e30,
    values that are not finite or too large) with and without q and c; every parcel in one cell; jumps across the whole grid;
    a compact drift: both forms give the restatement's integers, and the conservation identity holds."""
    q = P.weights_case(shape)
    for gname, g in P.GRIDS.items():
        runs = [("mixed", use_q, use_c) for use_q in (False, True) for use_c in (False, True)]
        runs += [(kind, True, True) for kind in ("one_cell", "jump", "drift")]
        for kind, use_q, use_c in runs:
            tx, ty, c, c_scale = P.KINDS[kind](n_levels, shape, dtype, g)
            qq, cc = (q if use_q else None), (c if use_c else None)
            want = P.fold(tx, ty, g, 0, True, qq, cc, c_scale)
            assert P.conserved(want, n_levels, qq, shape)
            for got in _both_forms(eng, dtype, use_c, lambda: eng.footprint_update(tx, ty, g.lat, g.lon, 0, True, qq, cc, c_scale if use_c else None,
                                                                                   None, g.cyclic)):
                assert P.same(got, want), (gname, kind, use_q, use_c)
                assert P.conserved(got, n_levels, qq, shape)
            if kind == "one_cell":
                assert np.count_nonzero(want["hits"]) == 1 and want["stats"].tolist() == [0, 0, 0, 0]
                assert want["csum"].min() == -(1 << 31) * want["chits"].max()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_position_on_a_cell_edge_goes_to_the_upper_cell(eng, dtype):
    g = P.GRID_HALF
    tx, ty = P.edge_case(dtype)
    want = P.fold(tx, ty, g)
    for got in _both_forms(eng, dtype, False, lambda: eng.footprint_update(tx, ty, g.lat, g.lon, 0, True, cyclic=True)):
        assert P.same(got, want) and P.conserved(got, 3, None, tx.shape[1:])
    assert want["stats"][0] > 0                                            # (the row edges below the first row and above the last)
    # only hits, only mass, only the value planes
    for keep in (("hits",), ("mass",)):
        for got in _both_forms(eng, dtype, False, lambda: eng.footprint_update(tx, ty, g.lat, g.lon, 0, True, cyclic=True, want=keep)):
            assert np.array_equal(got[keep[0]], want["hits"]) and all(got[k] is None for k in P.PLANES if k != keep[0])
    c = np.ones_like(tx)
    for got in _both_forms(eng, dtype, True, lambda: eng.footprint_update(tx, ty, g.lat, g.lon, 0, True, c=c, c_scale=3.0, cyclic=True, want=())):
        assert got["hits"] is None and np.array_equal(got["chits"], want["hits"]) and np.array_equal(got["csum"], 3 * want["hits"])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_any_split_into_blocks_gives_the_same_integers(eng, dtype):
    shape, g = (33, 130), P.GRID_CYCLIC
    q = P.weights_case(shape)
    tx, ty, c, c_scale = P.mixed_case(17, shape, dtype, g)
    want = P.fold(tx, ty, g, 0, True, q, c, c_scale)
    dev = [eng.to_device(a, dtype) for a in (tx, ty, c)]
    for form in (0, 1):
        eng.set_footprint_form(form)
        for block in (1, 2, 5, 16):
            acc = None
            for lo in range(0, 16, block):
                hi = min(lo + block, 16)
                acc = eng.footprint_update(dev[0][lo:hi + 1], dev[1][lo:hi + 1], g.lat, g.lon, lo, hi == 16, q, dev[2][lo:hi + 1], c_scale, acc, True)
            assert P.same(_host(acc), want), (form, block)
        # two runs bit for bit; a given acc is added into, not cleared
        again = eng.footprint_update(*dev[:2], g.lat, g.lon, 0, True, q, dev[2], c_scale, None, True)
        assert P.same(_host(again), want)
        twice = eng.footprint_update(*dev[:2], g.lat, g.lon, 0, True, q, dev[2], c_scale, again, True)
        assert twice is again and all(np.array_equal(_np(twice[k]), 2 * want[k]) for k in P.PLANES + ("stats",))
    eng.set_footprint_form(-1)


def test_the_census_form_counts_what_left_the_window(eng):
    g, shape = P.GRID_REGIONAL, (33, 130)
    eng.set_footprint_form("census")
    tx, ty, c, c_scale = P.drift_case(17, shape, np.float32, g)
    got = _host(eng.footprint_update(tx, ty, g.lat, g.lon, 0, True))
    assert eng.last_footprint_kernel() == _name(1, np.float32, False) and got["stats"].tolist() == [0, 0, 0, 0]     # nothing left
    tx, ty, c, c_scale = P.jump_case(17, shape, np.float32, g)
    got = _host(eng.footprint_update(tx, ty, g.lat, g.lon, 0, True))
    want = P.fold(tx, ty, g)
    assert 0 < got["stats"][2] <= want["hits"].sum() and np.array_equal(got["hits"], want["hits"])
    eng.set_footprint_form(-1)
    with pytest.raises(ValueError, match="form"):
        eng.set_footprint_form(3)


# ------------------------------------------------------------------ Engine.footprint end to end
def _expected_from_advect(eng, f, lat, lon, ts, g, weights, tracer, c_scale, t0, nsteps, kw):
    """The restatement applied to the trajectories Engine.advect returns for the same call (the advect kernels are pinned
    elsewhere), the values sampled by Engine.sample_tracer along them."""
    _, _, tx, ty = eng.advect(f, lat, lon, ts, t0=t0, nsteps=nsteps, return_traj=True, **kw)
    c = None if tracer is None else _np(eng.sample_tracer(tracer, tx, ty, level0=t0, interp_order=kw["interp_order"])[0][0])
    q, wscale = eng.footprint_weights(weights, (lat.size, lon.size))
    return P.fold(_np(tx), _np(ty), g, 0, True, q, c, c_scale), wscale


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_engine_footprint_streams_the_record_in_any_chunking(eng, dtype):
    """A cyclic 16-step record on the 24 x 48 global wind with weights (zeros and a NaN among them) and a tracer: level_chunk 1,
    3 and 16 give the integers of the restatement on advect's whole record; the float64 maps are those integers scaled."""
    u, v, lat, lon = (a.astype(dtype) for a in F.vortex_record(nt=17))
    f = eng.prepare_field(u, v, lat, lon, 1)
    tr = eng.prepare_tracer(u + 0.5 * v, None, lat, lon, 1, dtype=f.dtype)
    g = P.Grid(lat, lon, cyclic=True)
    w = np.cos(np.deg2rad(lat.astype(np.float64)))[:, None] * np.ones((1, lon.size))
    w[::3, ::2] = 0.0
    w[5, 7] = np.nan
    kw = dict(SETTLS_order=2, interp_order=1, cyclic_xboundary=True)
    ts, c_scale = -21600.0, 2.0 ** 20
    want, wscale = _expected_from_advect(eng, f, lat, lon, ts, g, w, tr, c_scale, 0, 16, kw)
    assert P.conserved(want, 17, np.where(np.isnan(w), 0, w), w.shape) and want["hits"].sum() > 0
    for form in (0, 1):
        eng.set_footprint_form(form)
        for chunk in (1, 3, 16):
            got = eng.footprint(f, lat, lon, ts, lat, lon, weights=w, tracer=tr, c_scale=c_scale, level_chunk=chunk, **kw)
            assert P.same(_host(got["acc"]), want), (form, chunk)
    eng.set_footprint_form(-1)
    assert got["grid"][-1] is True and got["wscale"] == wscale and got["half_step"] == 10800.0
    assert np.array_equal(_np(got["residence"]), want["hits"].astype(np.float64) * 10800.0)
    assert np.array_equal(_np(got["mass"]), (want["mass"].astype(np.float64) * wscale) * 10800.0)
    with np.errstate(invalid="ignore"):
        mean = (want["csum"].astype(np.float64) / want["chits"].astype(np.float64)) / c_scale
    assert np.array_equal(_np(got["mean_value"]), mean, equal_nan=True) and np.isnan(mean).any() and np.isfinite(mean).any()
    # the default c_scale; a window inside the record without weights or tracer; into= over two windows is the sum of the two
    auto = eng.footprint(f, lat, lon, ts, lat, lon, tracer=tr, **kw)
    assert auto["c_scale"] == float(1 << 30) / float(np.abs(_np(tr.c1)).max())
    a = eng.footprint(f, lat, lon, ts, lat, lon, t0=2, nsteps=5, level_chunk=2, **kw)
    b = eng.footprint(f, lat, lon, ts, lat, lon, t0=7, nsteps=6, level_chunk=4, **kw)
    wa, _ = _expected_from_advect(eng, f, lat, lon, ts, g, None, None, None, 2, 5, kw)
    wb, _ = _expected_from_advect(eng, f, lat, lon, ts, g, None, None, None, 7, 6, kw)
    assert P.same(_host(a["acc"]), wa) and P.same(_host(b["acc"]), wb) and a["mean_value"] is None
    both = eng.footprint(f, lat, lon, ts, lat, lon, t0=7, nsteps=6, level_chunk=4, into=a, **kw)
    assert both["acc"] is a["acc"] and all(np.array_equal(_np(both["acc"][k]), wa[k] + wb[k]) for k in ("hits", "mass", "stats"))
    assert np.array_equal(_np(both["residence"]), (wa["hits"] + wb["hits"]).astype(np.float64) * 10800.0)
    with pytest.raises(ValueError, match="into"):
        eng.footprint(f, lat, lon, 2 * ts, lat, lon, into=a, **kw)


def test_engine_footprint_on_a_regional_run_with_both_clamps(eng):
    """The regional box: the per-point clamp streams, the default outer clamp takes one block; a coarser target grid that
    does not cover the box, so that entries fall outside."""
    u, v, lat, lon = F.regional_record(nt=9)
    f = eng.prepare_field(u, v, lat, lon, 1)
    glat, glon = np.linspace(5.0, 14.0, 10), np.linspace(-58.0, -40.0, 10)
    g = P.Grid(glat, glon)
    ts = -21600.0
    for clamp in ("pointwise", None):
        kw = dict(SETTLS_order=2, interp_order=1, cyclic_xboundary=False, noncyclic_clamp=clamp)
        want, _ = _expected_from_advect(eng, f, lat, lon, ts, g, None, None, None, 0, 8, kw)
        assert want["stats"][0] > 0 and want["hits"].sum() > 0
        for form in (0, 1):
            eng.set_footprint_form(form)
            for chunk in (1, 3, 8):
                got = eng.footprint(f, lat, lon, ts, glat, glon, level_chunk=chunk, **kw)
                assert P.same(_host(got["acc"]), want) and got["grid"][-1] is False, (clamp, form, chunk)
    eng.set_footprint_form(-1)


# ------------------------------------------------------------------ the labelled surfaces
def _dataset(u, v, lat, lon, extra=None):
    times = pd.date_range("2010-01-01", periods=u.shape[0], freq="15min").values
    coords = {"latitude": lat, "longitude": lon, "time": times}
    mk = lambda a, name: labelled.DataArray(a.transpose(1, 2, 0), ["latitude", "longitude", "time"], coords, name=name)
    return labelled.Dataset({"u": mk(u, "u"), "v": mk(v, "v")}), times, (None if extra is None else mk(extra, "tcwv"))


def test_lcs_footprint_on_labelled_arrays(eng):
    """Receptors from a mask with NaN and 0, weights='area', C= and grid=: the restatement on advect's trajectories under the
    same float64 scaling, compared as equal; dims, coords, time labels and attrs."""
    from LagrangianCoherence.LCS.LCS import LCS
    from lagrangiancoherence_amd import dropin
    from lagrangiancoherence_amd.engine import Engine
    u, v, lat, lon = L.vortex_record(1.0, 9)
    tcwv = 30.0 + 0.1 * u - 0.2 * v
    ds, times, C = _dataset(u, v, lat, lon, tcwv)
    ridge = np.zeros((lat.size, lon.size))
    ridge[10:30:2, 5:45:3] = 1.0
    ridge[12, 8] = np.nan
    ridge[14, 11] = 0.0
    ridge[15, 12] = -2.0
    receptors = labelled.DataArray(ridge, ["latitude", "longitude"], {"latitude": lat, "longitude": lon}, name="ridges")
    glat, glon = np.linspace(-30.0, -12.0, 19), np.linspace(-70.0, -47.0, 24)      # smaller than the receptors' reach
    lcs = LCS(timestep=-900.0, SETTLS_order=2, return_dpts=True)
    residence, carried, x_dep, y_dep = lcs.footprint(ds, receptors=receptors, C=C, grid=(glat, glon), window=5, stride=2, traj_interp_order=1,
                                                     level_chunk=3, verbose=False)
    for a, name in ((residence, "residence"), (carried, "tcwv")):
        assert isinstance(a, labelled.DataArray) and a.dims == ("time", "latitude", "longitude") and a.name == name
        assert a.shape == (3, 19, 24) and a.values.dtype == np.float64
        assert np.array_equal(np.asarray(a.coords["latitude"]), glat) and np.array_equal(np.asarray(a.coords["longitude"]), glon)
        assert np.array_equal(np.asarray(a.coords["time"]), times[[0, 2, 4]])               # backward: each window's first time
        assert a.attrs["integration_time"] == 4 * 900.0
    assert x_dep.shape == (3, 41, 51)
    # the expected value: the engine the drop-in surface uses, its advect and its sampler; the restatement; the same scaling
    e = dropin.get_engine()
    f = e.prepare_field(u, v, lat, lon, 1)
    tr = e.prepare_tracer(tcwv, None, lat, lon, 1, dtype=f.dtype)
    mask = (ridge != 0) & ~np.isnan(ridge)
    assert mask[15, 12] and not mask[12, 8] and not mask[14, 11]
    w = np.where(mask, Engine.seed_cell_areas(lat, lon, 6371000), 0.0)
    c_scale = float(1 << 30) / np.abs(tcwv).max()
    g = P.Grid(glat, glon)
    kw = dict(SETTLS_order=2, interp_order=1, cyclic_xboundary=False)
    out = hits = drop = 0
    for k in range(3):
        want, wscale = _expected_from_advect(e, f, lat, lon, -900.0, g, w, tr, c_scale, 2 * k, 4, kw)
        assert np.array_equal(residence.values[k], (want["mass"].astype(np.float64) * wscale) * 450.0), k
        with np.errstate(invalid="ignore"):
            assert np.array_equal(carried.values[k], (want["csum"].astype(np.float64) / want["chits"].astype(np.float64)) / c_scale, equal_nan=True)
        out, hits, drop = out + int(want["stats"][0]), hits + int(want["hits"].sum()), drop + int(want["stats"][1])
    assert hits > 0 and out > 0
    assert residence.attrs == {"integration_time": 3600.0, "outside_fraction": out / (hits + out), "dropped_values": drop}
    # seconds without weights; a plain array for the receptors; the wind's own grid by default
    secs, none = LCS(timestep=-900.0, SETTLS_order=2).footprint(ds, receptors=ridge, weights=None, traj_interp_order=1, verbose=False)
    assert none is None and secs.shape == (1, 41, 51) and np.array_equal(np.asarray(secs.coords["longitude"]), lon)
    want, _ = _expected_from_advect(e, f, lat, lon, -900.0, P.Grid(lat, lon), mask.astype(np.float64), None, None, 0, 8,
                                    dict(kw, noncyclic_clamp=None))
    assert np.array_equal(secs.values[0], want["hits"].astype(np.float64) * 450.0)
    assert secs.values.sum() + want["stats"][0] * 450.0 == 8 * 900.0 * mask.sum()


def test_trajectory_density_on_trajectories_the_caller_has(eng):
    from LagrangianCoherence.LCS import tools
    g = P.GRID_CYCLIC
    tx, ty, c, _ = P.mixed_case(9, (7, 12), np.float64, g)
    times = pd.date_range("2010-01-01", periods=9, freq="6h").values
    coords = {"time": times, "latitude": np.arange(7.0), "longitude": np.arange(12.0)}
    mk = lambda a, name: labelled.DataArray(a, ["time", "latitude", "longitude"], coords, name=name)
    w = np.abs(np.sin(np.arange(84.0))).reshape(7, 12)
    w[2, 3], w[4, 5] = 0.0, np.nan
    count, mean = tools.trajectory_density(mk(tx, "x"), mk(ty, "y"), g.lat, g.lon, weights=w, values=mk(c, "tcwv"), cyclic=True)
    assert count.dims == ("latitude", "longitude") and count.shape == g.shape and count.name == "residence_count" and mean.name == "tcwv"
    assert np.array_equal(np.asarray(count.coords["latitude"]), g.lat) and np.array_equal(np.asarray(mean.coords["longitude"]), g.lon)
    from lagrangiancoherence_amd.engine import Engine
    q, wscale = Engine.footprint_weights(w, (7, 12))
    c_scale = float(1 << 30) / float(np.abs(c[np.isfinite(c)]).max())
    want = P.fold(tx, ty, g, 0, True, q, c, c_scale)
    assert np.array_equal(count.values, (want["mass"].astype(np.float64) * wscale) * 0.5)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(mean.values, (want["csum"].astype(np.float64) / want["chits"].astype(np.float64)) / c_scale, equal_nan=True)
    plain, none = tools.trajectory_density(tx.astype(np.float32), ty.astype(np.float32), g.lat, g.lon, cyclic=True)
    assert none is None and isinstance(plain, np.ndarray)
    assert np.array_equal(plain, P.fold(tx.astype(np.float32), ty.astype(np.float32), g)["hits"] * 0.5)
