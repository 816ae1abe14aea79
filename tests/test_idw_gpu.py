"""Inverse-distance weighting on the GPU against tests/idw.py, whose sums are math.fsum's: through Engine.idw_interp and once
through each function of tools.  The smallest shapes that cross every boundary of csrc/idw.hip: 1, 2, 255, 256, 257 and 513
sources (the staging chunk is 256) against 1, 255, 256, 257 and 700 targets (the workgroup is 256), as a grid and as scattered
points; 3000 sources against 40 targets, which splits the sources over five workgroups and combines their partial sums, beside
600 against 40, which does not; float32 and float64 values, 1 and 5 planes (a launch takes 4), the powers 1, 2 and 3.5; both
poles, the seam, longitudes beyond +-180, an antipodal pair, unsorted and descending grids; exact hits, NaN values, NaN
coordinates; bounds of 200 km, 1500 km and one that reaches across a pole, whose counts equal the oracle's integer for integer;
two calls bit for bit on every route; the kernels of every route by name.

The tolerance is tests/idw.py's (``bound_u``, ``bound_w``): (n + K) eps64 times the oracle's own sum(w |z|) / sum(w), n the
contributing sources of that target, K = 8 (E + 1) with E the measured distance in ulp between the device's single weight and
numpy's -- test_the_single_source_weight_is_within_E_ulp_of_numpys measures it again on every run and prints it (-s).  No case is
excluded from a comparison.  Every reference is computed once per case and shared.  The float buffers the module's engine
allocates start as NaN."""
import functools
import math

import numpy as np
import pytest

from tests import idw as IDW
from tests.labelled import DataArray

pytestmark = pytest.mark.gpu

N_SRC = (1, 2, 255, 256, 257, 513)
N_TGT = (1, 255, 256, 257, 700)
POWERS = (1, 2, 3.5)
SEARCH, COMBINE, RANGE = "idw_search_kernel", "idw_search_kernel+idw_combine_kernel", "idw_range_kernel+"


@pytest.fixture(scope="module")
def eng():
    from lagrangiancoherence_amd.engine import Engine
    e = Engine(0)
    e._poison = True
    yield e
    e.close()


def _np(t):
    return t.detach().cpu().numpy()


def _run(eng, x, y, z, xi, yi, **kw):
    """``(u, weight, count)`` as numpy arrays, flat over the targets as the oracle's are."""
    u, w, c = eng.idw_interp(x, y, z, xi, yi, return_weight=True, return_count=True, **kw)
    lead = () if np.ndim(z) == 1 else (np.shape(z)[0],)
    assert u.dtype == getattr(eng.torch, str(np.asarray(z).dtype)) and w.dtype == eng.torch.float64 and c.dtype == eng.torch.int32
    assert tuple(u.shape) == tuple(w.shape) == lead + tuple(c.shape)
    return _np(u).reshape(*lead, -1), _np(w).reshape(*lead, -1), _np(c).reshape(-1)


def _check(got, o, label=""):
    """The device's result against the oracle's: the count integer for integer, NaN where the oracle is NaN, +inf weights where
    it has a hit, 0 where nothing contributes, and everything else within the tolerance.  Prints the largest error in units of
    its bound."""
    u, w, c = got
    assert np.array_equal(c, o["count"])
    assert u.dtype == o["u"].dtype and np.array_equal(np.isnan(u), np.isnan(o["u64"]))
    f = ~np.isnan(o["u64"])
    err, bound = np.abs(u.astype(np.float64) - o["u64"])[f], IDW.bound_u(o, u.dtype)[f]
    assert np.array_equal(np.isposinf(w), np.isposinf(o["weight"])) and np.array_equal(w == 0, o["weight"] == 0)
    g = np.isfinite(o["weight"]) & (o["weight"] > 0)
    werr, wbound = np.abs(w[g] - o["weight"][g]), IDW.bound_w(o)[g]
    with np.errstate(invalid="ignore", divide="ignore"):
        ru = np.nanmax(np.where(bound > 0, err / bound, 0.0), initial=0.0)
        rw = np.nanmax(werr / wbound, initial=0.0)
    print(f"{label}: max |u - oracle| / bound = {ru:.3f}, max |W - oracle| / bound = {rw:.3f}")
    assert (err <= bound).all() and (werr <= wbound).all()


@functools.lru_cache(maxsize=None)
def _shape_case(n_src, n_tgt, grid):
    x, y = IDW.scattered(n_src, 100 + n_src)
    z = IDW.values(None, n_src, 300 + n_src)
    xi, yi = IDW.grid_of(n_tgt) if grid else IDW.scattered(n_tgt, 200 + n_tgt)
    for a in (x, y, xi, yi):             # shared among the tests: left unchanged (z too; it is handed to torch, which warns about
        a.setflags(write=False)          # a read-only array)
    return x, y, z, xi, yi


@functools.lru_cache(maxsize=None)
def _shape_oracle(n_src, n_tgt, grid, p=2):
    return IDW.oracle(*_shape_case(n_src, n_tgt, grid), grid=grid, p=p)


# ------------------------------------------------------------------ chunk and workgroup edges, both target forms
@pytest.mark.parametrize("n_tgt", N_TGT)
@pytest.mark.parametrize("n_src", N_SRC)
def test_every_chunk_and_workgroup_edge_as_a_grid_and_as_scattered_points(eng, n_src, n_tgt):
    for grid in (True, False):
        x, y, z, xi, yi = _shape_case(n_src, n_tgt, grid)
        u = eng.idw_interp(x, y, z, xi, yi, grid=grid)
        assert tuple(u.shape) == ((yi.size, xi.size) if grid else (n_tgt,)) and eng.last_idw_kernel == SEARCH
        got = _run(eng, x, y, z, xi, yi, grid=grid)
        assert np.array_equal(_np(u).ravel(), got[0])                              # with or without the other outputs: the same bits
        _check(got, _shape_oracle(n_src, n_tgt, grid), f"{n_src} -> {n_tgt} {'grid' if grid else 'scattered'}")


def test_the_single_source_weight_is_within_E_ulp_of_numpys(eng):
    """What K is made of (tests/idw.py): with one source the returned sum(w) is the device's weight itself.  Its largest
    distance from numpy's over every single-source pair of this module and the three powers, printed; E is recorded there."""
    worst = {}
    for p in POWERS:
        for n_tgt in N_TGT:
            for grid in (True, False):
                x, y, z, xi, yi = _shape_case(1, n_tgt, grid)
                _, w, _ = _run(eng, x, y, z, xi, yi, grid=grid, power=p)
                want = IDW.weights(IDW.costs(IDW.unit(xi, yi, grid), IDW.unit(x, y)), p)[:, 0]
                worst[p] = max(worst.get(p, 0.0), float(IDW.ulps(w, want).max()))
    print("largest |device weight - numpy weight| in ulp, by power:", worst, "-> E =", max(worst.values()), "recorded:", IDW.E)
    assert max(worst.values()) <= IDW.E


# ------------------------------------------------------------------ dtypes, planes, powers
@pytest.mark.parametrize("p", POWERS)
@pytest.mark.parametrize("n_planes", [1, 5])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_dtypes_planes_and_powers(eng, dtype, n_planes, p):
    x, y = IDW.scattered(257, 21)
    xi, yi = IDW.grid_of(300)
    z = IDW.values(n_planes, 257, 22, dtype)
    got = _run(eng, x, y, z, xi, yi, grid=True, power=p)
    assert eng.last_idw_kernel == SEARCH
    _check(got, IDW.oracle(x, y, z, xi, yi, grid=True, p=p), f"{np.dtype(dtype).name} x {n_planes} planes, p = {p}")
    if n_planes == 5:                                                              # a plane of a stack is the plane on its own
        alone = _run(eng, x, y, z[4], xi, yi, grid=True, power=p)
        assert np.array_equal(alone[0], got[0][4]) and np.array_equal(alone[1], got[1][4])


# ------------------------------------------------------------------ the split-and-combine route
@functools.lru_cache(maxsize=None)
def _few_targets(n_src):
    x, y = IDW.scattered(n_src, 31)
    xi, yi = IDW.scattered(40, 32)
    xi[:3], yi[:3] = x[[5, n_src // 2, n_src - 1]], y[[5, n_src // 2, n_src - 1]]      # three exact hits, in different pieces
    return x, y, xi, yi


@pytest.mark.parametrize("n_planes", [None, 5])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n_src, kernels", [(3000, COMBINE), (600, SEARCH)])
def test_few_targets_split_the_sources_and_combine_in_a_fixed_order(eng, n_src, kernels, dtype, n_planes):
    x, y, xi, yi = _few_targets(n_src)
    z = IDW.values(n_planes, n_src, 33, dtype)
    for p in POWERS:
        got = _run(eng, x, y, z, xi, yi, power=p)
        assert eng.last_idw_kernel == kernels
        o = IDW.oracle(x, y, z, xi, yi, p=p)
        _check(got, o, f"{n_src} -> 40, {np.dtype(dtype).name}, planes {n_planes}, p = {p}")
        assert np.array_equal(got[0][..., :3], z[..., [5, n_src // 2, n_src - 1]]) and np.isposinf(got[1][..., :3]).all()
    assert np.array_equal(_np(eng.idw_interp(x, y, z, xi, yi, power=3.5)).reshape(got[0].shape), got[0])    # without weight and count


# ------------------------------------------------------------------ geometry
def test_poles_seam_longitudes_beyond_180_and_an_antipodal_pair(eng):
    x, y = IDW.scattered(300, 41)
    x[:8] = [0.0, 77.0, 10.0, -200.0, 180.0, 540.0, -180.0, 359.0]
    y[:8] = [90.0, 90.0, -90.0, -90.0, 5.0, -30.0, -60.0, 0.0]
    z = IDW.values(2, 300, 42)
    xi = np.array([0.0, 123.0, -45.0, -180.0, 180.0, -180.0, 179.0, -1.0, 400.0, 181.0, 190.0, -170.0])
    yi = np.array([90.0, 90.0, -90.0, 5.0, -60.0, -30.0, 0.0, 0.0, 20.0, 0.0, 45.0, 45.0])
    got = _run(eng, x, y, z, xi, yi)
    _check(got, IDW.oracle(x, y, z, xi, yi), "poles and seam")
    assert np.abs(got[0][:, 3] - z[:, 4]).max() <= 1e-12 * np.abs(z[:, 4]).max()       # the source at 180 dominates the target at -180
    # one source, its antipode among the targets: the distance is half the circumference (asin(1), within 4 ulp, and three
    # roundings more, twice for the square: 1e-14 is three times that), the value the source's
    ax, ay = np.array([0.0]), np.array([0.0])
    u, w, c = _run(eng, ax, ay, np.array([2.5]), np.array([180.0, -180.0, 0.0, 90.0]), np.array([0.0, 0.0, 0.0, 0.0]))
    assert u[2] == 2.5 and np.isposinf(w[2]) and (c == 1).all()
    assert abs(w[0] * (math.pi * IDW.RADIUS) ** 2 - 1) <= 1e-14 and abs(w[3] * (math.pi * IDW.RADIUS / 2) ** 2 - 1) <= 1e-14
    _check((u, w, c), IDW.oracle(ax, ay, np.array([2.5]), np.array([180.0, -180.0, 0.0, 90.0]), np.zeros(4)), "antipode")


def test_unsorted_and_descending_grids_are_taken_as_given(eng):
    x, y = IDW.scattered(200, 51)
    z = IDW.values(None, 200, 52)
    lon, lat = np.linspace(-180.0, 175.0, 72), np.linspace(-87.5, 87.5, 36)
    want = _run(eng, x, y, z, lon, lat, grid=True)[0].reshape(36, 72)
    perm = np.random.default_rng(53).permutation(72)
    got = _run(eng, x, y, z, lon[perm], lat[::-1], grid=True)
    _check(got, IDW.oracle(x, y, z, lon[perm], lat[::-1], grid=True), "descending latitudes, shuffled longitudes")
    assert np.array_equal(got[0].reshape(36, 72), want[::-1][:, perm])                  # a node's value does not depend on its place


# ------------------------------------------------------------------ exact hits
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n_src, kernels", [(400, SEARCH), (2600, COMBINE)])
def test_targets_on_sources_reproduce_the_value_or_the_mean_of_duplicates_bit_for_bit(eng, n_src, kernels, dtype):
    x, y = IDW.scattered(n_src, 61)
    z = IDW.values(3, n_src, 62, dtype)
    pairs = [(70, 300), (190, n_src - 1), (256, 255)]                                # two sources in one place, with different values
    for a, b in pairs:
        x[b], y[b] = x[a], y[a]
    take = np.r_[0:50, [a for a, _ in pairs]]
    u, w, c = _run(eng, x, y, z, x[take], y[take])
    assert eng.last_idw_kernel == kernels
    want = z[:, take].copy()
    for k, (a, b) in enumerate(pairs):
        want[:, 50 + k] = ((z[:, a].astype(np.float64) + z[:, b].astype(np.float64)) / 2.0).astype(dtype)
    assert u.dtype == np.dtype(dtype) and np.array_equal(u, want) and np.isposinf(w).all() and (c == n_src).all()
    _check((u, w, c), IDW.oracle(x, y, z, x[take], y[take]), f"hits among {n_src}")


# ------------------------------------------------------------------ NaN values and NaN coordinates
@pytest.mark.parametrize("n_src, kernels", [(500, SEARCH), (2100, COMBINE)])
def test_nan_values_leave_one_plane_only_and_nan_coordinates_leave_the_source_out(eng, n_src, kernels):
    x, y = IDW.scattered(n_src, 71)
    xi, yi = IDW.scattered(90, 72)
    xi[:2], yi[:2] = x[[3, 4]], y[[3, 4]]                                             # source 3 will be NaN in plane 1: no hit there
    z = IDW.values(3, n_src, 73)
    holes = z.copy()
    holes[1, 3::7] = np.nan
    full, some = _run(eng, x, y, z, xi, yi), _run(eng, x, y, holes, xi, yi)
    assert eng.last_idw_kernel == kernels
    for k in (0, 1):
        assert np.array_equal(full[k][[0, 2]], some[k][[0, 2]])                        # the other planes: bit-identical
    assert np.array_equal(full[2], some[2]) and (some[2] == n_src).all()               # the count does not look at values
    assert np.isposinf(full[1][1, 0]) and np.isfinite(some[1][1, 0]) and np.isposinf(some[1][1, 1])
    _check(some, IDW.oracle(x, y, holes, xi, yi), f"NaN values among {n_src}")
    bx, by = x.copy(), y.copy()
    bx[11], by[200], by[n_src - 1], bx[4] = np.nan, 90.001, -np.inf, np.inf
    bad = _run(eng, bx, by, z, xi, yi)
    assert (bad[2] == n_src - 4).all() and np.isfinite(bad[1][:, 1]).all()             # the hit on source 4 is gone with it
    _check(bad, IDW.oracle(bx, by, z, xi, yi), f"NaN coordinates among {n_src}")
    ti = yi.copy()
    ti[5] = np.nan
    u, w, c = _run(eng, x, y, z, xi, ti)
    assert np.isnan(u[:, 5]).all() and not w[:, 5].any() and c[5] == 0                 # a target that is nowhere has no source


# ------------------------------------------------------------------ max_distance
@functools.lru_cache(maxsize=None)
def _bounded_case(n_src):
    x, y = IDW.scattered(n_src, 81, lat_max=90.0)
    xi, yi = IDW.scattered(700, 82, lat_max=90.0)
    xi[:6], yi[:6] = [0.0, 10.0, 20.0, -150.0, 30.0, 90.0], [89.9, 89.0, -89.5, 88.0, -90.0, 90.0]      # around both poles
    xi[6:10], yi[6:10] = x[:4], y[:4]
    z = IDW.values(2, n_src, 83)
    z[1, ::5] = np.nan
    return x, y, z, xi, yi


@pytest.mark.parametrize("reach", [200e3, 1500e3, 3000e3], ids=["200km", "1500km", "across-a-pole"])
@pytest.mark.parametrize("n_src, kernels", [(900, RANGE + SEARCH), (2000, RANGE + COMBINE)])
def test_a_bound_counts_what_the_oracle_counts_and_culling_changes_nothing(eng, n_src, kernels, reach):
    x, y, z, xi, yi = _bounded_case(n_src)
    got = _run(eng, x, y, z, xi, yi, max_distance=reach)
    assert eng.last_idw_kernel == kernels
    o = IDW.oracle(x, y, z, xi, yi, max_distance=reach)
    _check(got, o, f"{n_src} -> 700 within {reach / 1e3:.0f} km")                       # the count integer for integer among it
    assert np.array_equal(np.isnan(got[0][0]), got[2] == 0) and (got[2][6:10] > 0).all()
    if reach == 200e3:
        assert (got[2] == 0).any()
    if reach == 3000e3:                                                                # the pole's own reach crosses it
        cross = IDW.costs(IDW.unit(xi[4:6], yi[4:6]), IDW.unit(x, y)) <= IDW.chord2_of(reach)
        lon_spread = [np.ptp(x[row]) for row in cross]
        assert min(lon_spread) > 300.0
    other = _run(eng, x, y, z, xi, yi, max_distance=reach, radius=IDW.RADIUS)           # the default radius, spelled out
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(got, other))


@pytest.mark.parametrize("n_src, kernels", [(900, SEARCH), (2000, COMBINE)])
def test_no_bound_and_a_bound_of_half_the_circumference_are_one_call(eng, n_src, kernels):
    x, y, z, xi, yi = _bounded_case(n_src)
    free = _run(eng, x, y, z, xi, yi)
    half = _run(eng, x, y, z, xi, yi, max_distance=math.pi * IDW.RADIUS)
    assert eng.last_idw_kernel == kernels
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(free, half)) and (free[2] == n_src).all()
    o = IDW.oracle(x, y, z, xi, yi)
    _check(free, o, f"{n_src} -> 700 without a bound")
    other = _run(eng, x, y, z, xi, yi, radius=6378.1)                                  # the reference's radius: the same field,
    err = np.abs(other[0] - o["u64"])                                                  # within the same tolerance of the same oracle
    assert (err <= IDW.bound_u(o, np.float64)).all()


# ------------------------------------------------------------------ determinism
@pytest.mark.parametrize("n_src, n_tgt, reach, kernels", [(513, 700, None, SEARCH), (3000, 40, None, COMBINE), (900, 700, 1500e3, RANGE + SEARCH),
                                                          (2000, 700, 1500e3, RANGE + COMBINE)])
def test_two_calls_agree_bit_for_bit_on_every_route(eng, n_src, n_tgt, reach, kernels):
    x, y = IDW.scattered(n_src, 91)
    xi, yi = IDW.scattered(n_tgt, 92)
    z = IDW.values(5, n_src, 93, np.float32)
    first = _run(eng, x, y, z, xi, yi, power=3.5, max_distance=reach)
    assert eng.last_idw_kernel == kernels
    again = _run(eng, x, y, z, xi, yi, power=3.5, max_distance=reach)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(first, again))
    t = eng.torch
    dev = eng.idw_interp(t.as_tensor(x, device=eng.device), t.as_tensor(y, device=eng.device), t.as_tensor(z, device=eng.device),
                         t.as_tensor(xi, device=eng.device), t.as_tensor(yi, device=eng.device), power=3.5, max_distance=reach)
    assert np.array_equal(_np(dev), first[0], equal_nan=True)                           # device tensors in: the same call


# ------------------------------------------------------------------ the public surface
def test_xr_idx_interp_grids_a_labelled_array_of_points(eng):
    from lagrangiancoherence_amd import tools
    from lagrangiancoherence_amd.dropin import get_engine
    x, y = IDW.scattered(700, 95)
    z = IDW.values(3, 700, 96, np.float32)
    lon, lat = np.linspace(-180.0, 170.0, 36), np.linspace(80.0, -80.0, 17)
    da = DataArray(z, ("time", "points"), {"time": np.arange(3), "longitude": x, "latitude": y}, name="tracer")
    fields = []
    for reach in (None, 1200e3):
        u, w, c = tools.xr_idx_interp(da, lon, lat, p=3.5, max_distance=reach, return_weight=True, return_count=True)
        fields.append(u.values)
        assert get_engine().last_idw_kernel == (SEARCH if reach is None else RANGE + SEARCH)
        assert isinstance(u, DataArray) and u.dims == w.dims == ("time", "latitude", "longitude") and c.dims == ("latitude", "longitude")
        assert u.shape == (3, 17, 36) and u.dtype == np.float32 and u.name == "tracer" and c.dtype == np.int32 and w.dtype == np.float64
        assert np.array_equal(u.coords["latitude"], lat) and np.array_equal(u.coords["longitude"], lon) and np.array_equal(u.coords["time"], np.arange(3))
        o = IDW.oracle(x, y, z, lon, lat, grid=True, p=3.5, max_distance=reach)
        _check((u.values.reshape(3, -1), w.values.reshape(3, -1), c.values.reshape(-1)), o, f"xr_idx_interp within {reach}")
    plain = tools.xr_idx_interp(DataArray(z[0].astype(np.float64), ("points",), {"longitude": x, "latitude": y}), lon, lat)
    assert plain.dims == ("latitude", "longitude") and plain.dtype == np.float64
    o = IDW.oracle(x, y, z[0].astype(np.float64), lon, lat, grid=True)
    _check((plain.values.reshape(-1), o["weight"], o["count"]), o, "xr_idx_interp, one plane")
    swapped = tools.xr_idx_interp(DataArray(z.T.copy(), ("points", "time"), {"longitude": x, "latitude": y}), lon, lat, p=3.5)
    assert swapped.dims == ("time", "latitude", "longitude") and np.array_equal(swapped.values, fields[0])    # the points' dim is found


def test_inverse_weighted_interpolation_is_the_references_call(eng):
    from lagrangiancoherence_amd import tools
    x, y = IDW.scattered(50, 3)
    xi, yi = IDW.scattered(40, 4)
    z = IDW.values(None, 50, 5)
    got = tools.Inverse_weighted_interpolation(x, y, z, xi, yi)
    assert isinstance(got, np.ndarray) and got.shape == (40,) and got.dtype == np.float64
    o = IDW.oracle(x, y, z, xi, yi)
    _check((got, o["weight"], o["count"]), o, "Inverse_weighted_interpolation")
    want = IDW.reference_formula(x, y, z, xi, yi, 6378.1)                                # what the reference means, on its own radius
    assert np.abs(got - want).max() <= 1e-9 * o["scale"].max()
    cubed = tools.Inverse_weighted_interpolation(x, y, z.astype(np.float32), xi, yi, 3)
    assert cubed.dtype == np.float32
    o = IDW.oracle(x, y, z.astype(np.float32), xi, yi, p=3)
    _check((cubed, o["weight"], o["count"]), o, "Inverse_weighted_interpolation, float32, power 3")
