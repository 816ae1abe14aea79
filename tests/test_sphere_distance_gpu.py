"""The great-circle distance to the nearest ridge pixel on the GPU against tests/sphere_distance.py: squared chords and nearest
indices equal to the numpy oracle bit for bit (np.array_equal), from float32 and float64 masks, on the smallest planes that
cross every boundary of csrc/sphere_distance.hip: one pixel, one row, one column, sizes that are no multiple of the wave (64)
or of the 256-thread workgroup, workgroups that span several rows (67 columns) and rows that span several workgroups (513), a
list of 2, about 17, about 174, about 1740 and 8710 pixels -- shorter than the staging chunk of 256, many times it, and, in a
test of their own, 255, 256, 257, 512 and 513 --, rows without a pixel, several planes per launch, a bound with its band of
latitudes, a grid that is neither uniform nor global, one whose latitudes are not sorted, the seam, the pole, a tie that is
guaranteed bit for bit, NaN and negative mask values.

Distances: the argument of asin is bit-identical on both sides, each library's double asin is documented within 4 ulp, and
there are two roundings more on each side (the product with 2 radius among them): the bound is 16 ulp of the oracle's value.
The largest difference seen on an MI355X, over every case of this module, is 2 ulp (each check prints its own maximum; run
with -s).  A larger value is a finding to explain, not a bound to widen.

Every reference is computed once per case and shared.  The float buffers the module's engine allocates start as NaN.
"""
import functools

import numpy as np
import pytest

from tests import components as CO
from tests import distance as DT
from tests import sphere_distance as SD
from tests.labelled import DataArray

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
EXACT = ["1x1-foreground", "1x37", "37x1", "corners-67x130", "one-pixel-67x130",
         *[f"random-{s}-{d}" for s in ("67x130", "130x67") for d in (0.002, 0.02, 0.2)],
         "row-67x130", "column-67x130", "foreground-67x130", "nan-negative"]
BOUNDS = (60e3, 250e3, 1500e3)


@pytest.fixture(scope="module")
def eng():
    from lagrangiancoherence_amd.engine import Engine
    e = Engine(0)
    e._poison = True
    yield e
    e.close()


def _np(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _mask(name):
    m = DT.mask_of(name)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def _brute(name):
    """The unbounded oracle of a named plane on the global grid of its shape."""
    out = SD.brute(_mask(name), *SD.GRID(*_mask(name).shape))
    for a in out:
        a.setflags(write=False)
    return out


def _bounded(full, max_distance, radius=SD.RADIUS):
    """The unbounded result masked by ``cost <= cmax2``: what a bound is defined as."""
    dist, nearest, cost = full
    within = cost <= SD.chord2_of(max_distance, radius)
    return np.where(within, dist, np.inf), np.where(within, nearest, -1), np.where(within, cost, np.inf), within


def _ulps(got, want):
    """|got - want| in units of the spacing of want, where want is finite and not 0."""
    at = np.isfinite(want) & (want != 0)
    return np.abs(got[at] - want[at]) / np.spacing(want[at]) if at.any() else np.zeros(1)


def _check(got, want, label=""):
    """dist, nearest, cost of the device against the oracle's: cost and nearest bit for bit, dist exactly 0 where the cost is 0,
    +inf where it is +inf, within 16 ulp elsewhere."""
    (dist, nearest, cost), (want_d, want_n, want_c) = got, want
    assert np.array_equal(cost, want_c) and np.array_equal(nearest, want_n)
    assert not dist[want_c == 0].any() and np.array_equal(np.isposinf(dist), np.isposinf(want_d))
    print(f"{label}: max |dist - oracle| = {_ulps(dist, want_d).max():.2f} ulp")
    f = np.isfinite(want_d)
    assert (np.abs(dist[f] - want_d[f]) <= 16 * np.spacing(want_d[f])).all()


def _all(eng, mask, lat, lon, **kw):
    return tuple(_np(t) for t in eng.sphere_distance(mask, lat, lon, return_nearest=True, return_cost=True, **kw))


# ------------------------------------------------------------------ exactness
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("name", EXACT)
def test_distances_chords_and_nearest_pixels_equal_the_oracle(eng, name, dtype):
    mask = _mask(name).astype(dtype)
    lat, lon = SD.GRID(*mask.shape)
    dist, nearest, cost = eng.sphere_distance(mask, lat, lon, return_nearest=True, return_cost=True)
    assert dist.dtype == eng.torch.float64 == cost.dtype and nearest.dtype == eng.torch.int32
    assert tuple(dist.shape) == mask.shape == tuple(nearest.shape) == tuple(cost.shape)
    _check((_np(dist), _np(nearest), _np(cost)), _brute(name), name)
    fg = DT.foreground(mask)
    assert np.array_equal(_np(nearest)[fg], np.flatnonzero(fg))                     # a foreground pixel points at itself
    alone = eng.sphere_distance(mask, lat, lon)                                     # without index or cost: the same bits
    assert np.array_equal(_np(alone), _np(dist))
    only_n = eng.sphere_distance(mask, lat, lon, return_nearest=True)
    assert np.array_equal(_np(only_n[0]), _np(dist)) and np.array_equal(_np(only_n[1]), _np(nearest))


@pytest.mark.parametrize("count", [255, 256, 257, 512, 513])
def test_a_list_of_about_one_and_two_staging_chunks(eng, count):
    rng = np.random.default_rng([DT.SEED, count])
    mask = np.zeros(67 * 130)
    mask[rng.choice(mask.size, count, replace=False)] = 1
    mask = mask.reshape(67, 130)
    lat, lon = SD.GRID(67, 130)
    _check(_all(eng, mask, lat, lon), SD.brute(mask, lat, lon), f"{count} pixels")


def test_ties_go_to_the_smaller_index_on_the_device(eng):
    mask, lat, lon = SD.tie_grid()
    dist, nearest, cost = _all(eng, mask, lat, lon)
    assert (nearest[:, 65] == 262).all()
    _check((dist, nearest, cost), SD.brute(mask, lat, lon), "tie grid")


def test_the_seam_and_the_pole_are_no_obstacle(eng):
    lat, lon = SD.GRID(67, 130)
    mask = np.zeros((67, 130))
    mask[33, 129] = 1
    got = _all(eng, mask, lat, lon)
    step = SD.RADIUS * np.cos(np.deg2rad(lat[33])) * np.deg2rad(360 / 130)            # one column along the parallel: ~308 km
    assert 0.99 * step < got[0][33, 0] < 1.01 * step and got[0][33, 0] < got[0][33, 2] and got[1][33, 0] == 33 * 130 + 129
    _check(got, SD.brute(mask, lat, lon), "seam")
    mask = np.zeros((67, 130))
    mask[66, 0] = mask[40, 65] = 1
    got = _all(eng, mask, lat, lon)
    assert got[1][62, 65] == 66 * 130                                              # over the pole, not down its own meridian
    _check(got, SD.brute(mask, lat, lon), "pole")


def test_a_grid_that_is_neither_uniform_nor_global(eng):
    lat, lon = np.degrees(np.arcsin(np.linspace(-0.7, 0.95, 67))), np.linspace(-90, -32, 130)
    mask = _mask("random-67x130-0.02")
    full = SD.brute(mask, lat, lon)
    _check(_all(eng, mask, lat, lon), full, "regional")
    *want, within = _bounded(full, 250e3)
    assert 0 < within.mean() < 1
    _check(_all(eng, mask, lat, lon, max_distance=250e3), want, "regional, 250 km")


def test_latitudes_that_are_not_sorted_under_a_bound(eng):
    """The band of a row is then the smallest range of rows that holds every row within the bound: more work, the same result."""
    lat, lon = SD.GRID(67, 130)
    lat = lat[np.random.default_rng([DT.SEED, 67]).permutation(67)]
    mask = _mask("random-67x130-0.02")
    *want, within = _bounded(SD.brute(mask, lat, lon), 250e3)
    assert 0 < within.mean() < 1
    _check(_all(eng, mask, lat, lon, max_distance=250e3), want, "unsorted latitudes, 250 km")


@pytest.mark.parametrize("name", list(DT.EMPTY))
def test_a_plane_without_foreground_is_inf_and_minus_one(eng, name):
    mask = _mask(name)
    for kw in ({}, {"max_distance": 250e3}):
        dist, nearest, cost = _all(eng, mask, *SD.GRID(*mask.shape), **kw)
        assert np.isposinf(dist).all() and (nearest == -1).all() and np.isposinf(cost).all() and dist.shape == mask.shape


# ------------------------------------------------------------------ a bound
@pytest.mark.parametrize("bound", BOUNDS)
@pytest.mark.parametrize("name", ["random-67x130-0.02", "corners-67x130"])
def test_a_bound_keeps_what_is_within_it_and_nothing_else(eng, name, bound):
    *want, within = _bounded(_brute(name), bound)
    print(f"{name}, {bound / 1e3:g} km: {within.mean():.3f} of the points are within it")
    assert 0 < within.mean() < 1
    mask = _mask(name)
    lat, lon = SD.GRID(*mask.shape)
    _check(_all(eng, mask, lat, lon, max_distance=bound), want, f"{name}, {bound / 1e3:g} km")
    alone = _np(eng.sphere_distance(mask, lat, lon, max_distance=bound))
    assert np.array_equal(np.isposinf(alone), ~within)


def test_a_bound_of_half_the_circumference_is_none_and_a_radius_scales(eng):
    mask = _mask("random-67x130-0.02")
    lat, lon = SD.GRID(67, 130)
    _check(_all(eng, mask, lat, lon, max_distance=np.pi * SD.RADIUS), _brute("random-67x130-0.02"), "pi radius")
    full = SD.brute(mask, lat, lon, radius=1.0)
    _check(_all(eng, mask, lat, lon, radius=1.0), full, "unit sphere")
    *want, within = _bounded(full, 0.05, 1.0)
    assert 0 < within.mean() < 1
    _check(_all(eng, mask, lat, lon, radius=1.0, max_distance=0.05), want, "unit sphere, 0.05 rad")


# ------------------------------------------------------------------ a larger plane
def test_the_larger_plane_points_at_the_first_of_the_nearest(eng):
    """515 x 513 with about 5300 pixels: the full oracle would take tens of seconds."""
    name = "random-515x513-0.02"
    mask = _mask(name)
    ny, nx = mask.shape
    lat, lon = SD.GRID(ny, nx)
    dist, nearest, cost = _all(eng, mask, lat, lon)
    fg = DT.foreground(mask)
    assert nearest.min() >= 0 and fg.ravel()[nearest.ravel()].all()                 # every index points at a foreground pixel
    X, Y, Z = SD.unit_vectors(lat, lon)
    at = nearest.ravel()
    assert np.array_equal(SD.cost_of((X, Y, Z), (X[at], Y[at], Z[at])), cost.ravel())     # and the cost is the one of that pixel
    assert np.array_equal(np.isfinite(dist), np.ones_like(fg)) and not dist[cost == 0].any()
    want_d = SD.dist_of(cost)
    assert (np.abs(dist - want_d) <= 16 * np.spacing(want_d)).all()
    # no foreground pixel is nearer and none of a smaller index as near: 2000 pixels, each against all of them
    sample = np.random.default_rng([DT.SEED, 2000]).choice(mask.size, 2000, replace=False)
    idx = np.flatnonzero(fg)
    all_costs = SD.cost_of((X[sample, None], Y[sample, None], Z[sample, None]), (X[idx][None, :], Y[idx][None, :], Z[idx][None, :]))
    assert np.array_equal(all_costs.min(axis=1), cost.ravel()[sample])
    assert np.array_equal(idx[np.argmin(all_costs, axis=1)], nearest.ravel()[sample])


# ------------------------------------------------------------------ several planes
BATCH = ["random-67x130-0.02", "corners-67x130", "background-67x130", "random-67x130-0.2", "row-67x130"]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("bound", [None, 250e3], ids=["unbounded", "250km"])
def test_a_stack_equals_its_planes_one_by_one(eng, dtype, bound):
    stack = np.stack([_mask(n) for n in BATCH]).astype(dtype)
    lat, lon = SD.GRID(67, 130)
    got = _all(eng, stack, lat, lon, max_distance=bound)
    assert all(g.shape == stack.shape for g in got)
    for i, name in enumerate(BATCH):
        one = _all(eng, stack[i], lat, lon, max_distance=bound)
        assert all(np.array_equal(g[i], o) for g, o in zip(got, one))               # bit for bit, distances too
        if name in DT.EMPTY:                                                        # between two others, touching neither
            assert np.isposinf(got[0][i]).all() and (got[1][i] == -1).all()
        else:
            want = _brute(name) if bound is None else _bounded(_brute(name), bound)[:3]
            _check(tuple(g[i] for g in got), want, name)


def test_a_device_tensor_and_a_bool_mask_are_taken_as_they_are(eng):
    name = "random-67x130-0.02"
    mask = _mask(name)
    lat, lon = SD.GRID(67, 130)
    _check(_all(eng, eng.to_device(mask, np.float64), lat, lon), _brute(name), "device tensor")
    _check(_all(eng, eng.to_device(mask, np.float32), lat, lon), _brute(name), "float32 device tensor")
    _check(_all(eng, mask.astype(bool), lat, lon), _brute(name), "bool")


# ------------------------------------------------------------------ the labelled surface
def _close(got, want):
    assert np.array_equal(np.isposinf(got), np.isposinf(want)) and not got[want == 0].any()
    f = np.isfinite(want)
    assert (np.abs(got[f] - want[f]) <= 16 * np.spacing(want[f])).all()


def test_distance_to_ridges_on_the_sphere_sorts_and_returns_the_callers_order():
    from LagrangianCoherence.LCS.tools import distance_to_ridges
    name = "random-67x130-0.02"
    mask = _mask(name)
    lat, lon = SD.GRID(67, 130)
    want_d, want_n, want_c = _brute(name)
    # descending latitude, (longitude, latitude) order: the same field as the caller holds it
    ridges = DataArray(mask[::-1].T.copy(), ("longitude", "latitude"), {"latitude": lat[::-1], "longitude": lon}, name="ridges")
    out = distance_to_ridges(ridges, metric='sphere')
    assert type(out) is DataArray and out.dims == ("longitude", "latitude") and out.name == "ridges"
    assert np.array_equal(out.coords["latitude"], lat) and np.array_equal(out.coords["longitude"], lon)
    assert out.values.dtype == np.float64
    _close(out.values, want_d.T)
    dist, owner = distance_to_ridges(ridges, metric='sphere', return_labels=True)
    lab = CO.label(mask)[0]
    assert owner.dims == ("longitude", "latitude") and owner.values.dtype == np.int32
    assert np.array_equal(dist.values, out.values) and np.array_equal(owner.values, lab.ravel()[want_n].T)
    fg = DT.foreground(mask)
    assert np.array_equal(owner.values.T[fg], lab[fg]) and owner.values.min() >= 1        # every ridge pixel carries its own label
    # a bound, in the unit of the radius: the label is 0 where there is no ridge within it
    bd, bn, bc, within = _bounded(_brute(name), 250e3)
    dist, owner = distance_to_ridges(ridges, metric='sphere', max_distance=250e3, return_labels=True, connectivity=1)
    lab1 = CO.label(mask, 1)[0]
    assert np.array_equal(owner.values.T, np.where(within, lab1.ravel()[want_n], 0))
    _close(dist.values.T, bd)
    km = distance_to_ridges(ridges, metric='sphere', radius=6371.0)                    # another unit
    _close(km.values, SD.dist_of(want_c, 6371.0).T)
    index = distance_to_ridges(ridges)                                                 # the default is the index metric, as before
    assert np.array_equal(index.values, DT.brute(mask)[0].T)


def test_distance_to_ridges_on_the_sphere_of_a_stack_equals_its_planes():
    from lagrangiancoherence_amd.tools import distance_to_ridges
    names = ["random-67x130-0.02", "background-67x130", "random-67x130-0.2"]
    stack = np.stack([_mask(n) for n in names])
    lat, lon = SD.GRID(67, 130)
    coords = {"time": np.arange(3), "latitude": lat, "longitude": lon}
    dims = ("latitude", "time", "longitude")                            # the extra dimension in the middle
    dist, owner = distance_to_ridges(DataArray(stack.transpose(1, 0, 2), dims, coords), cyclic=True, metric='sphere', return_labels=True)
    assert dist.dims == dims == owner.dims and np.array_equal(dist.coords["time"], coords["time"])
    for i, name in enumerate(names):
        if name in DT.EMPTY:
            continue
        want_d, want_n, _ = _brute(name)
        lab = CO.label(stack[i], 2, cyclic=True)[0]                      # cyclic applies to the labels
        _close(dist.values[:, i, :], want_d)
        assert np.array_equal(owner.values[:, i, :], lab.ravel()[want_n])
    assert not owner.values[:, 1, :].any() and np.isposinf(dist.values[:, 1, :]).all()
