"""The distance transform on the GPU against tests/distance.py: distances equal to scipy.ndimage.distance_transform_edt bit for
bit (float64, np.array_equal) at unit sampling and at three samplings, from float32 and float64 masks; distances and nearest
indices equal to the brute-force minimum with the smallest-index rule on every plane up to 67 x 130 -- on the smallest planes
that cross every boundary of csrc/distance.hip: one pixel, one row, one column, sizes that are no multiple of the wave (64),
the workgroup (256) or the row segment (64), several segments (130 and 515 rows), more columns than one pass of a workgroup
(513), columns without a pixel, up / down ties, the seam, a bound, several planes per launch, NaN and negative mask values,
and the widest row the kernel stages (16384).

Every reference is computed once per case and shared.  The float buffers the module's engine allocates start as NaN.
"""
import functools

import numpy as np
import pytest

from tests import components as CO
from tests import distance as DT
from tests.labelled import DataArray

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
UNIT = (1.0, 1.0)
ALL_SAMPLINGS = [UNIT] + DT.SAMPLINGS
SID = [f"{a}x{b}" for a, b in ALL_SAMPLINGS]


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
def _brute(name, cyclic=False, sampling=UNIT):
    dist, nearest = DT.brute(_mask(name), cyclic, sampling)
    dist.setflags(write=False)
    nearest.setflags(write=False)
    return dist, nearest


@functools.lru_cache(maxsize=None)
def _scipy(name, cyclic=False, sampling=UNIT):
    d = DT.scipy_edt(_mask(name), cyclic, sampling)
    d.setflags(write=False)
    return d


# ------------------------------------------------------------------ distances and nearest pixels
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("sampling", ALL_SAMPLINGS, ids=SID)
@pytest.mark.parametrize("name", list(DT.SMALL))
def test_distance_equals_scipy_and_nearest_the_brute_force_oracle(eng, name, sampling, dtype):
    mask = _mask(name)
    dist, nearest = eng.distance_transform(mask.astype(dtype), sampling=sampling, return_nearest=True)
    assert dist.dtype == eng.torch.float64 and nearest.dtype == eng.torch.int32
    assert tuple(dist.shape) == mask.shape == tuple(nearest.shape)
    assert np.array_equal(_np(dist), _scipy(name, False, sampling))
    want_d, want_n = _brute(name, False, sampling)
    assert np.array_equal(_np(dist), want_d) and np.array_equal(_np(nearest), want_n)
    alone = eng.distance_transform(mask.astype(dtype), sampling=sampling)          # without the index: the same distances
    assert np.array_equal(_np(alone), want_d)


@pytest.mark.parametrize("name", list(DT.EMPTY))
def test_a_plane_without_foreground_is_inf_and_minus_one(eng, name):
    dist, nearest = eng.distance_transform(_mask(name), return_nearest=True)
    assert np.isposinf(_np(dist)).all() and (_np(nearest) == -1).all() and tuple(dist.shape) == _mask(name).shape


def test_the_foreground_plane_is_zero_and_points_at_itself(eng):
    mask = _mask("foreground-67x130")
    dist, nearest = eng.distance_transform(mask, return_nearest=True)
    assert not _np(dist).any() and np.array_equal(_np(nearest).ravel(), np.arange(mask.size))


def test_nan_is_background_and_negative_values_are_foreground(eng):
    mask = _mask("nan-negative")
    dist = _np(eng.distance_transform(mask))
    assert (dist[np.isnan(mask)] > 0).all() and not dist[mask < 0].any() and (dist[mask == 0] > 0).all()


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("sampling", ALL_SAMPLINGS, ids=SID)
def test_the_larger_plane_equals_scipy_and_its_nearest_pixels_are_the_first_of_the_nearest(eng, sampling, dtype):
    name = "random-515x513-0.02"
    mask = _mask(name)
    ny, nx = mask.shape
    dist, nearest = (_np(t) for t in eng.distance_transform(mask.astype(dtype), sampling=sampling, return_nearest=True))
    assert np.array_equal(dist, _scipy(name, False, sampling))
    fg = DT.foreground(mask)
    assert fg.ravel()[nearest.ravel()].all()                           # every index points at a foreground pixel
    r, c = np.divmod(np.arange(mask.size), nx)
    fr, fc = np.divmod(nearest.ravel().astype(np.int64), nx)
    cost = DT.cost_of(r - fr, c - fc, sampling)
    assert np.array_equal(np.sqrt(cost), dist.ravel())                 # and at the pixel the distance belongs to
    # no foreground pixel of a smaller index is as near: 2000 pixels, each against all of them
    sample = np.random.default_rng([DT.SEED, 2000]).choice(mask.size, 2000, replace=False)
    idx = np.flatnonzero(fg)
    ir, ic = np.divmod(idx, nx)
    all_costs = DT.cost_of(r[sample, None] - ir[None, :], c[sample, None] - ic[None, :], sampling)
    assert np.array_equal(all_costs.min(axis=1), cost[sample])
    assert np.array_equal(idx[np.argmin(all_costs, axis=1)], nearest.ravel()[sample])


def test_the_widest_row_the_kernel_stages(eng):
    """nx = 16384: the whole 64 KiB of offsets of a row in LDS."""
    mask = np.zeros((3, 16384), dtype=np.float32)
    mask[0, 5] = mask[2, 9000] = mask[1, 16383] = 1
    dist = _np(eng.distance_transform(mask))
    assert np.array_equal(dist, DT.scipy_edt(mask))


# ------------------------------------------------------------------ the seam
@pytest.mark.parametrize("name", ["cyclic-20x13", "cyclic-20x12", "cyclic-67x130-0.02"])
def test_cyclic_equals_scipy_on_the_tiled_plane(eng, name):
    dist, nearest = eng.distance_transform(_mask(name), cyclic=True, return_nearest=True)
    assert np.array_equal(_np(dist), _scipy(name, True))
    want_d, want_n = _brute(name, True)
    assert np.array_equal(_np(dist), want_d) and np.array_equal(_np(nearest), want_n)


def test_cyclic_differs_where_the_seam_is_the_shorter_way(eng):
    mask = _mask("cyclic-column-0")
    nx = mask.shape[1]
    plain, cyclic = _np(eng.distance_transform(mask)), _np(eng.distance_transform(mask, cyclic=True))
    assert np.array_equal(plain, np.broadcast_to(np.arange(nx, dtype=np.float64), mask.shape))
    assert (cyclic[:, nx - 1] == 1).all() and not np.array_equal(plain, cyclic)
    assert np.array_equal(cyclic, _scipy("cyclic-column-0", True))


# ------------------------------------------------------------------ a bound
@pytest.mark.parametrize("bound", [1, 2.5, 12])
@pytest.mark.parametrize("name, cyclic", [("corners-67x130", False), ("random-67x130-0.02", False), ("cyclic-67x130-0.02", True)])
def test_a_bound_keeps_what_is_within_it_and_nothing_else(eng, name, cyclic, bound):
    full_d, full_n = _brute(name, cyclic)
    within = full_d <= bound
    assert within.any() and (name != "corners-67x130" or within.mean() < 0.25)      # most of that plane is beyond every bound
    dist, nearest = eng.distance_transform(_mask(name), cyclic=cyclic, max_distance=bound, return_nearest=True)
    assert np.array_equal(_np(dist), np.where(within, full_d, np.inf))
    assert np.array_equal(_np(nearest), np.where(within, full_n, -1))


def test_a_bound_under_a_sampling(eng):
    sampling = (2.0, 0.5)
    full_d, full_n = _brute("random-67x130-0.02", False, sampling)
    dist, nearest = eng.distance_transform(_mask("random-67x130-0.02"), sampling=sampling, max_distance=2.5, return_nearest=True)
    assert np.array_equal(_np(dist), np.where(full_d <= 2.5, full_d, np.inf))
    assert np.array_equal(_np(nearest), np.where(full_d <= 2.5, full_n, -1))


# ------------------------------------------------------------------ several planes
BATCH = ["random-67x130-0.02", "corners-67x130", "background-67x130", "random-67x130-0.2", "row-67x130"]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
def test_a_stack_equals_its_planes_one_by_one(eng, dtype):
    stack = np.stack([_mask(n) for n in BATCH]).astype(dtype)
    dist, nearest = eng.distance_transform(stack, return_nearest=True)
    assert tuple(dist.shape) == stack.shape == tuple(nearest.shape)
    for i, name in enumerate(BATCH):
        one_d, one_n = eng.distance_transform(stack[i], return_nearest=True)
        assert np.array_equal(_np(dist[i]), _np(one_d)) and np.array_equal(_np(nearest[i]), _np(one_n))
        if name in DT.EMPTY:                                            # between two others, touching neither
            assert np.isposinf(_np(dist[i])).all() and (_np(nearest[i]) == -1).all()
        else:
            assert np.array_equal(_np(dist[i]), _brute(name)[0]) and np.array_equal(_np(nearest[i]), _brute(name)[1])


def test_a_device_tensor_and_another_dtype_are_taken_as_they_are(eng):
    mask = _mask("random-67x130-0.02")
    on_device = eng.to_device(mask, np.float64)
    assert np.array_equal(_np(eng.distance_transform(on_device)), _brute("random-67x130-0.02")[0])
    assert np.array_equal(_np(eng.distance_transform(mask.astype(bool))), _brute("random-67x130-0.02")[0])
    assert np.array_equal(_np(eng.distance_transform(mask, sampling=2.0)), DT.scipy_edt(mask, sampling=(2.0, 2.0)))


# ------------------------------------------------------------------ the labelled surface
def test_distance_to_ridges_sorts_and_returns_the_callers_order():
    from LagrangianCoherence.LCS.tools import distance_to_ridges
    mask = _mask("random-67x130-0.02")
    ny, nx = mask.shape
    lat, lon = np.linspace(-33.0, 33.0, ny), np.linspace(-60.0, 69.0, nx)
    want_d, want_n = _brute("random-67x130-0.02")
    # descending latitude, (longitude, latitude) order: the same field as the caller holds it
    ridges = DataArray(mask[::-1].T.copy(), ("longitude", "latitude"), {"latitude": lat[::-1], "longitude": lon}, name="ridges")
    out = distance_to_ridges(ridges)
    assert type(out) is DataArray and out.dims == ("longitude", "latitude") and out.name == "ridges"
    assert np.array_equal(out.coords["latitude"], lat) and np.array_equal(out.coords["longitude"], lon)
    assert out.values.dtype == np.float64 and np.array_equal(out.values, want_d.T)
    dist, owner = distance_to_ridges(ridges, return_labels=True)
    lab = CO.label(mask)[0]
    assert owner.dims == ("longitude", "latitude") and owner.values.dtype == np.int32
    assert np.array_equal(dist.values, want_d.T) and np.array_equal(owner.values, lab.ravel()[want_n].T)
    fg = DT.foreground(mask)
    assert np.array_equal(owner.values.T[fg], lab[fg]) and owner.values.min() >= 1        # every ridge pixel carries its own label
    # a bound: the label is 0 where there is no ridge within it
    dist, owner = distance_to_ridges(ridges, max_distance=2.5, return_labels=True, connectivity=1)
    lab1 = CO.label(mask, 1)[0]
    assert np.array_equal(owner.values.T, np.where(want_d <= 2.5, lab1.ravel()[want_n], 0))
    assert np.array_equal(dist.values.T, np.where(want_d <= 2.5, want_d, np.inf))


def test_distance_to_ridges_of_a_stack_equals_its_planes():
    from lagrangiancoherence_amd.tools import distance_to_ridges
    names = ["cyclic-67x130-0.02", "background-67x130", "random-67x130-0.2"]
    stack = np.stack([_mask(n) for n in names])
    ny, nx = stack.shape[1:]
    coords = {"time": np.arange(3), "latitude": np.linspace(-33.0, 33.0, ny), "longitude": np.linspace(-180.0, 177.0, nx)}
    dims = ("latitude", "time", "longitude")                            # the extra dimension in the middle
    kw = dict(cyclic=True, sampling=(1.0, 0.7), return_labels=True)
    dist, owner = distance_to_ridges(DataArray(stack.transpose(1, 0, 2), dims, coords), **kw)
    assert dist.dims == dims == owner.dims and np.array_equal(dist.coords["time"], coords["time"])
    for i, name in enumerate(names):
        want_d, want_n = _brute(name, True, (1.0, 0.7))
        lab = CO.label(stack[i], 2, cyclic=True)[0]
        assert np.array_equal(dist.values[:, i, :], want_d)
        assert np.array_equal(owner.values[:, i, :], np.where(want_n >= 0, lab.ravel()[np.maximum(want_n, 0)], 0))
    assert not owner.values[:, 1, :].any() and np.isposinf(dist.values[:, 1, :]).all()
