"""The local threshold on the GPU against tests/local_threshold.py: the threshold within the derived tolerance of
scipy.ndimage.gaussian_filter(mode='reflect', or ['reflect', 'wrap'] when cyclic) minus offset, the mask equal to scipy's
except where scipy's own threshold is within that tolerance of the field (capped at 0.1 % of a case; the CPU test shows there
are no such pixels), on the smallest shapes that cross every boundary of csrc/threshold.hip -- planes smaller than the radius
(the index folds up to 22 times), one run + 1 and one bundle + 1 on both axes, ragged edges that are walked for 1, 2, 4 and 8
outputs per thread, a ragged plane of more than two runs each way in three planes, the largest radius, a skipped axis -- and
the identities that need no tolerance: float32 against its widening,
a plane of a stack against the plane alone, the shared arithmetic against Engine.gaussian_filter, the mask against the
threshold of the same call, the mask alone against the mask of both.

Every reference is computed once per case (tests/local_threshold.py: case) and shared.  The float buffers the module's engine
allocates start as NaN.
"""
import ctypes as C

import numpy as np
import pytest

from lagrangiancoherence_amd import _capi
from tests import local_threshold as LT
from tests.labelled import DataArray

pytestmark = pytest.mark.gpu

BOTH_WANTED = ("threshold", "mask")


@pytest.fixture(scope="module")
def eng():
    from lagrangiancoherence_amd.engine import Engine
    e = Engine(0)
    e._poison = True
    yield e
    e.close()


def _np(t):
    return t.detach().cpu().numpy()


def _check_against_scipy(name, f, got_thr, got_mask, ref, tol):
    err = float(np.abs(got_thr - ref).max())
    print(f"{name}: max |device - scipy| = {err:.3e}, atol = {tol:.3e}")
    assert err <= tol
    differ = got_mask.astype(bool) != (f > ref)
    print(f"{name}: mask differs from scipy's on {int(differ.sum())} of {f.size} pixels")
    assert not (differ & ~LT.undecided(f, ref, tol)).any()
    assert differ.sum() <= 0.001 * f.size


# ------------------------------------------------------------------ against scipy
@pytest.mark.parametrize("name", list(LT.CASES))
def test_threshold_and_mask_against_scipy(eng, name):
    f, sigma, offset, cyclic, kernels, ref, tol = LT.case(name)
    res = eng.local_threshold(f, sigma, offset=offset, cyclic=cyclic, want=BOTH_WANTED)
    assert eng.last_threshold_kernel == kernels
    thr, mask = res["threshold"], res["mask"]
    assert thr.dtype == eng.torch.float64 and mask.dtype == eng.torch.uint8
    assert tuple(thr.shape) == f.shape == tuple(mask.shape)
    thr, mask = _np(thr), _np(mask)
    assert set(np.unique(mask)) <= {0, 1}
    _check_against_scipy(name, f, thr, mask, ref, tol)
    # the mask is the comparison with the threshold of the same call, exactly
    assert np.array_equal(mask.astype(bool), f > thr)
    # and the mask alone -- no threshold plane written -- is the same mask
    alone = eng.local_threshold(f, sigma, offset=offset, cyclic=cyclic, want=("mask",))
    assert list(alone) == ["mask"] and np.array_equal(_np(alone["mask"]), mask)
    only = eng.local_threshold(f, sigma, offset=offset, cyclic=cyclic)
    assert list(only) == ["threshold"] and np.array_equal(_np(only["threshold"]), thr)


@pytest.mark.parametrize("name", ["20x23-b1x7", "20x23-b7x1", "20x23-b1x1"])
def test_a_skipped_axis_is_the_identity(eng, name):
    """sigma 0 along an axis: every line along the other axis is filtered on its own, so transposing the roles of a line and
    its neighbours changes nothing -- each row (column) of the result is the 1-D filter of that row (column) alone."""
    f, sigma, offset, cyclic, kernels, _, tol = LT.case(name)
    thr = _np(eng.local_threshold(f, sigma, offset=offset, cyclic=cyclic)["threshold"])
    assert eng.last_threshold_kernel == kernels
    if name == "20x23-b1x1":
        assert np.array_equal(thr, f - offset)
        return
    from scipy import ndimage
    axis = 1 if sigma[0] == 0.0 else 0
    lines = ndimage.gaussian_filter1d(f, sigma[axis], axis=axis, mode="reflect") - offset
    assert np.abs(thr - lines).max() <= tol
    # one line alone gives that line's bits: nothing of a neighbour enters
    row = f[7:8, :] if axis == 1 else f[:, 7:8]
    one = _np(eng.local_threshold(np.ascontiguousarray(row), sigma, offset=offset)["threshold"])
    assert np.array_equal(one, thr[7:8, :] if axis == 1 else thr[:, 7:8])


def test_the_largest_radius_is_accepted_and_the_next_refused(eng):
    f = LT.field((5, 300), salt=2)
    res = eng.local_threshold(f, 64.0, offset=-0.8, want=BOTH_WANTED)           # radius int(256.5) = 256
    assert eng.last_threshold_kernel == LT.BOTH
    ref = LT.scipy_threshold(f, 64.0, -0.8)
    _check_against_scipy("5x300-sigma64", f, _np(res["threshold"]), _np(res["mask"]), ref, LT.atol(f, 64.0))
    eng.local_threshold(f, (0.0, 64.0))
    assert eng.last_threshold_kernel == LT.ONLY_X
    for sigma in (64.2, (1.0, 64.2), (64.2, 0.0)):                                # radius 257
        with pytest.raises(ValueError, match="needs radius 257 > 256"):
            eng.local_threshold(f, sigma)
        assert eng.last_threshold_kernel == LT.ONLY_X                            # unchanged: nothing was launched


def test_the_tools_accept_param_64_and_refuse_64_2():
    from lagrangiancoherence_amd import tools
    from lagrangiancoherence_amd.dropin import get_engine
    f = LT.field((5, 300), salt=2)
    da = DataArray(f, ("latitude", "longitude"), {"latitude": np.arange(5.0), "longitude": np.arange(300.0)})
    thr = tools.threshold_local(da, block_size=301, offset=-0.8, param=64.0)
    assert np.abs(thr.values - LT.scipy_threshold(f, 64.0, -0.8)).max() <= LT.atol(f, 64.0)
    before = get_engine().last_threshold_kernel
    assert before == LT.BOTH
    with pytest.raises(ValueError, match="needs radius 257 > 256"):
        tools.threshold_local(da, block_size=301, offset=-0.8, param=64.2)
    assert get_engine().last_threshold_kernel == before


def test_nan_and_inf_spread_exactly_as_in_scipy(eng):
    f = LT.with_nan_and_inf()
    sigma = LT.sigma_of(7)
    ref = LT.scipy_threshold(f, sigma, 0.1)
    res = eng.local_threshold(f, sigma, offset=0.1, want=BOTH_WANTED)
    thr, mask = _np(res["threshold"]), _np(res["mask"])
    assert np.array_equal(np.isnan(thr), np.isnan(ref)) and np.isnan(ref).any()
    assert np.array_equal(np.isposinf(thr), np.isposinf(ref)) and np.isposinf(ref).any() and not np.isneginf(thr).any()
    ok = np.isfinite(ref)
    assert ok.sum() > 100 and np.abs(thr[ok] - ref[ok]).max() <= LT.atol(f, sigma)
    with np.errstate(invalid="ignore"):
        assert np.array_equal(mask.astype(bool), f > thr)
    assert not mask[np.isnan(thr) | np.isnan(f)].any()                           # a NaN on either side: 0
    assert mask[15, 19] == 0                                                     # +inf > +inf is false


@pytest.mark.parametrize("name", ["9x11-b301-cyclic", f"{LT.TL_RUN + 1}x{LT.TL_RUN + 1}-b61", "20x23-b1x7", "20x23-b7x1"])
def test_float32_input_equals_its_float64_widening_bit_for_bit(eng, name):
    f, sigma, offset, cyclic, _, _, _ = LT.case(name)
    f32 = f.astype(np.float32)
    a = eng.local_threshold(f32, sigma, offset=offset, cyclic=cyclic, want=BOTH_WANTED)
    b = eng.local_threshold(f32.astype(np.float64), sigma, offset=offset, cyclic=cyclic, want=BOTH_WANTED)
    assert a["threshold"].dtype == eng.torch.float64
    assert np.array_equal(_np(a["threshold"]), _np(b["threshold"])) and np.array_equal(_np(a["mask"]), _np(b["mask"]))
    assert not np.array_equal(f32.astype(np.float64), f)                         # (the widening is not the float64 field)


@pytest.mark.parametrize("name", ["3x523x531-b301", "3x523x531-b301-cyclic"])
def test_a_plane_of_a_stack_equals_the_plane_alone_bit_for_bit(eng, name):
    f, sigma, offset, cyclic, _, _, _ = LT.case(name)
    stack = eng.local_threshold(f, sigma, offset=offset, cyclic=cyclic, want=BOTH_WANTED)
    thr, mask = _np(stack["threshold"]), _np(stack["mask"])
    for m in range(f.shape[0]):
        one = eng.local_threshold(f[m], sigma, offset=offset, cyclic=cyclic, want=BOTH_WANTED)
        assert tuple(one["threshold"].shape) == f.shape[1:]
        assert np.array_equal(_np(one["threshold"]), thr[m]) and np.array_equal(_np(one["mask"]), mask[m])


@pytest.mark.parametrize("shape, sigma", [((9, 11), 50.0), ((LT.TL_RUN + 1, LT.TL_RUN + 1), 10.0), ((1, 9), 1.0), ((523, 531), 2.0),
                                          ((20, 23), 0.5), ((LT.TL_RUN + 42, 20), 1.0), ((LT.TL_RUN + 107, 20), 10.0)])
def test_offset_zero_equals_the_engines_gaussian_filter_bit_for_bit(eng, shape, sigma):
    """The arithmetic of gauss_taps.h is one: the same weights, the same sum in the same order, out of LDS here and out of
    global memory there."""
    f = LT.field(shape, salt=9)
    thr = eng.local_threshold(f, sigma, offset=0.0)["threshold"]
    assert np.array_equal(_np(thr), _np(eng.gaussian_filter(f, sigma)))


# ------------------------------------------------------------------ refusals of a real context
def test_a_real_context_refuses_before_any_launch(eng):
    torch = eng.torch
    f = eng.to_device(LT.field((20, 23)), np.float64)
    eng.local_threshold(f, (0.0, 1.0))
    assert eng.last_threshold_kernel == LT.ONLY_X
    n = f.numel()
    work = torch.empty(n, dtype=torch.float64, device=eng.device)
    thr = torch.full((n,), 7.0, dtype=torch.float64, device=eng.device)
    mask = torch.full((n,), 7, dtype=torch.uint8, device=eng.device)
    good = dict(f=f.data_ptr(), dtype=_capi.LC_F64, ny=20, nx=23, n_members=1, sigma_y=1.0, sigma_x=1.0, offset=0.0, cyclic=0,
                work=work.data_ptr(), threshold_out=thr.data_ptr(), mask_out=mask.data_ptr())
    EINVAL, EUNSUPPORTED = _capi.LC_EINVAL, _capi.LC_EUNSUPPORTED
    refusals = [(dict(struct_size=8), EINVAL, b"struct_size"),
                (dict(dtype=3), EINVAL, b"bad dtype"),
                (dict(ny=0), EINVAL, b"bad size"),
                (dict(n_members=-1), EINVAL, b"bad size"),
                (dict(ny=1 << 16, nx=1 << 15), EINVAL, b"plane too large"),
                (dict(sigma_y=float("nan")), EINVAL, b"bad sigma_y"),
                (dict(offset=float("-inf")), EINVAL, b"bad offset"),
                (dict(threshold_out=None, mask_out=None), EINVAL, b"both NULL"),
                (dict(f=None), EINVAL, b"null pointer"),
                (dict(work=None), EINVAL, b"work must hold"),
                (dict(work=f.data_ptr()), EINVAL, b"f and work overlap"),
                (dict(threshold_out=f.data_ptr() + 8), EINVAL, b"f and threshold_out overlap"),
                (dict(mask_out=thr.data_ptr() + 7 * n), EINVAL, b"threshold_out and mask_out overlap"),
                (dict(threshold_out=work.data_ptr()), EINVAL, b"work and threshold_out overlap"),
                (dict(sigma_x=64.2), EUNSUPPORTED, b"needs radius 257 > 256")]
    for change, status, message in refusals:
        a = _capi.LocalThresholdArgs(struct_size=C.sizeof(_capi.LocalThresholdArgs))
        for k, v in {**good, **change}.items():
            setattr(a, k, v)
        assert eng.lib.lc_local_threshold(eng.ctx, C.byref(a)) == status, change
        assert message in eng.lib.lc_last_error(), change
        assert eng.last_threshold_kernel == LT.ONLY_X, change                    # unchanged: the call returned before its launches
    assert eng.lib.lc_local_threshold(eng.ctx, None) == EINVAL
    torch.cuda.synchronize()
    assert bool((thr == 7.0).all()) and bool((mask == 7).all())                 # and nothing was written
    a = _capi.LocalThresholdArgs(struct_size=C.sizeof(_capi.LocalThresholdArgs))
    for k, v in good.items():
        setattr(a, k, v)
    assert eng.lib.lc_local_threshold(eng.ctx, C.byref(a)) == _capi.LC_OK and eng.last_threshold_kernel == LT.BOTH
    torch.cuda.synchronize()
    assert np.array_equal(_np(thr).reshape(20, 23), _np(eng.local_threshold(f, 1.0)["threshold"]))


# ------------------------------------------------------------------ the labelled surface
def _labelled_record():
    f = LT.field((3, 20, 23), salt=3)
    lat, lon, time = np.linspace(-10.0, 9.0, 20), np.linspace(100.0, 122.0, 23), np.arange(3.0)
    return f, lat, lon, time


def test_tools_on_a_plane_with_descending_latitude():
    from lagrangiancoherence_amd import tools
    f, lat, lon, _ = _labelled_record()
    sigma = LT.sigma_of(7)
    ref = LT.scipy_threshold(f[0], sigma, 0.25)
    tol = LT.atol(f[0], sigma)
    da = DataArray(f[0][::-1].astype(np.float32), ("latitude", "longitude"), {"latitude": lat[::-1], "longitude": lon}, name="ftle")
    thr = tools.threshold_local(da, block_size=7, offset=0.25)
    assert isinstance(thr, DataArray) and thr.dims == ("latitude", "longitude") and thr.dtype == np.float64 and thr.name == "ftle"
    assert np.array_equal(thr.coords["latitude"], lat) and np.array_equal(thr.coords["longitude"], lon)   # sorted ascending
    f32 = f[0].astype(np.float32).astype(np.float64)
    assert np.abs(thr.values - LT.scipy_threshold(f32, sigma, 0.25)).max() <= LT.atol(f32, sigma)
    above = tools.above_local_threshold(da, 7, offset=0.25)
    assert above.dtype == np.bool_ and above.dims == ("latitude", "longitude")
    assert np.array_equal(above.values, f32 > thr.values) and above.values.any() and not above.values.all()
    # longitude first: the result comes back in the caller's dimension order
    db = DataArray(f[0].T, ("longitude", "latitude"), {"latitude": lat, "longitude": lon})
    thr_t = tools.threshold_local(db, block_size=(7, 7), offset=0.25)
    assert thr_t.dims == ("longitude", "latitude") and np.abs(thr_t.values.T - ref).max() <= tol
    assert np.array_equal(tools.above_local_threshold(db, (7, 7), offset=0.25).values.T, f[0] > thr_t.values.T)


def test_tools_on_a_record_of_three_planes():
    from lagrangiancoherence_amd import tools
    f, lat, lon, time = _labelled_record()
    da = DataArray(np.moveaxis(f, 0, 1), ("latitude", "time", "longitude"), {"latitude": lat, "longitude": lon, "time": time})
    thr = tools.threshold_local(da, block_size=(7, 31), offset=-0.8, cyclic=True)
    assert thr.dims == ("latitude", "time", "longitude") and thr.shape == (20, 3, 23) and thr.dtype == np.float64
    assert np.array_equal(thr.coords["time"], time)
    sigma = LT.sigma_of((7, 31))
    assert np.abs(np.moveaxis(thr.values, 1, 0) - LT.scipy_threshold(f, sigma, -0.8, True)).max() <= LT.atol(f, sigma)
    above = tools.above_local_threshold(da, (7, 31), offset=-0.8, cyclic=True)
    assert above.dims == thr.dims and above.dtype == np.bool_ and np.array_equal(above.values, da.values > thr.values)
    for m in range(3):      # every plane on its own: never smoothed across time
        one = tools.threshold_local(da.isel(time=m), block_size=(7, 31), offset=-0.8, cyclic=True)
        assert one.dims == ("latitude", "longitude") and np.array_equal(one.values, thr.values[:, m, :])
    ints = DataArray(np.arange(20 * 23).reshape(20, 23) % 7, ("latitude", "longitude"), {"latitude": lat, "longitude": lon})
    assert tools.threshold_local(ints, block_size=3).dtype == np.float64      # any other dtype: converted to float64
