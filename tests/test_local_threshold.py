"""The local threshold without a GPU: the host restatement of tests/local_threshold.py against scipy within the derived
tolerance, the tile constants of the case table against csrc/threshold.hip, the entry points in the header, the bindings and
the library, the refusals that need no context, the Python-side errors, and -- what makes the mask comparison of
tests/test_local_threshold_gpu.py sharp -- that no pixel of a mask case lies within the tolerance of scipy's own threshold."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from lagrangiancoherence_amd import _capi, build
from tests import local_threshold as LT
from tests.labelled import DataArray

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_CASES = [k for k in LT.CASES if not k.startswith("3x")]   # (the large case: its first plane, below)


# ------------------------------------------------------------------ the restatement against scipy
@pytest.mark.parametrize("name", HOST_CASES)
def test_the_restatement_equals_scipy_within_the_tolerance(name):
    f, sigma, offset, cyclic, _, ref, tol = LT.case(name)
    got = LT.threshold(f, sigma, offset, cyclic)
    assert got.dtype == np.float64 and got.shape == f.shape
    err = float(np.abs(got - ref).max())
    print(f"{name}: max |restatement - scipy| = {err:.3e}, atol = {tol:.3e}")
    assert err <= tol


@pytest.mark.parametrize("cyclic", [False, True], ids=["reflect", "cyclic"])
def test_the_restatement_equals_scipy_on_a_plane_of_the_drivers_case(cyclic):
    f, sigma, offset, _, _, ref, tol = LT.case("3x523x531-b301-cyclic" if cyclic else "3x523x531-b301")
    err = float(np.abs(LT.threshold(f[1], sigma, offset, cyclic) - ref[1]).max())
    print(f"max |restatement - scipy| = {err:.3e}, atol = {tol:.3e}")
    assert err <= tol


def test_the_restatement_follows_scipy_through_nan_and_inf():
    f = LT.with_nan_and_inf()
    sigma = LT.sigma_of(7)
    got, ref = LT.threshold(f, sigma, 0.1), LT.scipy_threshold(f, sigma, 0.1)
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.isnan(ref).any() and not np.isnan(ref).all()
    assert np.array_equal(np.isposinf(got), np.isposinf(ref)) and np.isposinf(ref).any() and not np.isneginf(ref).any()
    ok = np.isfinite(ref)
    assert ok.any() and np.abs(got[ok] - ref[ok]).max() <= LT.atol(f, sigma)


def test_the_fold_and_the_weights_are_scipys():
    from scipy import ndimage
    for n, far in ((4, 9), (1, 3), (11, 200), (9, 257)):        # numpy's padding folds at any distance too
        q = np.arange(-far, n + far)
        assert np.array_equal(LT.fold(q, n), np.pad(np.arange(n), far, mode="symmetric"))
        assert np.array_equal(LT.fold(q, n, periodic=True), np.pad(np.arange(n), far, mode="wrap"))
    assert np.array_equal(LT.fold(np.arange(-5, 9), 4), [3, 3, 2, 1, 0, 0, 1, 2, 3, 3, 2, 1, 0, 0])
    for sigma in (1.0, 10.0, 50.0, 64.0):
        r = LT.radius(sigma)
        delta = np.zeros(2 * r + 1)
        delta[r] = 1.0
        assert np.abs(LT.weights(sigma) - ndimage.gaussian_filter1d(delta, sigma, mode="constant")[r:]).max() < 2.0 ** -52
    assert (LT.radius(50.0), LT.radius(64.0), LT.radius(64.2)) == (200, LT.MAX_RADIUS, LT.MAX_RADIUS + 1)
    assert LT.sigma_of(301) == (50.0, 50.0) and LT.sigma_of((1, 7)) == (0.0, 1.0)


@pytest.mark.parametrize("name", LT.MASK_CASES)
def test_no_pixel_of_a_mask_case_is_within_the_tolerance_of_its_threshold(name):
    """With this the cap on undecided pixels in the GPU test cannot hide a failure: there are none to excuse."""
    f, _, _, _, _, ref, tol = LT.case(name)
    assert int(LT.undecided(f, ref, tol).sum()) == 0
    above = f > ref
    if f.size > 100:
        assert above.any() and not above.all()      # the mask is not trivial


# ------------------------------------------------------------------ the case table against the kernel
def test_the_tile_constants_of_the_case_table_are_the_kernels():
    src = build._strip_comments(open(os.path.join(build.CSRC, "threshold.hip")).read())

    def constant(name):
        return re.search(r"constexpr int %s = ([^;]+);" % name, src).group(1)
    assert int(constant("TL_THREADS")) == LT.TL_THREADS and int(constant("TL_RUN")) == LT.TL_RUN
    assert int(constant("TL_LINES")) == LT.TL_LINES
    assert constant("TL_PITCH") == "TL_RUN + 2 * GAUSS_W_CAPACITY"
    taps = build._strip_comments(open(os.path.join(build.CSRC, "gauss_taps.h")).read())
    assert int(re.search(r"constexpr int GAUSS_W_CAPACITY = (\d+);", taps).group(1)) == LT.MAX_RADIUS
    assert LT.TL_PITCH == LT.TL_RUN + 2 * LT.MAX_RADIUS
    assert LT.TL_LINES * LT.TL_PITCH * 8 <= 64 * 1024            # the tile: at most 64 KiB at every radius up to 256
    assert LT.TL_RUN * LT.TL_LINES == 8 * LT.TL_THREADS          # 8 outputs per thread
    assert "__shared__ double tile[TL_LINES * TL_PITCH]" in src and "extern __shared__" not in src


def test_the_tap_loop_reads_lds_only_and_shares_the_arithmetic_of_gauss_taps():
    taps = build._strip_comments(open(os.path.join(build.CSRC, "gauss_taps.h")).read())
    body = taps[taps.index("void gauss_taps_lds("):]
    body = body[:body.index("} // namespace") if "} // namespace" in body else len(body)]
    assert "%" not in body and "/" not in body and "reflect_index" not in body
    assert "acc[n] = centre[n * NEXT] * G.w[0];" in body and "for (int j = G.radius; j >= 1; --j)" in body
    assert "acc[n] += (lo[n * NEXT] + hi[n * NEXT]) * w;" in body
    src = build._strip_comments(open(os.path.join(build.CSRC, "threshold.hip")).read())
    assert src.count("gauss_taps_lds<") == 2 and "gauss_fill_weights(" in src and '#include "gauss_taps.h"' in src
    assert len(re.findall(r"__global__", src)) == 1 and "template <int AXIS> __global__" in src and "gauss_line_kernel" in src
    for word in ("cooperative", "grid_group", "this_grid", "__threadfence", "atomic", "while (", "for (;;)", "asm"):
        assert word not in src, word


# ------------------------------------------------------------------ header, bindings, library
@pytest.fixture(scope="module")
def lib():
    build.build_library(verbose=False)
    return _capi.load()


def test_the_entry_points_are_declared_prototyped_and_exported(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lcs_hip.h")).read(), flags=re.S)
    for name in ("lc_local_threshold", "lc_local_threshold_work_elems", "lc_ctx_last_threshold_kernel"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _capi.PROTOTYPES and hasattr(lib, name), name
    assert "threshold.hip" in build.SOURCES
    assert lib.lc_version() == 104 == _capi.LC_VERSION


def test_the_header_states_the_contract():
    text = " ".join(open(os.path.join(ROOT, "include", "lcs_hip.h")).read().split())
    section = text[text.index("adaptive local threshold"):text.index("int lc_local_threshold(")]
    for phrase in ("LCS/area_of_influence.py:194-199", "sigma <= 1e-15", "a NaN on either side gives 0", "one rounding",
                   "no threshold plane is written", "a radius above 256", "No kernel of this call waits for another workgroup"):
        assert phrase in section, phrase


def test_work_elems_is_pure_arithmetic(lib):
    assert lib.lc_local_threshold_work_elems(1, 1, 1) == 1 and lib.lc_local_threshold_work_elems(541, 781, 29) == 541 * 781 * 29
    assert lib.lc_local_threshold_work_elems(46340, 46340, 3) == 3 * 46340 ** 2
    assert lib.lc_local_threshold_work_elems(0, 5, 1) == 0 and lib.lc_local_threshold_work_elems(5, -1, 1) == 0
    assert lib.lc_local_threshold_work_elems(5, 5, 0) == 0


def test_the_structure_matches_the_library(lib):
    a = _capi.LocalThresholdArgs(struct_size=C.sizeof(_capi.LocalThresholdArgs) - 8)
    assert lib.lc_local_threshold(CTX, C.byref(a)) == _capi.LC_EINVAL and b"struct_size" in lib.lc_last_error()
    assert lib.lc_local_threshold(CTX, None) == _capi.LC_EINVAL and b"null argument structure" in lib.lc_last_error()
    assert lib.lc_local_threshold(None, None) == _capi.LC_EINVAL and b"null context" in lib.lc_last_error()
    a.struct_size = C.sizeof(_capi.LocalThresholdArgs)
    assert lib.lc_local_threshold(None, C.byref(a)) == _capi.LC_EINVAL and b"null context" in lib.lc_last_error()
    assert lib.lc_ctx_last_threshold_kernel(None) == b""


# A context nobody dereferences and pointers nobody follows: every call below is refused by its argument checks.
_BLOCK = C.create_string_buffer(1 << 16)
CTX = C.cast(_BLOCK, C.c_void_p)


def _at(offset):
    return C.c_void_p(C.addressof(_BLOCK) + offset)


# 4 x 6 x 2 float64: f 384 bytes at 0, work 384 at 1024, threshold 384 at 2048, mask 48 at 3072
GOOD = dict(ctx=CTX, dtype=_capi.LC_F64, ny=4, nx=6, n_members=2, sigma_y=1.0, sigma_x=1.0, offset=0.0, cyclic=0,
            f=_at(0), work=_at(1024), threshold_out=_at(2048), mask_out=_at(3072))
EINVAL, EUNSUPPORTED = _capi.LC_EINVAL, _capi.LC_EUNSUPPORTED
REFUSALS = [
    (dict(ctx=None), EINVAL, b"null context"),
    (dict(dtype=2), EINVAL, b"bad dtype"),
    (dict(dtype=-1), EINVAL, b"bad dtype"),
    (dict(ny=0), EINVAL, b"bad size"),
    (dict(nx=-2), EINVAL, b"bad size"),
    (dict(n_members=0), EINVAL, b"bad size"),
    (dict(ny=1 << 17, nx=1 << 14), EINVAL, b"plane too large"),
    (dict(ny=46341, nx=46341), EINVAL, b"plane too large"),
    (dict(sigma_y=float("nan")), EINVAL, b"bad sigma_y"),
    (dict(sigma_x=float("nan")), EINVAL, b"bad sigma_x"),
    (dict(offset=float("inf")), EINVAL, b"bad offset"),
    (dict(offset=float("nan")), EINVAL, b"bad offset"),
    (dict(threshold_out=None, mask_out=None), EINVAL, b"both NULL"),
    (dict(f=None), EINVAL, b"null pointer"),
    (dict(work=None), EINVAL, b"work must hold"),
    (dict(work=_at(8)), EINVAL, b"f and work overlap"),
    (dict(threshold_out=_at(376)), EINVAL, b"f and threshold_out overlap"),
    (dict(mask_out=_at(383)), EINVAL, b"f and mask_out overlap"),
    (dict(threshold_out=_at(1024 + 383)), EINVAL, b"work and threshold_out overlap"),
    (dict(mask_out=_at(1024)), EINVAL, b"work and mask_out overlap"),
    (dict(mask_out=_at(2048 + 383)), EINVAL, b"threshold_out and mask_out overlap"),
    (dict(sigma_y=64.2), EUNSUPPORTED, b"needs radius 257 > 256"),
    (dict(sigma_x=float("inf")), EUNSUPPORTED, b"needs radius inf > 256"),
    (dict(ny=(1 << 31) - 1, nx=1, n_members=64, f=C.c_void_p(1 << 42), work=C.c_void_p(2 << 42), threshold_out=C.c_void_p(3 << 42),
          mask_out=C.c_void_p(4 << 42)), EINVAL, b"too many planes"),
]


def _call(g):
    a = _capi.LocalThresholdArgs(struct_size=C.sizeof(_capi.LocalThresholdArgs))
    for k, v in g.items():
        if k != "ctx":
            setattr(a, k, v)
    return _capi.load().lc_local_threshold(g["ctx"], C.byref(a))


def _id(change):
    """A pointer into _BLOCK shows as its offset: the block's address differs from process to process, a test's name must not."""
    def show(v):
        v = getattr(v, "value", v)
        inside = isinstance(v, int) and 0 <= v - C.addressof(_BLOCK) < C.sizeof(_BLOCK)
        return f"block+{v - C.addressof(_BLOCK)}" if inside else v
    return "-".join(f"{k}={show(v)}" for k, v in change.items())


@pytest.mark.parametrize("change, status, message", REFUSALS, ids=[_id(c) for c, _, _ in REFUSALS])
def test_the_call_refuses_before_it_touches_a_device(lib, change, status, message):
    assert _call({**GOOD, **change}) == status
    err = lib.lc_last_error()
    assert message in err and b"lc_local_threshold" in err


def test_buffers_that_only_touch_are_not_an_overlap(lib):
    """f ends where work begins, and so on down the line: the call goes on to the one refusal that comes after the overlap
    check (more workgroups than a launch has), still before any device call."""
    ny, n = (1 << 31) - 1, 64
    points, base = ny * n, 1 << 42
    g = {**GOOD, "ny": ny, "nx": 1, "n_members": n, "f": C.c_void_p(base), "work": C.c_void_p(base + 8 * points),
         "threshold_out": C.c_void_p(base + 16 * points), "mask_out": C.c_void_p(base + 24 * points)}
    assert _call(g) == EINVAL and b"too many planes" in lib.lc_last_error()
    g["mask_out"] = C.c_void_p(base + 24 * points - 1)
    assert _call(g) == EINVAL and b"threshold_out and mask_out overlap" in lib.lc_last_error()


# ------------------------------------------------------------------ the Python surface
def test_the_shim_exports_both_functions():
    from LagrangianCoherence.LCS import tools as shim
    from lagrangiancoherence_amd import tools
    assert shim.threshold_local is tools.threshold_local and shim.above_local_threshold is tools.above_local_threshold
    assert "threshold_local" in tools.__all__ and "above_local_threshold" in tools.__all__
    assert "threshold_local" in tools.__doc__ and "LCS/area_of_influence.py:194-199" in tools.__doc__
    import inspect
    assert list(inspect.signature(tools.threshold_local).parameters) == ["da", "block_size", "method", "offset", "mode", "param",
                                                                         "cval", "cyclic"]
    assert list(inspect.signature(tools.above_local_threshold).parameters) == ["da", "block_size", "offset", "param", "cyclic"]


def test_the_python_side_errors_come_before_any_device():
    from lagrangiancoherence_amd import tools
    da = DataArray(np.ones((4, 5)), ("latitude", "longitude"), {"latitude": np.arange(4.0), "longitude": np.arange(5.0)})
    for bad in (4, (3, 4), (300, 301)):
        with pytest.raises(ValueError, match="odd"):
            tools.threshold_local(da, block_size=bad)
        with pytest.raises(ValueError, match="odd"):
            tools.above_local_threshold(da, bad)
    with pytest.raises(ValueError):
        tools.threshold_local(da, block_size=(3, 3, 3))
    for method in ("mean", "median", "generic"):
        with pytest.raises(NotImplementedError, match="method"):
            tools.threshold_local(da, block_size=3, method=method)
    for mode in ("constant", "nearest", "mirror", "wrap"):
        with pytest.raises(NotImplementedError, match="mode"):
            tools.threshold_local(da, block_size=3, mode=mode)
    bad_dims = DataArray(np.ones((2, 2, 4, 5)), ("a", "b", "latitude", "longitude"),
                         {"latitude": np.arange(4.0), "longitude": np.arange(5.0)})
    with pytest.raises(ValueError, match="dims"):
        tools.threshold_local(bad_dims, block_size=3)


def test_the_engine_checks_want_and_sigma_before_any_device():
    from lagrangiancoherence_amd.engine import Engine
    eng = Engine.__new__(Engine)             # no device: the checks come before anything is touched
    for want in ((), ("smooth",), ("threshold", "dist")):
        with pytest.raises(ValueError, match="want"):
            eng.local_threshold(np.ones((2, 2)), 1.0, want=want)
    with pytest.raises(ValueError, match="sigma"):
        eng.local_threshold(np.ones((2, 2)), (1.0, 2.0, 3.0))
