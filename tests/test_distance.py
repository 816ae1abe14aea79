"""The distance transform without a GPU: the two host oracles of tests/distance.py against each other (the brute-force minimum
of the kernels' cost expression equals scipy.ndimage.distance_transform_edt bit for bit, so either pins the kernels), the entry
point in the header, the bindings and the library, and every refusal of include/lcs_hip.h's contract -- each returned before
the device is touched."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from lagrangiancoherence_amd import _capi, build
from tests import distance as DT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (1, 37), (37, 1), (67, 130), (130, 67), (20, 13)]
DENSITIES = [0.002, 0.02, 0.2, 0.9]
PLANES = [(s, d) for s in SHAPES for d in DENSITIES]
IDS = [f"{ny}x{nx}-{d}" for (ny, nx), d in PLANES]


@functools.lru_cache(maxsize=None)
def _plane(shape, density):
    m = DT.random(*shape, density)
    m.setflags(write=False)
    return m


# ------------------------------------------------------------------ the oracles against each other
@pytest.mark.parametrize("shape, density", PLANES, ids=IDS)
def test_brute_force_equals_scipy_at_unit_sampling(shape, density):
    m = _plane(shape, density)
    dist, nearest = DT.brute(m)
    assert dist.dtype == np.float64 and np.array_equal(dist, DT.scipy_edt(m))
    fg = DT.foreground(m)
    assert fg.ravel()[nearest.ravel()].all() and np.array_equal(nearest[fg], np.flatnonzero(fg))
    r, c = np.divmod(np.arange(m.size), m.shape[1])
    fr, fc = np.divmod(nearest.ravel(), m.shape[1])
    assert np.array_equal(np.sqrt(DT.cost_of(r - fr, c - fc)), dist.ravel())


@pytest.mark.parametrize("shape, density", PLANES, ids=IDS)
def test_brute_force_equals_scipy_on_the_tiled_plane_when_cyclic(shape, density):
    m = _plane(shape, density)
    assert np.array_equal(DT.brute(m, cyclic=True)[0], DT.scipy_edt(m, cyclic=True))


@pytest.mark.parametrize("sampling", DT.SAMPLINGS, ids=[f"{a}x{b}" for a, b in DT.SAMPLINGS])
@pytest.mark.parametrize("shape, density", PLANES, ids=IDS)
def test_brute_force_equals_scipy_under_a_sampling(shape, density, sampling):
    m = _plane(shape, density)
    assert np.array_equal(DT.brute(m, sampling=sampling)[0], DT.scipy_edt(m, sampling=sampling))


def test_known_answers_of_the_brute_force_oracle():
    m = np.zeros((3, 5))
    m[1, 1] = m[1, 3] = 1
    dist, nearest = DT.brute(m)
    assert np.array_equal(dist[1], [1, 0, 1, 0, 1]) and np.array_equal(dist[0], np.sqrt([2, 1, 2, 1, 2]))
    assert np.array_equal(nearest[1], [6, 6, 6, 8, 8]) and nearest[0, 2] == 6          # the tie goes to the smaller index
    dist, nearest = DT.brute(m, cyclic=True, sampling=(1.0, 2.0), max_distance=2.0)
    assert np.array_equal(dist[1], [2, 0, 2, 0, 2]) and np.isinf(dist[0, 0]) and nearest[0, 0] == -1 and nearest[1, 4] == 8
    m = np.zeros((2, 6))
    m[0, 0] = 1
    assert DT.brute(m, cyclic=True)[0][0, 5] == 1 and DT.brute(m)[0][0, 5] == 5
    dist, nearest = DT.brute(np.zeros((2, 3)))
    assert np.isinf(dist).all() and (nearest == -1).all()
    assert np.array_equal(DT.foreground(np.array([[np.nan, -1.0, 0.0]])), [[False, True, False]])


def test_every_named_plane_is_what_its_test_needs():
    for name in DT.EMPTY:
        assert not DT.foreground(DT.mask_of(name)).any(), name
    for name in {**DT.SMALL, **DT.LARGE, **DT.CYCLIC}:
        assert DT.foreground(DT.mask_of(name)).any(), name
    m = DT.mask_of("nan-negative")
    assert np.isnan(m).any() and (m < 0).any() and (m > 0).any()
    assert np.count_nonzero(DT.mask_of("corners-67x130")) == 4


# ------------------------------------------------------------------ header, bindings, library
@pytest.fixture(scope="module")
def lib():
    build.build_library(verbose=False)
    return _capi.load()


def test_the_entry_point_is_declared_prototyped_and_exported(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lcs_hip.h")).read(), flags=re.S)
    for name in ("lc_distance_transform", "lc_distance_work_elems"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _capi.PROTOTYPES and hasattr(lib, name), name
    assert "distance.hip" in build.SOURCES
    assert lib.lc_version() == 104 == _capi.LC_VERSION


def test_the_header_states_the_contract():
    text = " ".join(open(os.path.join(ROOT, "include", "lcs_hip.h")).read().split())
    section = text[text.index("distance to the nearest ridge pixel"):text.index("int lc_distance_transform(")]
    for phrase in ("LCS/area_of_influence.py:231", "!= 0 and not NaN", "smallest linear index", "+inf everywhere", "nx <= 16384",
                   "No kernel of this call waits for another workgroup"):
        assert phrase in section, phrase


def test_work_elems_is_pure_arithmetic(lib):
    # the offsets of every pixel, and two summaries per column of each segment of 64 rows
    assert lib.lc_distance_work_elems(1, 1, 1) == 3 and lib.lc_distance_work_elems(64, 10, 1) == 660
    assert lib.lc_distance_work_elems(65, 10, 3) == 3 * (650 + 40) and lib.lc_distance_work_elems(4096, 4096, 1) == 4096 * (4096 + 128)
    assert lib.lc_distance_work_elems(0, 5, 1) == 0 and lib.lc_distance_work_elems(5, -1, 1) == 0 and lib.lc_distance_work_elems(5, 5, 0) == 0


def test_the_structure_matches_the_library(lib):
    a = _capi.DistanceArgs(struct_size=C.sizeof(_capi.DistanceArgs) - 8)
    assert lib.lc_distance_transform(CTX, C.byref(a)) == _capi.LC_EINVAL and b"struct_size" in lib.lc_last_error()
    assert lib.lc_distance_transform(CTX, None) == _capi.LC_EINVAL and b"null argument structure" in lib.lc_last_error()
    assert lib.lc_distance_transform(None, None) == _capi.LC_EINVAL and b"null context" in lib.lc_last_error()


# A context nobody dereferences and pointers nobody follows: every call below is refused by its argument checks.
_BLOCK = C.create_string_buffer(4096)
CTX = PTR = C.cast(_BLOCK, C.c_void_p)
GOOD = dict(ctx=CTX, dtype=_capi.LC_F64, ny=4, nx=6, n_members=2, sampling_y=1.0, sampling_x=1.0, max_distance=0.0,
            mask=PTR, dist_out=PTR, nearest_out=None, work_dev=PTR)
EINVAL, EUNSUPPORTED = _capi.LC_EINVAL, _capi.LC_EUNSUPPORTED
REFUSALS = [
    (dict(ctx=None), EINVAL, b"null context"),
    (dict(dtype=2), EINVAL, b"bad dtype"),
    (dict(dtype=-1), EINVAL, b"bad dtype"),
    (dict(ny=0), EINVAL, b"bad size"),
    (dict(nx=0), EINVAL, b"bad size"),
    (dict(n_members=0), EINVAL, b"bad size"),
    (dict(ny=-3), EINVAL, b"bad size"),
    (dict(ny=1 << 17, nx=1 << 14), EINVAL, b"plane too large"),
    (dict(ny=46341, nx=46341), EINVAL, b"plane too large"),
    (dict(nx=16385), EUNSUPPORTED, b"plane too wide"),
    (dict(ny=1, nx=(1 << 31) - 1), EUNSUPPORTED, b"plane too wide"),
    (dict(sampling_y=0.0), EINVAL, b"bad sampling"),
    (dict(sampling_x=-1.0), EINVAL, b"bad sampling"),
    (dict(sampling_y=float("inf")), EINVAL, b"bad sampling"),
    (dict(sampling_x=float("nan")), EINVAL, b"bad sampling"),
    (dict(max_distance=float("nan")), EINVAL, b"bad max_distance"),
    (dict(ny=(1 << 31) - 1, nx=1, n_members=2), EINVAL, b"too many planes"),
    (dict(mask=None), EINVAL, b"null pointer"),
    (dict(dist_out=None), EINVAL, b"null pointer"),
    (dict(work_dev=None), EINVAL, b"null pointer"),
]


def _call(g):
    a = _capi.DistanceArgs(struct_size=C.sizeof(_capi.DistanceArgs))
    for k, v in g.items():
        if k != "ctx":
            setattr(a, k, v)
    return _capi.load().lc_distance_transform(g["ctx"], C.byref(a))


@pytest.mark.parametrize("change, status, message", REFUSALS, ids=["-".join(f"{k}={v}" for k, v in c.items()) for c, _, _ in REFUSALS])
def test_the_call_refuses_before_it_touches_a_device(lib, change, status, message):
    assert _call({**GOOD, **change}) == status
    err = lib.lc_last_error()
    assert message in err and b"lc_distance_transform" in err


def test_the_widest_plane_is_not_refused_for_its_width(lib):
    """nx = 16384 passes the width check and 2^31 - 16384 pixels the size check: the call goes on to the next refusal (a null
    pointer), still before any device call."""
    g = {**GOOD, "ny": (1 << 17) - 1, "nx": 16384, "n_members": 1, "mask": None}
    assert _call(g) == EINVAL and b"null pointer" in lib.lc_last_error()


def test_the_kernels_never_wait_for_another_workgroup():
    """The rule of components.hip holds here too, and more simply: no atomic at all, no cooperative launch, no grid
    synchronisation, no loop without a counted end."""
    src = build._strip_comments(open(os.path.join(build.CSRC, "distance.hip")).read())
    for word in ("cooperative", "grid_group", "this_grid", "hipLaunchCooperativeKernel", "__threadfence", "atomic", "while (", "for (;;)"):
        assert word not in src, word


def test_the_engine_refuses_a_bound_that_is_not_positive():
    from lagrangiancoherence_amd.engine import Engine
    eng = Engine.__new__(Engine)             # no device: the check comes before anything is touched
    for bad in (0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="max_distance"):
            eng.distance_transform(np.ones((2, 2)), max_distance=bad)
    with pytest.raises(ValueError):
        eng.distance_transform(np.ones((2, 2)), sampling=(1.0, 2.0, 3.0))


def test_the_shim_exports_distance_to_ridges():
    from LagrangianCoherence.LCS import tools as shim
    from lagrangiancoherence_amd import tools
    assert shim.distance_to_ridges is tools.distance_to_ridges and "distance_to_ridges" in tools.__all__
    assert "great-circle" in " ".join(tools.distance_to_ridges.__doc__.split())
