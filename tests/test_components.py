"""The component filter without a GPU: known answers that pin the host restatement tests/components.py (what the GPU tests
compare the kernels with), the three entry points in the header, the bindings and the library, and every refusal of
include/lcs_hip.h's contract -- each returned before the device is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from lagrangiancoherence_amd import _capi, build
from tests import components as CO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("lc_label_components", "lc_component_sums", "lc_component_apply")


# ------------------------------------------------------------------ the restatement itself
def test_diagonal_arms_join_only_with_corners():
    m = np.array([[1, 1, 0, 0],
                  [0, 0, 1, 0],
                  [0, 0, 1, 1]], dtype=np.float64)
    lab1, n1 = CO.label(m, 1)
    lab2, n2 = CO.label(m, 2)
    assert n1 == 2 and n2 == 1
    assert np.array_equal(lab1, [[1, 1, 0, 0], [0, 0, 2, 0], [0, 0, 2, 2]]) and np.array_equal(lab2, (m != 0).astype(np.int32))


@pytest.mark.parametrize("L", [1, 2, 7, 30])
def test_a_horizontal_bar_has_the_axis_lengths_of_its_formula(L):
    m = np.zeros((5, 40))
    m[2, 3:3 + L] = 1
    lab, n = CO.label(m)
    p = CO.props(lab, n)
    assert n == 1 and p["area"][0] == L
    assert p["major_axis_length"][0] == pytest.approx(4 * np.sqrt((L * L - 1) / 12), rel=1e-14, abs=0)
    assert p["minor_axis_length"][0] == 0
    assert tuple(p["centroid"][0]) == (2, 3 + (L - 1) / 2)
    s = CO.sums(lab, n)
    assert s["root"][0] == 2 * 40 + 3
    assert list(s["moments"][:, 0]) == [0, L * (L - 1) // 2, 0, 0, (L - 1) * L * (2 * L - 1) // 6]


def test_a_seam_pair_joins_only_when_cyclic():
    m = np.zeros((4, 9))
    m[1, 0] = m[1, 8] = 1          # straight across
    m[3, 0] = m[2, 8] = 1          # by a corner; (2, 8) touches (1, 8) by an edge
    assert CO.label(m, 2)[1] == 3 and CO.label(m, 1)[1] == 3
    lab, n = CO.label(m, 2, cyclic=True)
    assert n == 1 and np.array_equal(lab, (m != 0).astype(np.int32))
    lab, n = CO.label(m, 1, cyclic=True)
    assert n == 2 and lab[1, 0] == lab[1, 8] == lab[2, 8] == 1 and lab[3, 0] == 2   # numbered by first pixel
    # across the seam the column offsets go the shorter way round: the pair (1, 0), (1, 8) is a bar of length 2
    pair = np.zeros((4, 9))
    pair[1, 0] = pair[1, 8] = 1
    assert CO.label(pair)[1] == 2
    lab, n = CO.label(pair, 1, cyclic=True)
    p = CO.props(lab, n, cyclic=True)
    assert n == 1 and p["major_axis_length"][0] == pytest.approx(4 * np.sqrt(3 / 12)) and tuple(p["centroid"][0]) == (1, 8.5)
    assert list(CO.sums(lab, n, cyclic=True)["moments"][:, 0]) == [0, -1, 0, 0, 1]


def test_nan_is_background_and_a_negative_value_is_foreground():
    m = np.array([[np.nan, -1.0, 0.0, 2.0]])
    assert np.array_equal(CO.foreground(m), [[False, True, False, True]])
    lab, n = CO.label(m)
    assert n == 2 and np.array_equal(lab, [[0, 1, 0, 2]])
    p = CO.props(lab, n, intensity=np.array([[1.0, np.nan, 5.0, -3.0]]))
    assert np.isnan(p["mean_intensity"][0]) and np.isnan(p["max_intensity"][0]) and np.isnan(p["min_intensity"][0])
    assert (p["mean_intensity"][1], p["max_intensity"][1], p["min_intensity"][1]) == (-3.0, -3.0, -3.0)


def test_the_checkerboard_has_the_counts_the_cases_rely_on():
    board = CO.mask_of("checkerboard-96x130")
    assert CO.label(board, 1)[1] == 6240 and CO.label(board, 2)[1] == 1


def test_filtered_keeps_what_reaches_every_threshold():
    m = np.zeros((6, 12))
    m[0, 0:2] = 1
    m[2, 0:5] = 3
    m[4, 0:9] = -1
    v = np.full((6, 12), 2.0)
    v[4] = np.nan
    got = CO.filtered(m, v, ["area", "mean_intensity"], [5, 2.0], fill=np.nan)
    want = np.full((6, 12), np.nan)
    want[2, 0:5] = 3                 # the pair is too small, the NaN mean of the long bar fails
    assert np.array_equal(got, want, equal_nan=True)


# ------------------------------------------------------------------ header, bindings, library
@pytest.fixture(scope="module")
def lib():
    build.build_library(verbose=False)
    return _capi.load()


def test_the_entry_points_are_declared_prototyped_and_exported(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lcs_hip.h")).read(), flags=re.S)
    for name in ENTRY_POINTS + ("lc_label_work_elems",):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _capi.PROTOTYPES and hasattr(lib, name), name
    assert "components.hip" in build.SOURCES
    assert lib.lc_version() == 104


def test_the_sums_structure_matches_the_library(lib):
    a = _capi.ComponentSumsArgs(struct_size=C.sizeof(_capi.ComponentSumsArgs) - 8)
    assert lib.lc_component_sums(None, C.byref(a)) == _capi.LC_EINVAL and b"struct_size" in lib.lc_last_error()
    assert lib.lc_component_sums(None, None) == _capi.LC_EINVAL and b"null argument structure" in lib.lc_last_error()


def test_work_elems_is_pure_arithmetic(lib):
    assert lib.lc_label_work_elems(1, 1, 1) == 1 and lib.lc_label_work_elems(32, 32, 3) == 3
    assert lib.lc_label_work_elems(33, 65, 2) == 2 * 3 and lib.lc_label_work_elems(4096, 4096, 1) == 16384
    assert lib.lc_label_work_elems(0, 5, 1) == 0 and lib.lc_label_work_elems(5, 5, 0) == 0


# A context nobody dereferences and pointers nobody follows: every call below is refused by its argument checks.
_BLOCK = C.create_string_buffer(4096)
CTX = PTR = C.cast(_BLOCK, C.c_void_p)
GOOD = dict(ctx=CTX, dtype=_capi.LC_F64, ny=4, nx=6, n_members=2)
REFUSALS = [
    (dict(ctx=None), b"null context"),
    (dict(dtype=2), b"bad dtype"),
    (dict(dtype=-1), b"bad dtype"),
    (dict(ny=0), b"bad size"),
    (dict(nx=0), b"bad size"),
    (dict(n_members=0), b"bad size"),
    (dict(ny=-3), b"bad size"),
    (dict(ny=1 << 16, nx=1 << 15), b"plane too large"),
    (dict(ny=46341, nx=46341), b"plane too large"),
]


def _label(g, connectivity=2, mask=PTR, labels=PTR, counts=PTR, work=PTR):
    return _capi.load().lc_label_components(g["ctx"], mask, g["dtype"], g["ny"], g["nx"], g["n_members"], connectivity, 0,
                                            labels, counts, work)


def _sums(g, n_max=8, intensity=PTR, **null):
    a = _capi.ComponentSumsArgs(struct_size=C.sizeof(_capi.ComponentSumsArgs))
    for k in ("labels", "counts", "root_out", "area_out", "moments_out", "sum_out", "max_out", "min_out"):
        setattr(a, k, None if null.get(k, False) else PTR)
    a.intensity = intensity
    a.dtype, a.ny, a.nx, a.n_members, a.n_max = g["dtype"], g["ny"], g["nx"], g["n_members"], n_max
    return _capi.load().lc_component_sums(g["ctx"], C.byref(a))


def _apply(g, n_max=8, labels=PTR, mask=PTR, keep=PTR, out=PTR):
    return _capi.load().lc_component_apply(g["ctx"], labels, mask, g["dtype"], g["ny"], g["nx"], g["n_members"], keep, n_max, 0.0, out)


@pytest.mark.parametrize("call", [_label, _sums, _apply], ids=ENTRY_POINTS)
@pytest.mark.parametrize("change, message", REFUSALS, ids=["-".join(f"{k}={v}" for k, v in c.items()) for c, _ in REFUSALS])
def test_every_entry_point_refuses_bad_geometry(lib, call, change, message):
    assert call({**GOOD, **change}) == _capi.LC_EINVAL
    err = lib.lc_last_error()
    assert message in err and ENTRY_POINTS[[_label, _sums, _apply].index(call)].encode() in err


def test_the_largest_plane_that_fits_is_not_refused_for_its_size(lib):
    """2^31 - 1 pixels pass the size check: the call goes on to the next refusal (a null pointer), still before any device call."""
    g = {**GOOD, "ny": 1, "nx": (1 << 31) - 1, "n_members": 1}
    assert _label(g, mask=None) == _capi.LC_EINVAL and b"null pointer" in lib.lc_last_error()


@pytest.mark.parametrize("connectivity", [0, 3, -1, 8])
def test_label_refuses_another_connectivity(lib, connectivity):
    assert _label(GOOD, connectivity=connectivity) == _capi.LC_EINVAL
    assert b"lc_label_components: bad connectivity" in lib.lc_last_error()


@pytest.mark.parametrize("which", ["mask", "labels", "counts", "work"])
def test_label_refuses_a_null_pointer(lib, which):
    assert _label(GOOD, **{which: None}) == _capi.LC_EINVAL and b"lc_label_components: null pointer" in lib.lc_last_error()


@pytest.mark.parametrize("which", ["labels", "counts", "root_out", "area_out", "moments_out"])
def test_sums_refuses_a_null_pointer(lib, which):
    assert _sums(GOOD, **{which: True}) == _capi.LC_EINVAL and b"lc_component_sums: null pointer" in lib.lc_last_error()


@pytest.mark.parametrize("which", ["sum_out", "max_out", "min_out"])
def test_sums_with_an_intensity_needs_its_three_outputs(lib, which):
    assert _sums(GOOD, **{which: True}) == _capi.LC_EINVAL and b"lc_component_sums: null pointer" in lib.lc_last_error()


def test_sums_and_apply_refuse_a_capacity_below_one(lib):
    assert _sums(GOOD, n_max=0) == _capi.LC_EINVAL and b"lc_component_sums: bad capacity" in lib.lc_last_error()
    assert _apply(GOOD, n_max=0) == _capi.LC_EINVAL and b"lc_component_apply: bad capacity" in lib.lc_last_error()


def test_sums_refuses_a_plane_whose_second_moments_overflow(lib):
    g = {**GOOD, "ny": (1 << 31) - 1, "nx": 1, "n_members": 1}
    assert _sums(g) == _capi.LC_EINVAL and b"do not fit int64" in lib.lc_last_error()


@pytest.mark.parametrize("which", ["labels", "mask", "keep", "out"])
def test_apply_refuses_a_null_pointer(lib, which):
    assert _apply(GOOD, **{which: None}) == _capi.LC_EINVAL and b"lc_component_apply: null pointer" in lib.lc_last_error()


def test_the_kernels_never_wait_for_another_workgroup():
    """The rule of the file: what a stage needs from every workgroup of the stage before arrives with the end of that launch.
    No cooperative launch, no grid synchronisation, no loop that spins on memory another workgroup writes (the only loops on
    shared memory are the walks of find_root, which end on their own: every step goes to a smaller index)."""
    src = build._strip_comments(open(os.path.join(build.CSRC, "components.hip")).read())
    for word in ("cooperative", "grid_group", "this_grid", "hipLaunchCooperativeKernel", "__threadfence", "while ("):
        assert word not in src, word
    assert src.count("for (;;)") == 2       # find_root and unite


def test_the_shim_exports_filter_ridges():
    from LagrangianCoherence.LCS import tools as shim
    from lagrangiancoherence_amd import tools
    assert shim.filter_ridges is tools.filter_ridges and "filter_ridges" in tools.__all__
