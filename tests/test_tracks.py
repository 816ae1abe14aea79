"""Ridge tracking without a GPU: the host restatement tests/tracks.py (what the GPU tests compare the kernels with) against
scipy.ndimage.label and hand-made known answers, the three entry points in the header, the bindings and the library, every
refusal of include/lcs_hip.h's contract -- each returned before the device is touched --, the argument checks of the two tools
functions, which run before an engine exists, and the file rule of csrc/tracks.hip."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from lagrangiancoherence_amd import _capi, build
from tests import tracks as TR
from tests.labelled import DataArray

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("lc_label_tracks", "lc_track_spans")


# ------------------------------------------------------------------ the restatement itself
@pytest.mark.parametrize("reach", [0, 1])
@pytest.mark.parametrize("connectivity", [1, 2])
def test_the_oracle_equals_scipy_label_with_the_matching_structure(connectivity, reach):
    from scipy import ndimage
    for draw in range(20):
        m = TR.random_record((5, 7, 9), 0.25, salt=draw)
        want, n = ndimage.label(m, structure=TR.structure(connectivity, reach))
        got, count = TR.label(m, connectivity, False, reach)
        assert count == n and got.dtype == np.int32 and np.array_equal(got, want), draw


def test_the_structures_are_scipys_own_at_the_two_named_corners():
    from scipy import ndimage
    assert np.array_equal(TR.structure(2, 1), ndimage.generate_binary_structure(3, 3))
    assert np.array_equal(TR.structure(1, 0), ndimage.generate_binary_structure(3, 1))


def test_a_blob_stepping_one_column_per_plane_is_one_track_only_within_reach():
    m = TR.moving_blob(6, 5, 12, step=1, size=1)
    lab, n = TR.label(m, 2, False, 1)
    assert n == 1 and np.array_equal(lab, (m != 0).astype(np.int32))
    lab, n = TR.label(m, 2, False, 0)
    assert n == 6 and [int(lab[t].max()) for t in range(6)] == [1, 2, 3, 4, 5, 6]
    s = TR.spans(lab, n)
    assert list(s["first"]) == list(s["last"]) == list(range(6)) and list(s["duration"]) == [1] * 6 and list(s["volume"]) == [1] * 6
    two = TR.moving_blob(6, 5, 16, step=2, size=1)
    assert TR.label(two, 2, False, 1)[1] == 6 and TR.label(two, 2, False, 2)[1] == 1


def test_ridges_that_meet_in_the_last_plane_carry_the_smaller_first_voxels_label():
    m = TR.meeting_ridges()
    lab, n = TR.label(m, 1, False, 0)
    assert n == 1 and np.array_equal(lab, (m != 0).astype(np.int32))
    apart, n = TR.label(m[:-1], 1, False, 0)                      # without the plane that joins them
    assert n == 2 and (apart[:, 1][m[:-1, 1] != 0] == 1).all() and (apart[:, 3][m[:-1, 3] != 0] == 2).all()
    s = TR.spans(apart, n)
    assert list(s["first"]) == [0, 1] and list(s["last"]) == [2, 2] and list(s["duration"]) == [3, 2] and list(s["volume"]) == [9, 6]


def test_the_seam_joins_in_time_only_when_cyclic_and_within_reach():
    m = TR.seam_in_time(4, 9)
    assert TR.label(m, 2, False, 1)[1] == 2 and TR.label(m, 2, True, 0)[1] == 2 and TR.label(m, 2, True, 1)[1] == 1
    d = TR.seam_in_time(5, 9, rows_apart=2)
    assert TR.label(d, 2, True, 1)[1] == 2 and TR.label(d, 2, True, 2)[1] == 1
    # the shorter way round: columns 1 and nx - 2 are three apart across the seam
    e = np.zeros((2, 1, 9))
    e[0, 0, 1] = e[1, 0, 7] = 1
    assert TR.label(e, 2, True, 2)[1] == 2 and TR.label(e, 2, True, 3)[1] == 1 and TR.label(e, 2, False, 5)[1] == 2


def test_nan_and_both_zeros_are_background_and_negative_values_foreground():
    m = np.array([[[np.nan, -1.0, 0.0, -0.0, 2.0]]])
    assert np.array_equal(TR.foreground(m), [[[False, True, False, False, True]]])
    assert np.array_equal(TR.label(m)[0], [[[0, 1, 0, 0, 2]]])


def test_filtered_and_tracked_drop_the_short_tracks_and_renumber_the_rest():
    m = np.zeros((4, 3, 8))
    m[0, 0, 0] = 5           # one plane
    m[:, 1, 3] = 2           # four planes
    m[1:3, 2, 6] = -1        # two planes
    got = TR.filtered(m, min_duration=2, reach=0, fill=np.nan)
    want = np.full(m.shape, np.nan)
    want[:, 1, 3], want[1:3, 2, 6] = 2, -1
    assert np.array_equal(got, want, equal_nan=True)
    assert np.array_equal(TR.filtered(m, min_volume=3, reach=0) != 0, m == 2)
    ids, table = TR.tracked(m, reach=0, min_duration=2)
    assert ids[0, 0, 0] == 0 and (ids[:, 1, 3] == 1).all() and (ids[1:3, 2, 6] == 2).all() and ids.max() == 2
    assert list(table["first"]) == [0, 1] and list(table["last"]) == [3, 2] and list(table["volume"]) == [4, 2]
    ids, table = TR.tracked(m, reach=0, min_duration=5)
    assert not ids.any() and all(v.size == 0 for v in table.values())


# ------------------------------------------------------------------ header, bindings, library
@pytest.fixture(scope="module")
def lib():
    build.build_library(verbose=False)
    return _capi.load()


def test_the_entry_points_are_declared_prototyped_and_exported(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lcs_hip.h")).read(), flags=re.S)
    for name in ENTRY_POINTS + ("lc_track_work_elems",):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _capi.PROTOTYPES and hasattr(lib, name), name
    assert "tracks.hip" in build.SOURCES
    assert lib.lc_version() == 104 == _capi.LC_VERSION
    assert re.search(r"#define\s+LC_TRACK_MAX_REACH\s+16\b", header) and _capi.LC_TRACK_MAX_REACH == 16


def test_the_spans_structure_matches_the_library(lib):
    a = _capi.TrackSpansArgs(struct_size=C.sizeof(_capi.TrackSpansArgs) - 8)
    assert lib.lc_track_spans(None, C.byref(a)) == _capi.LC_EINVAL and b"struct_size" in lib.lc_last_error()
    assert lib.lc_track_spans(None, None) == _capi.LC_EINVAL and b"lc_track_spans: null argument structure" in lib.lc_last_error()
    a.struct_size = C.sizeof(_capi.TrackSpansArgs)                 # the right size goes on to the next check
    assert lib.lc_track_spans(None, C.byref(a)) == _capi.LC_EINVAL and b"lc_track_spans: null context" in lib.lc_last_error()


def test_work_elems_is_pure_arithmetic(lib):
    w = lib.lc_track_work_elems
    assert w(1, 1, 1) == 1 and w(32, 32, 1) == 1 and w(32, 32, 3) == 3 and w(13, 17, 5) == 2
    assert w(33, 65, 3) == 7 and w(260, 257, 4) == 262 and w(721, 1440, 120) == (120 * 721 * 1440 + 1023) // 1024
    assert w(1, (1 << 31) - 1, 1) == 1 << 21 and w(1 << 10, 1 << 10, (1 << 11) - 1) == (1 << 21) - 1024
    assert w(0, 5, 1) == 0 and w(5, 0, 1) == 0 and w(5, 5, 0) == 0 and w(-1, 5, 5) == 0
    assert w(1 << 10, 1 << 10, 1 << 11) == 0 and w(1 << 16, 1 << 15, 1) == 0 and w((1 << 31) - 1, (1 << 31) - 1, (1 << 31) - 1) == 0


# A context nobody dereferences and pointers nobody follows: every call below is refused by its argument checks.
_BLOCK = C.create_string_buffer(4096)
CTX = PTR = C.cast(_BLOCK, C.c_void_p)
GOOD = dict(ctx=CTX, dtype=_capi.LC_F64, ny=4, nx=6, n_times=3)
GEOMETRY = [
    (dict(ctx=None), b"null context"),
    (dict(ny=0), b"bad size"),
    (dict(nx=0), b"bad size"),
    (dict(n_times=0), b"bad size"),
    (dict(ny=-3), b"bad size"),
    (dict(ny=1 << 16, nx=1 << 15, n_times=1), b"record too large"),
    (dict(ny=1 << 10, nx=1 << 10, n_times=1 << 11), b"record too large"),
    (dict(ny=46341, nx=46341, n_times=46341), b"record too large"),
]


def _label(g, connectivity=2, reach=1, mask=PTR, labels=PTR, count=PTR, work=PTR):
    return _capi.load().lc_label_tracks(g["ctx"], mask, g["dtype"], g["ny"], g["nx"], g["n_times"], connectivity, 0, reach,
                                        labels, count, work)


def _spans(g, n_max=8, **null):
    a = _capi.TrackSpansArgs(struct_size=C.sizeof(_capi.TrackSpansArgs))
    for k in ("labels", "count", "first_out", "last_out", "volume_out"):
        setattr(a, k, None if null.get(k, False) else PTR)
    a.ny, a.nx, a.n_times, a.n_max = g["ny"], g["nx"], g["n_times"], n_max
    return _capi.load().lc_track_spans(g["ctx"], C.byref(a))


@pytest.mark.parametrize("call", [_label, _spans], ids=ENTRY_POINTS)
@pytest.mark.parametrize("change, message", GEOMETRY, ids=["-".join(f"{k}={v}" for k, v in c.items()) for c, _ in GEOMETRY])
def test_every_entry_point_refuses_bad_geometry(lib, call, change, message):
    assert call({**GOOD, **change}) == _capi.LC_EINVAL
    err = lib.lc_last_error()
    assert message in err and ENTRY_POINTS[[_label, _spans].index(call)].encode() in err


@pytest.mark.parametrize("dtype", [2, -1])
def test_label_refuses_another_dtype(lib, dtype):
    assert _label({**GOOD, "dtype": dtype}) == _capi.LC_EINVAL and b"lc_label_tracks: bad dtype" in lib.lc_last_error()


def test_the_largest_record_that_fits_is_not_refused_for_its_size(lib):
    """2^31 - 1 voxels pass the size check: the call goes on to the next refusal (a null pointer), still before any device call."""
    for shape in (dict(ny=1, nx=(1 << 31) - 1, n_times=1), dict(ny=1, nx=1, n_times=(1 << 31) - 1), dict(ny=(1 << 10), nx=(1 << 10), n_times=(1 << 11) - 1)):
        assert _label({**GOOD, **shape}, mask=None) == _capi.LC_EINVAL and b"lc_label_tracks: null pointer" in lib.lc_last_error()
        assert _spans({**GOOD, **shape}, labels=True) == _capi.LC_EINVAL and b"lc_track_spans: null pointer" in lib.lc_last_error()


@pytest.mark.parametrize("connectivity", [0, 3, -1, 8])
def test_label_refuses_another_connectivity(lib, connectivity):
    assert _label(GOOD, connectivity=connectivity) == _capi.LC_EINVAL
    assert b"lc_label_tracks: bad connectivity" in lib.lc_last_error()


@pytest.mark.parametrize("reach", [-1, 17, 1 << 20, -(1 << 31)])
def test_label_refuses_a_reach_outside_its_range(lib, reach):
    assert _label(GOOD, reach=reach) == _capi.LC_EINVAL and b"lc_label_tracks: bad reach" in lib.lc_last_error()


def test_label_takes_both_ends_of_the_reach_range(lib):
    for reach in (0, 16):
        assert _label(GOOD, reach=reach, mask=None) == _capi.LC_EINVAL and b"null pointer" in lib.lc_last_error()


@pytest.mark.parametrize("which", ["mask", "labels", "count", "work"])
def test_label_refuses_a_null_pointer(lib, which):
    assert _label(GOOD, **{which: None}) == _capi.LC_EINVAL and b"lc_label_tracks: null pointer" in lib.lc_last_error()


@pytest.mark.parametrize("which", ["labels", "count", "first_out", "last_out", "volume_out"])
def test_spans_refuses_a_null_pointer(lib, which):
    assert _spans(GOOD, **{which: True}) == _capi.LC_EINVAL and b"lc_track_spans: null pointer" in lib.lc_last_error()


@pytest.mark.parametrize("n_max", [0, -5])
def test_spans_refuses_a_capacity_below_one(lib, n_max):
    assert _spans(GOOD, n_max=n_max) == _capi.LC_EINVAL and b"lc_track_spans: bad capacity" in lib.lc_last_error()


def test_the_kernels_never_wait_for_another_workgroup():
    """The rule of components.hip holds in tracks.hip: what a stage needs from every workgroup of the stage before arrives with
    the end of that launch.  No cooperative launch, no grid synchronisation, no loop that spins on memory another workgroup
    writes (the only loops on shared memory are the walks of find_root, which end on their own: every step goes to a smaller
    index)."""
    src = build._strip_comments(open(os.path.join(build.CSRC, "tracks.hip")).read())
    for word in ("cooperative", "grid_group", "this_grid", "hipLaunchCooperativeKernel", "__threadfence", "while ("):
        assert word not in src, word
    assert src.count("for (;;)") == 2       # find_root and unite


# ------------------------------------------------------------------ the labelled surface, before an engine exists
def _series(shape=(3, 4, 5), dims=("time", "latitude", "longitude")):
    coords = {"time": np.arange(shape[0]), "latitude": np.linspace(-10.0, 10.0, shape[1]), "longitude": np.linspace(0.0, 8.0, shape[2])}
    return DataArray(np.zeros(shape), dims, {d: coords[d] for d in dims})


@pytest.fixture
def no_engine(monkeypatch):
    """get_engine raises: a call that passes its argument checks is seen to reach for a device, every other one is not."""
    from lagrangiancoherence_amd import tools

    def refuse():
        raise AssertionError("an engine was asked for")
    monkeypatch.setattr(tools, "get_engine", refuse)


BAD_ARGUMENTS = [(dict(reach=-1), "reach"), (dict(reach=17), "reach"), (dict(reach=1.5), "reach"), (dict(reach=True), "reach"),
                 (dict(connectivity=0), "connectivity"), (dict(connectivity=3), "connectivity"),
                 (dict(min_duration=0), "min_duration"), (dict(min_duration=-2), "min_duration"), (dict(min_duration=1.5), "min_duration")]


@pytest.mark.parametrize("kw, word", BAD_ARGUMENTS, ids=[f"{k}={v}" for c, _ in BAD_ARGUMENTS for k, v in c.items()])
def test_the_tools_check_their_arguments_before_an_engine_is_created(no_engine, kw, word):
    from lagrangiancoherence_amd import tools
    with pytest.raises(ValueError, match=word):
        tools.track_ridges(_series(), **kw)
    with pytest.raises(ValueError, match=word):
        tools.persistent_ridges(_series(), **{"min_duration": 2, **kw})


def test_the_tools_need_exactly_one_dimension_beside_latitude_and_longitude(no_engine):
    from lagrangiancoherence_amd import tools
    plane = DataArray(np.zeros((4, 5)), ("latitude", "longitude"), {"latitude": np.arange(4.0), "longitude": np.arange(5.0)})
    four = DataArray(np.zeros((2, 3, 4, 5)), ("member", "time", "latitude", "longitude"),
                     {"member": np.arange(2), "time": np.arange(3), "latitude": np.arange(4.0), "longitude": np.arange(5.0)})
    for da in (plane, four):
        with pytest.raises(ValueError, match="exactly one more"):
            tools.track_ridges(da)
        with pytest.raises(ValueError, match="exactly one more"):
            tools.persistent_ridges(da, 2)
    with pytest.raises(AssertionError, match="an engine was asked for"):      # good arguments go on to the device
        tools.track_ridges(_series(), reach=16, connectivity=1, min_duration=3)


def test_the_engine_states_the_same_option_rules():
    from lagrangiancoherence_amd.engine import Engine
    assert Engine.checked_track_options(2, np.int64(16)) == (2, 16) and Engine.MAX_TRACK_REACH == 16
    for bad in ((2, 17), (2, -1), (0, 1), (2, 1.0)):
        with pytest.raises(ValueError):
            Engine.checked_track_options(*bad)


def test_the_shim_exports_the_tracking_functions():
    from LagrangianCoherence.LCS import tools as shim
    from lagrangiancoherence_amd import tools
    assert shim.track_ridges is tools.track_ridges and shim.persistent_ridges is tools.persistent_ridges
    assert "track_ridges" in tools.__all__ and "persistent_ridges" in tools.__all__
