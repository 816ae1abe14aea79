"""Ridge tracking on the GPU against tests/tracks.py (scipy.sparse.csgraph.connected_components + numpy): labels, counts,
spans, filtered masks, renumbered ids and the table, every comparison an integer (or value-for-value) equality -- on the
smallest records that cross every boundary of csrc/tracks.hip: one voxel, time only, one row, one column, records that are
no multiple of the 1024-voxel tile so that a tile straddles a plane boundary and ends ragged, more tiles than one pass of
the tile scan takes (256), a single plane (which must be Engine.label_components of it), every reach from the same pixel to a
window larger than the plane, the seam between planes, equivalences found last (a comb along time), the longest parent chains
(a serpentine through time), random records, NaN / negative / -0.0 values.

Every reference is computed once per case and shared.  The float buffers the module's engine allocates start as NaN."""
import functools

import numpy as np
import pytest

from tests import tracks as TR
from tests.labelled import DataArray

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
DTYPE_IDS = ["f32", "f64"]
TILE = 1024      # voxels per workgroup of csrc/tracks.hip (TR_TILE)


@pytest.fixture(scope="module")
def eng():
    from lagrangiancoherence_amd.engine import Engine
    e = Engine(0)
    e._poison = True
    yield e
    e.close()


def _np(t):
    return t.detach().cpu().numpy()


RECORDS = {
    "1x1x1": lambda: np.ones((1, 1, 1)),
    "1x1x1-empty": lambda: np.zeros((1, 1, 1)),
    "4x1x1": lambda: np.ones((4, 1, 1)),
    "3x1x9": lambda: TR.random_record((3, 1, 9), 0.6),
    "3x9x1": lambda: TR.random_record((3, 9, 1), 0.6),
    "5x13x17": lambda: TR.random_record((5, 13, 17), 0.3),
    "3x33x65": lambda: TR.random_record((3, 33, 65), 0.3),
    "4x260x257": lambda: TR.random_record((4, 260, 257), 0.1),
    "blob-12x9x40": lambda: TR.moving_blob(12, 9, 40, step=1),
    "blob2-12x9x40": lambda: TR.moving_blob(12, 9, 40, step=2),
    "blob-6x5x7": lambda: TR.moving_blob(6, 5, 7, step=3, size=1),
    "comb-5x33x65": lambda: TR.comb_in_time(5, 33, 65),
    "serpentine-67x3x130": lambda: TR.serpentine_in_time(67, 3, 130),
    "forms-5x13x17": lambda: TR.background_forms((5, 13, 17)),
    "empty-3x33x65": lambda: np.zeros((3, 33, 65)),
    "full-3x33x65": lambda: np.ones((3, 33, 65)),
    **{f"random-{d}": (lambda d=d: TR.random_record((6, 21, 37), d)) for d in (0.02, 0.1, 0.3)},
}


@functools.lru_cache(maxsize=None)
def _record(name):
    m = RECORDS[name]()
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def _ref(name, connectivity=2, cyclic=False, reach=1):
    lab, n = TR.label(_record(name), connectivity, cyclic, reach)
    lab.setflags(write=False)
    return lab, n


def _check(eng, name, connectivity, cyclic, reach, dtype):
    mask = _record(name)
    lab, n = _ref(name, connectivity, cyclic, reach)
    labels, count = eng.label_tracks(mask.astype(dtype), connectivity, cyclic, reach)
    assert labels.dtype == eng.torch.int32 and tuple(labels.shape) == mask.shape
    assert count.dtype == eng.torch.int32 and tuple(count.shape) == (1,)
    assert int(count[0]) == n
    assert np.array_equal(_np(labels), lab)
    return n


# ------------------------------------------------------------------ the smallest records, the tiles
SMALL = ["1x1x1", "1x1x1-empty", "4x1x1", "3x1x9", "3x9x1", "5x13x17", "3x33x65", "empty-3x33x65", "full-3x33x65"]


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("reach", [0, 1, 16])
@pytest.mark.parametrize("connectivity", [1, 2])
@pytest.mark.parametrize("name", SMALL)
def test_small_and_ragged_records_equal_the_oracle(eng, name, connectivity, reach, dtype):
    n = _check(eng, name, connectivity, False, reach, dtype)
    if name in ("4x1x1", "full-3x33x65"):
        assert n == 1            # time only, all foreground: one track at any reach
    if name.endswith("empty"):
        assert n == 0


def test_the_ragged_records_straddle_planes_and_tiles_as_intended(eng):
    w = eng.lib.lc_track_work_elems
    assert 5 * 13 * 17 == 1105 and w(13, 17, 5) == 2 and (13 * 17) % TILE and TILE % (13 * 17)      # tile 0 ends inside plane 4
    assert w(33, 65, 3) == 7 and (33 * 65) % TILE and (3 * 33 * 65) % TILE
    assert w(260, 257, 4) > 256                                      # more than one pass of the tile scan
    assert _ref("5x13x17", 2, False, 1)[1] > 1 and _ref("3x33x65", 1, False, 0)[1] > 256


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("connectivity, cyclic, reach", [(2, False, 1), (1, True, 0), (2, True, 2)])
def test_many_tiles_carry_the_tile_scan_from_pass_to_pass(eng, connectivity, cyclic, reach, dtype):
    assert _check(eng, "4x260x257", connectivity, cyclic, reach, dtype) > 256      # tracks in tiles of every pass


# ------------------------------------------------------------------ one plane is label_components
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("cyclic", [False, True], ids=["plain", "cyclic"])
@pytest.mark.parametrize("connectivity", [1, 2])
def test_a_single_plane_equals_label_components(eng, connectivity, cyclic, dtype):
    for shape in ((1, 33, 65), (1, 17, 2), (1, 9, 1), (1, 1, 1)):
        plane = TR.random_record(shape, 0.45, salt=3).astype(dtype)
        want, counts = eng.label_components(plane[0], connectivity, cyclic)
        for reach in (0, 16):
            labels, count = eng.label_tracks(plane, connectivity, cyclic, reach)
            assert int(count[0]) == int(counts[0]) and np.array_equal(_np(labels[0]), _np(want))
        lab, n = TR.label(plane, connectivity, cyclic, 1)
        assert int(counts[0]) == n and np.array_equal(_np(want), lab[0])


# ------------------------------------------------------------------ the reach
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("name, reach, tracks", [("blob-12x9x40", 0, 12), ("blob-12x9x40", 1, 1), ("blob-12x9x40", 2, 1),
                                                  ("blob-12x9x40", 16, 1), ("blob2-12x9x40", 0, 12), ("blob2-12x9x40", 1, 1),
                                                  ("blob2-12x9x40", 2, 1)])
def test_a_moving_blob_is_one_track_from_the_reach_that_covers_its_step(eng, name, reach, tracks, dtype):
    # the blob is two columns wide: at one column per plane it overlaps itself, at two it touches itself by a corner in time
    expected = {("blob-12x9x40", 0): 1, ("blob2-12x9x40", 0): 12}.get((name, reach), 1)
    assert _ref(name, 2, False, reach)[1] == expected
    assert _check(eng, name, 2, False, reach, dtype) == expected


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("cyclic", [False, True], ids=["plain", "cyclic"])
def test_a_single_pixel_stepping_three_columns_needs_reach_three(eng, cyclic, dtype):
    """On (6, 5, 7) the pixel wraps round the plane's end once; reach 16 is a window larger than the plane."""
    for reach, want in ((0, None), (1, None), (2, None), (3, None), (16, 1)):
        n = _check(eng, "blob-6x5x7", 2, cyclic, reach, dtype)
        assert want is None or n == want
    assert _ref("blob-6x5x7", 2, False, 2)[1] == 6 and _ref("blob-6x5x7", 2, True, 3)[1] == 1 and _ref("blob-6x5x7", 2, False, 3)[1] > 1


# ------------------------------------------------------------------ the seam in time
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("connectivity", [1, 2])
def test_the_seam_joins_adjacent_planes_only_when_cyclic_and_within_reach(eng, connectivity, dtype):
    def count(m, cyclic, reach):
        lab, n = TR.label(m, connectivity, cyclic, reach)
        labels, c = eng.label_tracks(m.astype(dtype), connectivity, cyclic, reach)
        assert int(c[0]) == n and np.array_equal(_np(labels), lab)
        return n
    straight = TR.seam_in_time(4, 9)
    assert count(straight, False, 1) == 2 and count(straight, True, 0) == 2 and count(straight, True, 1) == 1
    assert count(straight, False, 16) == 1          # a window as wide as the plane reaches the other end without the seam
    diagonal = TR.seam_in_time(6, 9, rows_apart=2)
    assert count(diagonal, True, 1) == 2 and count(diagonal, True, 2) == 1 and count(diagonal, False, 2) == 2
    short_way = np.zeros((2, 1, 9))
    short_way[0, 0, 1] = short_way[1, 0, 7] = 1     # three columns apart across the seam, six inside the plane
    assert count(short_way, True, 2) == 2 and count(short_way, True, 3) == 1 and count(short_way, False, 5) == 2
    assert count(short_way, False, 6) == 1


# ------------------------------------------------------------------ late equivalences, long chains
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("name, connectivity, reach", [("comb-5x33x65", 1, 0), ("comb-5x33x65", 2, 0), ("comb-5x33x65", 2, 1),
                                                        ("serpentine-67x3x130", 1, 0), ("serpentine-67x3x130", 2, 1)])
def test_equivalences_found_last_and_the_longest_chains(eng, name, connectivity, reach, dtype):
    assert _check(eng, name, connectivity, False, reach, dtype) == 1
    if name.startswith("comb"):     # without the last plane every tooth is a track of its own
        teeth = _record(name)[:-1]
        lab, n = TR.label(teeth, connectivity, False, reach)
        labels, count = eng.label_tracks(teeth.astype(dtype), connectivity, False, reach)
        assert n == 17 * 33 == int(count[0]) and np.array_equal(_np(labels), lab)


# ------------------------------------------------------------------ random records
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("cyclic", [False, True], ids=["plain", "cyclic"])
@pytest.mark.parametrize("reach", [0, 1, 2, 3])
@pytest.mark.parametrize("connectivity", [1, 2])
@pytest.mark.parametrize("density", [0.02, 0.1, 0.3])
def test_random_records_equal_the_oracle(eng, density, connectivity, reach, cyclic, dtype):
    _check(eng, f"random-{density}", connectivity, cyclic, reach, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("connectivity", [1, 2])
def test_nan_and_both_zeros_are_background_and_negative_values_foreground(eng, connectivity, dtype):
    mask = _record("forms-5x13x17")
    assert np.isnan(mask).any() and (mask < 0).any() and (np.signbit(mask) & (mask == 0)).any()
    _check(eng, "forms-5x13x17", connectivity, True, 1, dtype)
    got = _np(eng.label_tracks(mask.astype(dtype), connectivity, True, 1)[0])
    assert not got[np.isnan(mask)].any() and not got[mask == 0].any() and got[mask < 0].all()


# ------------------------------------------------------------------ spans
SPAN_CASES = [("random-0.1", 2, False, 1), ("random-0.3", 1, True, 0), ("random-0.02", 2, True, 3), ("5x13x17", 2, False, 1),
              ("blob-12x9x40", 2, False, 0), ("comb-5x33x65", 2, False, 0), ("4x1x1", 2, False, 0), ("4x260x257", 2, False, 1),
              ("forms-5x13x17", 2, True, 1)]


@pytest.mark.parametrize("name, connectivity, cyclic, reach", SPAN_CASES)
def test_spans_equal_the_oracle_and_the_tail_is_empty(eng, name, connectivity, cyclic, reach):
    lab, n = _ref(name, connectivity, cyclic, reach)
    ref = TR.spans(lab, n)
    labels, count = eng.label_tracks(_record(name).copy(), connectivity, cyclic, reach)
    got = {k: _np(v) for k, v in eng.track_spans(labels, count).items()}
    assert got["first"].dtype == got["last"].dtype == got["duration"].dtype == np.int32 and got["volume"].dtype == np.int64
    for k in ("first", "last", "duration", "volume"):
        assert got[k].shape == (max(n, 1),) and np.array_equal(got[k][:n], ref[k]), k
    big = {k: _np(v) for k, v in eng.track_spans(labels, count, n_max=n + 5).items()}
    for k in ("first", "last", "duration", "volume"):
        assert big[k].shape == (n + 5,) and np.array_equal(big[k][:n], ref[k]), k
    assert (big["first"][n:] == -1).all() and (big["last"][n:] == -1).all()
    assert not big["volume"][n:].any() and not big["duration"][n:].any()
    small = {k: _np(v) for k, v in eng.track_spans(labels, count, n_max=3).items()}      # labels past the capacity are not measured
    m = min(n, 3)
    for k in ("first", "last", "duration", "volume"):
        assert small[k].shape == (3,) and np.array_equal(small[k][:m], ref[k][:m]), k
    assert (small["first"][m:] == -1).all() and not small["volume"][m:].any()


def test_spans_of_a_record_without_tracks(eng):
    labels, count = eng.label_tracks(_record("empty-3x33x65").copy())
    got = {k: _np(v) for k, v in eng.track_spans(labels, count).items()}
    assert int(count[0]) == 0 and list(got["first"]) == [-1] and list(got["last"]) == [-1] and list(got["volume"]) == [0]


# ------------------------------------------------------------------ the filter
FILTER_CASES = [("random-0.1", 2, False, 1, 2, 1), ("random-0.1", 2, False, 1, 1, 4), ("random-0.3", 1, True, 0, 3, 1),
                ("random-0.02", 2, True, 3, 2, 3), ("random-0.02", 2, False, 2, 2, 1), ("forms-5x13x17", 1, True, 0, 2, 3)]


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("fill", [0.0, np.nan, -1.0], ids=["fill0", "fillnan", "fill-1"])
@pytest.mark.parametrize("name, connectivity, cyclic, reach, min_duration, min_volume", FILTER_CASES)
def test_filter_tracks_equals_the_oracle(eng, name, connectivity, cyclic, reach, min_duration, min_volume, fill, dtype):
    mask = (_record(name) * 3).astype(dtype)
    want = TR.filtered(mask, min_duration, min_volume, connectivity, cyclic, reach, fill)
    kept, all_ = np.count_nonzero(TR.foreground(want)), np.count_nonzero(TR.foreground(mask))
    if fill == -1.0:
        kept = np.count_nonzero(want != -1.0)
    assert 0 < kept < all_                                                    # some kept, some dropped
    got = _np(eng.filter_tracks(mask, min_duration, min_volume, connectivity, cyclic, reach, fill))
    assert got.dtype == mask.dtype and got.shape == mask.shape and np.array_equal(got, want, equal_nan=True)


def _labelled(record, dtype=np.float64):
    """The record as a caller might hold it: descending latitude, dims (latitude, time, longitude)."""
    nt, ny, nx = record.shape
    time = np.datetime64("2026-01-01T00") + np.arange(nt) * np.timedelta64(6, "h")
    lat, lon = np.linspace(-20.0, 20.0, ny), np.linspace(-180.0, 170.0, nx)
    da = DataArray(record[:, ::-1].transpose(1, 0, 2).astype(dtype), ("latitude", "time", "longitude"),
                   {"latitude": lat[::-1], "time": time, "longitude": lon}, name="ridges")
    return da, time, lat, lon


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("fill", [0.0, np.nan], ids=["fill0", "fillnan"])
def test_persistent_ridges_equals_the_oracle_in_the_callers_order(fill, dtype):
    from LagrangianCoherence.LCS.tools import persistent_ridges
    record = _record("random-0.1") * 2.5
    da, time, lat, lon = _labelled(record, dtype)
    want = TR.filtered(record.astype(dtype), min_duration=3, connectivity=1, cyclic=True, reach=2, fill=fill)
    assert 0 < np.count_nonzero(TR.foreground(want)) < np.count_nonzero(record)
    out = persistent_ridges(da, 3, reach=2, connectivity=1, cyclic=True, fill=fill)
    assert type(out) is DataArray and out.dims == da.dims and out.name == "ridges" and out.values.dtype == dtype
    assert np.array_equal(out.coords["latitude"], lat) and np.array_equal(out.coords["time"], time)
    assert np.array_equal(out.values, want.transpose(1, 0, 2), equal_nan=True)


# ------------------------------------------------------------------ track_ridges
@pytest.mark.parametrize("name, connectivity, cyclic, reach, min_duration", [("random-0.1", 2, False, 1, 1), ("random-0.1", 2, True, 1, 3),
                                                                           ("random-0.3", 1, False, 0, 2), ("blob2-12x9x40", 2, False, 2, 12)])
def test_track_ridges_renumbers_the_survivors_and_tabulates_them(name, connectivity, cyclic, reach, min_duration):
    from LagrangianCoherence.LCS.tools import track_ridges
    record = _record(name)
    da, time, lat, lon = _labelled(record)
    ids, table = TR.tracked(record, reach, connectivity, cyclic, min_duration)
    assert ids.max() == table["first"].size > 0
    out, got = track_ridges(da, reach=reach, connectivity=connectivity, cyclic=cyclic, min_duration=min_duration, return_table=True)
    assert type(out) is DataArray and out.dims == da.dims and out.values.dtype == np.int32
    assert np.array_equal(out.coords["latitude"], lat) and np.array_equal(out.coords["longitude"], lon)
    assert np.array_equal(out.values, ids.transpose(1, 0, 2))
    assert sorted(got) == ["duration", "first", "first_time", "last", "last_time", "volume"]
    for k in ("first", "last", "duration", "volume"):
        assert np.array_equal(got[k], table[k]), k
    assert np.array_equal(got["first_time"], time[table["first"]]) and np.array_equal(got["last_time"], time[table["last"]])
    alone = track_ridges(da, reach=reach, connectivity=connectivity, cyclic=cyclic, min_duration=min_duration)
    assert type(alone) is DataArray and np.array_equal(alone.values, out.values)


def test_a_min_duration_above_every_duration_leaves_nothing():
    from lagrangiancoherence_amd.tools import persistent_ridges, track_ridges
    record = _record("random-0.1")
    da = _labelled(record)[0]
    out, table = track_ridges(da, min_duration=record.shape[0] + 1, return_table=True)
    assert out.values.shape == da.values.shape and out.values.dtype == np.int32 and not out.values.any()
    assert sorted(table) == ["duration", "first", "first_time", "last", "last_time", "volume"]
    assert all(v.shape == (0,) for v in table.values())
    gone = persistent_ridges(da, record.shape[0] + 1, fill=np.nan)
    assert np.isnan(gone.values).all()
