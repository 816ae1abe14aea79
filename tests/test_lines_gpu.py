"""Ridge lines on the GPU (csrc/lines.hip, Engine.trace_lines, tools.ridge_lines) against the pixel walker of tests/lines.py.

Every integer output equals the walker's exactly: the link bytes, every per-line integer column, ``points.line`` and
``points.pixel``.  A link's length (``step``) is within 16 ulp of the walker's -- the bound tests/test_sphere_distance_gpu.py
derives for the same expression --, ``length`` and ``distance`` within ``2 (count + 16) spacing(want)`` of the walker's sequential
sum: 16 ulp per term and one rounding per addition, all terms positive.  ``metric='index'`` is bit-equal.  Every check prints its
own maximum.  On every case the doubling rounds are at most ``2 (ceil(log2(max(2, I))) + 1)`` for ``I`` the largest interior count.

The shapes are the smallest on which each part can go wrong; the references are computed once per case and shared.  The kernels
work on flat tiles of TILE pixels (or states) per workgroup and use no scan, so "no multiple of the tile" is a plane whose pixel
count is none (every hand-made mask, 21 x 37 = 777, 60 x 90) and several tiles are the skeletons and the 33 x 65 lines.  The float
buffers the module's engine allocates start as NaN."""
import functools
import math

import numpy as np
import pytest

from tests import lines as L
from tests import skeleton as SK
from tests.labelled import DataArray

pytestmark = pytest.mark.gpu

TILE = 256       # pixels (and states) per workgroup of csrc/lines.hip (LN_TILE)
DTYPES = [np.float32, np.float64]
DTYPE_IDS = ["f32", "f64"]


@pytest.fixture(scope="module")
def eng():
    from lagrangiancoherence_amd.engine import Engine
    e = Engine(0)
    e._poison = True
    yield e
    e.close()


def _np(t):
    return t.detach().cpu().numpy()


def _random(density):
    return L.random_mask(21, 37, density)


def _skeleton_input(salt=0):
    return SK._smooth(60, 90, salt=salt)


MASKS = {**{name: (lambda m=m: m) for name, (m, _) in L.CASES.items()},
         **{f"random-{d}": (lambda d=d: _random(d)) for d in (0.02, 0.1, 0.3, 0.6)}}
CYCLIC = {**{name: c for name, (_, c) in L.CASES.items()}}
CASES = [(name, CYCLIC[name]) for name in L.CASES] + [(f"random-{d}", c) for d in (0.02, 0.1, 0.3, 0.6) for c in (False, True)]
IDS = [f"{n}{'-cyclic' if c else ''}" for n, c in CASES]


@functools.lru_cache(maxsize=None)
def _want(name, cyclic, metric="sphere", sampling=None):
    mask = MASKS[name]()
    lat, lon = L.grid(*mask.shape)
    t = L.trace(mask, cyclic, metric=metric, lat=lat, lon=lon, sampling=sampling)
    for v in t.values():
        v.setflags(write=False)
    return t


def _bound(interior):
    return 2 * (math.ceil(math.log2(max(2, interior))) + 1)


def _compare(got, want, metric, what, rounds=None):
    got = {k: _np(v) for k, v in got.items()}
    assert np.array_equal(got["links"].reshape(want["links"].shape), want["links"]), "links"
    for k in L.LINE_INTS + L.POINT_INTS + ("key",):
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k
    links = want["links"].reshape(-1, *want["links"].shape[-2:])
    n = len(links)
    degree = L.POPCOUNT[links].reshape(n, -1)
    interior, lone = (degree == 2).sum(1), np.bincount(want["plane"][want["count"] == 1], minlength=n)
    foreground = (links.reshape(n, -1) != 0).sum(1) + lone                  # a pixel without a link is a line of one point
    assert np.array_equal(got["counts"], np.stack([foreground, interior, foreground - interior, degree.sum(1) // 2], axis=1)), "counts"
    if rounds is not None:
        print(f"{what}: rounds {rounds}, bound {_bound(int(interior.max()))}, interior {int(interior.max())}")
        assert rounds <= _bound(int(interior.max()))
    if metric == "index":
        for k in ("length", "distance", "step"):
            assert np.array_equal(got[k], want[k]), k
        return got
    per_point = want["count"][want["line"]] if want["line"].size else want["line"]
    for k, terms in (("step", None), ("length", want["count"]), ("distance", per_point)):
        err = np.abs(got[k] - want[k])
        allowed = 16 * np.spacing(want[k]) if terms is None else 2 * (terms + 16) * np.spacing(want[k])
        ratio = (err / allowed).max() if err.size else 0.0
        print(f"{what}: {k} largest error / allowed {ratio:.3g}")
        assert got[k].shape == want[k].shape and (err <= allowed).all(), k
    return got


@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("name,cyclic", CASES, ids=IDS)
def test_lines_equal_the_walker_on_the_sphere(eng, name, cyclic, dtype):
    mask = MASKS[name]()
    lat, lon = L.grid(*mask.shape)
    got = eng.trace_lines(mask.astype(dtype), cyclic, "sphere", lat, lon)
    _compare(got, _want(name, cyclic), "sphere", name, eng.last_lines_rounds())


@pytest.mark.parametrize("sampling", [None, (2.0, 3.0)], ids=["unit", "2x3"])
@pytest.mark.parametrize("name,cyclic", CASES, ids=IDS)
def test_index_lengths_are_bit_equal(eng, name, cyclic, sampling):
    mask = MASKS[name]()
    got = eng.trace_lines(mask, cyclic, "index", sampling=sampling)
    _compare(got, _want(name, cyclic, "index", sampling), "index", name, eng.last_lines_rounds())


def test_long_lines_need_more_than_ten_rounds(eng):
    for name in ("serpentine", "spiral"):
        mask = MASKS[name]()
        got = eng.trace_lines(mask, False, "index")
        assert int(_np(got["count"]).max()) > 1024 and _np(got["count"]).size == 1 and 10 < eng.last_lines_rounds() <= _bound(1119)


def test_a_ring_is_ranked_in_a_second_pass(eng):
    got = eng.trace_lines(MASKS["frame"](), False, "index")
    assert _np(got["closed"]).tolist() == [1] and _np(got["pixel"])[:3].tolist() == [0, 1, 2] and _np(got["pixel"])[-1] == 8
    assert eng.last_lines_rounds() == 10          # 24 interior pixels: 5 rounds see the whole ring, 5 more rank the broken one


def test_three_planes_equal_the_three_single_calls(eng):
    names = [("T", False), ("random-0.3", False), ("spiral", False)]
    planes = [np.zeros((33, 65)) for _ in names]
    for p, (n, _) in zip(planes, names):
        m = MASKS[n]()
        p[:m.shape[0], :m.shape[1]] = m
    stack = np.stack(planes)
    lat, lon = L.grid(33, 65)
    both = eng.trace_lines(stack, True, "sphere", lat, lon)
    want = L.trace_planes(stack, True, lat=lat, lon=lon)
    got = _compare(both, want, "sphere", "stack", eng.last_lines_rounds())
    at_line, at_point = 0, 0
    for i, plane in enumerate(planes):
        one = {k: _np(v) for k, v in eng.trace_lines(plane, True, "sphere", lat, lon).items()}
        nl, npt = one["count"].size, one["pixel"].size
        assert (got["plane"][at_line:at_line + nl] == i).all()
        for k in ("count", "closed", "first", "last", "first_degree", "last_degree", "n_edge", "n_diag", "key", "length"):
            assert np.array_equal(one[k], got[k][at_line:at_line + nl]), k          # floats too: a plane never reads another
        for k in ("pixel", "distance", "step"):
            assert np.array_equal(one[k], got[k][at_point:at_point + npt]), k
        assert np.array_equal(one["line"] + at_line, got["line"][at_point:at_point + npt])
        assert np.array_equal(one["offset"] + at_point, got["offset"][at_line:at_line + nl])
        at_line, at_point = at_line + nl, at_point + npt
    assert at_line == got["count"].size and at_point == got["pixel"].size


@pytest.mark.parametrize("cyclic", [False, True], ids=["plain", "cyclic"])
@pytest.mark.parametrize("method", SK.METHODS)
def test_skeletons_through_thin_then_trace(eng, method, cyclic):
    """Engine.thin's own output, uint8 on the device, straight into trace_lines: two planes of 60 x 90 = 5400 pixels, 22 tiles."""
    fields = np.stack([_skeleton_input(0), _skeleton_input(1)])
    thin = eng.thin(fields, eng.thinning_table(method), cyclic=cyclic)
    lat, lon = L.grid(60, 90)
    got = eng.trace_lines(thin, cyclic, "sphere", lat, lon)
    want = L.trace_planes(_np(thin).astype(np.float64), cyclic, lat=lat, lon=lon)
    L.invariants(want)
    assert want["count"].size > 10
    _compare(got, want, "sphere", f"{method}", eng.last_lines_rounds())


def test_refusals_reach_the_caller_as_value_errors(eng):
    lat, lon = L.grid(4, 6)
    with pytest.raises(ValueError, match="3 columns"):
        eng.trace_lines(np.ones((4, 2)), True, "index")
    with pytest.raises(ValueError, match="len"):
        eng.trace_lines(np.ones((5, 6)), False, "sphere", lat, lon)
    with pytest.raises(ValueError, match="metric"):
        eng.trace_lines(np.ones((4, 6)), False, "chord", lat, lon)


# ------------------------------------------------------------------ tools.ridge_lines
def _labelled(stack, lat, lon, name=None):
    """``(latitude, time, longitude)`` with latitude descending, as a reanalysis file has it."""
    coords = {"latitude": lat[::-1], "time": np.arange(stack.shape[0]) * 6, "longitude": lon}
    return DataArray(stack[:, ::-1].transpose(1, 0, 2).copy(), ("latitude", "time", "longitude"), coords, name=name)


def test_ridge_lines_tables_equal_the_walker(eng):
    from lagrangiancoherence_amd.tools import ridge_lines
    thin, _ = SK.thin(_skeleton_input(), SK.table("guohall"))
    seam = np.zeros((60, 90))
    seam[5] = 1                                   # a ring of 90 across the seam
    stack = np.stack([thin.astype(np.float64), _padded("lollipop"), np.zeros((60, 90)), seam])
    lat, lon = L.grid(60, 90)
    rng = np.random.default_rng(20261020)
    field = rng.standard_normal(stack.shape)
    lines, points = ridge_lines(_labelled(stack, lat, lon, "ridges"), _labelled(field, lat, lon), cyclic=True)
    want = L.trace_planes(stack, True, lat=lat, lon=lon)
    nx = lon.size
    for k in ("plane", "offset", "count", "closed", "first_degree", "last_degree"):
        assert np.array_equal(lines[k], want[k]), k
    assert np.array_equal(points["line"], want["line"]) and np.array_equal(points["row"] * nx + points["column"], want["pixel"])
    number = np.concatenate([np.arange((want["plane"] == m).sum()) for m in range(len(stack))])
    assert np.array_equal(lines["line"], number)
    # coordinates are the sorted array's
    assert np.array_equal(points["latitude"], lat[want["pixel"] // nx]) and np.array_equal(points["longitude"], lon[want["pixel"] % nx])
    for end in ("first", "last"):
        assert np.array_equal(lines[f"{end}_latitude"], lat[want[end] // nx]) and np.array_equal(lines[f"{end}_longitude"], lon[want[end] % nx])
    for k, got, terms in (("length", lines["length"], want["count"]), ("distance", points["distance"], want["count"][want["line"]])):
        allowed = 2 * (terms + 16) * np.spacing(want[k])
        print(f"ridge_lines: {k} largest error / allowed {(np.abs(got - want[k]) / allowed).max():.3g}")
        assert (np.abs(got - want[k]) <= allowed).all(), k
    # chord: the same formula between the end points; 0 for rings and loops; sinuosity follows
    chord = L.link_lengths(want["first"], want["last"], lat, lon)
    chord[want["closed"] != 0] = 0.0
    assert (np.abs(lines["chord"] - chord) <= 16 * np.spacing(chord)).all()
    loops = (want["closed"] != 0) | ((want["first"] == want["last"]))
    assert (lines["chord"][loops] == 0).all() and np.isnan(lines["sinuosity"][loops]).all() and loops.sum() >= 2
    open_ = ~loops
    assert np.array_equal(lines["sinuosity"][open_], lines["length"][open_] / lines["chord"][open_]) and (lines["sinuosity"][open_] >= 1 - 1e-12).all()
    # component joins the table to ridge_properties' labels
    labels, _ = eng.label_components(stack, 2, True)
    labels = _np(labels).reshape(len(stack), -1)
    assert np.array_equal(lines["component"], labels[want["plane"], want["first"]]) and (lines["component"] >= 1).all()
    assert np.array_equal(labels[want["plane"][want["line"]], want["pixel"]], lines["component"][want["line"]])      # one label per line
    # intensity: numpy on the walker's points
    value = field.reshape(len(stack), -1)[want["plane"][want["line"]], want["pixel"]]
    assert np.array_equal(points["intensity"], value)
    for i in range(want["count"].size):
        v = value[want["offset"][i]:want["offset"][i] + want["count"][i]]
        assert lines["max_intensity"][i] == v.max() and lines["min_intensity"][i] == v.min()
        assert abs(lines["mean_intensity"][i] - v.mean()) <= (v.size + 1) * np.spacing(np.abs(v).sum() / v.size)      # a sum of count terms


def _padded(name, shape=(60, 90)):
    out = np.zeros(shape)
    m = MASKS[name]()
    out[:m.shape[0], :m.shape[1]] = m
    return out


def test_ridge_lines_index_metric_and_two_dimensions(eng):
    from lagrangiancoherence_amd.tools import ridge_lines
    mask = MASKS["Y"]()
    lat, lon = L.grid(*mask.shape)
    lines, points = ridge_lines(DataArray(mask, ("latitude", "longitude"), {"latitude": lat, "longitude": lon}), metric="index")
    want = _want("Y", False, "index")
    assert np.array_equal(lines["length"], want["length"]) and np.array_equal(points["distance"], want["distance"])
    assert (lines["plane"] == 0).all() and "mean_intensity" not in lines and "intensity" not in points
    assert np.allclose(lines["chord"], [2 * np.sqrt(2), 2 * np.sqrt(2), 2.0]) and np.allclose(lines["sinuosity"], 1.0)


def test_a_mask_without_ridges_gives_empty_tables_with_every_key(eng):
    from lagrangiancoherence_amd import tools
    lat, lon = L.grid(7, 9)
    coords = {"latitude": lat, "longitude": lon}
    empty = DataArray(np.zeros((7, 9)), ("latitude", "longitude"), coords)
    lines, points = tools.ridge_lines(empty, empty)
    assert set(lines) == set(tools.LINE_COLUMNS) | {"mean_intensity", "max_intensity", "min_intensity"}
    assert set(points) == set(tools.POINT_COLUMNS) | {"intensity"}
    assert all(v.shape == (0,) for v in lines.values()) and all(v.shape == (0,) for v in points.values())
