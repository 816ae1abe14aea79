"""Great-circle transects across ridge lines on the GPU (csrc/transects.hip, Engine.ridge_transects, tools.ridge_transects)
against the numpy oracle of tests/transects.py, which also holds the cases and derives the bounds.

The cases (planes of at most 40 x 64): single serpentine lines of 1, 2, 3, 2 smooth, 2 smooth + 1 points and of the lengths
around the composite's chunk and the workgroup (both read from the source), each with 1 and 3 offsets, so that ``n_points * M``
passes 255, 256, 257; a ring, a junction and a lone pixel, as one plane and as a stack of 3 planes; 41 offsets; a line and
transects across the seam, on grids that start at -180 and at 20 degrees; transects that leave the grid at each edge; transects
over a pole on a grid with +-90 rows; Gaussian latitudes; 1, 2 and 5 fields (a launch takes 4) in float32 and float64; NaN
nodes; every orientation and both methods; descending coordinates and a dict of fields through ``tools``.

What is compared (tests/transects.py has the reasons): the lines and points exactly with the pixel walker; which points have
no tangent exactly; normals, tangents and their components to 16 eps64, headings to the angle that allows; positions to ``8 (E +
1) eps64`` radians of separation and of latitude, E measured here on every run and printed (-s); values against the oracle's
interpolation at the returned positions -- NaN masks identical, ``nearest`` bit for bit, ``linear`` within ``4 eps sum |w v|`` --;
the cell of the oracle's own position against the device's wherever it is not ambiguous; ``line_count`` exactly and
``line_mean`` within ``(n + 2) eps sum |v| / n`` of ``math.fsum`` over the device's own values.  Every reference is computed once
per case and shared.  The float buffers the module's engine allocates start as NaN."""
import functools
import os
import re

import numpy as np
import pytest

from lagrangiancoherence_amd import build
from tests import lines as L
from tests import transects as T
from tests.labelled import DataArray

pytestmark = pytest.mark.gpu

_SRC = open(os.path.join(build.CSRC, "transects.hip")).read()
TR_THREADS, TR_CHUNK, TR_FIELDS = (int(re.search(r"constexpr int %s = (\d+);" % n, _SRC).group(1)) for n in ("TR_THREADS", "TR_CHUNK", "TR_FIELDS"))
CASES = T.cases(TR_THREADS, TR_CHUNK)
KERNELS = "transect_normal_kernel+transect_sample_kernel+transect_composite_kernel"
VARIED = ("ring-junction-2d-f64x5", "shapes-3d-f32x5-M41", "seam", "seam-lon0-20", "edges", "pole", "pole-not-cyclic", "gaussian-latitudes")


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
def _prepared(name):
    case = CASES[name]
    fields, trace = T.case_fields(case), T.case_trace(case)
    for a in (fields, *trace.values()):
        a.setflags(write=False)
    return case, fields, trace


@functools.lru_cache(maxsize=None)
def _oracle_geometry(name, orient):
    """The oracle's normals and positions: they do not depend on the fields or the method."""
    case, _, trace = _prepared(name)
    K, s, c, sn = T.offsets(case["half_width"], case["spacing"])
    nrm = T.normals(trace, case["lat"], case["lon"], case["smooth"], orient)
    y, x = T.positions(nrm[:, :3], trace["pixel"], case["lat"], case["lon"], c, sn, case["cyclic"])
    return K, s, nrm, y, x


def _fields_for(case, fields):
    return fields if case["mask"].ndim == 3 else fields[:, 0]


def _run(eng, name, orient="left", method="linear", fields=None):
    case, all_fields, _ = _prepared(name)
    fields = all_fields if fields is None else fields
    trace = eng.trace_lines(case["mask"], case["cyclic"], "sphere", case["lat"], case["lon"])
    got = eng.ridge_transects(trace, _fields_for(case, fields), case["lat"], case["lon"], case["half_width"], case["spacing"],
                              case["smooth"], orient, method, case["cyclic"])
    assert eng.last_transects_kernel == KERNELS
    return {k: _np(v) for k, v in trace.items()}, {k: _np(v) for k, v in got.items()}


def _check(name, trace, got, orient, method, fields=None):
    case, all_fields, want_trace = _prepared(name)
    fields = all_fields if fields is None else fields
    lat, lon, cyclic = case["lat"], case["lon"], case["cyclic"]
    # the lines and points: ridge_lines' own, exactly
    for k in L.LINE_INTS + L.POINT_INTS:
        assert np.array_equal(trace[k], want_trace[k]), k
    K, s, nrm, oy, ox = _oracle_geometry(name, orient)
    n_points, n_lines, M, n_fields = want_trace["pixel"].size, want_trace["count"].size, 2 * K + 1, fields.shape[0]
    dtype = fields.dtype
    assert np.array_equal(got["offset"], s) and got["normal"].shape == (n_points, 3)
    assert got["latitude"].shape == got["longitude"].shape == (n_points, M) and got["latitude"].dtype == np.float64
    assert got["values"].shape == (n_fields, n_points, M) and got["values"].dtype == dtype
    assert got["line_mean"].shape == got["line_count"].shape == (n_fields, n_lines, M)
    assert got["line_mean"].dtype == dtype and got["line_count"].dtype == np.int32
    # normals and tangents: which points have none exactly, every component to NORMAL_TOL, the heading to what that allows
    mine = np.column_stack([got["normal"], got["normal_east"], got["normal_north"], got["tangent_east"], got["tangent_north"]])
    assert np.array_equal(np.isnan(mine), np.isnan(nrm))
    has = ~np.isnan(nrm[:, 0])
    worst_n = float(np.abs(mine - nrm)[has].max(initial=0.0))
    worst_h = float(T.heading_difference(T.heading(mine[has, 5], mine[has, 6]), T.heading(nrm[has, 5], nrm[has, 6])).max(initial=0.0))
    assert worst_n <= T.NORMAL_TOL and worst_h <= T.HEADING_TOL
    # positions: NaN exactly where there is no tangent; separation and latitude difference within POSITION_BOUND radians
    y, x = got["latitude"], got["longitude"]
    assert np.array_equal(np.isnan(y), np.isnan(oy)) and np.array_equal(np.isnan(x), np.isnan(ox))
    assert np.array_equal(np.isnan(y), np.broadcast_to(~has[:, None], y.shape))
    sep, dlat = T.separation(oy, ox, y, x)[has], np.radians(np.abs(y - oy))[has]
    worst_p = float(max(sep.max(initial=0.0), dlat.max(initial=0.0)))
    assert worst_p <= T.POSITION_BOUND
    if cyclic:
        assert (x[has] >= lon[0]).all() and (x[has] < lon[0] + 360.0).all()
    # values: the oracle's interpolation at the returned positions
    plane_of_point = want_trace["plane"][want_trace["line"]]
    eps = float(np.finfo(dtype).eps)
    worst_v = worst_m = 0.0
    for f in range(n_fields):
        want, scale = T.interpolate(fields[f], plane_of_point, y, x, lat, lon, cyclic, method)
        v = got["values"][f]
        assert np.array_equal(np.isnan(v), np.isnan(want))
        ok = ~np.isnan(want)
        if method == "nearest":
            assert np.array_equal(v[ok], want.astype(dtype)[ok])
        else:
            err, bound = np.abs(v.astype(np.float64) - want)[ok], 4 * eps * scale[ok]
            assert (err <= bound).all()
            worst_v = max(worst_v, float((err[bound > 0] / bound[bound > 0]).max(initial=0.0)))
        # the composite, from the device's own values
        mean, num, mscale = T.composite(v, want_trace["offset"], want_trace["count"])
        assert np.array_equal(got["line_count"][f], num)
        assert np.array_equal(np.isnan(got["line_mean"][f]), num == 0)
        some = num > 0
        err, bound = np.abs(got["line_mean"][f].astype(np.float64) - mean)[some], ((num + 2) * eps * mscale)[some]
        assert (err <= bound).all()
        worst_m = max(worst_m, float((err[bound > 0] / bound[bound > 0]).max(initial=0.0)))
    # the cell of the oracle's own position is the device's, wherever that is not a matter of the last bits
    mine_c, want_c = T.cells(y, x, lat, lon, cyclic), T.cells(oy, ox, lat, lon, cyclic)
    clear = has[:, None] & ~T.ambiguous(oy, ox, lat, lon, cyclic, method) & ~T.on_a_grid_line(nrm, K)
    assert np.array_equal(mine_c["inside"][clear], want_c["inside"][clear])
    both = clear & want_c["inside"]
    nodes = (T.nearest_nodes(y, x, mine_c), T.nearest_nodes(oy, ox, want_c)) if method == "nearest" else \
        ((mine_c["j0"], mine_c["i0"]), (want_c["j0"], want_c["i0"]))
    for a, b in zip(*nodes):
        assert np.array_equal(a[both], b[both])
    print(f"{name} {orient} {method}: {n_lines} lines, {n_points} points, M = {M}; normal error {worst_n / T.EPS64:.2f} eps64 (16), heading "
          f"{worst_h:.2e} deg ({T.HEADING_TOL:.2e}), position {worst_p / T.EPS64:.2f} eps64 ({T.POSITION_BOUND / T.EPS64:.0f}), value error / bound "
          f"{worst_v:.3f}, mean error / bound {worst_m:.3f}, clear samples {int(clear.sum())} of {clear.size}")


# ------------------------------------------------------------------ every case against the oracle
@pytest.mark.parametrize("name", list(CASES))
def test_every_case_against_the_oracle(eng, name):
    trace, got = _run(eng, name)
    _check(name, trace, got, "left", "linear")


@pytest.mark.parametrize("method", T.METHODS)
@pytest.mark.parametrize("orient", T.ORIENTS)
@pytest.mark.parametrize("name", VARIED)
def test_every_orientation_and_both_methods(eng, name, orient, method):
    trace, got = _run(eng, name, orient, method)
    _check(name, trace, got, orient, method)
    has = ~np.isnan(got["normal_north"])
    if orient == "north":
        assert (got["normal_north"][has] >= 0).all()
    if orient == "east":
        assert (got["normal_east"][has] >= 0).all()


def test_the_devices_atan2_is_within_E_ulp_of_numpys(eng):
    """What POSITION_BOUND is made of (tests/transects.py): the arguments of the two atan2 are formed with numpy from the
    device's own normals, operation for operation, so the returned positions differ from numpy's only by atan2 itself.  Its
    largest distance over every sample of every case of this module that the wrap left alone, printed; E is recorded there."""
    worst, n = {"latitude": 0.0, "longitude": 0.0}, 0
    for name, case in CASES.items():
        for orient in T.ORIENTS:
            trace, got = _run(eng, name, orient)
            K, s, c, sn = T.offsets(case["half_width"], case["spacing"])
            y, x, _ = T.raw_positions(got["normal"], trace["pixel"], case["lat"], case["lon"], c, sn)
            ok = ~np.isnan(y)
            same = ok & (T.wrap(x, case["lon"][0]) == x) if case["cyclic"] else ok
            worst["latitude"] = max(worst["latitude"], float(T.ulps(got["latitude"][ok], y[ok]).max(initial=0.0)))
            worst["longitude"] = max(worst["longitude"], float(T.ulps(got["longitude"][same], x[same]).max(initial=0.0)))
            n += int(ok.sum()) + int(same.sum())
    print(f"largest |device atan2 - numpy atan2| in ulp over {n} evaluations:", worst, "-> E =", max(worst.values()), "recorded:", T.E)
    assert max(worst.values()) <= T.E


# ------------------------------------------------------------------ what the cases are there for
def test_the_cases_reach_the_edges_the_seam_and_the_pole(eng):
    case, _, _ = _prepared("edges")
    _, got = _run(eng, "edges")
    y, x, v = got["latitude"], got["longitude"], got["values"][0]
    lat, lon = case["lat"], case["lon"]
    for out in (y < lat[0], y > lat[-1], x < lon[0], x > lon[-1]):                   # each of the four edges is crossed ...
        assert out.any() and np.isnan(v[out]).all()                                # ... and beyond it there is no value
    inside = (y >= lat[0]) & (y <= lat[-1]) & (x >= lon[0]) & (x <= lon[-1])
    assert not np.isnan(v[inside]).any() and np.array_equal(np.isnan(v), ~inside)
    for name in ("seam", "seam-lon0-20"):
        case, _, want = _prepared(name)
        trace, got = _run(eng, name)
        assert want["count"].size == 3 and not np.isnan(got["values"]).any()         # the row across the seam is one line
        x, lon = got["longitude"], case["lon"]
        crossing = (x.max(axis=1) - x.min(axis=1)) > 180.0                          # a transect with samples at both ends of the range
        assert crossing.any() and (x >= lon[0]).all() and (x < lon[0] + 360.0).all()
        assert (x > lon[-1]).any()                                                 # samples in the seam cell
    for name in ("pole", "pole-not-cyclic"):
        case, _, _ = _prepared(name)
        trace, got = _run(eng, name)
        y, x = got["latitude"], got["longitude"]
        over = (np.abs(x - x[:, [y.shape[1] // 2]]) > 90.0) & (np.abs(x - x[:, [y.shape[1] // 2]]) < 270.0)   # beyond the pole: the far meridian
        assert over[y > 80].any() and over[y < -80].any() and y.max() > 89.0 and y.min() < -89.0
        assert not np.isnan(got["values"][:, over & (x >= case["lon"][0]) & (x <= case["lon"][-1])]).any()


def test_fields_share_positions_and_a_launch_of_four_changes_nothing(eng):
    """5 fields take two launches, the second of which reads the stored positions: every field equals the field sampled on its
    own, bit for bit, in both dtypes and with a stack of planes; a plane of a stack equals the plane on its own."""
    for name in ("ring-junction-2d-f64x5", "shapes-3d-f32x5-M41"):
        case, fields, _ = _prepared(name)
        assert fields.shape[0] == 5 > TR_FIELDS
        for method in T.METHODS:
            _, got = _run(eng, name, "north", method)
            for f in range(5):
                _, alone = _run(eng, name, "north", method, fields=fields[f:f + 1])
                for k in ("latitude", "longitude", "normal"):
                    assert np.array_equal(alone[k], got[k], equal_nan=True)
                assert np.array_equal(alone["values"][0], got["values"][f], equal_nan=True)
                assert np.array_equal(alone["line_mean"][0], got["line_mean"][f], equal_nan=True)
                assert np.array_equal(alone["line_count"][0], got["line_count"][f])
    case, fields, want = _prepared("shapes-3d-f32x5-M41")
    trace, got = _run(eng, "shapes-3d-f32x5-M41")
    for m in range(3):
        t = eng.trace_lines(case["mask"][m], False, "sphere", case["lat"], case["lon"])
        one = eng.ridge_transects(t, fields[:, m], case["lat"], case["lon"], case["half_width"], case["spacing"])
        rows = np.flatnonzero(want["plane"][want["line"]] == m)
        assert rows.size == t["pixel"].numel() and np.array_equal(_np(one["values"]), got["values"][:, rows], equal_nan=True)
        assert np.array_equal(_np(one["line_mean"]), got["line_mean"][:, want["plane"] == m], equal_nan=True)


def test_nan_nodes_make_their_cells_nan_and_the_composite_leaves_them_out(eng):
    for name in ("shapes-3d-f64x1-nan", "ring-2d-f32x1-nan"):
        case, fields, want = _prepared(name)
        _, got = _run(eng, name)
        _, filled = _run(eng, name, fields=np.nan_to_num(fields, nan=1.0))
        holes = np.isnan(got["values"]) & ~np.isnan(filled["values"])
        assert holes.any() and (got["line_count"] < filled["line_count"]).any() and (got["line_count"] <= filled["line_count"]).all()
        assert np.array_equal(got["values"][~holes], filled["values"][~holes], equal_nan=True)
        _, near = _run(eng, name, method="nearest")
        assert np.isnan(near["values"]).sum() < np.isnan(got["values"]).sum()           # one node, not four


@pytest.mark.parametrize("name", ["line-%d-M1" % (TR_CHUNK + 1), "shapes-3d-f32x5-M41", "pole", "gaussian-latitudes"])
def test_two_calls_agree_bit_for_bit(eng, name):
    case, fields, _ = _prepared(name)
    _, first = _run(eng, name, "east", "linear")
    _, again = _run(eng, name, "east", "linear")
    assert first.keys() == again.keys() and all(np.array_equal(first[k], again[k], equal_nan=True) for k in first)
    t = eng.torch
    trace = eng.trace_lines(t.as_tensor(case["mask"], device=eng.device), case["cyclic"], "sphere", case["lat"], case["lon"])
    dev = eng.ridge_transects(trace, t.as_tensor(_fields_for(case, fields), device=eng.device), case["lat"], case["lon"], case["half_width"],
                              case["spacing"], case["smooth"], "east", "linear", case["cyclic"])
    assert eng.last_transects_kernel == KERNELS
    assert all(np.array_equal(_np(dev[k]), first[k], equal_nan=True) for k in first)      # device tensors in: the same call


def test_an_empty_mask_gives_empty_tables_and_a_lone_pixel_gives_nan(eng):
    lat, lon = T.regional_grid(12, 16)
    trace = eng.trace_lines(np.zeros((12, 16)), False, "sphere", lat, lon)
    got = eng.ridge_transects(trace, np.ones((2, 12, 16)), lat, lon, 500e3, 25e3)
    assert tuple(got["values"].shape) == (2, 0, 41) and tuple(got["line_mean"].shape) == (2, 0, 41) and tuple(got["normal"].shape) == (0, 3)
    _, got = _run(eng, "line-1-M3")
    assert np.isnan(got["values"]).all() and np.isnan(got["latitude"]).all() and not got["line_count"].any() and np.isnan(got["line_mean"]).all()
    with pytest.raises(ValueError, match="traced mask"):
        eng.ridge_transects(trace, np.ones((2, 3, 12, 16)), lat, lon, 500e3, 25e3)


# ------------------------------------------------------------------ the public surface
def test_ridge_transects_through_tools_with_descending_coordinates_and_named_fields(eng):
    from lagrangiancoherence_amd import tools
    from lagrangiancoherence_amd.dropin import get_engine
    case, fields, want = _prepared("shapes-3d-f32x5-M41")
    lat, lon, mask = case["lat"], case["lon"], case["mask"]
    coords = {"time": np.arange(3), "latitude": lat[::-1].copy(), "longitude": lon}
    dims = ("time", "latitude", "longitude")
    ridges = DataArray(mask[:, ::-1].copy(), dims, coords)
    named = {"pr": DataArray(fields[0][:, ::-1].copy(), dims, coords),
             "tcwv": DataArray(fields[1][:, ::-1].transpose(1, 2, 0).copy(), ("latitude", "longitude", "time"), coords)}
    lines, points, tr = tools.ridge_transects(ridges, named, case["half_width"], case["spacing"], orient="north")
    assert get_engine().last_transects_kernel == KERNELS
    want_lines, want_points = tools.ridge_lines(ridges, None, False, "sphere")
    assert lines.keys() == want_lines.keys() and all(np.array_equal(lines[k], want_lines[k], equal_nan=True) for k in lines)
    assert set(points) == set(want_points) | {"normal_east", "normal_north", "heading"}
    assert all(np.array_equal(points[k], want_points[k], equal_nan=True) for k in want_points)
    _, got = _run(eng, "shapes-3d-f32x5-M41", "north", fields=fields[:2])
    assert set(tr) == {"offset", "latitude", "longitude", "values", "line_mean", "line_count"}
    assert set(tr["values"]) == set(tr["line_mean"]) == set(tr["line_count"]) == {"pr", "tcwv"}
    for k, key in enumerate(("pr", "tcwv")):
        assert tr["values"][key].dtype == np.float32 and np.array_equal(tr["values"][key], got["values"][k], equal_nan=True)
        assert np.array_equal(tr["line_mean"][key], got["line_mean"][k], equal_nan=True)
        assert np.array_equal(tr["line_count"][key], got["line_count"][k])
    for k in ("offset", "latitude", "longitude"):
        assert np.array_equal(tr[k], got[k], equal_nan=True)
    assert np.array_equal(points["normal_east"], got["normal_east"], equal_nan=True)
    assert np.array_equal(points["normal_north"], got["normal_north"], equal_nan=True)
    nrm = _oracle_geometry("shapes-3d-f32x5-M41", "north")[2]
    has = ~np.isnan(nrm[:, 0])
    assert np.array_equal(np.isnan(points["heading"]), ~has) and ((points["heading"][has] >= 0) & (points["heading"][has] < 360)).all()
    assert T.heading_difference(points["heading"][has], T.heading(nrm[has, 5], nrm[has, 6])).max() <= T.HEADING_TOL
    # one array, 2-D, float64: arrays instead of dicts, and the driver's one-liners
    K = case["half_width"] // case["spacing"]
    one = tools.ridge_transects(DataArray(mask[0], dims[1:], {"latitude": lat, "longitude": lon}),
                                DataArray(fields[0, 0].astype(np.float64), dims[1:], {"latitude": lat, "longitude": lon}),
                                case["half_width"], case["spacing"])[2]
    K = int(K)
    assert one["values"].shape[0] == 1 and one["values"].shape[2] == 2 * K + 1 and one["values"].dtype == np.float64
    gradient = (one["values"][:, :, K + 1] - one["values"][:, :, K - 1]) / (2 * case["spacing"])
    assert gradient.shape == one["values"].shape[:2] and np.isfinite(gradient).any()
