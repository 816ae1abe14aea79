"""Great-circle transects across ridge lines without a GPU: the numpy oracle of tests/transects.py against independent facts --
the haversine distance of every sample from its point, the right angle to the chord, a meridional line, a reversed line, a
field that is linear in latitude and longitude, an argmin lookup --, the cases of tests/test_transects_gpu.py searched for
samples whose cell is ambiguous, the two entry points in the header, the bindings and the library, every refusal of
include/lcs_hip.h's contract -- each returned before the device is touched -- and the argument checks of
Engine.ridge_transects and tools.ridge_transects, which run before an engine exists."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from lagrangiancoherence_amd import _capi, build
from tests import lines as L
from tests import transects as T
from tests.labelled import DataArray

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _single(mask, lat, lon, cyclic=False):
    return L.trace_planes(np.asarray(mask)[None], cyclic, metric="sphere", lat=lat, lon=lon)


@pytest.fixture(scope="module")
def shapes():
    """Ring, junction and a lone pixel on a regional 16 x 24 grid, with the oracle's normals for every orientation."""
    mask = np.maximum(T.ring_mask(16, 24), np.roll(T.junction_mask(16, 24), 11, axis=1))
    lat, lon = T.regional_grid(16, 24)
    trace = _single(mask, lat, lon)
    return mask, lat, lon, trace, {o: T.normals(trace, lat, lon, 3, o) for o in T.ORIENTS}


# ------------------------------------------------------------------ the oracle against independent facts
def test_every_sample_lies_at_its_offset_from_its_point(shapes):
    """The haversine distance from the point to sample k is |s_k|, to tests/test_sphere_distance.py's 1e-7 m."""
    _, lat, lon, trace, nrm = shapes
    K, s, c, sn = T.offsets(500e3, 25e3)
    worst = 0.0
    for orient in T.ORIENTS:
        y, x, _ = T.raw_positions(nrm[orient][:, :3], trace["pixel"], lat, lon, c, sn)
        for i, p in enumerate(trace["pixel"]):
            if np.isnan(y[i, 0]):
                continue
            for k in range(2 * K + 1):
                d = T.haversine(lon[p % lon.size], lat[p // lon.size], x[i, k], y[i, k])
                worst = max(worst, abs(d - abs(s[k])))
    print(f"max | haversine distance - |s_k| | = {worst:.3e} m")
    assert worst <= 1e-7


def test_the_transect_is_at_right_angles_to_the_chord(shapes):
    """n . (p_b - p_a) = 0: n = p x t with t the chord made perpendicular to p, so the chord lies in the plane of p and t.  The
    roundings of t, n and the product are relative ones: NORMAL_TOL times the chord's length covers them.  And n . p = 0."""
    _, lat, lon, trace, nrm = shapes
    tab = T.tables(lat, lon)
    worst = 0.0
    for off, cnt, closed in zip(trace["offset"], trace["count"], trace["closed"]):
        for j in range(cnt):
            a, b = T.chord_ends(j, int(cnt), bool(closed), 3)
            n = nrm["left"][off + j, :3]
            if np.isnan(n[0]):
                assert a == b
                continue
            pa, pb, p = (np.array(T.unit(tab, trace["pixel"][off + q], lon.size)) for q in (a, b, j))
            d = pb - pa
            worst = max(worst, abs(float(n @ d)) / float(np.linalg.norm(d)), abs(float(n @ p)))
            assert abs(float(np.linalg.norm(n)) - 1.0) <= T.NORMAL_TOL
    print(f"max |n . chord| / |chord|, |n . p| = {worst:.3e}")
    assert worst <= T.NORMAL_TOL


def test_a_meridional_line_is_crossed_along_the_tangent_great_circle_of_its_parallel():
    """A line along a meridian is travelled northwards (its first dart is the smaller one), so the left normal points west: no
    north and no vertical component, heading 0, and on that great circle sin(latitude) = cos(s / R) sin(latitude of the point)."""
    lat, lon = T.regional_grid(16, 24)
    mask = np.zeros((16, 24))
    mask[2:13, 9] = 1
    trace = _single(mask, lat, lon)
    nrm = T.normals(trace, lat, lon, 3, "left")
    assert np.abs(nrm[:, 2]).max() <= T.NORMAL_TOL and np.abs(nrm[:, 4]).max() <= T.NORMAL_TOL
    assert np.abs(nrm[:, 3] + 1.0).max() <= T.NORMAL_TOL and T.heading_difference(T.heading(nrm[:, 5], nrm[:, 6]), 0.0).max() <= T.HEADING_TOL
    K, s, c, sn = T.offsets(500e3, 25e3)
    y, x, _ = T.raw_positions(nrm[:, :3], trace["pixel"], lat, lon, c, sn)
    own = lat[trace["pixel"] // 24]
    want = np.degrees(np.arcsin(c[None, :] * np.sin(np.radians(own))[:, None]))
    assert np.abs(y - want).max() <= 1e-12                      # degrees: a few ulp of 70 through arcsin near its steep end
    assert (np.diff(x, axis=1) < 0).all() and np.abs(x[:, K] - lon[9]).max() <= 1e-13      # westwards, through the point
    east = T.normals(trace, lat, lon, 3, "east")
    assert np.array_equal(east[:, :5], -nrm[:, :5]) and np.array_equal(east[:, 5:], nrm[:, 5:])


def test_reversing_a_line_reverses_left_but_not_north(shapes):
    _, lat, lon, trace, nrm = shapes
    rev = {k: np.array(v) for k, v in trace.items()}
    for off, cnt in zip(trace["offset"], trace["count"]):
        rev["pixel"][off:off + cnt] = trace["pixel"][off:off + cnt][::-1]

    def back(a):                                                # the reversed line's rows in the original order of the points
        out = a.copy()
        for off, cnt in zip(trace["offset"], trace["count"]):
            out[off:off + cnt] = a[off:off + cnt][::-1]
        return out
    left, north, east = (back(T.normals(rev, lat, lon, 3, o)) for o in T.ORIENTS)
    assert np.array_equal(left, -nrm["left"], equal_nan=True)                                  # normal and tangent, exactly
    for got, want in ((north, nrm["north"]), (east, nrm["east"])):
        assert np.array_equal(got[:, :5], want[:, :5], equal_nan=True) and np.array_equal(got[:, 5:], -want[:, 5:], equal_nan=True)
    ok = ~np.isnan(nrm["north"][:, 0])
    assert (nrm["north"][ok, 4] >= 0).all() and (nrm["east"][ok, 3] >= 0).all() and (nrm["left"][ok, 4] < 0).any()


@pytest.mark.parametrize("grid", ["regional", "gaussian-cyclic"])
def test_a_field_linear_in_latitude_and_longitude_is_reproduced(grid):
    """f = a + b latitude + c longitude on the nodes (on the seam cell's far side: + 360 c): bilinear weights reproduce it up to
    the rounding of four products and three sums of terms bounded by |a| + |b| 90 + |c| 540: 8 eps64 of that."""
    mask = np.maximum(T.ring_mask(16, 24), T.junction_mask(16, 24))
    cyclic = grid != "regional"
    lat, lon = T.regional_grid(16, 24) if not cyclic else T.gaussian_like_grid(16, 24)
    trace = _single(mask, lat, lon, cyclic)
    K, s, c, sn = T.offsets(800e3, 50e3)
    nrm = T.normals(trace, lat, lon, 3, "north")
    y, x = T.positions(nrm[:, :3], trace["pixel"], lat, lon, c, sn, cyclic)
    a, b, cc = 3.0, -0.25, 0.0 if cyclic else 0.125               # across the seam only a field without a longitude term is linear
    f = a + b * lat[:, None] + cc * lon[None, :]
    v, scale = T.interpolate(f[None], np.zeros(len(trace["pixel"]), dtype=int), y, x, lat, lon, cyclic)
    inside = ~np.isnan(v)
    assert inside.sum() > 0.5 * v.size
    err = np.abs(v - (a + b * y + cc * x))[inside]
    assert err.max() <= 8 * T.EPS64 * (abs(a) + abs(b) * 90 + abs(cc) * 540)


def test_nearest_is_an_argmin_lookup_away_from_ties(shapes):
    _, lat, lon, trace, nrm = shapes
    K, s, c, sn = T.offsets(800e3, 50e3)
    y, x = T.positions(nrm["left"][:, :3], trace["pixel"], lat, lon, c, sn)
    f = T.fields_of(1, (1, 16, 24), 11)[0]
    v, _ = T.interpolate(f, np.zeros(len(trace["pixel"]), dtype=int), y, x, lat, lon, False, "nearest")
    tie = T.ambiguous(y, x, lat, lon, False, "nearest")
    inside = (y >= lat[0]) & (y <= lat[-1]) & (x >= lon[0]) & (x <= lon[-1]) & ~tie
    j, i = np.abs(y[..., None] - lat).argmin(-1), np.abs(x[..., None] - lon).argmin(-1)
    assert inside.sum() > 1000 and np.array_equal(v[inside], f[0][j, i][inside])
    assert np.isnan(v[~np.isnan(y) & ((y < lat[0]) | (y > lat[-1]) | (x < lon[0]) | (x > lon[-1]))]).all()
    # a tie goes to the lower index, in both axes
    yy, xx = np.array([[(lat[3] + lat[4]) / 2]]), np.array([[(lon[5] + lon[6]) / 2]])
    assert yy[0, 0] - lat[3] == lat[4] - yy[0, 0] and xx[0, 0] - lon[5] == lon[6] - xx[0, 0]
    assert T.interpolate(f, [0], yy, xx, lat, lon, False, "nearest")[0][0, 0] == f[0, 3, 5]


def test_the_seam_cell_and_the_wrap():
    lat, lon = np.array([-10.0, 0.0, 10.0]), np.array([-180.0, -90.0, 0.0, 90.0])
    x = T.wrap(np.array([-180.0, 180.0, 179.0, -181.0, 540.0, 90.0]), lon[0])
    assert np.array_equal(x, [-180.0, -180.0, 179.0, 179.0, -180.0, 90.0])
    f = np.arange(12.0).reshape(1, 3, 4)
    y = np.zeros((1, 3))
    v, _ = T.interpolate(f, [0], y, np.array([[135.0, 90.0, 179.0]]), lat, lon, True)
    assert v[0, 0] == (f[0, 1, 3] + f[0, 1, 0]) / 2 and v[0, 1] == f[0, 1, 3] and abs(v[0, 2] - (f[0, 1, 3] * 1 + f[0, 1, 0] * 89) / 90) < 1e-14
    assert np.isnan(T.interpolate(f, [0], y, np.array([[135.0, 90.5, -181.0]]), lat, lon, False)[0]).all()
    last = T.interpolate(f, [0], np.array([[10.0, 10.0]]), np.array([[90.0, 0.0]]), lat, lon, False)[0]      # the last row and column themselves
    assert last[0, 0] == f[0, 2, 3] and last[0, 1] == f[0, 2, 2]
    g = f.copy()
    g[0, 2, 3] = np.nan                                           # a NaN corner with weight 0 still makes the sample NaN
    assert np.isnan(T.interpolate(g, [0], np.array([[0.0]]), np.array([[0.0]]), lat, lon, False)[0][0, 0])
    assert np.isnan(T.interpolate(g, [0], np.array([[5.0]]), np.array([[45.0]]), lat, lon, False)[0][0, 0])


def test_the_composite_counts_finite_values_only():
    v = np.array([[1.0, np.nan], [2.0, np.nan], [np.inf, 4.0], [5.0, 6.0]])
    mean, n, scale = T.composite(v, [0, 3], [3, 1])
    assert np.array_equal(n, [[2, 1], [1, 1]]) and np.array_equal(mean, [[1.5, 4.0], [5.0, 6.0]])
    mean, n, _ = T.composite(v[:2], [0], [2])
    assert n[0, 1] == 0 and np.isnan(mean[0, 1])


def test_no_sample_of_the_gpu_cases_has_an_ambiguous_cell():
    """tests/test_transects_gpu.py exempts from its comparison of cells the samples within the position bound of a node's
    latitude or longitude, of a midpoint (nearest) or of the domain's edge.  Samples at offset 0 lie on their own node and the
    transects of points whose normal has no east component follow their meridian: those are on a grid line by construction.
    Beside them the oracle finds none in the cases used, for either method and every orientation."""
    for name, case in T.cases().items():
        trace, fields = T.case_trace(case), T.case_fields(case)
        for orient in T.ORIENTS:
            o = T.oracle(trace, fields[:1], case["lat"], case["lon"], case["half_width"], case["spacing"], case["smooth"], orient,
                         "linear", case["cyclic"])
            for method in T.METHODS:
                amb = T.ambiguous(o["latitude"], o["longitude"], case["lat"], case["lon"], case["cyclic"], method)
                amb &= ~np.isnan(o["latitude"]) & ~T.on_a_grid_line(o["normal"], o["K"])
                assert not amb.any(), (name, orient, method, int(amb.sum()))


# ------------------------------------------------------------------ header, bindings, library
@pytest.fixture(scope="module")
def lib():
    build.build_library(verbose=False)
    return _capi.load()


NAMES = ("lc_ridge_transects", "lc_ctx_last_transects_kernel")


def test_the_entry_points_are_declared_prototyped_and_exported(lib):
    text = open(os.path.join(ROOT, "include", "lcs_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _capi.PROTOTYPES and hasattr(lib, name), name
    section = text[text.index("great-circle transects across ridge lines"):text.index("int lc_ridge_transects(")]
    assert "LCS/area_of_influence.py:17-87" in section and section.count("area_of_influence.py:17-87") >= 2      # both symbols cite it
    assert "transects.hip" in build.SOURCES
    assert lib.lc_version() == 104 == _capi.LC_VERSION
    assert lib.lc_ctx_last_transects_kernel(None) == b""
    assert (_capi.LC_ORIENT_LEFT, _capi.LC_ORIENT_NORTH, _capi.LC_ORIENT_EAST) == (0, 1, 2)
    assert re.search(r"LC_ORIENT_LEFT = 0, LC_ORIENT_NORTH = 1, LC_ORIENT_EAST = 2", header)
    assert re.search(r"LC_TRANSECT_LINEAR = 0, LC_TRANSECT_NEAREST = 1", header)


# A context nobody dereferences and pointers nobody follows: every call below is refused by its argument checks.
_BLOCK = C.create_string_buffer(4096)
CTX = PTR = C.cast(_BLOCK, C.c_void_p)
POINTERS = ("pixel", "point_line", "line_offset", "line_count", "line_plane", "line_closed", "cos_lat", "sin_lat", "cos_lon", "sin_lon",
            "lat_deg", "lon_deg", "cos_off", "sin_off", "fields", "normal_out", "lat_out", "lon_out", "values_out", "mean_out", "count_out")
GOOD = dict(ctx=CTX, dtype=_capi.LC_F64, ny=5, nx=7, n_planes=1, n_points=9, n_lines=2, n_offsets=5, n_fields=2, smooth=3, orient=0,
            method=0, cyclic_x=0, **{p: PTR for p in POINTERS})
EINVAL, EUNSUPPORTED = _capi.LC_EINVAL, _capi.LC_EUNSUPPORTED
REFUSALS = [
    (dict(ctx=None), EINVAL, b"null context"),
    (dict(dtype=2), EINVAL, b"bad dtype"),
    (dict(ny=1), EINVAL, b"bad size"),
    (dict(nx=1), EINVAL, b"bad size"),
    (dict(n_planes=0), EINVAL, b"bad size"),
    (dict(n_points=0), EINVAL, b"bad size"),
    (dict(n_lines=-1), EINVAL, b"bad size"),
    (dict(n_fields=0), EINVAL, b"bad size"),
    (dict(n_offsets=0), EINVAL, b"bad n_offsets"),
    (dict(n_offsets=4), EINVAL, b"bad n_offsets"),
    (dict(smooth=0), EINVAL, b"bad smooth"),
    (dict(orient=3), EINVAL, b"bad orient"),
    (dict(orient=-1), EINVAL, b"bad orient"),
    (dict(method=2), EINVAL, b"bad method"),
    (dict(cyclic_x=1, nx=2), EINVAL, b"cyclic_x needs at least 3 columns"),
    (dict(ny=1 << 16, nx=1 << 15), EUNSUPPORTED, b"too large"),
    (dict(n_points=1 << 28, n_offsets=9), EUNSUPPORTED, b"too large"),
    (dict(n_lines=1 << 28, n_points=1 << 20, n_offsets=9), EUNSUPPORTED, b"too large"),
    (dict(n_fields=65536), EUNSUPPORTED, b"too large"),
] + [({p: None}, EINVAL, b"null pointer") for p in POINTERS]


def _call(g):
    a = _capi.TransectsArgs(struct_size=C.sizeof(_capi.TransectsArgs))
    for k, v in g.items():
        if k != "ctx":
            setattr(a, k, v)
    return _capi.load().lc_ridge_transects(g["ctx"], C.byref(a))


@pytest.mark.parametrize("change, status, message", REFUSALS, ids=["-".join(f"{k}={v}" for k, v in c.items()) for c, _, _ in REFUSALS])
def test_the_call_refuses_before_it_touches_a_device(lib, change, status, message):
    assert _call({**GOOD, **change}) == status
    err = lib.lc_last_error()
    assert message in err and b"lc_ridge_transects" in err


def test_the_structure_matches_the_library(lib):
    size = C.sizeof(_capi.TransectsArgs)
    a = _capi.TransectsArgs(struct_size=size - 8)
    assert lib.lc_ridge_transects(CTX, C.byref(a)) == EINVAL
    err = lib.lc_last_error()
    assert b"struct_size %d" % (size - 8) in err and b"this library has %d" % size in err      # both numbers
    assert lib.lc_ridge_transects(CTX, None) == EINVAL and b"null argument structure" in lib.lc_last_error()
    assert lib.lc_ridge_transects(None, None) == EINVAL and b"null context" in lib.lc_last_error()


def test_the_kernels_never_wait_and_none_takes_a_trigonometric_function_of_a_coordinate():
    """No atomic, no cooperative launch, no fence, no inline assembly, no loop without a counted end; every kernel forbids
    contraction; atan2 is the only library function of an angle."""
    src = open(os.path.join(build.CSRC, "transects.hip")).read()
    code = build._strip_comments(src)
    for word in ("cooperative", "grid_group", "this_grid", "__threadfence", "atomic", "while (", "for (;;)", "volatile", "asm", "torch"):
        assert word not in code, word
    for kernel in ("transect_normal_kernel", "transect_sample_kernel", "transect_composite_kernel"):
        body = src[src.index("void " + kernel):]
        assert body[body.index("{"):].lstrip("{ \n").startswith("#pragma clang fp contract(off)"), kernel
    for word in ("cos(", "sin(", "sincos", "tan(", "hypot("):
        assert word not in code, word
    assert code.count("atan2(") == 2


# ------------------------------------------------------------------ the engine's and the surface's own refusals
GRID = (np.linspace(-40.0, 40.0, 9), np.linspace(-180.0, 135.0, 8))
HOST_REFUSALS = [
    (dict(spacing=0.0), "spacing"), (dict(spacing=-1.0), "spacing"), (dict(spacing=np.nan), "spacing"), (dict(spacing=np.inf), "spacing"),
    (dict(half_width=-1.0), "half_width"), (dict(half_width=np.inf), "half_width"), (dict(half_width=np.nan), "half_width"),
    (dict(half_width=T.RADIUS * np.pi / 2), "quarter of the circumference"), (dict(half_width=2.0, radius=1.0), "quarter of the circumference"),
    (dict(smooth=0), "smooth"), (dict(smooth=-2), "smooth"), (dict(smooth=1.5), "smooth"),
    (dict(orient="right"), "orient"), (dict(orient=None), "orient"), (dict(method="cubic"), "method"),
    (dict(lat=np.array([0.0, 1.0, 1.0, 2, 3, 4, 5, 6, 7])), "distinct"), (dict(lon=GRID[1][::-1]), "distinct"),
    (dict(lat=np.linspace(-91.0, 40.0, 9)), r"within \[-90, 90\]"), (dict(lat=np.linspace(-40.0, 40.0, 8)), "len"),
    (dict(lat=np.array([0.0, np.nan, 1, 2, 3, 4, 5, 6, 7])), "finite"),
    (dict(radius=0.0), "radius"), (dict(radius=np.inf), "radius"),
    (dict(cyclic=True, lon=np.array([0.0, 180.0]), shape=(9, 2)), "at least 3 columns"),
    (dict(cyclic=True, lon=np.linspace(0.0, 360.0, 8)), "less than 360"), (dict(cyclic=True, lon=np.linspace(0.0, 400.0, 8)), "less than 360"),
    (dict(n_points=1 << 26, half_width=16 * 25e3), "too large"), (dict(n_lines=1 << 26, half_width=16 * 25e3), "too large"),
    (dict(shape=(9,)), "plane"), (dict(shape=(1, 8), lat=np.array([0.0])), "at least two"),
]


@pytest.mark.parametrize("change, match", HOST_REFUSALS, ids=[f"{i}-" + "-".join(c) for i, (c, _) in enumerate(HOST_REFUSALS)])
def test_the_host_check_refuses_every_bad_option_without_a_device(change, match):
    from lagrangiancoherence_amd.engine import Engine
    good = dict(shape=(9, 8), lat=GRID[0], lon=GRID[1], half_width=500e3, spacing=25e3)
    with pytest.raises(ValueError, match=match):
        Engine.checked_transect_options(**{**good, **change})


def test_the_host_check_returns_the_oracles_tables():
    from lagrangiancoherence_amd.engine import Engine
    opt = Engine.checked_transect_options((3, 9, 8), GRID[0], GRID[1], 510e3, 25e3, smooth=2, orient="east", method="nearest", cyclic=True)
    K, s, c, sn = T.offsets(510e3, 25e3)
    assert (opt["K"], opt["M"]) == (K, 2 * K + 1) == (20, 41) and opt["smooth"] == 2
    assert (opt["orient"], opt["method"]) == (_capi.LC_ORIENT_EAST, _capi.LC_TRANSECT_NEAREST)
    for got, want in zip((opt["offset"], opt["cos_off"], opt["sin_off"], *opt["tables"]), (s, c, sn, *T.tables(*GRID))):
        assert got.dtype == np.float64 and np.array_equal(got, want)
    assert Engine.checked_transect_options((9, 8), GRID[0], GRID[1], 0.0, 25e3)["M"] == 1
    assert Engine.checked_transect_options((9, 8), GRID[0], GRID[1], 24.9e3, 25e3)["M"] == 1


def _ridges(lead=None, descending=False):
    lat, lon = GRID
    lat = lat[::-1] if descending else lat
    m = np.zeros((9, 8))
    m[4, 1:7] = 1
    coords = {"latitude": lat, "longitude": lon}
    if lead:
        return DataArray(np.stack([m] * lead), ("time", "latitude", "longitude"), {**coords, "time": np.arange(lead)})
    return DataArray(m, ("latitude", "longitude"), coords)


def test_the_tool_checks_its_arguments_before_it_creates_an_engine(monkeypatch):
    from lagrangiancoherence_amd import tools

    def no_engine():
        raise AssertionError("an engine was asked for")
    monkeypatch.setattr(tools, "get_engine", no_engine)
    r = _ridges()
    for kw, match in ((dict(spacing=0), "spacing"), (dict(half_width=-1), "half_width"), (dict(half_width=1.1e7), "quarter"),
                      (dict(smooth=0), "smooth"), (dict(orient="up"), "orient"), (dict(method="spline"), "method"), (dict(radius=-1.0), "radius")):
        for ridges in (r, _ridges(lead=2)):
            with pytest.raises(ValueError, match=match):
                tools.ridge_transects(ridges, ridges, **{**dict(half_width=500e3, spacing=25e3), **kw})
    other = DataArray(np.zeros((9, 8)), ("latitude", "longitude"), {"latitude": GRID[0] + 1.0, "longitude": GRID[1]})
    with pytest.raises(ValueError, match="coordinates"):
        tools.ridge_transects(r, other, 500e3, 25e3)
    with pytest.raises(ValueError, match=r"fields\['pr'\] differ in their coordinates"):
        tools.ridge_transects(r, {"ok": r, "pr": other}, 500e3, 25e3)
    with pytest.raises(ValueError, match="dims"):
        tools.ridge_transects(r, _ridges(lead=2), 500e3, 25e3)
    with pytest.raises(ValueError, match="dims"):
        tools.ridge_transects(r, np.zeros((9, 8)), 500e3, 25e3)
    with pytest.raises(ValueError, match="shapes"):
        tools.ridge_transects(_ridges(lead=3), _ridges(lead=2), 500e3, 25e3)
    with pytest.raises(ValueError, match="at least one"):
        tools.ridge_transects(r, {}, 500e3, 25e3)
    twice = DataArray(np.zeros((9, 8)), ("latitude", "longitude"), {"latitude": np.r_[GRID[0][:8], GRID[0][0]], "longitude": GRID[1]})
    with pytest.raises(ValueError):                              # coordinates that are not distinct (the area tables refuse them first)
        tools.ridge_transects(twice, twice, 500e3, 25e3)
    wide = DataArray(np.zeros((9, 8)), ("latitude", "longitude"), {"latitude": GRID[0], "longitude": np.linspace(0.0, 360.0, 8)})
    with pytest.raises(ValueError):
        tools.ridge_transects(wide, wide, 500e3, 25e3, cyclic=True)


def test_the_name_is_exported_from_both_tools_modules():
    import inspect
    from LagrangianCoherence.LCS import tools as shim
    from lagrangiancoherence_amd import tools
    from lagrangiancoherence_amd.engine import Engine
    assert "ridge_transects" in tools.__all__ and shim.ridge_transects is tools.ridge_transects and "ridge_transects" in tools.__doc__
    p = inspect.signature(tools.ridge_transects).parameters
    assert list(p) == ["ridges", "fields", "half_width", "spacing", "smooth", "orient", "method", "cyclic", "radius"]
    assert (p["smooth"].default, p["orient"].default, p["method"].default, p["cyclic"].default, p["radius"].default) == (3, "left", "linear", False, 6371000.0)
    p = inspect.signature(Engine.ridge_transects).parameters
    assert list(p)[:7] == ["self", "trace", "fields", "lat", "lon", "half_width", "spacing"]
    assert inspect.signature(tools.ridge_lines).parameters.keys() == {"ridges", "intensity", "cyclic", "metric", "radius"}
