"""Inverse-distance weighting on the sphere without a GPU: the numpy oracle of tests/idw.py against the textbook haversine
formula and against what the reference's formula means, the oracle's own rules (exact hits, NaN values, left-out points, an
empty reach, the count), the entry points in the header, the bindings and the library, every refusal of include/lcs_hip.h's
contract -- each returned before the device is touched -- and the argument checks of Engine.idw_interp,
tools.Inverse_weighted_interpolation and tools.xr_idx_interp, which run before an engine exists."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from lagrangiancoherence_amd import _capi, build
from tests import idw as IDW
from tests.labelled import DataArray

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the oracle
def test_the_oracles_distance_is_the_haversine_distance():
    """About 200 random pairs plus pole, seam and antipode: <= 1e-7 m on a sphere of 6371 km, the figure of
    tests/test_sphere_distance.py."""
    lon1, lat1 = IDW.scattered(200, 1, lat_max=90.0)
    lon2, lat2 = IDW.scattered(200, 2, lat_max=90.0)
    special = [(0.0, 90.0, 123.0, -90.0), (10.0, 90.0, -170.0, 89.0), (180.0, 5.0, -180.0, 5.0), (179.5, -3.0, -179.5, 3.0),
               (0.0, 0.0, 180.0, 0.0), (37.0, 41.0, -143.0, -41.0), (12.0, 34.0, 12.0, 34.0), (0.0, -90.0, 77.0, -90.0)]
    lon1, lat1, lon2, lat2 = (np.concatenate([a, [s[k] for s in special]]) for k, a in enumerate((lon1, lat1, lon2, lat2)))
    worst = 0.0
    for k in range(lon1.size):                                              # a plain double loop: one pair at a time
        cost = IDW.costs(IDW.unit(lon2[k:k + 1], lat2[k:k + 1]), IDW.unit(lon1[k:k + 1], lat1[k:k + 1]))
        worst = max(worst, abs(float(IDW.distances(cost)[0, 0]) - IDW.haversine(lon1[k], lat1[k], lon2[k], lat2[k])))
    print(f"max |chord form - haversine| over {lon1.size} pairs = {worst:.3e} m")
    assert worst <= 1e-7
    seam = IDW.costs(IDW.unit([-180.0], [5.0]), IDW.unit([180.0], [5.0]))
    assert IDW.distances(seam)[0, 0] <= 1e-7
    anti = IDW.distances(IDW.costs(IDW.unit([180.0], [0.0]), IDW.unit([0.0], [0.0])))[0, 0]
    assert abs(anti - math.pi * IDW.RADIUS) <= 1e-7


def test_the_oracle_is_what_the_references_formula_means_and_no_radius_enters():
    """50 sources x 40 targets: sum(z / d^2) / sum(1 / d^2) with the textbook haversine on the reference's R = 6378.1 against the
    oracle on 6371000 m.  Both evaluate one quotient of sums of positive weights: the weights agree to the 1e-7 m of the test
    above, relative to distances of 100 km and more, so 1e-9 relative to the values' scale is a hundred times what that allows."""
    x, y = IDW.scattered(50, 3)
    xi, yi = IDW.scattered(40, 4)
    z = IDW.values(None, 50, 5)
    want = IDW.reference_formula(x, y, z, xi, yi, 6378.1)
    o = IDW.oracle(x, y, z, xi, yi)
    assert np.abs(o["u"] - want).max() <= 1e-9 * o["scale"].max()
    other = IDW.oracle(x, y, z, xi, yi, radius=6378.1)
    assert np.abs(other["u"] - o["u"]).max() <= 1e-13 * o["scale"].max() and (other["count"] == 50).all()


def test_the_hit_rule_averages_coincident_sources():
    x, y, z = np.array([10.0, 10.0, 50.0, -120.0]), np.array([20.0, 20.0, -5.0, 60.0]), np.array([3.0, 6.0, 100.0, -7.0])
    o = IDW.oracle(x, y, z, np.array([10.0, 50.0, 0.0]), np.array([20.0, -5.0, 0.0]))
    assert o["u"][0] == 4.5 and o["u"][1] == 100.0 and np.isposinf(o["weight"][:2]).all() and np.isfinite(o["weight"][2])
    assert -7.0 < o["u"][2] < 100.0 and (o["n"] == [2, 1, 4]).all() and (o["count"] == 4).all()
    o32 = IDW.oracle(x, y, z.astype(np.float32), np.array([10.0]), np.array([20.0]))
    assert o32["u"].dtype == np.float32 and o32["u"][0] == np.float32(4.5)


def test_nan_values_are_left_out_plane_by_plane_and_bad_coordinates_altogether():
    x, y = IDW.scattered(30, 6)
    xi, yi = IDW.scattered(12, 7)
    z = IDW.values(3, 30, 8)
    holes = z.copy()
    holes[1, ::3] = np.nan
    o, h = IDW.oracle(x, y, z, xi, yi), IDW.oracle(x, y, holes, xi, yi)
    assert np.array_equal(o["u"][[0, 2]], h["u"][[0, 2]]) and (h["n"][1] == 20).all() and (h["count"] == 30).all()
    assert np.array_equal(h["u"][1], IDW.oracle(x[holes[1] == holes[1]], y[holes[1] == holes[1]], z[1][holes[1] == holes[1]], xi, yi)["u"])
    hit = IDW.oracle(x, y, holes, x[:1], y[:1])                    # a source on the target whose value is NaN in plane 1 only
    assert np.isposinf(hit["weight"][[0, 2], 0]).all() and np.isfinite(hit["weight"][1, 0]) and hit["count"][0] == 30
    bx, by = x.copy(), y.copy()
    bx[4], by[9], by[11] = np.nan, 90.5, np.inf
    keep = np.ones(30, dtype=bool)
    keep[[4, 9, 11]] = False
    b = IDW.oracle(bx, by, z, xi, yi)
    assert np.array_equal(b["u"], IDW.oracle(x[keep], y[keep], z[:, keep], xi, yi)["u"]) and (b["count"] == 27).all()


def test_an_empty_reach_is_nan_with_count_zero_and_the_count_is_the_brute_force_count():
    x, y = IDW.scattered(80, 9)
    xi, yi = IDW.scattered(25, 10)
    z = IDW.values(None, 80, 11)
    for reach in (300e3, 1500e3, 7000e3):
        o = IDW.oracle(x, y, z, xi, yi, max_distance=reach)
        want = np.array([sum(IDW.haversine(x[s], y[s], xi[p], yi[p]) <= reach for s in range(80)) for p in range(25)])
        assert np.array_equal(o["count"], want)                    # no pair of these lies within 1e-7 m of the bound
        assert np.array_equal(np.isnan(o["u"]), o["count"] == 0) and not o["weight"][o["count"] == 0].any()
    assert (IDW.oracle(x, y, z, xi, yi, max_distance=300e3)["count"] == 0).any()
    far = IDW.oracle(x, y, z, xi, yi, max_distance=math.pi * IDW.RADIUS)
    assert np.array_equal(far["u"], IDW.oracle(x, y, z, xi, yi)["u"]) and (far["count"] == 80).all()


def test_grid_targets_are_the_scattered_targets_of_their_mesh():
    lon, lat = np.array([170.0, -180.0, 30.0]), np.array([80.0, -90.0, 0.0, 90.0])
    Lon, Lat = np.meshgrid(lon, lat)
    for a, b in zip(IDW.unit(lon, lat, grid=True), IDW.unit(Lon.ravel(), Lat.ravel())):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------ header, bindings, library
@pytest.fixture(scope="module")
def lib():
    build.build_library(verbose=False)
    return _capi.load()


NAMES = ("lc_idw_interp", "lc_idw_work_elems", "lc_ctx_last_idw_kernel")


def test_the_entry_points_are_declared_prototyped_and_exported(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lcs_hip.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _capi.PROTOTYPES and hasattr(lib, name), name
    assert "idw.hip" in build.SOURCES
    assert lib.lc_version() == 104 == _capi.LC_VERSION
    assert lib.lc_ctx_last_idw_kernel(None) == b""


def test_work_elems_is_pure_arithmetic(lib):
    """One float64 per workgroup of 256 targets (its two int32 range ends); where the sources are split -- fewer than 256
    workgroups of targets, at least 2 x 512 sources -- into min(ceil(512 / workgroups), n_src // 512) pieces: four float64 per
    piece, plane and target and one int32 per piece and target."""
    f = lib.lc_idw_work_elems
    assert f(1, 1, 1) == 1 and f(1023, 257, 3) == 2 and f(513, 700, 5) == 3
    assert f(3000, 40, 1) == 1 + 5 * 40 * 4 + 100 and f(3000, 40, 5) == 1 + 5 * 40 * 20 + 100
    assert f(16020, 16020, 2) == 63 + 9 * 16020 * 8 + 9 * 16020 // 2
    assert f(1 << 20, 256 * 256, 1) == 256 and f(1 << 20, 256 * 255, 1) == 255 + 3 * 65280 * 4 + 3 * 65280 // 2
    assert f(0, 5, 1) == 0 and f(5, -1, 1) == 0 and f(5, 5, 0) == 0 and f(-2, -2, -2) == 0


# A context nobody dereferences and pointers nobody follows: every call below is refused by its argument checks.
_BLOCK = C.create_string_buffer(4096)
CTX = PTR = C.cast(_BLOCK, C.c_void_p)
GOOD = dict(ctx=CTX, dtype=_capi.LC_F64, n_src=7, n_tgt=9, n_planes=2, power=2.0, radius=IDW.RADIUS, max_chord2=0.0, max_distance=0.0,
            src_x=PTR, src_y=PTR, src_z=PTR, values=PTR, tgt_x=PTR, tgt_y=PTR, tgt_z=PTR, out=PTR, weight_out=None, count_out=None,
            work_dev=PTR)
EINVAL = _capi.LC_EINVAL
REFUSALS = [
    (dict(ctx=None), b"null context"),
    (dict(dtype=2), b"bad dtype"),
    (dict(dtype=-1), b"bad dtype"),
    (dict(n_src=0), b"bad size"),
    (dict(n_tgt=-1), b"bad size"),
    (dict(n_planes=0), b"bad size"),
    (dict(power=0.0), b"bad power"),
    (dict(power=-2.0), b"bad power"),
    (dict(power=16.5), b"bad power"),
    (dict(power=float("nan")), b"bad power"),
    (dict(radius=0.0), b"bad radius"),
    (dict(radius=-1.0), b"bad radius"),
    (dict(radius=float("inf")), b"bad radius"),
    (dict(radius=float("nan")), b"bad radius"),
    (dict(max_chord2=float("nan")), b"bad max_chord2"),
    (dict(max_chord2=0.01, max_distance=0.0), b"bad max_distance"),
    (dict(max_chord2=0.01, max_distance=float("nan")), b"bad max_distance"),
    (dict(src_x=None), b"null pointer"),
    (dict(src_z=None), b"null pointer"),
    (dict(values=None), b"null pointer"),
    (dict(tgt_y=None), b"null pointer"),
    (dict(out=None), b"null pointer"),
    (dict(work_dev=None), b"null pointer"),
]


def _call(g):
    a = _capi.IdwArgs(struct_size=C.sizeof(_capi.IdwArgs))
    for k, v in g.items():
        if k != "ctx":
            setattr(a, k, v)
    return _capi.load().lc_idw_interp(g["ctx"], C.byref(a))


@pytest.mark.parametrize("change, message", REFUSALS, ids=["-".join(f"{k}={v}" for k, v in c.items()) for c, _ in REFUSALS])
def test_the_call_refuses_before_it_touches_a_device(lib, change, message):
    assert _call({**GOOD, **change}) == EINVAL
    err = lib.lc_last_error()
    assert message in err and b"lc_idw_interp" in err


def test_the_structure_matches_the_library(lib):
    size = C.sizeof(_capi.IdwArgs)
    a = _capi.IdwArgs(struct_size=size - 8)
    assert lib.lc_idw_interp(CTX, C.byref(a)) == EINVAL
    err = lib.lc_last_error()
    assert b"struct_size %d" % (size - 8) in err and b"this library has %d" % size in err      # both numbers
    assert lib.lc_idw_interp(CTX, None) == EINVAL and b"null argument structure" in lib.lc_last_error()
    assert lib.lc_idw_interp(None, None) == EINVAL and b"null context" in lib.lc_last_error()


def test_the_kernels_never_wait_for_another_workgroup():
    """No atomic at all, no cooperative launch, no grid synchronisation, no fence, no loop without a counted end."""
    src = build._strip_comments(open(os.path.join(build.CSRC, "idw.hip")).read())
    for word in ("cooperative", "grid_group", "this_grid", "hipLaunchCooperativeKernel", "__threadfence", "atomic", "while (", "for (;;)",
                 "volatile"):
        assert word not in src, word


def test_every_kernel_that_forms_the_cost_forbids_contraction_and_none_takes_a_coordinate():
    src = open(os.path.join(build.CSRC, "idw.hip")).read()
    for kernel in ("idw_range_kernel", "idw_search_kernel"):
        body = src[src.index("void " + kernel):]
        assert body[body.index("{"):].lstrip("{ \n").startswith("#pragma clang fp contract(off)"), kernel
    code = build._strip_comments(src)
    for word in ("cos(", "sin(", "sincos", "tan(", "torch"):
        assert word not in code.replace("asin(", ""), word


# ------------------------------------------------------------------ the engine's and the surface's own refusals
def test_the_engine_refuses_bad_arguments_without_a_device():
    from lagrangiancoherence_amd.engine import Engine
    eng = Engine.__new__(Engine)             # no device: the checks come before anything is touched
    x, y, z = np.arange(5.0), np.arange(5.0), np.arange(5.0)
    xi, yi = np.arange(3.0), np.arange(3.0)
    good = dict(src_lon=x, src_lat=y, values=z, tgt_lon=xi, tgt_lat=yi)
    for kw in (dict(src_lat=y[:4]), dict(values=z[:4]), dict(values=np.ones((2, 4))), dict(values=np.ones((2, 2, 5))), dict(tgt_lat=yi[:2]),
               dict(src_lon=x[None], src_lat=y[None]), dict(src_lon=x[:0], src_lat=y[:0], values=z[:0]), dict(tgt_lon=xi[:0], tgt_lat=yi[:0]),
               dict(grid=True, tgt_lon=np.ones((2, 2)), tgt_lat=np.ones((2, 2))), dict(grid=True, tgt_lat=yi[:0]),
               dict(power=0), dict(power=-1), dict(power=16.5), dict(power=float("nan")),
               dict(radius=0.0), dict(radius=-1.0), dict(radius=np.inf), dict(radius=np.nan),
               dict(max_distance=0.0), dict(max_distance=-5.0), dict(max_distance=float("nan")), dict(max_distance=1e-300)):
        with pytest.raises(ValueError):
            eng.idw_interp(**{**good, **kw})


def test_the_plan_is_the_oracles_points_and_bound():
    from lagrangiancoherence_amd.engine import Engine
    x, y = IDW.scattered(40, 12)
    y[3], x[7] = 91.0, np.nan
    lon, lat = np.array([170.0, -180.0, 30.0, 400.0]), np.array([80.0, -90.0, 0.0])
    plan = Engine.idw_plan(x, y, (2, 40), lon, lat, grid=True, max_distance=250e3)
    assert plan["shape"] == (3, 4) and plan["n_planes"] == 2 and plan["max_chord2"] == IDW.chord2_of(250e3) and plan["max_distance"] == 250e3
    for got, want in zip(plan["tgt"], IDW.unit(lon, lat, grid=True)):
        assert got.dtype == np.float64 and np.array_equal(got, want)
    order = plan["order"]
    assert sorted(order) == list(range(40)) and set(order[-2:]) == {3, 7}                     # the points left out come last
    for got, want in zip(plan["src"], IDW.unit(x, y)):
        assert np.array_equal(got, want[order], equal_nan=True)
    assert (np.diff(plan["src"][2][:-2]) >= 0).all()
    free = Engine.idw_plan(x, y, (40,), x[:5], y[:5])
    assert free["order"] is None and free["n_planes"] is None and free["shape"] == (5,) and free["max_chord2"] == 0.0
    assert Engine.idw_plan(x, y, (40,), x[:5], y[:5], radius=2.0, max_distance=2.0 * np.pi)["max_chord2"] == 0.0     # >= pi radius: unbounded


def _points(n=6, lead=None):
    coords = {"longitude": np.linspace(-50.0, 50.0, n), "latitude": np.linspace(-20.0, 20.0, n)}
    if lead:
        return DataArray(np.ones((lead, n)), ("time", "points"), {**coords, "time": np.arange(lead)})
    return DataArray(np.ones(n), ("points",), coords)


def test_the_tools_check_their_arguments_before_they_create_an_engine(monkeypatch):
    from lagrangiancoherence_amd import tools

    def no_engine():
        raise AssertionError("an engine was asked for")
    monkeypatch.setattr(tools, "get_engine", no_engine)
    lon, lat = np.arange(4.0), np.arange(3.0)
    for kw, match in ((dict(p=0), "power"), (dict(p=17), "power"), (dict(radius=-1.0), "radius"), (dict(radius=np.inf), "radius"),
                      (dict(max_distance=0), "max_distance"), (dict(max_distance=-3.0), "max_distance")):
        with pytest.raises(ValueError, match=match):
            tools.xr_idx_interp(_points(), lon, lat, **kw)
        with pytest.raises(ValueError, match=match):
            tools.xr_idx_interp(_points(lead=2), lon, lat, **kw)
    with pytest.raises(ValueError, match="grid=True"):
        tools.xr_idx_interp(_points(), np.ones((2, 2)), lat)
    bad = DataArray(np.ones((2, 6)), ("time", "points"), {"longitude": np.arange(5.0), "latitude": np.arange(6.0)})
    with pytest.raises(ValueError, match="src_lon"):
        tools.xr_idx_interp(bad, lon, lat)
    with pytest.raises(ValueError, match="dims"):
        tools.xr_idx_interp(DataArray(np.ones((2, 2, 6)), ("a", "b", "points"), {"longitude": np.arange(6.0), "latitude": np.arange(6.0)}), lon, lat)
    x, y, z = np.arange(5.0), np.arange(5.0), np.arange(5.0)
    for args, match in (((x, y[:4], z, lon, lon), "src_lon"), ((x, y, z[:3], lon, lon), "values"), ((x, y, z, lon, lat), "grid=False")):
        with pytest.raises(ValueError, match=match):
            tools.Inverse_weighted_interpolation(*args)
    for power in (0, -2, 16.5):
        with pytest.raises(ValueError, match="power"):
            tools.Inverse_weighted_interpolation(x, y, z, lon, lon, power)
    with pytest.raises(ValueError, match="one-dimensional"):
        tools.Inverse_weighted_interpolation(x, y, np.ones((2, 5)), lon, lon)


def test_the_names_are_exported_from_both_tools_modules_with_the_references_signatures():
    import inspect
    from LagrangianCoherence.LCS import tools as shim
    from lagrangiancoherence_amd import tools
    from lagrangiancoherence_amd.engine import Engine
    for name in ("Inverse_weighted_interpolation", "xr_idx_interp"):
        assert name in tools.__all__ and getattr(shim, name) is getattr(tools, name)
    p = inspect.signature(tools.Inverse_weighted_interpolation).parameters
    assert list(p) == ["x", "y", "z", "xi", "yi", "power"] and p["power"].default == 2
    p = inspect.signature(tools.xr_idx_interp).parameters
    assert list(p) == ["ds_y_for_spline", "lon", "lat", "p", "max_distance", "radius", "return_weight", "return_count"]
    assert p["p"].default == 2 and p["max_distance"].default is None and p["radius"].default == 6371000.0
    p = inspect.signature(Engine.idw_interp).parameters
    assert list(p) == ["self", "src_lon", "src_lat", "values", "tgt_lon", "tgt_lat", "grid", "power", "radius", "max_distance",
                       "return_weight", "return_count"]
    assert p["grid"].default is False and p["power"].default == 2 and p["radius"].default == 6371000.0
    assert "Inverse_weighted_interpolation" in tools.__doc__ and "IDW regridding" not in tools.__doc__
