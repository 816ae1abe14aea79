"""The great-circle distance to the nearest ridge pixel without a GPU: the numpy oracle of tests/sphere_distance.py against the
textbook haversine formula (the chord form is the definition; haversine is what a user means by it), a grid on which a tie is
guaranteed bit for bit, the entry point in the header, the bindings and the library, every refusal of include/lcs_hip.h's
contract -- each returned before the device is touched -- and the argument checks of Engine.sphere_distance and
tools.distance_to_ridges(metric='sphere'), which run before an engine exists."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from lagrangiancoherence_amd import _capi, build
from tests import distance as DT
from tests import sphere_distance as SD
from tests.labelled import DataArray

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("name", ["random-67x130-0.02", "random-130x67-0.2", "corners-67x130", "random-67x130-0.002"])
def test_the_oracle_is_the_haversine_distance(name):
    """<= 1e-7 m on a sphere of 6371 km: 16 times the largest difference seen (6.1e-9 m, relative 5.6e-14, near-antipodal
    distances of 20015 km included), the factor for another libm."""
    mask = DT.mask_of(name)
    lat, lon = SD.GRID(*mask.shape)
    dist, nearest, cost = SD.brute(mask, lat, lon)
    want = SD.haversine_min(mask, lat, lon)
    err = np.abs(dist - want).max()
    print(f"{name}: max |chord form - haversine| = {err:.3e} m, largest distance {want.max() / 1e3:.1f} km")
    assert err <= 1e-7
    fg = DT.foreground(mask)
    assert not dist[fg].any() and not cost[fg].any() and np.array_equal(nearest[fg], np.flatnonzero(fg))
    assert fg.ravel()[nearest.ravel()].all() and np.array_equal(dist, SD.dist_of(cost))


def test_a_guaranteed_tie_goes_to_the_smaller_index():
    mask, lat, lon = SD.tie_grid()
    X, Y, Z = SD.unit_vectors(lat, lon)
    col = np.arange(5) * 131 + 65
    first, second = 2 * 131, 2 * 131 + 130
    a = SD.cost_of((X[col], Y[col], Z[col]), (X[first], Y[first], Z[first]))
    b = SD.cost_of((X[col], Y[col], Z[col]), (X[second], Y[second], Z[second]))
    assert np.array_equal(a, b) and lon[65] == 0.0                 # bit-equal along the whole column
    dist, nearest, cost = SD.brute(mask, lat, lon)
    assert (nearest[:, 65] == 262).all() and np.array_equal(cost[:, 65], a)


def test_known_answers_of_the_oracle():
    lat, lon = np.array([0.0, 90.0]), np.array([0.0, 90.0, 180.0, -90.0])
    mask = np.zeros((2, 4))
    mask[0, 0] = 1
    dist, nearest, cost = SD.brute(mask, lat, lon, radius=1.0)
    assert np.allclose(dist[0], [0, np.pi / 2, np.pi, np.pi / 2], rtol=0, atol=1e-15) and np.allclose(dist[1], np.pi / 2, rtol=0, atol=1e-15)
    assert dist[0, 0] == 0 and (nearest == 0).all() and np.allclose(cost[0], [0, 2, 4, 2], rtol=0, atol=1e-15)
    dist, nearest, cost = SD.brute(mask, lat, lon, max_distance=2.0, radius=1.0)       # the antipode is beyond it
    assert np.isposinf(dist[0, 2]) and nearest[0, 2] == -1 and np.isposinf(cost[0, 2]) and np.isfinite(dist[0, 1]) and nearest[1, 3] == 0
    dist, nearest, cost = SD.brute(mask, lat, lon, max_distance=np.pi, radius=1.0)     # half the circumference: no bound
    assert np.isfinite(dist).all()
    dist, nearest, cost = SD.brute(np.zeros((2, 4)), lat, lon)
    assert np.isposinf(dist).all() and (nearest == -1).all() and np.isposinf(cost).all()


# ------------------------------------------------------------------ header, bindings, library
@pytest.fixture(scope="module")
def lib():
    build.build_library(verbose=False)
    return _capi.load()


def test_the_entry_point_is_declared_prototyped_and_exported(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lcs_hip.h")).read(), flags=re.S)
    for name in ("lc_sphere_distance", "lc_sphere_distance_work_elems"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _capi.PROTOTYPES and hasattr(lib, name), name
    assert "sphere_distance.hip" in build.SOURCES
    assert lib.lc_version() == 104 == _capi.LC_VERSION


def test_the_header_states_the_contract():
    text = " ".join(open(os.path.join(ROOT, "include", "lcs_hip.h")).read().split())
    section = text[text.index("great-circle distance to the nearest ridge pixel"):text.index("int lc_sphere_distance(")]
    for phrase in ("LCS/area_of_influence.py:231", "!= 0 and not NaN", "smallest linear index", "+inf everywhere", "nothing fused",
                   "no culling changes a result", "No kernel of this call waits for another workgroup"):
        assert phrase in section, phrase


def test_work_elems_is_pure_arithmetic(lib):
    # per plane three float64 and one int32 per pixel and ny + 1 row starts; once, two band rows per row
    f = lib.lc_sphere_distance_work_elems
    assert f(1, 1, 1) == 7 + 2 + 2 and f(67, 130, 1) == 7 * 8710 + 68 + 134 and f(67, 130, 5) == 5 * (7 * 8710 + 68) + 134
    assert f(0, 5, 1) == 0 and f(5, -1, 1) == 0 and f(5, 5, 0) == 0 and f(-2, -2, 1) == 0
    assert f(1 << 17, 1 << 14, 1) == 0 and f(46341, 46341, 1) == 0 and f(1, (1 << 31) - 1, 1) != 0      # ny nx >= 2^31
    assert f(46340, 46340, (1 << 31) - 1) == 0                                                        # past a size_t


# A context nobody dereferences and pointers nobody follows: every call below is refused by its argument checks.
_BLOCK = C.create_string_buffer(4096)
CTX = PTR = C.cast(_BLOCK, C.c_void_p)
GOOD = dict(ctx=CTX, dtype=_capi.LC_F64, ny=4, nx=6, n_members=2, radius=SD.RADIUS, max_chord2=0.0, max_distance=0.0,
            mask=PTR, cos_lat=PTR, sin_lat=PTR, cos_lon=PTR, sin_lon=PTR, dist_out=PTR, nearest_out=None, cost_out=None, work_dev=PTR)
EINVAL = _capi.LC_EINVAL
REFUSALS = [
    (dict(ctx=None), b"null context"),
    (dict(dtype=2), b"bad dtype"),
    (dict(ny=0), b"bad size"),
    (dict(nx=-1), b"bad size"),
    (dict(n_members=0), b"bad size"),
    (dict(ny=1 << 17, nx=1 << 14), b"plane too large"),
    (dict(ny=46341, nx=46341), b"plane too large"),
    (dict(ny=(1 << 31) - 1, nx=1, n_members=2), b"too many planes"),
    (dict(radius=0.0), b"bad radius"),
    (dict(radius=float("inf")), b"bad radius"),
    (dict(radius=float("nan")), b"bad radius"),
    (dict(max_chord2=float("nan")), b"bad max_chord2"),
    (dict(max_chord2=0.01, max_distance=0.0), b"bad max_distance"),
    (dict(max_chord2=0.01, max_distance=float("nan")), b"bad max_distance"),
    (dict(mask=None), b"null pointer"),
    (dict(cos_lat=None), b"null pointer"),
    (dict(sin_lon=None), b"null pointer"),
    (dict(work_dev=None), b"null pointer"),
    (dict(dist_out=None), b"no output"),
]


def _call(g):
    a = _capi.SphereDistanceArgs(struct_size=C.sizeof(_capi.SphereDistanceArgs))
    for k, v in g.items():
        if k != "ctx":
            setattr(a, k, v)
    return _capi.load().lc_sphere_distance(g["ctx"], C.byref(a))


@pytest.mark.parametrize("change, message", REFUSALS, ids=["-".join(f"{k}={v}" for k, v in c.items()) for c, _ in REFUSALS])
def test_the_call_refuses_before_it_touches_a_device(lib, change, message):
    assert _call({**GOOD, **change}) == EINVAL
    err = lib.lc_last_error()
    assert message in err and b"lc_sphere_distance" in err


def test_the_structure_matches_the_library(lib):
    size = C.sizeof(_capi.SphereDistanceArgs)
    a = _capi.SphereDistanceArgs(struct_size=size - 8)
    assert lib.lc_sphere_distance(CTX, C.byref(a)) == EINVAL
    err = lib.lc_last_error()
    assert b"struct_size %d" % (size - 8) in err and b"this library has %d" % size in err      # both numbers
    assert lib.lc_sphere_distance(CTX, None) == EINVAL and b"null argument structure" in lib.lc_last_error()
    assert lib.lc_sphere_distance(None, None) == EINVAL and b"null context" in lib.lc_last_error()
    assert lib.lc_sphere_distance(None, C.byref(a)) == EINVAL and b"null context" in lib.lc_last_error()


def test_the_kernels_never_wait_for_another_workgroup():
    """No atomic at all, no cooperative launch, no grid synchronisation, no fence, no loop without a counted end."""
    src = build._strip_comments(open(os.path.join(build.CSRC, "sphere_distance.hip")).read())
    for word in ("cooperative", "grid_group", "this_grid", "hipLaunchCooperativeKernel", "__threadfence", "atomic", "while (", "for (;;)",
                 "volatile"):
        assert word not in src, word


def test_every_function_that_evaluates_the_cost_forbids_contraction():
    """A fused multiply-add in a product of the tables or in the cost would round once where the definition rounds twice."""
    src = open(os.path.join(build.CSRC, "sphere_distance.hip")).read()
    for kernel in ("sd_scatter_kernel", "sd_band_kernel", "sd_search_kernel"):
        body = src[src.index("void " + kernel):]
        assert body[body.index("{"):].lstrip("{ \n").startswith("#pragma clang fp contract(off)"), kernel
    assert "torch" not in src and "nonzero" not in src


# ------------------------------------------------------------------ the engine's and the surface's own refusals
def test_the_engine_refuses_bad_coordinates_and_bounds_without_a_device():
    from lagrangiancoherence_amd.engine import Engine
    eng = Engine.__new__(Engine)             # no device: the checks come before anything is touched
    mask, lat, lon = np.ones((3, 4)), np.array([-10.0, 0.0, 10.0]), np.array([0.0, 1.0, 2.0, 3.0])
    for kw in (dict(lat=[-91.0, 0.0, 10.0]), dict(lat=[0.0, 90.5, 10.0]), dict(lat=[0.0, np.nan, 1.0]), dict(lon=[0.0, np.inf, 1.0, 2.0]),
               dict(lat=lat[:2]), dict(lon=lon[:3]), dict(lat=lat[None]), dict(radius=0.0), dict(radius=-1.0), dict(radius=np.inf),
               dict(max_distance=0.0), dict(max_distance=-5.0), dict(max_distance=float("nan"))):
        with pytest.raises(ValueError):
            eng.sphere_distance(mask, **{"lat": lat, "lon": lon, **kw})
    with pytest.raises(ValueError):
        eng.sphere_distance(np.ones((2, 2, 3, 4)), lat, lon)


def test_the_host_tables_are_numpys_and_the_bound_is_the_squared_chord():
    from lagrangiancoherence_amd.engine import Engine
    lat, lon = SD.GRID(67, 130)
    cl, sl, cx, sx, radius, chord2, bound = Engine.sphere_tables(lat, lon, max_distance=250e3)
    for got, want in zip((cl, sl, cx, sx), SD.tables(lat, lon)):
        assert got.dtype == np.float64 and np.array_equal(got, want)
    assert radius == SD.RADIUS and chord2 == SD.chord2_of(250e3) and bound == 250e3
    assert Engine.sphere_tables(lat, lon)[5:] == (0.0, 0.0)
    assert Engine.sphere_tables(lat, lon, 2.0, max_distance=2.0 * np.pi)[5:] == (0.0, 0.0)          # >= pi radius: unbounded
    assert Engine.sphere_tables(lat, lon, 2.0, max_distance=6.0)[5] == SD.chord2_of(6.0, 2.0) > 0


def test_distance_to_ridges_checks_its_arguments_before_it_creates_an_engine(monkeypatch):
    from lagrangiancoherence_amd import tools

    def no_engine():
        raise AssertionError("an engine was asked for")
    monkeypatch.setattr(tools, "get_engine", no_engine)
    ridges = DataArray(np.ones((3, 4)), ("latitude", "longitude"), {"latitude": np.array([-10.0, 0.0, 10.0]), "longitude": np.arange(4.0)})
    with pytest.raises(ValueError, match="sampling"):
        tools.distance_to_ridges(ridges, metric='sphere', sampling=2.0)
    with pytest.raises(ValueError, match="metric"):
        tools.distance_to_ridges(ridges, metric='km')
    with pytest.raises(ValueError, match="max_distance"):
        tools.distance_to_ridges(ridges, metric='sphere', max_distance=0)
    with pytest.raises(ValueError, match="radius"):
        tools.distance_to_ridges(ridges, metric='sphere', radius=-1.0)
    bad = DataArray(np.ones((3, 4)), ("latitude", "longitude"), {"latitude": np.array([-100.0, 0.0, 10.0]), "longitude": np.arange(4.0)})
    with pytest.raises(ValueError, match="lat"):
        tools.distance_to_ridges(bad, metric='sphere')


def test_the_signature_keeps_its_order_and_gains_two_keywords():
    import inspect
    from LagrangianCoherence.LCS import tools as shim
    from lagrangiancoherence_amd import tools
    p = inspect.signature(tools.distance_to_ridges).parameters
    assert list(p) == ["ridges", "cyclic", "sampling", "max_distance", "return_labels", "connectivity", "metric", "radius"]
    assert p["metric"].default == "index" and p["radius"].default == 6371000.0
    assert shim.distance_to_ridges is tools.distance_to_ridges
