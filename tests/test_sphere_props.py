"""Host-side checks of the spherical ridge properties (no GPU): Engine.sphere_cell_tables against the restatement of
tests/sphere_props.py and against closed values, every refusal of the tables and of the two public functions -- raised before
an engine exists --, the new C entry point's refusals before it touches a device, and the restatement's own closed cases."""
import ctypes as C
import inspect
import math

import numpy as np
import pytest

from lagrangiancoherence_amd import _capi, build
from lagrangiancoherence_amd.engine import Engine
from tests import sphere_props as SP
from tests.labelled import DataArray

EPS = 2.0 ** -53


@pytest.fixture(scope="module")
def lib():
    build.build_library(verbose=False)
    return _capi.load()


# ------------------------------------------------------------------ the cell tables
@pytest.mark.parametrize("ny, nx", [(7, 8), (19, 36), (180, 360), (720, 1440)])
def test_the_weights_of_a_global_grid_sum_to_four_pi(ny, nx):
    """Cell-centred global grid: the band edges telescope from -90 to 90 and the columns close the circle.  Bound: every row
    weight is a difference of two sines of magnitude <= 1, each within an ulp of its edge's (<= 2 u), rounded once more (u):
    3 u per row, relative to the total 2 of the rows; the columns are one rounded product each, a relative u; plus the product."""
    lat = -90.0 + 180.0 * (np.arange(ny) + 0.5) / ny
    lon = -180.0 + 360.0 * np.arange(nx) / nx
    rw, cw = Engine.sphere_cell_tables(lat, lon, cyclic=True)
    assert rw.shape == (ny,) and cw.shape == (nx,) and (rw > 0).all() and (cw > 0).all()
    total = math.fsum(rw) * math.fsum(cw)
    err, bound = abs(total - 4 * math.pi), (3 * ny / 2 + 4) * EPS * 4 * math.pi
    print(f"{ny}x{nx}: 4 pi off by {err / (4 * math.pi * 2 * EPS):.2f} ulp, bound {bound / (4 * math.pi * 2 * EPS):.0f} ulp")
    assert err <= bound
    if ny <= 19:
        assert err <= 8 * 2 * EPS * 4 * math.pi          # a few ulp where there are few rows
    assert abs(math.fsum(cw) - 2 * math.pi) <= 4 * EPS * 2 * math.pi


def test_the_outer_bands_are_clipped_at_the_poles():
    lat, lon = np.linspace(-90.0, 90.0, 19), np.arange(0.0, 360.0, 10.0)
    rw, cw = Engine.sphere_cell_tables(lat, lon, cyclic=True)
    # the polar caps: from the pole to 5 degrees from it, not from 5 degrees beyond it
    assert rw[0] == np.sin(-85.0 * np.pi / 180) - np.sin(-90.0 * np.pi / 180) and rw[-1] == np.sin(90.0 * np.pi / 180) - np.sin(85.0 * np.pi / 180)
    assert abs(rw[0] - (1 - math.cos(math.radians(5.0)))) <= 4 * EPS and abs(math.fsum(rw) - 2.0) <= 19 * 3 * EPS
    assert abs(math.fsum(rw) * math.fsum(cw) - 4 * math.pi) <= (3 * 19 / 2 + 4) * EPS * 4 * math.pi
    # an axis that ends short of the poles is not clipped: the outer edges lie half a spacing out
    rw, _ = Engine.sphere_cell_tables(np.array([-20.0, -10.0, 10.0]), lon)
    edges = np.array([-25.0, -15.0, 0.0, 20.0])
    assert np.array_equal(rw, np.diff(np.sin(edges * np.pi / 180)))


def test_non_cyclic_and_cyclic_columns():
    lat = np.array([0.0, 1.0])
    lon = np.array([0.0, 1.0, 3.0, 7.0])
    _, cw = Engine.sphere_cell_tables(lat, lon)
    assert np.array_equal(cw, np.array([1.0, 1.5, 3.0, 4.0]) * np.pi / 180)          # edges -0.5, 0.5, 2, 5, 9
    _, cw = Engine.sphere_cell_tables(lat, lon, cyclic=True)                      # the gap 0 + 360 - 7 = 353 is shared
    assert np.array_equal(cw, np.array([177.0, 1.5, 3.0, 178.5]) * np.pi / 180)      # edges -176.5, 0.5, 2, 5, 183.5
    assert abs(math.fsum(cw) - 2 * math.pi) <= 4 * EPS * 2 * math.pi


@pytest.mark.parametrize("variant", ["uniform", "gauss", "global"])
@pytest.mark.parametrize("cyclic", [False, True])
def test_the_engines_tables_are_the_restatements_bit_for_bit(variant, cyclic):
    """What makes the device's terms the restatement's terms: the six tables are equal, not close."""
    lat, lon = SP.coordinates((33, 65), variant)
    cl, sl, rw, cx, sx, cw = SP.tables(lat, lon, cyclic)
    got = Engine.sphere_tables(lat, lon)
    for a, b in zip((cl, sl, cx, sx), got[:4]):
        assert np.array_equal(a, b)
    grw, gcw = Engine.sphere_cell_tables(lat, lon, cyclic)
    assert np.array_equal(rw, grw) and np.array_equal(cw, gcw) and grw.dtype == gcw.dtype == np.float64
    assert (variant == "global") == (lat[0] - (lat[1] - lat[0]) / 2 < -90.0)       # only that variant is clipped


BAD_TABLES = [
    (dict(lat=[0.0], lon=[0.0, 1.0]), "at least two"),
    (dict(lat=[0.0, 1.0], lon=[5.0]), "at least two"),
    (dict(lat=[[0.0, 1.0]], lon=[0.0, 1.0]), "one-dimensional"),
    (dict(lat=[0.0, 1.0, 1.0], lon=[0.0, 1.0]), "strictly ascending"),
    (dict(lat=[0.0, 1.0], lon=[0.0, 2.0, 1.0]), "strictly ascending"),
    (dict(lat=[2.0, 1.0], lon=[0.0, 1.0]), "strictly ascending"),
    (dict(lat=[0.0, np.nan], lon=[0.0, 1.0]), "finite"),
    (dict(lat=[0.0, 1.0], lon=[0.0, np.inf]), "finite"),
    (dict(lat=[-90.5, 0.0], lon=[0.0, 1.0]), r"within \[-90, 90\]"),
    (dict(lat=[0.0, 91.0], lon=[0.0, 1.0]), r"within \[-90, 90\]"),
    (dict(lat=[0.0, 1.0], lon=[0.0, 180.0, 360.0], cyclic=True), "gap"),
    (dict(lat=[0.0, 1.0], lon=[-10.0, 180.0, 400.0], cyclic=True), "gap"),
]


@pytest.mark.parametrize("kw, message", BAD_TABLES, ids=[f"{i}-{m.split()[0]}" for i, (_, m) in enumerate(BAD_TABLES)])
def test_sphere_cell_tables_refuses(kw, message):
    with pytest.raises(ValueError, match=message):
        Engine.sphere_cell_tables(**kw)
    if "cyclic" in kw:          # the same axis is fine when it need not close
        Engine.sphere_cell_tables(kw["lat"], kw["lon"])


# ------------------------------------------------------------------ the public surface, without a device
def _arrays(ny=5, nx=6, lead=None):
    lat, lon = np.linspace(-20.0, 20.0, ny), np.linspace(0.0, 50.0, nx)
    dims, coords, shape = ("latitude", "longitude"), {"latitude": lat, "longitude": lon}, (ny, nx)
    if lead:
        dims, coords, shape = (lead, *dims), {lead: np.arange(2), **coords}, (2, ny, nx)
    return DataArray(np.ones(shape), dims, coords), DataArray(np.full(shape, 2.0), dims, coords)


def test_the_public_functions_check_their_arguments_before_they_create_an_engine(monkeypatch):
    from lagrangiancoherence_amd import tools

    def no_engine():
        raise AssertionError("an engine was asked for")
    monkeypatch.setattr(tools, "get_engine", no_engine)
    ridges, ftle = _arrays()
    for call in (lambda **kw: tools.ridge_properties(ridges, ftle, **kw),
                 lambda **kw: tools.filter_ridges(ridges, ftle, ["area"], [1.0], **kw)):
        with pytest.raises(ValueError, match="metric"):
            call(metric="km")
        with pytest.raises(ValueError, match="radius"):
            call(metric="sphere", radius=0.0)
    with pytest.raises(ValueError, match="criterion"):
        tools.filter_ridges(ridges, ftle, ["perimeter"], [1.0], metric="sphere")
    with pytest.raises(ValueError, match="criterion"):
        tools.filter_ridges(ridges, ftle, ["perimeter"], [1.0])
    with pytest.raises(ValueError, match="connectivity"):
        tools.ridge_properties(ridges, connectivity=3)
    # coordinates the sphere cannot take: a repeated latitude, a latitude beyond the pole, an axis that does not close
    for bad, cyclic, message in (({"latitude": np.array([-20.0, -10.0, -10.0, 10.0, 20.0])}, False, "strictly ascending"),
                                 ({"latitude": np.linspace(-95.0, 20.0, 5)}, False, "within"),
                                 ({"longitude": np.linspace(0.0, 360.0, 6)}, True, "gap")):
        coords = {"latitude": ridges.coords["latitude"], "longitude": ridges.coords["longitude"], **bad}
        r, f = (DataArray(a.values, a.dims, coords) for a in (ridges, ftle))
        with pytest.raises(ValueError, match=message):
            tools.ridge_properties(r, f, cyclic=cyclic)
        with pytest.raises(ValueError, match=message):
            tools.filter_ridges(r, f, ["area"], [1.0], cyclic=cyclic, metric="sphere")
    # an intensity on other dims or coordinates
    stack, _ = _arrays(lead="time")
    with pytest.raises(ValueError, match="dims"):
        tools.ridge_properties(ridges, stack)
    other = DataArray(ftle.values, ftle.dims, {"latitude": ftle.coords["latitude"] + 1.0, "longitude": ftle.coords["longitude"]})
    with pytest.raises(ValueError, match="coordinates"):
        tools.ridge_properties(ridges, other)
    with pytest.raises(ValueError, match="coordinates"):
        tools.filter_ridges(ridges, other, ["area"], [1.0], metric="sphere")
    four = DataArray(np.ones((1, 2, 5, 6)), ("member", "time", "latitude", "longitude"),
                     {"member": [0], "time": [0, 1], "latitude": ridges.coords["latitude"], "longitude": ridges.coords["longitude"]})
    with pytest.raises(ValueError, match="at most one more"):
        tools.ridge_properties(four)
    # labels: whole numbers up to 2^31 - 1
    for bad, message in ((1.5, "whole number"), (2.0 ** 31, "at most")):
        lab = ridges.copy()
        lab.values[2, 3] = bad
        with pytest.raises(ValueError, match=message):
            tools.ridge_properties(lab, labelled=True)
    # ... and what is NOT refused reaches the engine: negative values, NaN and 0 are background
    lab = ridges.copy()
    lab.values[0, :3] = [-1.5, np.nan, 0.0]
    with pytest.raises(AssertionError, match="an engine was asked for"):
        tools.ridge_properties(lab, labelled=True)


def test_signatures_defaults_and_exports():
    from LagrangianCoherence.LCS import tools as shim
    from lagrangiancoherence_amd import tools
    assert shim.ridge_properties is tools.ridge_properties and "ridge_properties" in tools.__all__
    p = inspect.signature(tools.ridge_properties).parameters
    assert list(p) == ["ridges", "intensity", "connectivity", "cyclic", "metric", "radius", "labelled"]
    assert (p["intensity"].default, p["connectivity"].default, p["cyclic"].default, p["metric"].default, p["radius"].default,
            p["labelled"].default) == (None, 2, False, "sphere", 6371000.0, False)
    p = inspect.signature(tools.filter_ridges).parameters
    assert list(p) == ["ridges", "ftle", "criteria", "thresholds", "verbose", "connectivity", "cyclic", "fill", "metric", "radius"]
    assert p["metric"].default == "index" and p["radius"].default == 6371000.0
    p = inspect.signature(Engine.filter_components).parameters
    assert list(p)[-4:] == ["metric", "lat", "lon", "radius"] and p["metric"].default == "index" and p["lat"].default is None
    assert list(inspect.signature(Engine.component_sphere_props).parameters) == [
        "self", "labels", "counts", "lat", "lon", "intensity", "cyclic", "radius", "n_max", "return_sums"]
    assert "ridge_properties" in tools.__doc__ and "chord" in tools.ridge_properties.__doc__.lower()
    assert "run to run" in tools.ridge_properties.__doc__ and "run to run" in tools.filter_ridges.__doc__


# ------------------------------------------------------------------ the C entry point
def _args(**kw):
    a = _capi.ComponentSphereSumsArgs(struct_size=C.sizeof(_capi.ComponentSphereSumsArgs))
    a.dtype, a.ny, a.nx, a.n_members, a.n_max, a.radius = _capi.LC_F64, 4, 4, 1, 4, 1.0
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_the_entry_point_validates_before_touching_a_device(lib):
    """The pattern of test_new_entry_points_validate_before_touching_a_device: a null context and null arguments."""
    assert lib.lc_component_sphere_sums(None, C.byref(_args())) == _capi.LC_EINVAL
    assert b"lc_component_sphere_sums: null context" in lib.lc_last_error()
    assert lib.lc_component_sphere_sums(None, None) == _capi.LC_EINVAL
    assert _capi.LC_VERSION == 104 == lib.lc_version()
    with pytest.raises(ValueError):
        _capi.check(lib.lc_component_sphere_sums(None, None), lib)


@pytest.mark.parametrize("change, message", [
    (dict(struct_size=C.sizeof(_capi.ComponentSphereSumsArgs) - 8), b"struct_size"),
    (dict(struct_size=0), b"struct_size"),
    (dict(ny=0), b"bad size"), (dict(nx=-1), b"bad size"), (dict(n_members=0), b"bad size"),
    (dict(dtype=7), b"bad dtype"),
    (dict(n_max=0), b"bad capacity"),
    (dict(radius=0.0), b"bad radius"), (dict(radius=float("inf")), b"bad radius"), (dict(radius=float("nan")), b"bad radius"),
    (dict(), b"null pointer"),
], ids=["size-8", "size0", "ny0", "nx-1", "members0", "dtype7", "nmax0", "radius0", "radiusinf", "radiusnan", "pointers"])
def test_the_entry_point_refuses_bad_arguments(lib, change, message):
    """With a stand-in for the context (never dereferenced before the last refusal, which is the null-pointer check: every
    buffer of these arguments is null), so that the refusals behind the context check are reached without a device."""
    ctx = C.create_string_buffer(4096)
    a = _args(**change)
    assert lib.lc_component_sphere_sums(ctx, C.byref(a)) == _capi.LC_EINVAL
    err = lib.lc_last_error()
    assert message in err and b"lc_component_sphere_sums" in err
    assert lib.lc_component_sphere_sums(ctx, None) == _capi.LC_EINVAL and b"null argument structure" in lib.lc_last_error()


# ------------------------------------------------------------------ the restatement on closed cases
def test_the_restatement_on_lines_it_can_be_checked_by_hand():
    """A zonal line of L pixels at latitude phi on a grid of spacing h (radians) is an arc of a small circle of radius cos phi:
    for a short one the major axis is 4 R sqrt((L^2 - 1) / 12) h cos phi up to the chord's curvature, O((L h)^2) relative."""
    ny, nx, L, R = 9, 1440, 21, 6371000.0
    lat, lon = np.array([-1.0, -0.75, -0.5, -0.25, 0.0, 59.75, 60.0, 60.25, 60.5]), -180.0 + 0.25 * np.arange(nx)
    lab = np.zeros((ny, nx), np.int32)
    lab[4, 100:100 + L] = 1          # the equator
    lab[6, 300:300 + L] = 2          # 60 degrees
    lab[1:4, 700] = 3                # meridional
    s = SP.sums(lab, 3, lat, lon, np.ones((ny, nx)), cyclic=True)
    p = SP.props(s, lat, lon, R)
    h = math.radians(0.25)
    flat = 4 * R * math.sqrt((L * L - 1) / 12) * h
    assert abs(p["major_axis_length"][0] / flat - 1) < (L * h) ** 2 and abs(p["major_axis_length"][1] / (flat * 0.5) - 1) < (L * h) ** 2
    # an axis has no sign: -90 + 1e-15 and 90 are the same orientation
    assert (SP.angle_difference(p["orientation"], [0.0, 0.0, 90.0], 180.0) < 1e-9).all() and np.allclose(
        p["minor_axis_length"][:2], 0.0, atol=R * (L * h) ** 2)          # the arc's own sagitta: 0.149 R cos phi (L h)^2
    # the mean of the arc's nodes lies inside its small circle: the direction is polewards of 60 by sin(phi) cos(phi) (L h)^2 / 24 radians
    assert np.allclose(p["centroid_latitude"], [0.0, 60.0 + math.degrees(math.sin(math.radians(120.0)) / 2 * (L * h) ** 2 / 24), -0.5], atol=1e-4)
    assert np.allclose(p["centroid_longitude"], [lon[110], lon[310], lon[700]], atol=1e-9)
    # the area of L cells: R^2 h (sin of the band's edges) L -- the equator's band reaches half way to the next latitude, 59.75;
    # the mean of a constant is the constant
    assert np.allclose(p["area"][0], R * R * h * (math.sin(math.radians(29.875)) + math.sin(h / 2)) * L, rtol=1e-12) and np.allclose(p["mean_intensity"], 1.0, rtol=1e-14)
    assert np.allclose(p["total_intensity"], p["area"], rtol=1e-14)
