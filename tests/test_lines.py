"""Ridge lines without a GPU: the pixel walker of tests/lines.py against its own invariants and against answers read off
hand-made masks, the refusals tools.ridge_lines and the C ABI make before any device is touched, and the build list."""
import ctypes as C

import numpy as np
import pytest

from lagrangiancoherence_amd import _capi, build
from tests import lines as L
from tests import skeleton as SK
from tests.labelled import DataArray

RANDOM = [(d, cyclic) for d in (0.02, 0.1, 0.3, 0.6) for cyclic in (False, True)]


def _trace(mask, cyclic, **kw):
    lat, lon = L.grid(*mask.shape)
    return L.trace(mask, cyclic, lat=lat, lon=lon, **kw)


@pytest.mark.parametrize("name", sorted(L.CASES))
def test_walker_invariants_on_the_hand_made_masks(name):
    mask, cyclic = L.CASES[name]
    L.invariants(_trace(mask, cyclic))


@pytest.mark.parametrize("density,cyclic", RANDOM)
def test_walker_invariants_on_random_masks(density, cyclic):
    L.invariants(_trace(L.random_mask(21, 37, density), cyclic))


@pytest.mark.parametrize("method", SK.METHODS)
def test_walker_invariants_on_skeletons(method):
    """Thinned smooth fields are what the walker is for: nearly every pixel has degree 2, a few junctions have degree 3."""
    thin, _ = SK.thin(SK._smooth(60, 90), SK.table(method))
    t = _trace(thin.astype(np.float64), False)
    L.invariants(t)
    degree = L.POPCOUNT[t["links"]][thin != 0]
    assert degree.max() <= 4 and (degree == 2).mean() > 0.8
    stack = np.stack([thin.astype(np.float64), L.random_mask(60, 90, 0.1)])
    lat, lon = L.grid(60, 90)
    L.invariants(L.trace_planes(stack, True, lat=lat, lon=lon))


@pytest.mark.parametrize("name", sorted(L.EXPECT))
def test_hand_made_answers(name):
    mask, cyclic = L.CASES[name]
    t = _trace(mask, cyclic)
    got = [tuple(int(t[k][i]) for k in ("count", "closed", "first", "last", "n_edge", "n_diag")) for i in range(t["count"].size)]
    assert got == L.EXPECT[name]


def test_hand_made_details():
    t = _trace(*L.CASES["full-5x7"])
    assert t["count"].size == 54 and int(L.POPCOUNT[t["links"]].sum()) // 2 == 58       # the walker's numbers, not a formula's
    t = _trace(*L.CASES["lollipop"])
    assert t["closed"].tolist() == [0, 0] and t["first"][0] == t["last"][0] == 12 and t["first_degree"].tolist() == [3, 3]
    assert t["pixel"][:9].tolist() == [12, 13, 8, 3, 2, 1, 6, 11, 12]
    t = _trace(*L.CASES["two-junctions"])
    assert (t["count"] == 2).all() and t["count"].size == 5
    t = _trace(*L.CASES["values"])          # NaN and -0.0 are background, negative values foreground
    assert t["links"].astype(bool).sum() == 2 and t["first_degree"].tolist() == [0, 1]
    for name in ("serpentine", "spiral"):
        t = _trace(*L.CASES[name])
        assert t["count"].tolist() == [1121] and t["closed"].tolist() == [0]          # more than 1024 points: more than 10 rounds
    t = _trace(*L.CASES["block-2x2"])
    assert t["pixel"].tolist() == [5, 6, 10, 9] and t["first_degree"].tolist() == [2] == t["last_degree"].tolist()
    t = _trace(*L.CASES["diagonal"], metric="index", sampling=(2.0, 3.0))
    assert t["length"][0] == 4 * np.sqrt(13.0) and t["distance"].tolist() == [k * np.sqrt(13.0) for k in range(5)]
    t = _trace(*L.CASES["row-cyclic"])
    assert np.array_equal(t["distance"], np.concatenate([[0.0], np.cumsum(t["step"][1:])])) and t["length"][0] > t["distance"][-1]


def test_sphere_lengths_are_great_circle_arcs():
    """A meridian line: its length is radius times the latitude it spans, to a few ulp per link."""
    lat, lon = np.linspace(-10.0, 10.0, 9), np.linspace(0.0, 8.0, 5)
    mask = np.zeros((9, 5))
    mask[:, 2] = 1
    t = L.trace(mask, False, lat=lat, lon=lon)
    assert t["count"].tolist() == [9] and abs(t["length"][0] / (L.RADIUS * np.radians(20.0)) - 1) < 1e-12


def _da(mask, lat=None, lon=None, dims=("latitude", "longitude")):
    ny, nx = mask.shape[-2:]
    g = L.grid(ny, nx)
    return DataArray(mask, dims, {"latitude": g[0] if lat is None else lat, "longitude": g[1] if lon is None else lon})


def test_ridge_lines_refuses_on_the_host():
    """Every refusal is a ValueError raised before an engine exists (without a GPU, creating one is a RuntimeError)."""
    from lagrangiancoherence_amd import tools
    from LagrangianCoherence.LCS.tools import ridge_lines
    assert ridge_lines is tools.ridge_lines and "ridge_lines" in tools.__all__
    mask = L.CASES["T"][0]
    with pytest.raises(ValueError, match="metric"):
        ridge_lines(_da(mask), metric="euclid")
    with pytest.raises(ValueError, match="dims"):
        ridge_lines(DataArray(mask[None, None], ("a", "b", "latitude", "longitude"), {}))
    with pytest.raises(ValueError, match="3 columns"):
        ridge_lines(_da(np.ones((4, 2))), cyclic=True, metric="index")
    with pytest.raises(ValueError, match="radius"):
        ridge_lines(_da(mask), radius=-1.0)
    with pytest.raises(ValueError, match="lat"):
        ridge_lines(_da(mask, lat=np.linspace(-100, 100, mask.shape[0])))
    with pytest.raises(ValueError, match="dims"):
        ridge_lines(_da(mask), intensity=DataArray(mask[None], ("time", "latitude", "longitude"), {}))
    with pytest.raises(ValueError, match="coordinates"):
        ridge_lines(_da(mask), intensity=_da(mask, lon=np.arange(mask.shape[1]) + 0.5))


def test_engine_line_options_refuse_on_the_host():
    from lagrangiancoherence_amd.engine import Engine
    lat, lon = L.grid(4, 6)
    check = Engine.checked_line_options
    assert check((4, 6), False, "index", None, None, 1.0, (2, 3))[2:] == (2.0, 3.0)
    assert len(check((2, 4, 6), True, "sphere", lat, lon, 10.0, None)[0]) == 4
    for bad in (dict(shape=(6,)), dict(shape=(0, 6)), dict(metric="x"), dict(cyclic=True, shape=(4, 2), metric="index"),
                dict(sampling=1.0), dict(lat=None), dict(lat=lat[:3]), dict(radius=0.0), dict(metric="index", sampling=-1.0),
                dict(metric="index", sampling=(1, 2, 3)), dict(shape=(2 ** 14, 2 ** 14), metric="index")):
        kw = dict(shape=(4, 6), cyclic=False, metric="sphere", lat=lat, lon=lon, radius=1.0, sampling=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            check(**kw)


@pytest.fixture(scope="module")
def lib():
    build.build_library(verbose=False)
    return _capi.load()


def test_the_build_list_holds_the_kernels_and_the_library_exports_them(lib):
    assert "lines.hip" in build.SOURCES and build.ARCH == "gfx950"
    assert all(hasattr(lib, name) for name in ("lc_trace_lines", "lc_lines_work_elems", "lc_line_link_lengths"))
    assert lib.lc_version() == 104


def test_work_elems_is_linear_in_pixels(lib):
    """96 bytes per pixel (two states of 16 bytes and a float64, in two buffers) and 512 bytes, in int32 elements."""
    assert lib.lc_lines_work_elems(720, 1440, 8) == 128 + 24 * 720 * 1440 * 8
    assert lib.lc_lines_work_elems(0, 4, 1) == 0 and lib.lc_lines_work_elems(2 ** 14, 2 ** 14, 1) == 0


def _args(**kw):
    a = _capi.LinesArgs(struct_size=C.sizeof(_capi.LinesArgs))
    a.dtype, a.ny, a.nx, a.n_members, a.radius = _capi.LC_F64, 4, 6, 1, 1.0
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_the_c_abi_refuses_before_any_device(lib):
    """The order of the checks: with a null context every call below ends at 'null context'; a context cannot be made here, so
    the later refusals are exercised through a pointer that is never dereferenced before they fire."""
    assert lib.lc_trace_lines(None, C.byref(_args())) == _capi.LC_EINVAL and b"null context" in lib.lc_last_error()
    fake = C.c_void_p(8)          # a context no check reads before the argument checks are through
    assert lib.lc_trace_lines(fake, None) == _capi.LC_EINVAL and b"null argument" in lib.lc_last_error()
    for kw, word in ((dict(struct_size=8), b"struct_size"), (dict(dtype=7), b"dtype"), (dict(ny=0), b"bad size"),
                     (dict(n_members=-1), b"bad size"), (dict(ny=2 ** 14, nx=2 ** 14), b"too large"),
                     (dict(nx=2, cyclic_x=1), b"nx >= 3"), (dict(cos_lat=8), b"come together"), (dict(), b"null pointer")):
        assert lib.lc_trace_lines(fake, C.byref(_args(**kw))) == _capi.LC_EINVAL, kw
        assert word in lib.lc_last_error(), (kw, lib.lc_last_error())
    b = _capi.LinkLengthsArgs(struct_size=C.sizeof(_capi.LinkLengthsArgs))
    assert lib.lc_line_link_lengths(None, C.byref(b)) == _capi.LC_EINVAL and b"null context" in lib.lc_last_error()
    for kw, word in ((dict(struct_size=4), b"struct_size"), (dict(ny=0, nx=3), b"bad size"), (dict(ny=3, nx=3, n_pairs=-1), b"n_pairs"),
                     (dict(ny=3, nx=3, n_pairs=1, radius=0.0), b"radius"), (dict(ny=3, nx=3, n_pairs=1, radius=1.0), b"null pointer")):
        b = _capi.LinkLengthsArgs(struct_size=C.sizeof(_capi.LinkLengthsArgs))
        for k, v in kw.items():
            setattr(b, k, v)
        assert lib.lc_line_link_lengths(fake, C.byref(b)) == _capi.LC_EINVAL and word in lib.lc_last_error(), kw
