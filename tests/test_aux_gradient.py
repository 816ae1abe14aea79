"""The auxiliary-grid gradient on the CPU: the numpy restatement of csrc/aux_gradient.hip against its longdouble form and an
exact value, ``Engine.aux_seeds``, the argument checks of ``lc_aux_gradient`` before any device call, and the refusals of
``LCS(aux_grid=)``.  No GPU."""
import ctypes as C
import inspect

import numpy as np
import pytest

from lagrangiancoherence_amd import _capi, build, dropin
from lagrangiancoherence_amd.engine import Engine
from tests import aux_gradient as AG
from tests.test_capi_symbols import declared_symbols

K = np.pi / 180


@pytest.fixture(scope="module")
def lib():
    build.build_library(verbose=False)
    return _capi.load()


def _rel(a, b):
    return float(np.max(np.abs((np.asarray(a, dtype=np.longdouble) - b) / b)))


# ------------------------------------------------------------------ the formulas
@pytest.mark.parametrize("delta", [0.01, 0.25])
def test_float64_restatement_against_longdouble(delta):
    """About 20 rounded operations at 1.1e-16 each between the inputs and s1, s2: 1e-13 leaves a margin of about 50."""
    assert np.finfo(np.longdouble).eps < 2e-19, "np.longdouble is not an extended type here: no reference to judge float64 by"
    lat, lon, box = AG.global_grid(37, 64)
    seeds = Engine.aux_seeds(lat, lon, delta, box, np.float64)
    assert seeds.row_valid.all() and seeds.col_valid.all()
    p = AG.planes_of_map(AG.smooth_map, lat, lon, seeds, np.float64)
    got = AG.restatement(p, lat, seeds.sep_lat, seeds.sep_lon, np.float64)
    ref = AG.restatement(p, lat, seeds.sep_lat, seeds.sep_lon, np.longdouble)
    e1, e2 = _rel(got["s1"], ref["s1"]), _rel(got["s2"], ref["s2"])
    print(f"delta {delta}: float64 restatement vs longdouble: s1 {e1:.2e} s2 {e2:.2e}")
    assert e1 <= 1e-13 and e2 <= 1e-13
    # the naive Cartesian difference is harmless in float64 (1e-12 to 1e-10): it is float32 the half-angle form is for
    nv = AG.naive(p, lat, seeds.sep_lat, seeds.sep_lon, np.float64)
    assert _rel(nv["s1"], ref["s1"]) < 1e-9


@pytest.mark.parametrize("delta", [0.01, 0.25])
@pytest.mark.parametrize("T", [np.float64, np.longdouble])
def test_identity_map_is_sin_over_its_argument(delta, T):
    """Two points d degrees either side of a seed lie 2 R sin(k d) apart: both stretch factors are sin(k d) / (k d)."""
    lat, lon, box = AG.global_grid(37, 64)
    seeds = Engine.aux_seeds(lat, lon, delta, box, np.float64)
    p = AG.planes_of_map(AG.identity_map, lat, lon, seeds, np.float64)
    got = AG.restatement(p, lat, seeds.sep_lat, seeds.sep_lon, T)
    want = np.sin(K * delta) / (K * delta)
    assert np.abs(got["s1"] - want).max() <= 1e-13 and np.abs(got["s2"] - want).max() <= 1e-13
    assert np.abs(got["sigma"] - want).max() <= 1e-13


@pytest.mark.parametrize("lat_edge", [70.0, 89.75])
def test_float32_half_angle_form_does_not_cancel_and_the_naive_form_does(lat_edge):
    """The bound: some 20 rounded operations at float32's 6e-8, plus the rounding of the argument x of cos(k lat) in the metric
    and of sin a in the chord, which the function amplifies by x tan x towards the poles (3.4 at 70 degrees, 360 at 89.75: the
    reference's formulation in float32, not a cancellation of the difference).  The naive difference loses 3 to 4 digits."""
    lat, lon, box = AG.global_grid(37, 64, np.float32, lat_edge)
    seeds = Engine.aux_seeds(lat, lon, 0.01, box, np.float32)
    p = AG.planes_of_map(AG.smooth_map, lat, lon, seeds, np.float32)
    ref = AG.restatement(p, lat, seeds.sep_lat, seeds.sep_lon, np.longdouble)
    half = _rel(AG.restatement(p, lat, seeds.sep_lat, seeds.sep_lon, np.float32)["s1"], ref["s1"])
    naive = _rel(AG.naive(p, lat, seeds.sep_lat, seeds.sep_lon, np.float32)["s1"], ref["s1"])
    x = K * lat_edge
    bound = 6e-8 * (20 + 2 * x * np.tan(x))
    print(f"float32, delta 0.01, rows to {lat_edge}: half-angle {half:.2e} (bound {bound:.2e}), naive {naive:.2e}")
    assert half <= bound and naive > 1e-4 and naive > 10 * bound


# ------------------------------------------------------------------ Engine.aux_seeds
def test_aux_seeds_clips_marks_and_measures_the_rounded_arrays():
    lat = np.array([-90.0, -89.9, -45.0, 0.0, 89.9, 90.0], dtype=np.float32)
    lon = np.array([-180.0, -179.9, 0.3, 179.7, 179.95], dtype=np.float32)
    box = (-90.0, 90.0, -180.0, 179.95)
    d = 0.05
    s = Engine.aux_seeds(lat, lon, d, box, np.float32)
    for a in (s.lat_n, s.lat_s, s.lon_e, s.lon_w, s.sep_lat, s.sep_lon):
        assert a.dtype == np.float32
    f = np.float32
    # shifted in float32, then clipped into the box: no seed starts outside the field
    assert np.array_equal(s.lat_n, np.clip(lat + f(d), f(-90), f(90))) and np.array_equal(s.lat_s, np.clip(lat - f(d), f(-90), f(90)))
    assert np.array_equal(s.lon_e, np.clip(lon + f(d), f(-180), f(179.95))) and np.array_equal(s.lon_w, np.clip(lon - f(d), f(-180), f(179.95)))
    assert s.lat_s.min() >= f(-90) and s.lat_n.max() <= f(90) and s.lon_w.min() >= f(-180) and s.lon_e.max() <= f(179.95)
    # valid iff both shifted coordinates lie inside the box
    assert s.row_valid.tolist() == [False, True, True, True, True, False]
    assert s.col_valid.tolist() == [False, True, True, True, False]
    # NaN exactly on the invalid rows / columns; elsewhere the difference of the rounded arrays, exactly
    assert np.array_equal(np.isnan(s.sep_lat), ~s.row_valid) and np.array_equal(np.isnan(s.sep_lon), ~s.col_valid)
    assert np.array_equal(s.sep_lat[s.row_valid], (s.lat_n - s.lat_s)[s.row_valid])
    assert np.array_equal(s.sep_lon[s.col_valid], (s.lon_e - s.lon_w)[s.col_valid])
    # ... which is not 2 d in float32: the point of handing the separations to the kernel
    assert np.any(s.sep_lon[s.col_valid] != f(2 * d)) and np.abs(s.sep_lon[s.col_valid] / f(2 * d) - 1).max() < 1e-3
    # a cyclic (global) field is no exception: the seam columns are invalid
    g = Engine.aux_seeds(np.array([0.0]), np.array([-180.0, 0.0, 179.5]), 0.25, (-90.0, 90.0, -180.0, 179.5), np.float64)
    assert g.col_valid.tolist() == [False, True, False]


def test_aux_seeds_takes_both_forms_of_delta_and_refuses_the_rest():
    lat, lon, box = np.linspace(-10, 10, 5), np.linspace(20, 40, 6), (-20.0, 20.0, 10.0, 50.0)
    one = Engine.aux_seeds(lat, lon, 0.5, box, np.float64)
    two = Engine.aux_seeds(lat, lon, (0.5, 0.5), box, np.float64)
    for a, b in zip(one, two):
        assert np.array_equal(a, b)
    s = Engine.aux_seeds(lat, lon, (0.25, 1.0), box, np.float64)
    assert np.array_equal(s.sep_lat, (lat + 0.25) - (lat - 0.25)) and np.array_equal(s.sep_lon, (lon + 1.0) - (lon - 1.0))
    for bad in (0, -0.1, float("nan"), float("inf"), (0.1, 0.0), (0.1, 0.2, 0.3), None, "x"):
        with pytest.raises(ValueError, match="delta"):
            Engine.aux_seeds(lat, lon, bad, box, np.float64)
    with pytest.raises(ValueError, match="dtype"):
        Engine.aux_seeds(lat, lon, 0.5, box, np.float16)
    with pytest.raises(ValueError, match="field_box"):
        Engine.aux_seeds(lat, lon, 0.5, (20.0, -20.0, 10.0, 50.0), np.float64)
    with pytest.raises(ValueError, match="1-D"):
        Engine.aux_seeds(lat[:, None], lon, 0.5, box, np.float64)


# ------------------------------------------------------------------ C ABI
def test_symbols_in_header_prototypes_library_and_sources(lib):
    for name in ("lc_aux_gradient", "lc_ctx_last_aux_kernel"):
        assert name in declared_symbols() and name in _capi.PROTOTYPES and hasattr(lib, name)
    assert lib.lc_version() == 104 == _capi.LC_VERSION          # additive: no argument list changed
    assert "aux_gradient.hip" in build.SOURCES and build.ARCH == "gfx950"
    assert lib.lc_ctx_last_aux_kernel(None) == b""


def test_lc_aux_gradient_checks_arguments_before_any_device_call(lib):
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p).value
    ctx = C.c_void_p(1)             # never dereferenced: every case below is refused by the checks that precede the first HIP call

    def args(**kw):
        a = _capi.AuxGradientArgs(struct_size=C.sizeof(_capi.AuxGradientArgs), dtype=_capi.LC_F64, ny=4, nx=4, n_members=1,
                                  seed_lat_dev=p, sep_lat_dev=p, sep_lon_dev=p, tensor_layout=_capi.LC_LAYOUT_PHYSICAL, s1_out=p,
                                  **{k: p for k in AG.PLANES})
        for k, v in kw.items():
            setattr(a, k, v)
        return C.byref(a)

    def refused(ctx_, a, text):
        return lib.lc_aux_gradient(ctx_, a) == _capi.LC_EINVAL and text in lib.lc_last_error()
    assert refused(None, args(), b"lc_aux_gradient: null context")
    assert refused(ctx, None, b"lc_aux_gradient: null argument structure")
    wrong = C.sizeof(_capi.AuxGradientArgs) - 8
    assert refused(ctx, args(struct_size=wrong), b"struct_size %d, this library has %d" % (wrong, wrong + 8))
    assert refused(ctx, args(dtype=7), b"bad dtype 7") and refused(ctx, args(dtype=_capi.LC_F64_WIND_F32), b"bad dtype")
    assert refused(ctx, args(ny=0), b"bad grid 0x4") and refused(ctx, args(nx=0), b"bad grid 4x0")
    assert refused(ctx, args(ny=1 << 16, nx=1 << 15), b"2^31")
    assert refused(ctx, args(n_members=0), b"bad n_members 0") and refused(ctx, args(n_members=65536), b"bad n_members 65536")
    assert refused(ctx, args(tensor_layout=2), b"bad tensor_layout 2")
    for k in AG.PLANES + ("seed_lat_dev", "sep_lat_dev", "sep_lon_dev"):
        assert refused(ctx, args(**{k: None}), b"null input pointer"), k
    assert refused(ctx, args(s1_out=None), b"no output requested")
    with pytest.raises(ValueError, match="lc_aux_gradient"):
        _capi.check(lib.lc_aux_gradient(None, args()), lib)


# ------------------------------------------------------------------ the drop-in's argument
def test_lcs_aux_grid_argument_and_refusals():
    from LagrangianCoherence.LCS.LCS import LCS
    assert LCS is dropin.LCS
    params = list(inspect.signature(LCS.__init__).parameters)
    assert params == ["self", "timestep", "timedim", "SETTLS_order", "subdomain", "return_dpts", "gauss_sigma", "aux_grid"]
    assert inspect.signature(LCS.__init__).parameters["aux_grid"].default is None
    assert LCS().aux_grid is None and LCS(aux_grid=0.05).aux_grid == 0.05 and LCS(aux_grid=1).aux_grid == 1.0
    for bad in (0, -0.05, float("nan"), float("inf"), True, "0.1", (0.1, 0.1)):
        with pytest.raises(ValueError, match="aux_grid"):
            LCS(aux_grid=bad)
    with pytest.raises(ValueError, match="gauss_sigma"):
        LCS(aux_grid=0.05, gauss_sigma=1.5)
    LCS(aux_grid=0.05, gauss_sigma=None)
    sig = inspect.signature(Engine.lcs_aux).parameters
    assert list(sig)[:9] == ["self", "field", "seed_lat", "seed_lon", "timestep", "nsteps", "n_windows", "t0", "t0_stride"]
    assert sig["aux_delta"].kind is inspect.Parameter.KEYWORD_ONLY and sig["aux_delta"].default is inspect.Parameter.empty
    assert sig["n_dirs"].default == 1 and sig["want"].default == ("sigma",) and sig["centre"].default is False
