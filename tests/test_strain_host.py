"""``LCS.strain`` and ``lc_strain`` on the CPU: the symbols and their argument checks before any device call, the signatures
of the engine and drop-in methods, the drop-in's argument handling (window / stride validation, window count, time labels for
both signs of ``timestep``, the ``subdomain`` crop, the ``return_dpts`` tuple) through a stand-in engine answering with the CPU
oracle, the one intake of the four call forms (what each hands to the engine, bit for bit), and the closed form the kernel implements, stated in numpy (tests/_strain.py), against ``numpy.linalg.svd`` on the
golden departure fields.  The arithmetic on the GPU is tests/test_strain_gpu.py's."""
import inspect

import numpy as np
import pandas as pd
import pytest
import torch

from lagrangiancoherence_amd import _capi, build, dropin, flows, preprocess
from lagrangiancoherence_amd.engine import Engine
from oracle import lcs_oracle as O
from oracle import preprocess_oracle as P
from tests import _strain as S
from tests import labelled
from tests.test_bidir_host import OracleBidirEngine
from tests.test_capi_symbols import declared_symbols
from tests.test_series_host import OracleSeriesEngine


@pytest.fixture(scope="module")
def lib():
    build.build_library(verbose=False)
    return _capi.load()


# ------------------------------------------------------------------ C ABI
def test_symbols_in_header_prototypes_and_library(lib):
    for name in ("lc_strain", "lc_ctx_last_strain_kernel"):
        assert name in declared_symbols() and name in _capi.PROTOTYPES and hasattr(lib, name)
    assert lib.lc_version() == 104 == _capi.LC_VERSION          # additive: no argument list changed
    assert "strain.hip" in build.SOURCES
    assert lib.lc_ctx_last_strain_kernel(None) == b""


def test_lc_strain_checks_arguments_before_any_device_call(lib):
    import ctypes as C
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    ctx = C.c_void_p(1)             # never dereferenced: every case below is refused by the checks that precede the first HIP call
    args = lambda **kw: [kw.get("ctx", ctx), p, p, kw.get("dtype", _capi.LC_F64), kw.get("ny", 8), kw.get("nx", 8), p, 1.0, 1.0, 1,
                         kw.get("n", 1), kw.get("s1", p), None, None, None]
    assert lib.lc_strain(*args(ctx=None)) == _capi.LC_EINVAL and b"lc_strain: null context" in lib.lc_last_error()
    assert lib.lc_strain(*args(dtype=7)) == _capi.LC_EINVAL and b"lc_strain: bad dtype 7" in lib.lc_last_error()
    assert lib.lc_strain(*args(dtype=_capi.LC_F64_WIND_F32)) == _capi.LC_EINVAL and b"lc_strain: bad dtype" in lib.lc_last_error()
    assert lib.lc_strain(*args(ny=4)) == _capi.LC_EINVAL and b"lc_strain: grid 4x8 too small" in lib.lc_last_error()
    assert lib.lc_strain(*args(nx=4)) == _capi.LC_EINVAL and b"lc_strain: grid 8x4 too small" in lib.lc_last_error()
    assert lib.lc_strain(*args(n=0)) == _capi.LC_EINVAL and b"lc_strain: bad n_members 0" in lib.lc_last_error()
    assert lib.lc_strain(*args(s1=None)) == _capi.LC_EINVAL and b"lc_strain: null pointer" in lib.lc_last_error()
    with pytest.raises(ValueError, match="lc_strain"):
        _capi.check(lib.lc_strain(*args(ctx=None)), lib)


def test_signatures():
    from LagrangianCoherence.LCS.LCS import LCS
    assert LCS is dropin.LCS
    sig = inspect.signature(LCS.strain)
    assert list(sig.parameters) == ["self", "ds", "u", "v", "window", "stride", "verbose", "s", "resample", "s_is_error", "isglobal",
                                    "interp_to_common_grid", "traj_interp_order", "truncation"]
    d = {k: p.default for k, p in sig.parameters.items() if k != "self"}
    assert d == dict(ds=None, u=None, v=None, window=None, stride=1, verbose=True, s=None, resample=None, s_is_error=False,
                     isglobal=False, interp_to_common_grid=True, traj_interp_order=3, truncation=20)
    sig = inspect.signature(Engine.strain)
    assert list(sig.parameters) == ["self", "x_dep", "y_dep", "seed_lat", "dlat", "dlon", "fd_fp32_cast", "want"]
    assert sig.parameters["fd_fp32_cast"].default is True and sig.parameters["want"].default == ("s1", "s2", "e_lon", "e_lat")
    assert callable(Engine.last_strain_kernel)
    sig = inspect.signature(Engine.lcs_strain)
    series = inspect.signature(Engine.lcs_series)
    assert list(sig.parameters)[:9] == ["self", "field", "seed_lat", "seed_lon", "timestep", "nsteps", "n_windows", "t0", "t0_stride"]
    assert sig.parameters["n_windows"].default == 1 and sig.parameters["t0"].default == 0 and sig.parameters["t0_stride"].default == 1
    # the advection arguments of lcs_series, all of them (tensor_layout has no meaning here: the layout is the physical one)
    assert set(series.parameters) - set(sig.parameters) == {"tensor_layout"}
    # all four call forms take their record from the one intake
    for f in (LCS.__call__, LCS.series, LCS.bidirectional, LCS.strain):
        assert "_record_intake" in inspect.getsource(f)


# ------------------------------------------------------------------ drop-in adapter through a stand-in engine
class OracleStrainEngine(OracleSeriesEngine):
    """OracleSeriesEngine plus ``lcs_strain``: the oracle's advection and tensor, the closed form of tests/_strain.py."""
    strain_calls = []

    def lcs_strain(self, f, slat, slon, timestep, nsteps, n_windows=1, t0=0, t0_stride=1, SETTLS_order=0, interp_order=1,
                   cyclic_xboundary=True, gauss_sigma=None, fd_fp32_cast=True, noncyclic_clamp=None):
        self.strain_calls.append(dict(nt=f.nt, nsteps=nsteps, n_windows=n_windows, t0=t0, t0_stride=t0_stride, timestep=timestep,
                                      cyclic=cyclic_xboundary))
        outs = []
        for m in range(n_windows):
            x, y = (t.numpy() for t in self.advect(f, slat, slon, timestep, SETTLS_order, interp_order, cyclic_xboundary,
                                                   t0 + m * t0_stride, nsteps))
            tens = O.flowmap_gradient(x, y, np.asarray(slat), np.asarray(slon), sigma=gauss_sigma, fd_fp32_cast=fd_fp32_cast)
            outs.append((*S.closed_form(tens), x, y))
        return {k: torch.as_tensor(np.stack([o[i] for o in outs]))
                for i, k in enumerate(("s1", "s2", "e_lon", "e_lat", "x_dep", "y_dep"))}


@pytest.fixture(autouse=True)
def oracle_engine(monkeypatch):
    eng = OracleStrainEngine()
    eng.strain_calls, eng.series_calls = [], []
    monkeypatch.setattr(dropin, "_ENGINE", eng)
    monkeypatch.setattr(dropin, "get_engine", lambda: eng)
    return eng


def _dataset(nt=9, freq="6h", start="2000-01-01"):
    u, v, lat, lon = flows.config1()
    u, v = np.concatenate([u] * 2)[:nt], np.concatenate([v] * 2)[:nt]
    times = pd.date_range(start, periods=nt, freq=freq).values
    coords = {"latitude": lat, "longitude": lon, "time": times}
    U = labelled.DataArray(u.transpose(1, 2, 0), ["latitude", "longitude", "time"], coords, name="u")
    V = labelled.DataArray(v.transpose(1, 2, 0), ["latitude", "longitude", "time"], coords, name="v")
    return labelled.Dataset({"u": U, "v": V}), times, lat, lon


def test_argument_checks():
    from LagrangianCoherence.LCS.LCS import LCS
    ds, times, lat, lon = _dataset(nt=6)
    lcs = LCS(timestep=-6 * 3600, timedim="time", SETTLS_order=1)
    for bad in (1, 0, -3, 2.5, True):
        with pytest.raises(ValueError, match="window"):
            lcs.strain(ds, window=bad, verbose=False)
    for bad in (0, -1, 1.5, False):
        with pytest.raises(ValueError, match="stride"):
            lcs.strain(ds, window=3, stride=bad, verbose=False)
    with pytest.raises(ValueError, match="longer than the record"):
        lcs.strain(ds, window=7, verbose=False)
    with pytest.raises(TypeError):
        lcs.strain(ds, window=3, return_traj=True, verbose=False)
    with pytest.raises(AssertionError, match="latitude and longitude only"):
        lcs.strain(u=ds.u.isel(time=0), v=ds.v.isel(time=0), verbose=False)


@pytest.mark.parametrize("timestep", [6 * 3600, -6 * 3600])
@pytest.mark.parametrize("resample", [None, "3h"])
def test_window_count_and_time_labels(oracle_engine, timestep, resample):
    from LagrangianCoherence.LCS.LCS import LCS
    nt, window, stride = 9, 4, 2
    ds, times, lat, lon = _dataset(nt=nt)
    lcs = LCS(timestep=timestep, timedim="time", SETTLS_order=1, return_dpts=True)
    out = lcs.strain(ds, window=window, stride=stride, resample=resample, verbose=False, traj_interp_order=1)
    assert len(out) == 5
    s1, s2, direction, xd, yd = out
    n = (nt - window) // stride + 1
    first = np.arange(n) * stride
    want = times[first + window - 1] if timestep > 0 else times[first]      # LCS.py:158 per window
    assert s1.dims == s2.dims == xd.dims == yd.dims == ("time", "latitude", "longitude")
    assert direction.dims == ("component", "time", "latitude", "longitude")
    assert list(direction.coords["component"]) == ["east", "north"]
    assert s1.shape == s2.shape == xd.shape == yd.shape == (n, lat.size, lon.size) and direction.shape == (2,) + s1.shape
    for a in out:
        assert np.array_equal(a.coords["time"], want)
    r = 2 if resample else 1
    call, = oracle_engine.strain_calls
    assert call == dict(nt=(nt - 1) * r + 1, nsteps=(window - 1) * r, n_windows=n, t0=0, t0_stride=stride * r,
                        timestep=np.sign(timestep) * 6 * 3600 / r, cyclic=False)
    # the departure points are series'
    sig, xs, ys = LCS(timestep=timestep, timedim="time", SETTLS_order=1, return_dpts=True).series(
        ds, window=window, stride=stride, resample=resample, verbose=False, traj_interp_order=1)
    assert np.array_equal(xd.values, xs.values) and np.array_equal(yd.values, ys.values)
    assert np.array_equal(sig.coords["time"], s1.coords["time"])
    assert np.all(s1.values >= s2.values) and np.all(s2.values >= 0)
    np.testing.assert_allclose(np.hypot(direction.values[0], direction.values[1]), 1.0, rtol=0, atol=1e-12)


@pytest.mark.parametrize("timestep", [6 * 3600, -6 * 3600])
def test_whole_record_is_one_entry_labelled_as_call(oracle_engine, timestep):
    from LagrangianCoherence.LCS.LCS import LCS
    ds, times, lat, lon = _dataset(nt=5)
    out = LCS(timestep=timestep, timedim="time", SETTLS_order=1).strain(ds, verbose=False, traj_interp_order=1, isglobal=True,
                                                                       interp_to_common_grid=False, truncation=None)
    assert len(out) == 3                                          # no return_dpts
    s1, s2, direction = out
    assert s1.shape == (1, lat.size, lon.size) and direction.shape == (2, 1, lat.size, lon.size)
    one = LCS(timestep=timestep, timedim="time", SETTLS_order=1)(ds, verbose=False, traj_interp_order=1, isglobal=True,
                                                                 interp_to_common_grid=False, truncation=None)
    assert s1.coords["time"][0] == one.coords["time"][0] == (times[-1] if timestep > 0 else times[0])
    call, = oracle_engine.strain_calls
    assert call == dict(nt=5, nsteps=4, n_windows=1, t0=0, t0_stride=1, timestep=timestep, cyclic=True)


def test_subdomain_crop_applies_to_the_fields_not_to_the_departure_points():
    from LagrangianCoherence.LCS.LCS import LCS
    ds, times, lat, lon = _dataset(nt=5)
    sub = {"latitude": slice(-40, 40), "longitude": slice(-100, 100)}
    s1, s2, direction, xd, yd = LCS(timestep=-6 * 3600, timedim="time", SETTLS_order=1, subdomain=sub, return_dpts=True).strain(
        ds, window=3, verbose=False, traj_interp_order=1)
    mlat, mlon = (lat > -40) & (lat < 40), (lon > -100) & (lon < 100)          # strict, LCS/tools.py:158-187
    assert s1.shape == s2.shape == (3, mlat.sum(), mlon.sum()) and direction.shape == (2, 3, mlat.sum(), mlon.sum())
    for a in (s1, s2, direction):
        assert np.array_equal(a.coords["latitude"], lat[mlat]) and np.array_equal(a.coords["longitude"], lon[mlon])
    assert xd.shape == yd.shape == (3, lat.size, lon.size)
    whole = LCS(timestep=-6 * 3600, timedim="time", SETTLS_order=1).strain(ds, window=3, verbose=False, traj_interp_order=1)
    assert np.array_equal(s2.values, whole[1].values[:, mlat][:, :, mlon])
    assert np.array_equal(direction.values, whole[2].values[:, :, mlat][:, :, :, mlon])
    # isglobal drops the subdomain, as __call__ does (LCS.py:119-120)
    g = LCS(timestep=-6 * 3600, timedim="time", SETTLS_order=1, subdomain=sub).strain(
        ds, window=3, verbose=False, traj_interp_order=1, isglobal=True, interp_to_common_grid=False, truncation=None)
    assert g[0].shape == (3, lat.size, lon.size)


# ------------------------------------------------------------------ one intake for the four call forms
class IntakeRecorder(OracleStrainEngine, OracleBidirEngine):
    """The stand-in engines of the four call forms in one, recording what each is handed: the wind of ``lcs_wind``, the pack of
    ``prepare_field``, the arguments of the windowed calls.  ``regrid`` and ``spectral_truncate`` answer with the oracle's."""

    def __init__(self):
        self.wind, self.packed, self.windows = [], [], []
        self.series_calls, self.bidir_calls, self.strain_calls = [], [], []

    def regrid(self, u, lat, lon, lats, lons):
        return torch.as_tensor(np.ascontiguousarray(P.regrid_common_grid(np.asarray(u), lat, lon, lats, lons)[0]))

    def spectral_truncate(self, f, T=20, gridtype="regular"):
        return torch.as_tensor(np.ascontiguousarray(P.spectral_truncate(np.asarray(f), T, gridtype)))

    def lcs_wind(self, u, v, lat, lon, slat, slon, timestep, **kw):
        self.wind.append(dict(u=np.asarray(u).copy(), v=np.asarray(v).copy(), lat=lat, lon=lon, slat=slat, slon=slon,
                              step=abs(timestep), order=kw["interp_order"], K=kw["SETTLS_order"], cyclic=kw["cyclic_xboundary"],
                              gauss=kw["gauss_sigma"]))
        n = len(self.packed)
        res = super().lcs_wind(u, v, lat, lon, slat, slon, timestep, **kw)
        del self.packed[n:]                         # (the stand-in's lcs_wind packs through prepare_field)
        return res

    def prepare_field(self, u, v, lat, lon, interp_order=1, dtype=None, fuse_levels=None, ext_image=None):
        self.packed.append(dict(u=np.asarray(u).copy(), v=np.asarray(v).copy(), lat=lat, lon=lon, order=interp_order,
                                fuse_levels=fuse_levels, ext_image=ext_image))
        return super().prepare_field(u, v, lat, lon, interp_order, dtype, fuse_levels, ext_image)

    def _windowed(name):
        def call(self, f, slat, slon, timestep, nsteps, n_windows=1, t0=0, t0_stride=1, **kw):
            # (t0_stride is left out: with one window it has no meaning, and series(window=nt) and window=None differ in it)
            self.windows.append(dict(slat=slat, slon=slon, step=abs(timestep), nsteps=nsteps, n_windows=n_windows, t0=t0,
                                     order=kw["interp_order"], K=kw["SETTLS_order"], cyclic=kw["cyclic_xboundary"],
                                     gauss=kw["gauss_sigma"]))
            return getattr(super(IntakeRecorder, self), name)(f, slat, slon, timestep, nsteps, n_windows, t0, t0_stride, **kw)
        return call

    lcs_series, lcs_bidirectional, lcs_strain = _windowed("lcs_series"), _windowed("lcs_bidirectional"), _windowed("lcs_strain")
    del _windowed


def _same_bits(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
        else:
            assert a[k] == b[k] and type(a[k]) is type(b[k]), k


@pytest.mark.parametrize("timestep", [6 * 3600, -6 * 3600])
@pytest.mark.parametrize("isglobal", [False, True])
def test_the_four_call_forms_hand_the_engine_the_same_record(monkeypatch, timestep, isglobal):
    """One record through every branch of the intake -- descending latitude, unsorted longitude, a ``resample`` that halves the
    spacing, a ``subdomain``, both signs of ``timestep``; with ``isglobal`` the 0.5 degree regrid, the T20 truncation and the
    ``subdomain = None`` rule -- and through ``__call__``, ``series(window=nt)``, ``bidirectional(window=None)`` and
    ``strain(window=None)``: what reaches the engine is the same bit for bit (``__call__``: the wind and the coordinates of
    ``lcs_wind``; the others: the pack of ``prepare_field`` with the options ``_pack_options`` chose, and the step's magnitude and
    the window geometry of the windowed call), and sigma and its time label are the same in the three forms that return one."""
    from LagrangianCoherence.LCS.LCS import LCS
    nt = 2 if isglobal else 3                   # (the 0.5 degree grid has 16 times the cells: the oracle's time)
    ds, times, lat, lon = _dataset(nt=nt)
    ilat, ilon = np.arange(lat.size)[::-1], np.roll(np.arange(lon.size), 7)
    ds = labelled.Dataset({k: ds[k].isel(latitude=ilat, longitude=ilon) for k in ("u", "v")})
    assert ds.u.coords["latitude"][0] > ds.u.coords["latitude"][1] and np.any(np.diff(ds.u.coords["longitude"]) < 0)
    sub = {"latitude": slice(-40, 40), "longitude": slice(-100, 100)}
    ctor = dict(timestep=timestep, timedim="time", SETTLS_order=1, subdomain=sub, gauss_sigma=1.0)
    call = dict(resample="3h", isglobal=isglobal, verbose=False, traj_interp_order=1)
    forms = {"call": lambda l: l(ds, **call), "series": lambda l: l.series(ds, window=nt, **call),
             "bidirectional": lambda l: l.bidirectional(ds, **call), "strain": lambda l: l.strain(ds, **call)}
    out, rec = {}, {}
    for name, form in forms.items():
        rec[name] = eng = IntakeRecorder()
        monkeypatch.setattr(dropin, "_ENGINE", eng)
        monkeypatch.setattr(dropin, "get_engine", lambda eng=eng: eng)
        lcs = LCS(**ctor)
        out[name] = form(lcs)
        assert (lcs.subdomain is None) == isglobal                     # LCS.py:119-120
    # what the engine was handed
    wind, = rec["call"].wind
    assert not rec["call"].packed and not rec["call"].windows
    glat, glon = (preprocess.COMMON_LATS, preprocess.COMMON_LONS) if isglobal else (lat, lon)
    assert np.array_equal(wind["lat"], glat) and np.array_equal(wind["lon"], glon)
    assert wind["u"].shape == (2 * nt - 1, glat.size, glon.size) and wind["step"] == 3 * 3600.0 and wind["cyclic"] is isglobal
    for name in ("series", "bidirectional", "strain"):
        assert not rec[name].wind
        (packed,), (windows,) = rec[name].packed, rec[name].windows
        for got, keys in ((packed, ("u", "v", "lat", "lon", "order")), (windows, ("slat", "slon", "step", "K", "cyclic", "gauss"))):
            _same_bits({k: got[k] for k in keys}, {k: wind[k] for k in keys})
        _same_bits(packed, rec["series"].packed[0])
        _same_bits(windows, rec["series"].windows[0])
        assert (packed["fuse_levels"], packed["ext_image"]) == Engine._pack_options(np.dtype(np.float64), 1, False, None)
        assert (windows["nsteps"], windows["n_windows"], windows["t0"]) == (2 * nt - 2, 1, 0)
    # sigma and its label
    one, ser, both = out["call"], out["series"], out["bidirectional"][timestep > 0]
    for a in (ser, both):
        assert a.dims == one.dims and a.shape == one.shape and np.array_equal(a.values, one.values)
        for k in one.coords:
            assert np.array_equal(np.asarray(a.coords[k]), np.asarray(one.coords[k])), k
    assert one.coords["time"][0] == (times[-1] if timestep > 0 else times[0]) == out["strain"][0].coords["time"][0]
    mlat, mlon = (lat > -40) & (lat < 40), (lon > -100) & (lon < 100)
    assert one.shape == ((1, glat.size, glon.size) if isglobal else (1, mlat.sum(), mlon.sum())) == out["strain"][0].shape


# ------------------------------------------------------------------ the closed form against numpy's SVD
@pytest.mark.parametrize("name", ["g1_bwd_k4_o3", "g1_fwd_k4_o1"])
def test_closed_form_against_numpy_svd_on_the_golden_departure_fields(name):
    """The formulas of the kernel (tests/_strain.py::closed_form) against numpy.linalg.svd of F from the oracle's tensor.  Measured
    with numpy 1.26 / OpenBLAS on the two fields: |s1 - svd| / s1 <= 7e-16, |s2 - svd| / s2 <= 8e-14, eigen-residual
    ||C e - lam e|| / lam <= 5e-16; asserted at 100 x those (another LAPACK or numpy).  The cancelling form
    sqrt(0.5 ((p + q) - disc)) of s2 misses the s2 bound by orders of magnitude on g1_fwd_k4_o1, which is why the kernel
    takes |col1 x col2| / s1."""
    _, _, lat, lon = flows.config1()
    x, y = S.golden(name)
    tens = O.flowmap_gradient(x, y, lat, lon)
    s1, s2, ex, ey = S.closed_form(tens)
    r1, r2, v1 = S.svd_reference(tens)
    e1, e2 = np.abs(s1 - r1) / r1, np.abs(s2 - r2) / r2
    res = S.eigen_residual(tens, ex, ey, s1 * s1) / (s1 * s1)
    p, q, r = S.gram(tens)
    naive = np.sqrt(np.maximum(0.5 * ((p + q) - np.sqrt((p - q) ** 2 + 4 * r * r)), 0.0))
    print(f"{name}: s1 {e1.max():.2e}  s2 {e2.max():.2e}  residual {res.max():.2e}  cancelling s2 {(np.abs(naive - r2) / r2).max():.2e}")
    assert e1.max() <= 7e-14 and e2.max() <= 8e-12 and res.max() <= 5e-14
    np.testing.assert_allclose(np.hypot(ex, ey), 1.0, rtol=0, atol=1e-15)
    assert S.sign_convention_holds(ex, ey)
    gap = r2 / r1 <= 0.99
    assert gap.mean() >= 0.99 and S.sine_of_angle(ex, ey, v1)[gap].max() <= 1e-7
    assert np.array_equal(s1, O.sigma_max_closed_form(tens, "physical"))


def test_closed_form_rule_cases():
    z = np.zeros((1, 1))
    T = lambda a, b, c, d, e, f: np.stack([z + a, z + b, z + c, z + d, z + e, z + f, z, z, z])
    one = lambda t: tuple(float(v[0, 0]) for v in S.closed_form(t))
    assert one(T(2, 0, 0, 2, 0, 0)) == (2.0, 2.0, 1.0, 0.0)            # isotropic: (1, 0)
    assert one(T(0, 0, 0, 0, 0, 0)) == (0.0, 0.0, 1.0, 0.0)            # s1 == 0: s2 = 0
    assert one(T(1, 0, 0, 3, 0, 0)) == (3.0, 1.0, 0.0, 1.0)            # e_lon == 0: e_lat > 0
    assert one(T(3, 0, 0, 1, 0, 0)) == (3.0, 1.0, 1.0, 0.0)
    s1, s2, ex, ey = one(T(1, -1, 0, 1, 0, 0))                          # shear: the stretched direction has e_lon > 0
    assert ex > 0 and ey < 0 and abs(s1 * s2 - 1.0) < 1e-15
    assert all(np.isnan(v) for v in one(T(np.nan, 1, 0, 1, 0, 0)))     # NaN in: NaN in all four
