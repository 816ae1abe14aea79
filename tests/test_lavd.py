"""Vorticity, LAVD, rotation and path length without a device: the C boundary of lc_vorticity and lc_lavd_update (symbols,
structure sizes, every refusal before the first HIP call), the host-side refusals of Engine.vorticity / Engine.lavd_update /
Engine.lavd / LCS.lavd, and the numpy restatements of the two definitions (tests/lavd.py) against analytic fields, hand-worked
records, themselves cut into blocks, and the CPU oracle's trajectories of a moving vortex."""
import ctypes as C
import inspect
import os
import types

import numpy as np
import pandas as pd
import pytest

from lagrangiancoherence_amd import _capi, build, dropin
from lagrangiancoherence_amd.engine import Engine
from tests import labelled
from tests import lavd as L
from tests.test_capi_symbols import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lc_vorticity", "lc_vorticity_work_elems", "lc_ctx_last_vorticity_kernel", "lc_lavd_update", "lc_ctx_last_lavd_kernel")


@pytest.fixture(scope="module")
def lib():
    build.build_library(verbose=False)
    return _capi.load()


# ------------------------------------------------------------------ C ABI
def test_symbols_in_header_prototypes_library_and_sources(lib):
    for name in SYMBOLS:
        assert name in declared_symbols() and name in _capi.PROTOTYPES and hasattr(lib, name), name
    assert lib.lc_version() == 104 == _capi.LC_VERSION          # additive: no argument list changed
    assert "vorticity.hip" in build.SOURCES and "lavd.hip" in build.SOURCES and build.ARCH == "gfx950"
    assert lib.lc_ctx_last_vorticity_kernel(None) == b"" and lib.lc_ctx_last_lavd_kernel(None) == b""
    assert (_capi.LC_VORT_DEVIATION_DOMAIN, _capi.LC_VORT_DEVIATION_NONE, _capi.LC_VORT_DEVIATION_GIVEN) == (0, 1, 2)
    header = open(os.path.join(ROOT, "include", "lcs_hip.h")).read()
    assert "enum lc_vort_deviation { LC_VORT_DEVIATION_DOMAIN = 0, LC_VORT_DEVIATION_NONE = 1, LC_VORT_DEVIATION_GIVEN = 2 };" in header
    assert _capi.VorticityArgs._fields_[0][0] == "struct_size" == _capi.LavdArgs._fields_[0][0]
    # two float64 per workgroup of 4 rows x 64 columns; 0 for sizes the call refuses
    assert lib.lc_vorticity_work_elems(97, 720, 1440) == 97 * 180 * 23 * 2 and lib.lc_vorticity_work_elems(1, 4, 4) == 2
    assert lib.lc_vorticity_work_elems(1, 3, 4) == 0 and lib.lc_vorticity_work_elems(0, 4, 4) == 0


def test_the_kernel_sources_keep_to_their_means():
    """No atomics (the sums are fixed trees and index-order adds), no inline assembly; the fold shares fsle.hip's separation."""
    for name in ("vorticity.hip", "lavd.hip"):
        code = build._strip_comments(open(os.path.join(build.CSRC, name)).read())
        for word in ("atomic", "asm(", "asm volatile", "cooperative", "__threadfence"):
            assert word not in code, (name, word)
    vort = build._strip_comments(open(os.path.join(build.CSRC, "vorticity.hip")).read())
    assert "__shfl_down" in vort and "__shared__" in vort
    fold = build._strip_comments(open(os.path.join(build.CSRC, "lavd.hip")).read())
    fsle = build._strip_comments(open(os.path.join(build.CSRC, "fsle.hip")).read())
    assert '#include "great_circle.h"' in fold and '#include "great_circle.h"' in fsle and "fsle_sep(" in fold


def test_lc_vorticity_checks_arguments_before_any_device_call(lib):
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p).value
    ctx = C.c_void_p(1)             # never dereferenced: every case below is refused by the checks that precede the first HIP call

    def args(**kw):
        a = _capi.VorticityArgs(struct_size=C.sizeof(_capi.VorticityArgs), u=p, v=p, dtype=_capi.LC_F64, nt=2, ny_f=5, nx_f=6,
                                lat_min=-40.0, lat_max=0.0, lon_min=-80.0, lon_max=-30.0, cyclic_x=0,
                                deviation=_capi.LC_VORT_DEVIATION_DOMAIN, radius=6371000.0, given_dev=None, omega=p, level_mean=p, work_dev=p)
        for k, v in kw.items():
            setattr(a, k, v)
        return C.byref(a)

    def refused(ctx_, a, text):
        return lib.lc_vorticity(ctx_, a) == _capi.LC_EINVAL and text in lib.lc_last_error()
    assert refused(None, args(), b"lc_vorticity: null context")
    assert refused(ctx, None, b"lc_vorticity: null argument structure")
    wrong = C.sizeof(_capi.VorticityArgs) - 8
    assert refused(ctx, args(struct_size=wrong), b"struct_size %d, this library has %d" % (wrong, wrong + 8))
    assert refused(ctx, args(dtype=7), b"bad dtype 7") and refused(ctx, args(dtype=_capi.LC_F64_WIND_F32), b"bad dtype")
    assert refused(ctx, args(nt=0), b"bad record 0x5x6") and refused(ctx, args(ny_f=3), b"bad record 2x3x6")
    assert refused(ctx, args(nx_f=3), b"bad record 2x5x3")
    assert refused(ctx, args(ny_f=1 << 16, nx_f=1 << 15), b"2^31")
    assert refused(ctx, args(nt=1 << 20, ny_f=1 << 10, nx_f=1 << 10), b"too large")
    for kw in (dict(lat_min=float("nan")), dict(lat_max=float("inf")), dict(lat_min=-91.0), dict(lat_max=90.5), dict(lat_min=0.0, lat_max=0.0),
               dict(lat_min=10.0, lat_max=-10.0)):
        assert refused(ctx, args(**kw), b"bad latitudes"), kw
    for kw in (dict(lon_min=float("nan")), dict(lon_max=float("inf")), dict(lon_min=-30.0, lon_max=-80.0), dict(lon_min=5.0, lon_max=5.0)):
        assert refused(ctx, args(**kw), b"bad longitudes"), kw
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert refused(ctx, args(radius=bad), b"radius"), bad
    assert refused(ctx, args(deviation=3), b"bad deviation mode 3") and refused(ctx, args(deviation=-1), b"bad deviation mode -1")
    for k in ("u", "v", "omega", "level_mean", "work_dev"):
        assert refused(ctx, args(**{k: None}), b"null pointer"), k
    assert refused(ctx, args(deviation=_capi.LC_VORT_DEVIATION_GIVEN), b"without given_dev")
    with pytest.raises(ValueError, match="lc_vorticity"):
        _capi.check(lib.lc_vorticity(None, args()), lib)


def test_lc_lavd_update_checks_arguments_before_any_device_call(lib):
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p).value
    ctx = C.c_void_p(1)

    def args(**kw):
        a = _capi.LavdArgs(struct_size=C.sizeof(_capi.LavdArgs), traj_x=p, traj_y=p, c=p, dtype=_capi.LC_F32, n=8, n_levels=3, level0=0,
                           timestep=-900.0, radius=6371000.0, acc=p, lavd=p, rotation=p, length=p)
        for k, v in kw.items():
            setattr(a, k, v)
        return C.byref(a)

    def refused(ctx_, a, text):
        return lib.lc_lavd_update(ctx_, a) == _capi.LC_EINVAL and text in lib.lc_last_error()
    assert refused(None, args(), b"lc_lavd_update: null context")
    assert refused(ctx, None, b"lc_lavd_update: null argument structure")
    wrong = C.sizeof(_capi.LavdArgs) + 8
    assert refused(ctx, args(struct_size=wrong), b"struct_size %d, this library has %d" % (wrong, wrong - 8))
    assert refused(ctx, args(dtype=7), b"bad dtype 7")
    assert refused(ctx, args(n=0), b"n 0") and refused(ctx, args(n=-3), b"n -3")
    assert refused(ctx, args(n_levels=1), b"n_levels 1") and refused(ctx, args(n_levels=0), b"n_levels 0")
    assert refused(ctx, args(level0=-1), b"level0 -1")
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert refused(ctx, args(radius=bad), b"radius"), bad
    for bad in (0.0, float("nan"), float("inf"), -float("inf")):
        assert refused(ctx, args(timestep=bad), b"timestep"), bad
    for k in ("traj_x", "traj_y", "acc"):
        assert refused(ctx, args(**{k: None}), b"null pointer"), k
    assert refused(ctx, args(c=None), b"lavd and rotation need c") and refused(ctx, args(c=None, lavd=None), b"need c")
    with pytest.raises(ValueError, match="lc_lavd_update"):
        _capi.check(lib.lc_lavd_update(None, args()), lib)


# ------------------------------------------------------------------ the Python surfaces refuse before any device work
def test_the_engine_refuses_bad_arguments_without_a_device():
    eng = Engine.__new__(Engine)             # no device: the checks come before anything is touched
    lat, lon = np.linspace(-40.0, 0.0, 5), np.linspace(-80.0, -30.0, 6)
    u = np.zeros((3, 5, 6))
    good = dict(u=u, v=u, lat_f=lat, lon_f=lon)
    uneven = lat.copy()
    uneven[2] += 1.0
    for kw in (dict(u=u[0]), dict(v=u[:2]), dict(u=u[:, :3], v=u[:, :3], lat_f=lat[:3]), dict(u=u[:, :, :3], v=u[:, :, :3], lon_f=lon[:3]),
               dict(lat_f=lat[:4]), dict(lon_f=lon[::-1]), dict(lat_f=lat[::-1]), dict(lat_f=uneven), dict(lat_f=lat * 3),
               dict(lat_f=np.where(np.arange(5) == 1, np.nan, lat)), dict(lat_f="north"), dict(deviation="zonal"), dict(deviation=[0.0, 0.0]),
               dict(deviation=[0.0, np.nan, 0.0]), dict(deviation=[[0.0, 0.0, 0.0]]), dict(deviation=[]), dict(deviation=object()),
               dict(radius=0.0), dict(radius=-1.0), dict(radius=np.inf), dict(radius="big")):
        with pytest.raises(ValueError, match="vorticity"):
            eng.vorticity(**{**good, **kw})
    nt, ny_f, nx_f, mode, given, radius = Engine.checked_vorticity_options(u.shape, u.shape, lat, lon, [1e-6, 0.0, -1e-6], 1.0)
    assert (nt, ny_f, nx_f, mode, radius) == (3, 5, 6, _capi.LC_VORT_DEVIATION_GIVEN, 1.0) and given.tolist() == [1e-6, 0.0, -1e-6]
    assert Engine.checked_vorticity_options(u.shape, u.shape, lat.astype(np.float32), lon, "none")[3:5] == (_capi.LC_VORT_DEVIATION_NONE, None)
    assert Engine.checked_deviation("domain") == (_capi.LC_VORT_DEVIATION_DOMAIN, None)

    traj = np.zeros((4, 3, 5))
    good = dict(traj_x=traj, traj_y=traj, c=traj, timestep=-900.0, level0=0)
    for kw in (dict(timestep=0.0), dict(timestep=np.nan), dict(timestep="fast"), dict(radius=0.0), dict(radius=np.inf), dict(level0=-1),
               dict(traj_x=traj[0, 0, :1][0]), dict(traj_y=traj[:3]), dict(c=traj[:, :2]), dict(traj_x=traj[:1], traj_y=traj[:1], c=traj[:1]),
               dict(level0=2)):
        with pytest.raises(ValueError, match="lavd_update"):
            eng.lavd_update(**{**good, **kw})

    field = types.SimpleNamespace(order=1, nt=6, ny_f=5, nx_f=6, lat_min=-40.0, lat_max=0.0, lon_min=-80.0, lon_max=-30.0, dtype=np.dtype(np.float64))
    good = dict(field=field, tracer=None, seed_lat=lat, seed_lon=lon, timestep=900.0)
    other = types.SimpleNamespace(**{**vars(field), "dtype": np.dtype(np.float32)})
    shifted = types.SimpleNamespace(**{**vars(field), "lon_max": -20.0})
    for kw in (dict(timestep=0), dict(timestep=np.inf), dict(radius=np.nan), dict(interp_order=3), dict(t0=-1), dict(nsteps=0), dict(nsteps=6),
               dict(t0=3, nsteps=3), dict(t0=5), dict(level_chunk=0), dict(seed_lat=lat[None]), dict(tracer=other), dict(tracer=shifted),
               dict(cyclic_xboundary=False, noncyclic_clamp="nearest")):
        with pytest.raises(ValueError):
            eng.lavd(**{**good, **kw})
    sig = inspect.signature(Engine.lavd).parameters
    assert list(sig)[:6] == ["self", "field", "tracer", "seed_lat", "seed_lon", "timestep"]
    assert sig["level_chunk"].default == 16 and sig["cyclic_xboundary"].default is True and sig["t0"].default == 0
    assert list(inspect.signature(Engine.lavd_update).parameters)[1:8] == ["traj_x", "traj_y", "c", "timestep", "level0", "acc", "final"]
    assert list(inspect.signature(Engine.vorticity).parameters)[1:9] == ["u", "v", "lat_f", "lon_f", "cyclic", "deviation", "radius", "dtype"]


def _dataset(u, v, lat, lon):
    times = pd.date_range("2010-01-01", periods=u.shape[0], freq="15min").values
    coords = {"latitude": lat, "longitude": lon, "time": times}
    U = labelled.DataArray(u.transpose(1, 2, 0), ["latitude", "longitude", "time"], coords, name="u")
    V = labelled.DataArray(v.transpose(1, 2, 0), ["latitude", "longitude", "time"], coords, name="v")
    return labelled.Dataset({"u": U, "v": V}), times


def test_lcs_lavd_refuses_bad_arguments_before_an_engine_is_asked_for(monkeypatch):
    from LagrangianCoherence.LCS.LCS import LCS
    assert LCS is dropin.LCS

    def no_engine():
        raise AssertionError("an engine was asked for")
    monkeypatch.setattr(dropin, "get_engine", no_engine)
    u, v, lat, lon = L.vortex_record(d=5.0, nt=4)
    ds, _ = _dataset(u, v, lat, lon)
    lcs = LCS(**L.PHYSICAL)
    with pytest.raises(ValueError, match="aux"):
        LCS(aux_grid=0.05, **L.PHYSICAL).lavd(ds)
    with pytest.raises(ValueError, match="timestep"):
        LCS(timestep=0).lavd(ds)
    for kw in (dict(window=1), dict(window=2.5), dict(window=True), dict(window=5), dict(window=2, stride=0)):
        with pytest.raises(ValueError, match="window|stride"):
            lcs.lavd(ds, verbose=False, **kw)
    for bad in ([0.0] * 3, [0.0] * 5, "zonal", [np.nan] * 4, [[0.0] * 4]):
        with pytest.raises(ValueError, match="deviation"):
            lcs.lavd(ds, deviation=bad, verbose=False)
    with pytest.raises(ValueError, match="deviation"):
        lcs.lavd(u=ds.u, v=ds.v, deviation=[0.0] * 3, verbose=False)
    with pytest.raises(ValueError, match="level_chunk"):
        lcs.lavd(ds, level_chunk=0, verbose=False)
    with pytest.raises(AssertionError, match="an engine was asked for"):       # ... and a good call does ask for one
        lcs.lavd(ds, deviation=[0.0] * 4, verbose=False)
    params = inspect.signature(LCS.lavd).parameters
    assert list(params)[:7] == ["self", "ds", "u", "v", "window", "stride", "deviation"] and params["level_chunk"].default == 16
    assert params["deviation"].default == "domain" and set(inspect.signature(LCS.strain).parameters) <= set(params)
    from LagrangianCoherence.LCS import tools
    assert list(inspect.signature(tools.relative_vorticity).parameters)[:4] == ["u", "v", "cyclic", "deviation"]
    assert inspect.signature(tools.relative_vorticity).parameters["deviation"].default == "none"
    with pytest.raises(ValueError, match="deviation"):
        tools.relative_vorticity(ds.u, ds.v, deviation="zonal")


# ------------------------------------------------------------------ the vorticity restatement against analytic fields
def _solid_body_error(d, T=np.float64):
    u, v, lat, lon, exact = L.solid_body(d)
    om = L.vorticity(u, v, lat[0], lat[-1], lon[0], lon[-1], T, cyclic=True, deviation="none")["omega"][0]
    assert np.ptp(om, axis=1).max() <= 1e-9 * np.abs(exact).max()           # zonally uniform
    return lat, om[:, 0].astype(np.float64), exact


def test_solid_body_rotation_is_second_order_everywhere():
    """u = Omega R cos phi, v = 0 has vorticity 2 Omega sin phi.  Interior rows: the error falls by 4 when the spacing halves
    (a factor between 3 and 5 is asserted, 5 -> 2.5 degrees); on a 5 degree grid the interior is within 1 % and the one-sided
    edge rows at +-80 degrees within 2 % (first-order edges would be wrong by 23 %)."""
    lat5, om5, ex5 = _solid_body_error(5.0)
    lat2, om2, ex2 = _solid_body_error(2.5)
    assert np.array_equal(lat2[::2], lat5)
    e5, e2 = np.abs(om5 - ex5), np.abs(om2 - ex2)[::2]
    inner = slice(1, -1)
    factor = e5[inner].max() / e2[1:-1].max()
    assert 3 < factor < 5, factor
    rows = np.abs(lat5[inner]) >= 10                                        # (at the equator both errors vanish)
    per_row = e5[inner][rows] / e2[inner][rows]
    assert np.all((per_row > 3) & (per_row < 5)), per_row
    scale = np.abs(ex5).max()
    assert e5[inner].max() <= 0.01 * scale and e5[[0, -1]].max() <= 0.02 * np.abs(ex5[[0, -1]]).max()
    assert e5[[0, -1]].max() > e5[inner].max()                              # the edges are the weaker rows, as stated


def test_a_zonal_jet_and_a_meridional_wave_have_their_closed_forms():
    """u = U cos^2 phi alone: omega = 3 U sin phi cos phi / R... checked through d(u cos phi)/dphi; v = V cos(m lambda) alone:
    omega = -m V sin(m lambda) / (R cos phi).  Fine grid, float64: both to 0.1 %."""
    lat, lon = np.linspace(-60, 60, 241), np.arange(0.0, 360.0, 0.5)
    la, lo = L.K * lat[None, :, None], L.K * lon[None, None, :]
    U, V, m = 30.0, 12.0, 3
    u = np.broadcast_to(U * np.cos(la) ** 2, (1, lat.size, lon.size)).copy()
    v = np.broadcast_to(V * np.cos(m * lo), (1, lat.size, lon.size)).copy()
    zero = np.zeros_like(u)
    jet = L.vorticity(u, zero, lat[0], lat[-1], lon[0], lon[-1], np.float64, True, "none")["omega"][0]
    exact = 3 * U * np.cos(la[0]) * np.sin(la[0]) / L.R_EARTH + 0 * lo[0]
    assert np.abs(jet - exact).max() <= 1e-3 * np.abs(exact).max()
    wave = L.vorticity(zero, v, lat[0], lat[-1], lon[0], lon[-1], np.float64, True, "none")["omega"][0]
    exact = -m * V * np.sin(m * lo[0]) / (L.R_EARTH * np.cos(la[0]))
    assert np.abs(wave - exact).max() <= 1e-3 * np.abs(exact).max()
    # the seam: on a periodic grid the cyclic stencil is the interior one, and the one-sided columns differ from it
    open_ = L.vorticity(zero, v, lat[0], lat[-1], lon[0], lon[-1], np.float64, False, "none")["omega"][0]
    assert np.array_equal(open_[:, 1:-1], wave[:, 1:-1]) and not np.array_equal(open_[:, 0], wave[:, 0])


def test_pole_rows_nan_and_the_domain_mean():
    u, v, lat, lon = L.wind_case(19, 36, 2, np.float64, poles=True)
    R = L.vorticity(u, v, lat[0], lat[-1], lon[0], lon[-1], np.float64, True, "none")
    om = R["omega"]
    assert R["pole_rows"] == [0, 18] and np.all(np.isfinite(om))
    for r, adj in ((0, 1), (18, 17)):
        assert np.all(om[:, r, :] == om[:, r, :1]) and np.allclose(om[:, r, 0], om[:, adj, :].mean(axis=1), rtol=1e-13)
    w = np.cos(L.K * lat)[None, :, None] * np.ones_like(om)
    w[:, [0, 18]] = 0
    np.testing.assert_allclose(R["level_mean"], (w * om).sum(axis=(1, 2)) / w.sum(axis=(1, 2)), rtol=1e-12)
    dom = L.vorticity(u, v, lat[0], lat[-1], lon[0], lon[-1], np.float64, True, "domain")
    np.testing.assert_allclose(dom["omega"], om - R["level_mean"][:, None, None], rtol=0, atol=1e-18)
    assert np.array_equal(dom["level_mean"], R["level_mean"])
    giv = L.vorticity(u, v, lat[0], lat[-1], lon[0], lon[-1], np.float64, True, [1e-6, -2e-6])
    np.testing.assert_allclose(giv["omega"][1], om[1] + 2e-6, rtol=0, atol=1e-18)
    # one NaN in u beside the pole row: the latitude stencil of a node skips its own row, so (1, 5) keeps its value; (2, 5)
    # reads it and is NaN; the pole row reads it too but holds the adjacent row's mean, which is unchanged
    bad = u.copy()
    bad[0, 1, 5] = np.nan
    nb = L.vorticity(bad, v, lat[0], lat[-1], lon[0], lon[-1], np.float64, True, "none")["omega"]
    assert sorted(zip(*np.nonzero(np.isnan(nb)))) == [(0, 2, 5)]
    assert np.array_equal(nb[0, :2], om[0, :2]) and np.array_equal(nb[1], om[1])
    # one row further in, the NaN reaches the row beside the pole: the pole row's mean leaves that node out and stays finite
    bad = u.copy()
    bad[0, 2, 5] = np.nan
    nb = L.vorticity(bad, v, lat[0], lat[-1], lon[0], lon[-1], np.float64, True, "none")["omega"]
    assert sorted(zip(*np.nonzero(np.isnan(nb)))) == [(0, 1, 5), (0, 3, 5)]
    assert np.all(np.isfinite(nb[0, 0])) and nb[0, 0, 0] != om[0, 0, 0] and np.array_equal(nb[1], om[1])
    # a NaN in v on the seam column of a cyclic grid reaches across the seam; on the corner of an open grid it stays in its row
    bad = v.copy()
    bad[1, 7, 0] = np.nan
    nb = L.vorticity(u, bad, lat[0], lat[-1], lon[0], lon[-1], np.float64, True, "none")["omega"]
    assert sorted(zip(*np.nonzero(np.isnan(nb)))) == [(1, 7, 1), (1, 7, 35)]
    nb = L.vorticity(u, bad, lat[0], lat[-1], lon[0], lon[-1], np.float64, False, "none")["omega"]
    assert sorted(zip(*np.nonzero(np.isnan(nb)))) == [(1, 7, 0), (1, 7, 1)]
    # no finite node at all: the mean is NaN
    assert np.isnan(L.vorticity(u * np.nan, v, lat[0], lat[-1], lon[0], lon[-1], np.float64, True, "none")["level_mean"]).all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_error_measure_of_the_test_records(dtype):
    """E on the records the GPU tests use: a small fraction of the output's scale (the issue's CPU trial: 1e-11 against 2e-5 1/s in
    float32), and never 0 on them."""
    for (ny, nx), poles in (((4, 4), False), ((5, 7), False), ((33, 130), False), ((19, 36), True)):
        u, v, lat, lon = L.wind_case(ny, nx, 3, dtype, poles)
        box = (lat[0], lat[-1], lon[0], lon[-1])
        a = L.vorticity(u, v, *box, dtype, True)["omega"]
        j = L.vorticity(u, v, *box, np.longdouble, True)["omega"]
        scale = L.vorticity_scale(u, v, *box)
        E = L.error_measure(a, j, dtype, scale)
        assert 0 < E <= 64 * np.finfo(dtype).eps * scale, (ny, nx, E, scale)


# ------------------------------------------------------------------ the fold restatement
def test_hand_worked_fold_records():
    for tx, ty, c, dt, (lavd, rot, length) in L.hand_cases():
        acc, a, r, ln = L.fold(tx, ty, c, dt, np.float64)
        np.testing.assert_allclose(a.ravel(), [lavd], rtol=1e-14)
        np.testing.assert_allclose(r.ravel(), [rot], rtol=1e-14, atol=1e-22)
        np.testing.assert_allclose(ln.ravel(), [length], rtol=1e-11)
        assert np.array_equal(acc[2].astype(np.float64), ln)
        only = L.fold(tx, ty, None, dt, np.float64)
        assert only[1] is None and only[2] is None and np.array_equal(only[3], ln)
    cases = list(L.hand_cases())
    assert cases[0][0].shape[0] == 2                                        # two levels
    _, a, r, _ = L.fold(*cases[1][:4], np.float64)
    assert a[0, 0] > 0 and r[0, 0] == 0                                      # lavd != |rotation| where c changes sign
    assert abs(cases[2][0][1, 0, 0] - cases[2][0][0, 0, 0]) == 359           # the seam step: the raw difference is the long way round


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_fold_is_split_invariant_and_a_nan_stays_in_its_parcel(dtype):
    tx, ty, c = L.walk_case(17, (7, 5), dtype)
    whole = L.fold(tx, ty, c, -900.0, dtype)
    for block in (1, 3, 5, 16):
        cut = L.fold_in_blocks(tx, ty, c, -900.0, dtype, block)
        assert all(np.array_equal(a, b) for a, b in zip(cut, whole)), block
    assert np.all(np.isfinite(whole[0])) and np.all(whole[1] >= np.abs(whole[2])) and np.any(whole[1] > 1.01 * np.abs(whole[2]))
    # the walks do what they are for: a raw longitude step near 360 (the seam), a parcel within a degree of a pole
    assert np.abs(np.diff(tx.astype(np.float64), axis=0)).max() > 350 and np.abs(ty).max() > 89
    bad_c = c.copy()
    bad_c[4, 2, 3] = np.nan
    got = L.fold(tx, ty, bad_c, -900.0, dtype)
    hit = np.zeros((7, 5), bool)
    hit[2, 3] = True
    assert np.array_equal(np.isnan(got[1]), hit) and np.array_equal(np.isnan(got[2]), hit) and np.array_equal(got[3], whole[3])
    bad_x = tx.copy()
    bad_x[9, 6, 0] = np.nan
    got = L.fold(bad_x, ty, c, -900.0, dtype)
    hit = np.zeros((7, 5), bool)
    hit[6, 0] = True
    assert np.array_equal(np.isnan(got[3]), hit) and np.array_equal(got[1], whole[1]) and np.array_equal(got[2], whole[2])


# ------------------------------------------------------------------ the physical check: a vortex is a LAVD maximum
def test_a_moving_vortex_is_the_lavd_maximum_of_the_oracle_chain():
    """The regional box at 0.5 degrees, 25 levels of 900 s, SETTLS order 2, interpolation order 1, pointwise clamp: the oracle's
    trajectories, the numpy vorticity deviation sampled along them by the oracle's xr_map_coordinates, the numpy fold.  Measured:
    the maximum at (-20.5, -55.0), 5.93, against a median of 0.084."""
    u, v, lat, lon = L.vortex_record(0.5, 25)
    assert lat.size == 81 and lon.size == 101
    lavd, rot, length, tx, ty = L.oracle_chain(u, v, lat, lon, order=1)
    where, top, median = L.physical_assertions(lavd, lat, lon)
    print(f"LAVD maximum {top:.3f} at {where}, median {median:.4f}")
    # the vortex turns one way: the rotation there has the LAVD's size, and the parcels in it travel several times as far as most (measured: 2400 km against a median of 480 km)
    j, i = np.unravel_index(np.argmax(lavd), lavd.shape)
    assert abs(rot[j, i]) > 0.9 * lavd[j, i]
    assert length[j - 4:j + 5, i - 4:i + 5].max() > 3 * np.median(length)
