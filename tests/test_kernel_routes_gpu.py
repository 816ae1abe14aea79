"""Every route of tests/kernel_routes.py forced on the GPU, its kernel name asserted, its result compared with the
float64 CPU oracle (oracle/lcs_oracle.py) and, where the table names one, with its direct-gather sibling bit for bit.

Inputs (kernel_routes.FLOW ...): a smooth global flow (flows.era5_like at 5 degrees), a 45 x 76 seed grid (ragged
against every tile shape, global first and last rows included), 10 steps in level chunks of 4, both signs of the
time step; parcels cross +-180 (cyclic) or leave the box (pointwise / outer clamp).  On this flow the oracle itself
moves by <= 6e-12 degrees when the seeds shift by 1e-12 degrees, so the float64 bounds below measure the kernels.

Every route runs on the three longitude grids of kernel_routes.GRIDS: the flow's own (-180 ... 175, test ids as before the
grids were added) and two with the +-180 meridian inside the field (``name@e0``, ``name@seam_inside``), where the reference's
hard-coded wrap (Q7) happens in the field's interior.  There the float32 band leaves out the seeds whose float64 oracle
position comes within 1e-2 degrees of +-180 at any update (tests/_seam.py; at most 1 % of them)."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import lcs_oracle as O
from tests import _seam as S
from tests import kernel_routes as KR
from tests._fullsize import band, lon_err, positions_check

pytestmark = pytest.mark.gpu

ADVECT = [n for n in KR.ROUTES if not n.startswith("sigma")]
SIGMA = [n for n in KR.ROUTES if n.startswith("sigma")]
_ENGINES = {}
FLOORS32 = (5e-6, 5e-5, 5e-4)          # float32 band floors (median, p99, max) in degrees, 10 steps


@pytest.fixture(scope="module", autouse=True)
def _engines():
    yield
    for e in _ENGINES.values():
        e.close()
    _ENGINES.clear()


def _engine(monkeypatch, env):
    """One Engine per distinct tuple of context-creation knobs (read once, in lc_ctx_create)."""
    key = tuple(sorted(env.items()))
    if key not in _ENGINES:
        for k in KR.ENV_KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        from lagrangiancoherence_amd.engine import Engine
        _ENGINES[key] = Engine(0)
    return _ENGINES[key]


class _Setters:
    """Apply a route's context setters; restore the defaults afterwards (the engines are shared)."""
    RESET = {"set_lds_tiles": -1, "set_verify": 0, "set_level_chunk": -1, "set_sigma_march": -1, "set_f64_fidelity": "auto"}

    def __init__(self, eng, setters):
        self.eng, self.setters = eng, dict(setters)

    def __enter__(self):
        for k, v in self.setters.items():
            getattr(self.eng, k)(v)

    def __exit__(self, *exc):
        for k in list(self.setters) + ["set_level_chunk", "set_lds_tiles"]:
            getattr(self.eng, k)(self.RESET[k])


def _np(t):
    return t.detach().cpu().numpy()


_flow64 = S.flow64
_inputs = S.inputs           # (kind, grid="m180")


@functools.lru_cache(maxsize=None)
def _oracle(kind, order, K, dt, xmode, t0, arith, grid="m180"):
    """Oracle trajectories (nsteps + 1, ny, nx) on the route's inputs in `arith` arithmetic."""
    u, v, lat, lon, slat, slon = _inputs(kind, grid)
    if arith == "float64" and kind == "float32":
        u, v, lat, lon, slat, slon = (a.astype(np.float64) for a in (u, v, lat, lon, slat, slon))
    kw = dict(timestep=dt, SETTLS_order=K, interp_order=order, cyclic_xboundary=xmode == "cyclic", return_traj=True,
              t0=t0, nsteps=KR.NSTEPS, noncyclic_clamp="pointwise" if xmode == "pointwise" else "reference_outer")
    return O.parcel_propagation(u, v, lat, lon, seed_lat=slat, seed_lon=slon, **kw)


_FIELDS = {}


def _field(eng, r, grid="m180"):
    key = (id(eng), r["dtype"], r["order"], tuple(sorted(r["prepare"].items())), grid)
    if key not in _FIELDS:
        u, v, lat, lon, _, _ = _inputs(r["dtype"], grid)
        _FIELDS[key] = eng.prepare_field(u, v, lat, lon, r["order"], **r["prepare"])
    return _FIELDS[key]


def _xkw(xmode):
    return dict(cyclic_xboundary=xmode == "cyclic", noncyclic_clamp=None if xmode == "cyclic" else xmode)


def _run(eng, r, field, K, dt, grid="m180"):
    """The route's call.  Returns (name, [(t0, x, y, traj_x or None, traj_y or None) per member])."""
    _, _, _, _, slat, slon = _inputs(r["dtype"], grid)
    order, call, M = r["order"], r["call"], r["members"]
    if call == "advect":
        res = eng.advect(field, slat, slon, dt, K, order, t0=KR.T0, nsteps=KR.NSTEPS, return_traj=r["traj"], **_xkw(r["xmode"]))
        out = [(KR.T0,) + tuple(res) + ((None, None) if not r["traj"] else ())]
    elif call == "batch":
        x, y = eng.advect_batch(field, slat, slon, dt, M, KR.NSTEPS, K, order, True, t0=KR.T0, t0_stride=1)
        out = [(KR.T0 + m, x[m], y[m], None, None) for m in range(M)]
    elif call == "abi_batch":
        # the C ABI's ensemble form with the per-point clamp (Engine.advect_batch is cyclic only)
        from lagrangiancoherence_amd import _capi
        sl, so = eng.to_device(slat, field.dtype), eng.to_device(slon, field.dtype)
        ny, nx = sl.numel(), so.numel()
        x, y = eng._empty((M, ny, nx), field.dtype), eng._empty((M, ny, nx), field.dtype)
        a = eng._advect_args(field, order, sl, ny, so, nx, dt, K, _capi.LC_X_CLAMP_POINT, row0=0, ny_global=ny, t0=KR.T0,
                             nsteps=KR.NSTEPS, n_members=M, t0_stride=1, out=(x, y))
        _capi.check(eng.lib.lc_advect_ex(eng.ctx, C.byref(a)), eng.lib)
        out = [(KR.T0 + m, x[m], y[m], None, None) for m in range(M)]
    elif call == "series":
        s = eng.lcs_series(field, slat, slon, dt, KR.NSTEPS, M, t0=KR.T0, t0_stride=1, SETTLS_order=K, interp_order=order,
                           cyclic_xboundary=False)
        out = [(KR.T0 + m, s["x_dep"][m], s["y_dep"][m], None, None) for m in range(M)]
    else:
        raise AssertionError(call)
    eng.synchronize()
    return eng.last_advect_kernel(), out


def _compare(eng, r, field, K, dt, t0, x, y, tx, ty, label, grid="m180"):
    kind, order, xmode = r["dtype"], r["order"], r["xmode"]
    xg, yg = _np(x).astype(np.float64), _np(y).astype(np.float64)
    o64 = _oracle(kind, order, K, dt, xmode, t0, "float64", grid)
    if r["tol"] in ("exact64", "fast64"):
        tol = KR.TOL[r["tol"]]
        ex, ey = lon_err(xg, o64[0][-1]).max(), np.abs(yg - o64[1][-1]).max()
        assert max(ex, ey) <= tol, f"{label}: |dx| {ex:.2e} |dy| {ey:.2e} > {tol:.0e} degrees"
        if tx is not None:
            et = max(lon_err(_np(tx), o64[0]).max(), np.abs(_np(ty) - o64[1]).max())
            assert et <= tol, f"{label}: trajectories off by {et:.2e} degrees"
        return
    o32 = _oracle(kind, order, K, dt, xmode, t0, "float32", grid)
    _, _, _, _, slat, slon = _inputs(kind, grid)
    ny, nx = KR.SEEDS
    leave_out = None
    if grid != "m180" and xmode == "cyclic":
        # float32 and float64 can wrap a parcel that comes this close to +-180 on different iterations, and then sample two
        # cells apart: left out of the statistics, at most 1 % of the seeds
        leave_out = S.near_seam(kind, order, K, dt, t0, grid)
        assert leave_out.sum() <= leave_out.size // 100, f"{label}: {leave_out.sum()} seeds near +-180"
    keep = positions_check(eng, field, slat, slon, np.arange(ny), np.arange(nx), xg, yg, (o32[0][-1], o32[1][-1]),
                           (o64[0][-1], o64[1][-1]), label, FLOORS32, interp_order=order, leave_out=leave_out, K=K,
                           timestep=dt, t0=t0, nsteps=KR.NSTEPS)
    if tx is not None:
        txg, tyg = _np(tx).astype(np.float64), _np(ty).astype(np.float64)
        eg = np.maximum(lon_err(txg, o64[0]), np.abs(tyg - o64[1]))[:, keep]
        eo = np.maximum(lon_err(o32[0], o64[0]), np.abs(o32[1].astype(np.float64) - o64[1]))[:, keep]
        band(eg, eo, f"{label} trajectories", *FLOORS32)


def _same_bits(a, b):
    return all(eng_equal(p, q) for p, q in zip(a, b))


def eng_equal(p, q):
    if p is None or q is None:
        return p is None and q is None
    import torch
    return torch.equal(p, q)


def _cases(names):
    """(route, grid) per test case: the ``m180`` cases first under the route's bare name, then ``name@grid``."""
    return [pytest.param((n, g), id=n if g == "m180" else f"{n}@{g}") for g in KR.GRIDS for n in names]


@pytest.mark.parametrize("case", _cases([n for n in ADVECT if KR.ROUTES[n]["call"] != "tracer"]))
def test_advect_route_vs_oracle(monkeypatch, case):
    name, grid = case
    r = KR.ROUTES[name]
    want = KR.name_on(r, grid)
    eng = _engine(monkeypatch, r["env"])
    field = _field(eng, r, grid)
    for K in KR.grid_ks(r, grid):
        for dt in KR.TIMESTEPS:
            label = f"{name} K={K} dt={dt:+.0f}" + ("" if grid == "m180" else f" {grid}")
            with _Setters(eng, dict(r["setters"], set_level_chunk=KR.LEVEL_CHUNK)):
                got, out = _run(eng, r, field, K, dt, grid)
                if "set_verify" in r["setters"]:
                    audit = eng.read_verify()
                    assert audit["tile_changed"] == 0 and audit["entries_changed"] == 0, (label, audit)
            assert got == want, f"{label}: dispatched {got}"
            if r["call"] == "advect" and r["xmode"] != "reference_outer":
                assert eng.last_advect_launches() >= 3, f"{label}: {eng.last_advect_launches()} launches, not level chunks"
            for m, (t0, x, y, tx, ty) in enumerate(out):
                _compare(eng, r, field, K, dt, t0, x, y, tx, ty, f"{label} member {m}" if len(out) > 1 else label, grid)
            if r["sibling"]:
                with _Setters(eng, dict(r["setters"], set_lds_tiles=0, set_level_chunk=KR.LEVEL_CHUNK)):
                    sib, out2 = _run(eng, r, field, K, dt, grid)
                assert sib == r["sibling"], f"{label}: sibling dispatched {sib}"
                for (_, *a), (_, *b) in zip(out, out2):
                    assert _same_bits(a, b), f"{label}: differs from {sib} bit for bit"


def test_outer_clamp_routes_leave_the_box(monkeypatch):
    """The outer-clamp routes only report their sub-step kernels if a parcel left the box: make sure one does."""
    u, v, lat, lon, slat, slon = _inputs("float64")
    for dt in KR.TIMESTEPS:
        x, y = _oracle("float64", 1, 0, dt, "pointwise", KR.T0, "float64")
        assert np.any(x[1:] == lon[-1]) or np.any(x[1:] == lon[0]), dt
        xc, _ = _oracle("float64", 1, 0, dt, "cyclic", KR.T0, "float64")
        x0 = np.meshgrid(slon, slat)[0]
        assert np.any(np.abs(xc[-1] - x0) > 180.0), dt        # cyclic parcels cross +-180


# ------------------------------------------------------------------ tracers
def _oracle_levels(c, lat, lon, tx, ty, t0, order):
    return np.stack([O.xr_map_coordinates(c[t0 + i], lat, lon, tx[i], ty[i], order=order) for i in range(tx.shape[0])])


@pytest.mark.parametrize("case", _cases([n for n in ADVECT if KR.ROUTES[n]["call"] == "tracer"]))
def test_tracer_route_vs_oracle(monkeypatch, case):
    name, grid = case
    r = KR.ROUTES[name]
    eng = _engine(monkeypatch, r["env"])
    kind, order = r["dtype"], r["order"]
    u, v, lat, lon, slat, slon = _inputs(kind, grid)
    c64 = np.hypot(_flow64()[0], _flow64()[1]) + 20.0 * np.cos(np.deg2rad(_flow64()[2]))[None, :, None]
    field = _field(eng, r, grid)
    tr = eng.prepare_tracer(c64.astype(field.dtype), None, lat, lon, order, dtype=field.dtype)
    crange = float(c64.max() - c64.min())
    for K in KR.grid_ks(r, grid):
        for dt in KR.TIMESTEPS:
            label = f"{name} K={K} dt={dt:+.0f}" + ("" if grid == "m180" else f" {grid}")
            with _Setters(eng, {"set_level_chunk": KR.LEVEL_CHUNK}):
                res = eng.advect_tracer(field, tr, slat, slon, dt, K, order, True, t0=KR.T0, nsteps=KR.NSTEPS,
                                        return_traj=True, tracer_traj=True)
            assert eng.last_tracer_kernel() == name, f"{label}: {eng.last_tracer_kernel()}"
            cg, mean = _np(res["c"]).astype(np.float64), _np(res["mean"]).astype(np.float64)
            if kind == "float64":
                tx, ty = _oracle(kind, order, K, dt, "cyclic", KR.T0, "float64", grid)
                want = _oracle_levels(c64, lat, lon, tx, ty, KR.T0, order)
                tol = 1e-10 * crange
                assert np.abs(cg - want).max() <= tol, (label, np.abs(cg - want).max())
                assert np.abs(mean - want.mean(axis=0)).max() <= tol, label
            else:
                # on the GPU's own trajectories, inside the float32 oracle's own error there
                txg, tyg = _np(res["traj_x"]), _np(res["traj_y"])
                want = _oracle_levels(c64, lat.astype(np.float64), lon.astype(np.float64), txg.astype(np.float64),
                                      tyg.astype(np.float64), KR.T0, order)
                o32 = _oracle_levels(c64.astype(np.float32), lat, lon, txg, tyg, KR.T0, order)
                e_gpu, e_or = np.abs(cg - want).max(), np.abs(o32 - want).max()
                assert e_gpu <= 4 * e_or + 1e-6 * crange, (label, e_gpu, e_or)
                assert np.abs(mean - want.mean(axis=0)).max() <= 4 * e_or + 1e-6 * crange, label


# ------------------------------------------------------------------ sigma
def _sigma_inputs(ny, nx, lat_edge, seed, nan=False):
    rng = np.random.default_rng(seed)
    lat = np.linspace(-lat_edge, lat_edge, ny)
    lon = -180.0 + (360.0 / nx) * np.arange(nx)
    X, Y = np.meshgrid(lon, lat)
    xd = X + rng.uniform(-3, 3, X.shape)
    yd = np.clip(Y + rng.uniform(-3, 3, X.shape), -90.0, 90.0)
    if nan:
        xd[ny // 2, nx // 2] = np.nan
    return lat, lon, xd, yd


def _sigma_ref(xd, yd, lat, lon, cast, layout):
    return O.sigma_max(O.flowmap_gradient(xd, yd, lat, lon, fd_fp32_cast=cast), layout)


def _sigma_check(r, got, xd, yd, lat, lon, layout, label, tensor=False):
    cast = r["fd_fp32_cast"]
    ref_fn = (lambda *a: O.flowmap_gradient(*a[:4], fd_fp32_cast=cast)) if tensor else \
        (lambda *a: _sigma_ref(*a[:4], cast, layout))
    if r["dtype"] == "float64":
        ref = ref_fn(xd, yd, lat, lon)
        assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{label}: NaN footprint"
        ok = ~np.isnan(ref)
        rtol = KR.TOL[r["tol"]]
        err = np.abs(got[ok] - ref[ok]) / np.maximum(np.abs(ref[ok]), np.abs(ref[ok]).max() * 1e-12 if tensor else 0)
        assert err.max() <= rtol, f"{label}: relative error {err.max():.2e} > {rtol:.0e}"
        return
    f32 = np.float32
    ref = ref_fn(*(a.astype(f32).astype(np.float64) for a in (xd, yd, lat, lon)))
    o32 = ref_fn(*(a.astype(f32) for a in (xd, yd, lat, lon)))
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{label}: NaN footprint"
    ok = ~np.isnan(ref)
    scale = np.abs(ref[ok]).max()
    e_gpu = np.abs(got[ok] - ref[ok]).max() / scale
    e_or = np.abs(o32[ok].astype(np.float64) - ref[ok]).max() / scale
    assert e_gpu <= 4 * e_or + 1e-6, f"{label}: error {e_gpu:.2e}, float32 oracle's own {e_or:.2e}"


@pytest.mark.parametrize("name", SIGMA)
def test_sigma_route_vs_oracle(monkeypatch, name):
    r = KR.ROUTES[name]
    eng = _engine(monkeypatch, r["env"])
    dt = np.dtype(r["dtype"])
    cases = [(ny, nx, edge, nan) for nx in r["widths"] for ny in KR.SIGMA_ROWS for edge in (90.0, 89.5)
             for nan in (False, True) if not (nan and nx < 5)]
    for i, (ny, nx, edge, nan) in enumerate(cases):
        lat, lon, xd, yd = _sigma_inputs(ny, nx, edge, 100 + i, nan)
        dlat, dlon = float(lat[1] - lat[0]), float(lon[1] - lon[0])
        a = [q.astype(dt) for q in (xd, yd, lat)]
        for layout in ("reference", "physical"):
            label = f"{name} {ny}x{nx} +-{edge} nan={nan} {layout}"
            with _Setters(eng, r["setters"]):
                if r["call"] == "sigma":
                    got = eng.sigma(a[0], a[1], a[2], dlat, dlon, fd_fp32_cast=r["fd_fp32_cast"], tensor_layout=layout)
                elif r["call"] == "batch":
                    got = eng.sigma_batch(np.stack([a[0], a[0][::-1].copy()]), np.stack([a[1], a[1]]), a[2], dlat, dlon,
                                          fd_fp32_cast=r["fd_fp32_cast"], tensor_layout=layout)
                else:
                    got = eng.flowmap_gradient(a[0], a[1], a[2], dlat, dlon, fd_fp32_cast=r["fd_fp32_cast"])
                eng.synchronize()
                assert eng.last_sigma_kernel() == name, f"{label}: {eng.last_sigma_kernel()}"
            got = _np(got).astype(np.float64)
            if r["call"] == "batch":
                _sigma_check(r, got[0], xd, yd, lat, lon, layout, label + " member 0")
                _sigma_check(r, got[1], xd[::-1], yd, lat, lon, layout, label + " member 1")
            else:
                _sigma_check(r, got, xd, yd, lat, lon, layout, label, tensor=r["call"] == "tensor")
            if r["call"] == "tensor":
                break
    if r["call"] != "sigma":
        return
    # a row window with its 2-row halo: rows [4, 9) of 13 from input rows [2, 11), against the whole grid's oracle
    for nx in r["widths"]:
        lat, lon, xd, yd = _sigma_inputs(13, nx, 89.5, 7)
        dlat, dlon = float(lat[1] - lat[0]), float(lon[1] - lon[0])
        a = [q.astype(dt) for q in (xd, yd, lat)]
        with _Setters(eng, r["setters"]):
            blk = eng.sigma(a[0][2:11].copy(), a[1][2:11].copy(), a[2][2:11].copy(), dlat, dlon, ny_global=13, in_row0=2,
                            out_row0=4, n_out_rows=5, fd_fp32_cast=r["fd_fp32_cast"])
            eng.synchronize()
            assert eng.last_sigma_kernel() == name
            full = eng.sigma(a[0], a[1], a[2], dlat, dlon, fd_fp32_cast=r["fd_fp32_cast"])
        assert np.array_equal(_np(blk), _np(full)[4:9]), f"{name} window nx={nx}"
        full_ref = _sigma_ref(xd, yd, lat, lon, r["fd_fp32_cast"], "reference") if r["dtype"] == "float64" else None
        if full_ref is not None:
            np.testing.assert_allclose(_np(blk), full_ref[4:9], rtol=KR.TOL[r["tol"]], atol=0)
