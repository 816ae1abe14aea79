"""The auxiliary-grid FTLE on the GPU (``lc_aux_gradient``, ``Engine.aux_gradient``, ``Engine.lcs_aux``, ``LCS(aux_grid=)``).

The expected value never comes from the engine: the kernel is judged by the numpy restatement of its formulas in
``np.longdouble`` (tests/aux_gradient.py) and by ``sin(k d) / (k d)``, the exact stretch of the identity map; the pipeline by
the CPU oracle's ``parcel_propagation`` on the four shifted seed grids fed to that restatement.

Measured on an MI355X (this file's own prints): see the docstrings of the float32 and end-to-end tests."""
import ctypes as C

import numpy as np
import pandas as pd
import pytest

from lagrangiancoherence_amd import _capi
from tests import _fullsize as FS
from tests import _strain as S
from tests import aux_gradient as AG
from tests import labelled

pytestmark = pytest.mark.gpu

POS_ATOL64 = 1e-9       # tests/test_gpu_parity.py, tests/test_series_gpu.py: float64 positions of the advect routes against the oracle
K = np.pi / 180
OUTS = ("sigma", "s1", "s2", "e_lon", "e_lat")
GRIDS = [(37, 64, 1), (7, 5, 1), (33, 130, 3)]        # odd tile remainders, smaller than a block, several blocks x 3 members


@pytest.fixture(scope="module")
def eng():
    from lagrangiancoherence_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _np(t):
    return t.detach().cpu().numpy()


def _same(a, b):
    return np.array_equal(_np(a), _np(b), equal_nan=True)


def _case(ny, nx, n, delta, dtype, fmap=AG.smooth_map, lat_edge=89.75):
    """(lat, lon, seeds, planes) of ``fmap`` on a global grid; member m of a batch is the map of the seeds moved m * 7 degrees
    east and squeezed towards the equator, so the members differ."""
    from lagrangiancoherence_amd.engine import Engine
    lat, lon, box = AG.global_grid(ny, nx, dtype, lat_edge)
    seeds = Engine.aux_seeds(lat, lon, delta, box, dtype)
    assert seeds.row_valid.all() and seeds.col_valid.all()
    members = [AG.planes_of_map(lambda x, y, m=m: fmap(x + 7 * m, y * (1 - 0.05 * m)), lat, lon, seeds, dtype) for m in range(n)]
    planes = {k: (np.stack([p[k] for p in members]) if n > 1 else members[0][k]) for k in AG.PLANES}
    return lat, lon, seeds, planes


def _run(eng, lat, seeds, planes, want=OUTS, layout="physical"):
    got = eng.aux_gradient(planes, lat, seeds.sep_lat, seeds.sep_lon, want=want, tensor_layout=layout)
    return {k: _np(v) for k, v in got.items()}


# ------------------------------------------------------------------ 1. the identity map, float64
@pytest.mark.parametrize("ny,nx,n", GRIDS)
@pytest.mark.parametrize("delta", [0.01, 0.25])
def test_identity_map_float64(eng, ny, nx, n, delta):
    lat, lon, seeds, planes = _case(ny, nx, 1, delta, np.float64, AG.identity_map)
    assert lat[0] == -89.75 and lat[-1] == 89.75 and lon[0] == -180.0
    got = _run(eng, lat, seeds, planes)
    assert eng.last_aux_kernel() == "aux_gradient_kernel<double>"
    want = np.sin(K * delta) / (K * delta)
    e1, e2 = np.abs(got["s1"] - want).max(), np.abs(got["s2"] - want).max()
    print(f"identity {ny}x{nx} delta {delta}: |s1 - sinc| {e1:.2e} |s2 - sinc| {e2:.2e}")
    assert e1 <= 1e-13 and e2 <= 1e-13
    assert np.array_equal(got["sigma"], got["s1"])              # the physical layout's sigma IS s1


# ------------------------------------------------------------------ 2. the analytic map, float64, against longdouble
@pytest.mark.parametrize("ny,nx,n", GRIDS)
@pytest.mark.parametrize("delta", [0.01, 0.25])
def test_analytic_map_float64_against_longdouble(eng, ny, nx, n, delta):
    lat, lon, seeds, planes = _case(ny, nx, n, delta, np.float64)
    got = _run(eng, lat, seeds, planes)
    ref = AG.restatement(planes, lat, seeds.sep_lat, seeds.sep_lon, np.longdouble)
    assert all(got[k].dtype == np.float64 and got[k].shape == planes["x_e"].shape and np.isfinite(got[k]).all() for k in OUTS)
    e1 = np.abs((got["s1"] - ref["s1"]) / ref["s1"]).max()
    e2 = np.abs((got["s2"] - ref["s2"]) / ref["s1"]).max()
    ex, ey = got["e_lon"], got["e_lat"]
    unit = np.abs(np.hypot(ex, ey) - 1.0).max()
    tens = np.stack(AG.derivatives(planes, lat, seeds.sep_lat, seeds.sep_lon, np.longdouble)).astype(np.float64)
    res = (S.eigen_residual(tens, ex, ey, got["s1"] ** 2) / got["s1"] ** 2).max()
    print(f"analytic {ny}x{nx}x{n} delta {delta}: s1 {float(e1):.2e} s2/s1 {float(e2):.2e} |e|-1 {unit:.2e} residual {res:.2e}")
    assert e1 <= 1e-13 and e2 <= 1e-13
    assert np.all(got["s1"] >= got["s2"]) and np.all(got["s2"] > 0)
    assert unit <= 1e-12 and S.sign_convention_holds(ex, ey) and res <= 1e-8        # the strain tests' rules and bounds
    assert np.array_equal(got["sigma"], got["s1"])
    for layout in ("reference", "physical"):
        sig = _run(eng, lat, seeds, planes, want=("sigma",), layout=layout)["sigma"]
        rs = AG.restatement(planes, lat, seeds.sep_lat, seeds.sep_lon, np.longdouble, layout)["sigma"]
        assert np.abs((sig - rs) / rs).max() <= 1e-13, layout
    assert np.abs(ref["sigma"] - AG.restatement(planes, lat, seeds.sep_lat, seeds.sep_lon, np.longdouble, "reference")["sigma"]).max() > 1e-3


# ------------------------------------------------------------------ 3. the analytic map, float32
@pytest.mark.parametrize("ny,nx,n", GRIDS)
@pytest.mark.parametrize("delta", [0.01, 0.25])
def test_analytic_map_float32(eng, ny, nx, n, delta):
    """Inputs rounded to float32, the expected value longdouble on those inputs.  The bound on s1 is 4 x the largest error the
    numpy float32 restatement shows on the same inputs (the margin covers the device's sin / cos); the naive float32 Cartesian
    difference misses that bound at delta = 0.01, which is what the half-angle form is for.  Rows to +-70 degrees.
    Measured on an MI355X, 37 x 64: device 4.98e-07 at delta 0.01 and 5.54e-07 at 0.25, the numpy float32 restatement the same to
    three digits (bounds 1.99e-06, 2.22e-06); largest over the three grids 5.95e-07; naive 1.25e-03 at 0.01, 3.88e-05 at 0.25."""
    lat, lon, seeds, planes = _case(ny, nx, n, delta, np.float32, lat_edge=70.0)
    assert all(planes[k].dtype == np.float32 for k in AG.PLANES)
    got = _run(eng, lat, seeds, planes)
    assert eng.last_aux_kernel() == "aux_gradient_kernel_f32"
    assert all(got[k].dtype == np.float32 and np.isfinite(got[k]).all() for k in OUTS)
    ref = AG.restatement(planes, lat, seeds.sep_lat, seeds.sep_lon, np.longdouble)
    rel = lambda s1: float(np.abs((s1.astype(np.longdouble) - ref["s1"]) / ref["s1"]).max())
    own = rel(AG.restatement(planes, lat, seeds.sep_lat, seeds.sep_lon, np.float32)["s1"].astype(np.float32))
    dev = rel(got["s1"])
    naive = rel(AG.naive(planes, lat, seeds.sep_lat, seeds.sep_lon, np.float32)["s1"].astype(np.float32))
    print(f"float32 {ny}x{nx}x{n} delta {delta}: device {dev:.2e}, numpy float32 restatement {own:.2e} (bound {4 * own:.2e}), naive {naive:.2e}")
    assert dev <= 4 * own
    if delta == 0.01:
        assert naive > 4 * own
    rel2 = lambda s2: float(np.abs((s2.astype(np.longdouble) - ref["s2"]) / ref["s1"]).max())      # on the scale of s1
    own2 = rel2(AG.restatement(planes, lat, seeds.sep_lat, seeds.sep_lon, np.float32)["s2"].astype(np.float32))
    print(f"    s2: device {rel2(got['s2']):.2e}, restatement {own2:.2e}")
    assert rel2(got["s2"]) <= 4 * own2
    ex, ey = got["e_lon"].astype(np.float64), got["e_lat"].astype(np.float64)
    assert np.abs(np.hypot(ex, ey) - 1).max() <= 2 * np.finfo(np.float32).eps and S.sign_convention_holds(ex, ey)
    assert np.array_equal(got["sigma"], got["s1"])


# ------------------------------------------------------------------ 4. NaN locality
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_nan_stays_in_its_cell_row_or_column(eng, dtype):
    ny, nx, n = 33, 130, 3
    lat, lon, seeds, planes = _case(ny, nx, n, 0.25, dtype)
    for i, k in enumerate(AG.PLANES):
        m, r, c = i % n, (5 * i + 3) % ny, (37 * i + 1) % nx
        p = {q: v.copy() for q, v in planes.items()}
        p[k][m, r, c] = np.nan
        for layout in ("reference", "physical"):
            got = _run(eng, lat, seeds, p, layout=layout)
            hit = np.zeros((n, ny, nx), bool)
            hit[m, r, c] = True
            for o in OUTS:
                assert np.array_equal(np.isnan(got[o]), hit), (k, layout, o)
    row, col = 32, 129
    sl, so = seeds.sep_lat.copy(), seeds.sep_lon.copy()
    sl[row] = np.nan
    got = {o: _np(v) for o, v in eng.aux_gradient(planes, lat, sl, seeds.sep_lon).items()}
    hit = np.zeros((n, ny, nx), bool)
    hit[:, row, :] = True
    assert all(np.array_equal(np.isnan(got[o]), hit) for o in OUTS)
    so[col] = so[0] = np.nan
    got = {o: _np(v) for o, v in eng.aux_gradient(planes, lat, seeds.sep_lat, so).items()}
    hit = np.zeros((n, ny, nx), bool)
    hit[:, :, [0, col]] = True
    assert all(np.array_equal(np.isnan(got[o]), hit) for o in OUTS)


# ------------------------------------------------------------------ 5. batch and options
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_batch_equals_single_calls_and_unrequested_planes_are_not_written(eng, dtype):
    ny, nx, n = 33, 130, 3
    lat, lon, seeds, planes = _case(ny, nx, n, 0.05, dtype)
    for layout in ("reference", "physical"):
        got = _run(eng, lat, seeds, planes, layout=layout)
        for m in range(n):
            one = _run(eng, lat, seeds, {k: v[m] for k, v in planes.items()}, layout=layout)
            for o in OUTS:
                assert one[o].shape == (ny, nx) and np.array_equal(got[o][m], one[o]), (layout, m, o)
    assert eng.last_aux_kernel() == ("aux_gradient_kernel_f32" if dtype == np.float32 else "aux_gradient_kernel<double>")
    # the order of want is the order of the result, and a mapping or a sequence of planes is the same call
    sub = eng.aux_gradient([planes[k] for k in AG.PLANES], lat, seeds.sep_lat, seeds.sep_lon, want=("e_lat", "s1"), tensor_layout="physical")
    assert list(sub) == ["e_lat", "s1"] and np.array_equal(_np(sub["s1"]), got["s1"]) and np.array_equal(_np(sub["e_lat"]), got["e_lat"])
    with pytest.raises(ValueError, match="want"):
        eng.aux_gradient(planes, lat, seeds.sep_lat, seeds.sep_lon, want=())
    with pytest.raises(ValueError, match="want"):
        eng.aux_gradient(planes, lat, seeds.sep_lat, seeds.sep_lon, want=("s3",))
    # a NULL output is not written: every plane pre-filled with a sentinel, each subset asked for through the C entry itself
    torch = eng.torch
    dev = {k: eng.to_device(v, dtype) for k, v in planes.items()}
    co = [eng.to_device(a, dtype) for a in (lat, seeds.sep_lat, seeds.sep_lon)]
    for subset in (("s2",), ("sigma", "e_lon"), ("s1", "e_lat"), OUTS):
        bufs = {o: torch.full((n, ny, nx), -77.0, dtype=dev["x_e"].dtype, device=eng.device) for o in OUTS}
        a = _capi.AuxGradientArgs(struct_size=C.sizeof(_capi.AuxGradientArgs), dtype=_capi.LC_F32 if dtype == np.float32 else _capi.LC_F64,
                                  ny=ny, nx=nx, n_members=n, seed_lat_dev=co[0].data_ptr(), sep_lat_dev=co[1].data_ptr(),
                                  sep_lon_dev=co[2].data_ptr(), tensor_layout=_capi.LC_LAYOUT_PHYSICAL,
                                  **{k: t.data_ptr() for k, t in dev.items()}, **{o + "_out": bufs[o].data_ptr() for o in subset})
        eng._use_current_stream()
        _capi.check(eng.lib.lc_aux_gradient(eng.ctx, C.byref(a)), eng.lib)
        eng.synchronize()
        for o in OUTS:
            b = _np(bufs[o])
            assert (np.array_equal(b, got[o]) if o in subset else np.all(b == -77.0)), (subset, o)


# ------------------------------------------------------------------ 6. plumbing: the planes are Engine.advect's
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("order", [1, 3])
def test_position_planes_are_advect_on_the_shifted_grids(eng, dtype, order):
    from lagrangiancoherence_amd import flows
    u, v, lat, lon = (a.astype(dtype) for a in flows.config1())
    f = eng.prepare_field(u, v, lat, lon, order)
    kw = dict(SETTLS_order=4, interp_order=order, cyclic_xboundary=True)
    n, nsteps, ts = 2, 5, -21600.0
    res = eng.lcs_aux(f, lat, lon, ts, nsteps, n, t0=1, t0_stride=1, aux_delta=(0.05, 0.1), centre=True, return_planes=True,
                      want=("sigma", "s1"), **kw)
    s = res["seeds"]
    assert s.sep_lat.dtype == dtype and np.nanmax(np.abs(s.sep_lat - 0.1)) < 1e-4 and np.nanmax(np.abs(s.sep_lon - 0.2)) < 1e-4
    grids = {"e": (lat, s.lon_e), "w": (lat, s.lon_w), "n": (s.lat_n, lon), "s": (s.lat_s, lon)}
    for m in range(n):
        for d, (la, lo) in grids.items():
            x, y = eng.advect(f, la, lo, ts, 4, order, True, t0=1 + m, nsteps=nsteps)
            assert _same(res["x_" + d][m], x) and _same(res["y_" + d][m], y), (m, d)
        x, y = eng.advect(f, lat, lon, ts, 4, order, True, t0=1 + m, nsteps=nsteps)
        assert _same(res["x_dep"][m], x) and _same(res["y_dep"][m], y), m
    one = eng.lcs_series(f, lat, lon, ts, nsteps, n, t0=1, t0_stride=1, **kw)
    assert _same(res["x_dep"], one["x_dep"]) and _same(res["y_dep"], one["y_dep"])
    # and the results are the kernel's on those planes
    again = eng.aux_gradient({k: res[k] for k in AG.PLANES}, lat, s.sep_lat, s.sep_lon, want=("sigma", "s1"))
    assert _same(again["sigma"], res["sigma"]) and _same(again["s1"], res["s1"])
    frame = ~(s.row_valid[:, None] & s.col_valid[None, :])
    assert frame[0].all() and frame[-1].all() and frame[:, 0].all() and frame[:, -1].all() and frame.sum() == 2 * 89 + 2 * 180 - 4
    assert np.array_equal(np.isnan(_np(res["sigma"])), np.broadcast_to(frame, (n, *frame.shape)))


# ------------------------------------------------------------------ 7. / 8. end to end against the oracle
E2E = dict(timestep=-21600.0, SETTLS_order=4, interp_order=3, cyclic_xboundary=True)
_ORACLE = {}


def _oracle_sigma(delta, dtype):
    """sigma (reference layout) and s1 of the oracle's planes on the example's shape (89 x 180, 7 steps, order 3, K = 4), the
    planes and the restatement in ``dtype``; computed once per (delta, dtype)."""
    if (delta, dtype) not in _ORACLE:
        from lagrangiancoherence_amd import flows
        from lagrangiancoherence_amd.engine import Engine
        from oracle import lcs_oracle as O
        u, v, lat, lon = (a.astype(dtype) for a in flows.config1())
        seeds = Engine.aux_seeds(lat, lon, delta, (lat.min(), lat.max(), lon.min(), lon.max()), dtype)
        planes = AG.aux_planes_from_oracle(O, u, v, lat, lon, lat, lon, seeds, **E2E)
        T = np.float32 if dtype == np.float32 else np.float64
        _ORACLE[(delta, dtype)] = (seeds, {lay: AG.restatement(planes, lat, seeds.sep_lat, seeds.sep_lon, T, lay)
                                           for lay in ("reference", "physical")})
    return _ORACLE[(delta, dtype)]


@pytest.mark.parametrize("delta", [0.05, 0.25])
def test_end_to_end_float64_against_the_oracle(eng, delta):
    """|sigma - oracle| <= 4 eps / delta, eps = 1e-9 degrees: the position tolerance of the float64 parity tests of this advect
    route (POS_ATOL64).  A position error eps in each of a pair's two parcels moves their difference by at most 2 eps over a
    separation of 2 delta, and sigma is the 2-norm of derivatives of order one; the factor 4 covers both pairs.
    Measured on an MI355X: 2.5e-12 at delta 0.05 (bound 8e-8), 3.1e-13 at 0.25 (bound 1.6e-8), sigma up to 214."""
    from lagrangiancoherence_amd import flows
    u, v, lat, lon = flows.config1()
    assert (u.shape[0] - 1, lat.size, lon.size) == (7, 89, 180)
    f = eng.prepare_field(u, v, lat, lon, 3, fuse_levels=False)        # the oracle's operation order (tests/test_series_gpu.py)
    seeds, ref = _oracle_sigma(delta, np.float64)
    valid = seeds.row_valid[:, None] & seeds.col_valid[None, :]
    assert valid.sum() == 87 * 178
    for layout in ("reference", "physical"):
        got = eng.lcs_aux(f, lat, lon, E2E["timestep"], 7, SETTLS_order=4, interp_order=3, cyclic_xboundary=True, aux_delta=delta,
                          tensor_layout=layout, want=("sigma", "s1", "s2"))
        sig = _np(got["sigma"])[0]
        assert np.array_equal(np.isnan(sig), ~valid) and np.array_equal(np.isnan(ref[layout]["sigma"]), ~valid)
        err = np.abs(sig - ref[layout]["sigma"])[valid].max()
        e1 = np.abs(_np(got["s1"])[0] - ref[layout]["s1"])[valid].max()
        print(f"end to end float64 delta {delta} {layout}: |dsigma| {err:.2e} |ds1| {e1:.2e} bound {4 * POS_ATOL64 / delta:.2e} "
              f"(sigma up to {np.nanmax(sig):.1f})")
        assert err <= 4 * POS_ATOL64 / delta and e1 <= 4 * POS_ATOL64 / delta


@pytest.mark.parametrize("delta", [0.05, 0.25])
def test_end_to_end_float32_in_the_float32_oracles_band(eng, delta):
    """float32 through the engine against the float64 oracle, judged by the numpy float32 oracle's own error against it
    (tests/_fullsize.band: median, 99th percentile, maximum); relative to sigma.  float32 positions carry ulp(180) = 1.5e-5
    degrees, so either error is of order ulp / delta.  Measured on an MI355X (engine | numpy float32 oracle): delta 0.05 median
    6.18e-05 | 6.18e-05, maximum 2.39e-03 | 2.39e-03; delta 0.25 median 1.26e-05 | 1.27e-05, maximum 3.87e-04 | 3.89e-04."""
    from lagrangiancoherence_amd import flows
    u, v, lat, lon = (a.astype(np.float32) for a in flows.config1())
    f = eng.prepare_field(u, v, lat, lon, 3)
    seeds, ref64 = _oracle_sigma(delta, np.float64)
    seeds32, ref32 = _oracle_sigma(delta, np.float32)
    valid = seeds32.row_valid[:, None] & seeds32.col_valid[None, :]
    assert np.array_equal(valid, seeds.row_valid[:, None] & seeds.col_valid[None, :])
    got = eng.lcs_aux(f, lat, lon, E2E["timestep"], 7, SETTLS_order=4, interp_order=3, cyclic_xboundary=True, aux_delta=delta)
    sig = _np(got["sigma"])[0]
    assert sig.dtype == np.float32 and np.array_equal(np.isnan(sig), ~valid)
    truth = ref64["reference"]["sigma"][valid]
    eg = np.abs(sig[valid].astype(np.float64) - truth) / truth
    eo = np.abs(ref32["reference"]["sigma"][valid] - truth) / truth
    eps = float(np.finfo(np.float32).eps)
    FS.band(eg, eo, f"aux sigma float32 delta {delta}", 4 * eps, 4 * eps, 4 * eps)


# ------------------------------------------------------------------ 9. what it fixes
def test_regional_domain_at_rest_stencil_edges_against_the_auxiliary_grid(eng):
    """No wind on a regional box: the flow map is the identity and sigma is 1 everywhere.  The stencil's longitude derivative is
    cyclic whatever the domain (tools.derivative_spherical_coords' isglobal=True), so its two first and last columns difference
    across the whole box; the auxiliary grid gives sin(k d) / (k d) at every cell it can seed and NaN on the frame it cannot."""
    ny, nx, nt, delta = 21, 31, 4, 0.25
    lat, lon = np.linspace(10.0, 30.0, ny), np.linspace(-70.0, -40.0, nx)
    u = np.zeros((nt, ny, nx))
    f = eng.prepare_field(u, u.copy(), lat, lon, 1)
    kw = dict(SETTLS_order=2, interp_order=1, cyclic_xboundary=False, tensor_layout="physical")
    stencil = _np(eng.lcs(f, lat, lon, 3600.0, **kw)["sigma"])
    edge = np.r_[0, 1, nx - 2, nx - 1]
    print(f"at rest: stencil sigma in the edge columns {stencil[:, edge].min():.2f} .. {stencil[:, edge].max():.2f}, "
          f"inside |sigma - 1| <= {np.abs(stencil[2:-2, 2:-2] - 1).max():.1e}")
    assert np.all(np.abs(stencil[:, edge] - 1) > 0.5)                      # the defect, on record
    assert np.abs(stencil[2:-2, 2:-2] - 1).max() < 1e-3
    got = eng.lcs_aux(f, lat, lon, 3600.0, nt - 1, aux_delta=delta, want=("sigma", "s1", "s2"), **kw)
    s = got["seeds"]
    assert s.row_valid.tolist() == [False] + [True] * (ny - 2) + [False] and s.col_valid.tolist() == [False] + [True] * (nx - 2) + [False]
    valid = s.row_valid[:, None] & s.col_valid[None, :]
    want = np.sin(K * delta) / (K * delta)
    for k in ("sigma", "s1", "s2"):
        a = _np(got[k])[0]
        assert np.array_equal(np.isnan(a), ~valid), k
        assert np.abs(a[valid] - want).max() <= 1e-13, k


# ------------------------------------------------------------------ 10. grouping
def _moving_wind(dtype, nt=20, ny=19, nx=61):
    rng = np.random.default_rng(9)
    lat, lon = np.linspace(10.0, 30.0, ny).astype(dtype), np.linspace(-70.0, -40.0, nx).astype(dtype)
    u = (3.0 * rng.standard_normal((nt, ny, nx))).astype(dtype)
    v = (1.5 * rng.standard_normal((nt, ny, nx))).astype(dtype)
    u[10:] = u[10:] * 10 + 40.0          # a jet in the later levels pushes the eastern columns out of the box
    return u, v, lat, lon


@pytest.mark.parametrize("cyclic", [True, False])
def test_memory_capped_groups_give_the_bits_of_one_group(eng, monkeypatch, cyclic):
    u, v, lat, lon = _moving_wind(np.float32)
    f = eng.prepare_field(u, v, lat, lon, 3)
    kw = dict(SETTLS_order=2, interp_order=3, cyclic_xboundary=cyclic, aux_delta=0.1)
    forms = {"series": dict(n_dirs=1, want=("sigma",)), "bidirectional": dict(n_dirs=2, want=("sigma",), centre=True),
             "strain": dict(n_dirs=1, want=("s1", "s2", "e_lon", "e_lat"), centre=True)}
    n, nsteps = 5, 8
    for name, form in forms.items():
        whole = eng.lcs_aux(f, lat, lon, 3600.0, nsteps, n, t0=0, t0_stride=2, **kw, **form)
        seeds = form["n_dirs"] * lat.size * lon.size
        per = (8 + len(form["want"]) + (2 if form.get("centre") else 0) + (0 if cyclic else 4)) * seeds * 4
        assert eng.aux_group(np.float32, seeds, n, cyclic, len(form["want"]), form.get("centre", False)) == n
        keys = [k for k in whole if k != "seeds"]
        assert np.isfinite(_np(whole[form["want"][0]])).any()
        for g in (1, 2):
            monkeypatch.setattr(eng, "SERIES_MEM_CAP", g * per)
            assert eng.aux_group(np.float32, seeds, n, cyclic, len(form["want"]), form.get("centre", False)) == g
            part = eng.lcs_aux(f, lat, lon, 3600.0, nsteps, n, t0=0, t0_stride=2, **kw, **form)
            monkeypatch.undo()
            for k in keys:
                assert _same(whole[k], part[k]), (name, g, k)


def test_lcs_aux_refuses_smoothing_and_bad_arguments(eng):
    u, v, lat, lon = _moving_wind(np.float32, nt=4)
    f = eng.prepare_field(u, v, lat, lon, 1)
    with pytest.raises(ValueError, match="gauss_sigma"):
        eng.lcs_aux(f, lat, lon, 3600.0, 3, aux_delta=0.1, gauss_sigma=1.5)
    with pytest.raises(ValueError, match="delta"):
        eng.lcs_aux(f, lat, lon, 3600.0, 3, aux_delta=0.0)
    with pytest.raises(ValueError, match="n_dirs"):
        eng.lcs_aux(f, lat, lon, 3600.0, 3, aux_delta=0.1, n_dirs=3)
    with pytest.raises(ValueError, match="want"):
        eng.lcs_aux(f, lat, lon, 3600.0, 3, aux_delta=0.1, want=("x_dep",))
    with pytest.raises(TypeError):
        eng.lcs_aux(f, lat, lon, 3600.0, 3)


# ------------------------------------------------------------------ 11. the drop-in
def _record(nt=6, ny=25, nx=33):
    lat = np.linspace(20.0, 30.0, ny).astype(np.float32)
    lon = np.linspace(-60.0, -45.0, nx).astype(np.float32)
    t = np.arange(nt)[:, None, None]
    yy, xx = lat[None, :, None].astype(np.float64), lon[None, None, :].astype(np.float64)
    # a gentle flow: about a degree in the record's 30 hours, so no parcel seeded inside the subdomain reaches the box's edge
    u = ((1.0 + 0.8 * np.sin(0.3 * yy + 0.5 * t) * np.cos(0.2 * xx)) * np.ones((nt, ny, nx))).astype(np.float32)
    v = (0.6 * np.cos(0.25 * xx - 0.4 * t) * np.sin(0.3 * yy) * np.ones((nt, ny, nx))).astype(np.float32)
    times = pd.date_range("2010-01-01", periods=nt, freq="6h").values
    coords = {"latitude": lat, "longitude": lon, "time": times}
    U = labelled.DataArray(u.transpose(1, 2, 0), ["latitude", "longitude", "time"], coords, name="u")
    V = labelled.DataArray(v.transpose(1, 2, 0), ["latitude", "longitude", "time"], coords, name="v")
    return labelled.Dataset({"u": U, "v": V})


def _flat(out):
    res = []
    for o in (out if isinstance(out, tuple) else (out,)):
        res.extend(_flat(o) if isinstance(o, tuple) else [o])
    return res


def _same_labels(a, b):
    assert type(a) is type(b) and a.dims == b.dims and a.name == b.name and a.values.dtype == b.values.dtype and a.shape == b.shape
    assert set(a.coords) == set(b.coords)
    for k in a.coords:
        assert np.array_equal(np.asarray(a.coords[k]), np.asarray(b.coords[k])), k


FORMS = {"call": (lambda L, ds: L(ds, verbose=False, return_traj=True), 5, (1, 2, 3, 4)),
         "series": (lambda L, ds: L.series(ds, window=4, stride=1, verbose=False), 3, (1, 2)),
         "bidirectional": (lambda L, ds: L.bidirectional(ds, verbose=False), 6, (1, 2, 4, 5)),
         "bidirectional_windows": (lambda L, ds: L.bidirectional(ds, window=4, stride=2, verbose=False), 6, (1, 2, 4, 5)),
         "strain": (lambda L, ds: L.strain(ds, window=4, stride=1, verbose=False), 5, (3, 4))}


@pytest.mark.parametrize("form", list(FORMS))
def test_dropin_aux_grid_returns_the_same_labelled_arrays(form):
    """Dims, coords, names, time stamps and dtypes of every call form are the non-aux call's; the departure points and
    trajectories returned are the output grid's, bit for bit the non-aux call's; the values come from the auxiliary grid:
    NaN on the frame within aux_grid of the box's edge, and within the subdomain (which lies inside it) finite and, over most
    of it, close to the stencil's on this smooth flow."""
    from LagrangianCoherence.LCS.LCS import LCS
    call, n_out, centre = FORMS[form]
    ds = _record()
    ctor = dict(timestep=-6 * 3600, SETTLS_order=2, return_dpts=True,
                subdomain={"latitude": slice(21.0, 29.0), "longitude": slice(-58.0, -47.0)})
    plain = _flat(call(LCS(**ctor), ds))
    aux = _flat(call(LCS(**ctor, aux_grid=0.05), ds))
    assert len(plain) == len(aux) == n_out
    for i, (a, b) in enumerate(zip(aux, plain)):
        _same_labels(a, b)
        if i in centre:
            assert np.array_equal(a.values, b.values), i          # the centre grid's departure points / trajectories
        else:
            assert np.isfinite(a.values).all() and not np.array_equal(a.values, b.values), i
            if b.name != "direction":
                # (the median: near the crop's edge the stencil reaches rows whose parcels were clamped at the box's edge)
                assert np.median(np.abs(a.values / b.values - 1)) < 0.01, i
    # without the subdomain crop the frame shows
    whole = _flat(call(LCS(timestep=-6 * 3600, SETTLS_order=2, aux_grid=0.05), ds))[0].values
    frame = np.ones(whole.shape[-2:], bool)
    frame[1:-1, 1:-1] = False
    assert np.array_equal(np.isnan(whole), np.broadcast_to(frame, whole.shape))


def test_dropin_aux_grid_refusals():
    from LagrangianCoherence.LCS.LCS import LCS
    for bad in (0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="aux_grid"):
            LCS(aux_grid=bad)
    with pytest.raises(ValueError, match="gauss_sigma"):
        LCS(aux_grid=0.05, gauss_sigma=2.0)
    L = LCS(timestep=-6 * 3600, aux_grid=0.05)
    L.gauss_sigma = 2.0                                         # set behind the constructor's back: the engine refuses
    with pytest.raises(ValueError, match="gauss_sigma"):
        L(_record(), verbose=False)
