"""Stretch factors and stretching direction on the GPU (``lc_strain``, ``Engine.strain``, ``Engine.lcs_strain``, ``LCS.strain``).

The expected value is always ``oracle.flowmap_gradient`` -> F -> ``numpy.linalg.svd`` (tests/_strain.py), never the engine:

  * float64, both values of ``fd_fp32_cast``, on the golden departure fields of config 1 and on a smooth random perturbation of
    a 37 x 64 seed grid (an odd tile remainder in both directions): ``s1`` at the tensor's own tolerance, ``s2`` at that tolerance
    on the scale of ``s1`` (Weyl), ``s1`` bit-equal to ``Engine.sigma(tensor_layout="physical")``, the direction by its eigen-residual
    on every cell and against numpy's ``v1`` where the spectral gap allows;
  * the rule cases: identity map, one NaN departure point;
  * batches against single calls, the kernel names;
  * the identities that hold because sigma and strain run one gradient core (csrc/flowmap_gradient.h), at every tile and strip edge;
  * float32 inside the band of the float32 oracle's own error around the float64 answer, small fields and a 4096 x 4096 run;
  * the memory-capped grouping of ``lcs_strain`` gives the bits of one group;
  * the drop-in contract of ``LCS.strain``."""
import numpy as np
import pandas as pd
import pytest

from lagrangiancoherence_amd import flows
from tests import _strain as S
from tests import labelled
from tests._fullsize import band, dilate
from tests.test_series_gpu import _diverging_wind

pytestmark = pytest.mark.gpu

KERNELS = {(np.float32, True): "strain_kernel_f32", (np.float32, False): "strain_kernel_f32",
           (np.float64, True): "strain_kernel<double, float>", (np.float64, False): "strain_kernel<double, double>"}
PLANES = ("s1", "s2", "e_lon", "e_lat")


@pytest.fixture(scope="module")
def eng():
    from lagrangiancoherence_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def O():
    from oracle import lcs_oracle
    return lcs_oracle


def _np(t):
    return t.detach().cpu().numpy()


def _fields():
    """name -> (x_dep, y_dep, lat, lon) in float64."""
    _, _, lat, lon = flows.config1()
    out = {name: (*S.golden(name), lat, lon) for name in ("g1_bwd_k4_o3", "g1_fwd_k4_o1")}
    out["perturbed_37x64"] = S.perturbed_seed_grid()
    return out


FIELDS = _fields()


def _strain(eng, x, y, lat, lon, cast=True, want=PLANES):
    res = eng.strain(x, y, lat, float(lat[1] - lat[0]), float(lon[1] - lon[0]), fd_fp32_cast=cast, want=want)
    return {k: _np(v) for k, v in res.items()}


# ------------------------------------------------------------------------------------------ float64
@pytest.mark.parametrize("cast", [True, False])
@pytest.mark.parametrize("name", list(FIELDS))
def test_float64_against_numpy_svd(eng, O, name, cast):
    x, y, lat, lon = FIELDS[name]
    got = _strain(eng, x, y, lat, lon, cast)
    assert eng.last_strain_kernel() == KERNELS[(np.float64, cast)]
    tens = O.flowmap_gradient(x, y, lat, lon, fd_fp32_cast=cast)
    r1, r2, v1 = S.svd_reference(tens)
    s1, s2, ex, ey = (got[k] for k in PLANES)
    assert all(a.dtype == np.float64 and a.shape == x.shape and np.isfinite(a).all() for a in (s1, s2, ex, ey))
    e1, e2 = np.abs(s1 - r1) / r1, np.abs(s2 - r2) / r1
    unit = np.abs(np.hypot(ex, ey) - 1.0)
    res = S.eigen_residual(tens, ex, ey, s1 * s1) / (s1 * s1)
    gap = r2 / r1 <= 0.99
    sine = S.sine_of_angle(ex, ey, v1)[gap]
    print(f"{name} cast={cast}: s1 {e1.max():.2e}  s2/s1 {e2.max():.2e}  |e|-1 {unit.max():.2e}  residual {res.max():.2e}  "
          f"sine {sine.max():.2e}  left out {1 - gap.mean():.4%}")
    # s1 at the tolerance test_subdomain_crop_and_flowmap_gradient gives the tensor itself; s2 at that tolerance on the scale of
    # s1: a perturbation of F moves every singular value by at most its 2-norm (Weyl)
    np.testing.assert_allclose(s1, r1, rtol=1e-9, atol=0)
    assert np.all(np.abs(s2 - r2) <= 1e-9 * r1)
    sig = _np(eng.sigma(x, y, lat, float(lat[1] - lat[0]), float(lon[1] - lon[0]), fd_fp32_cast=cast, tensor_layout="physical"))
    assert np.array_equal(s1, sig)
    # direction
    assert unit.max() <= 1e-12 and S.sign_convention_holds(ex, ey)
    assert res.max() <= 1e-8                                   # every cell, whatever the spectral gap
    assert 1 - gap.mean() <= 0.01 and sine.max() <= 1e-7        # against numpy's v1 where s2 / s1 <= 0.99


# ------------------------------------------------------------------------------------------ rule cases
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_identity_map(eng, dtype):
    _, _, lat, lon = (a.astype(dtype) for a in FIELDS["perturbed_37x64"])
    x, y = np.broadcast_to(lon[None, :], (lat.size, lon.size)).copy(), np.broadcast_to(lat[:, None], (lat.size, lon.size)).copy()
    got = _strain(eng, x, y, lat, lon)
    assert all(np.isfinite(got[k]).all() and got[k].dtype == dtype for k in PLANES)
    np.testing.assert_allclose(np.hypot(got["e_lon"].astype(np.float64), got["e_lat"].astype(np.float64)), 1.0, rtol=0,
                               atol=1e-12 if dtype == np.float64 else 2 * np.finfo(np.float32).eps)
    assert np.all(got["s1"] >= got["s2"]) and np.all(got["s2"] > 0)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("where", [(17, 30), (1, 0)])
def test_one_nan_departure_point(eng, O, dtype, where):
    """NaN in all four outputs on exactly the cells whose stencil touches the point -- what the oracle's tensor says: the arms
    of the 5-point stencils (the cells ``dilate(r=2)`` marks in the point's row and column) without the point's own cell, on
    which a centred stencil puts no weight; in the first rows the one-sided rule of Q12 -- and every other cell bit-equal to
    the run without the NaN."""
    x, y, lat, lon = (a.astype(dtype) for a in FIELDS["perturbed_37x64"])
    clean = _strain(eng, x, y, lat, lon)
    xn = x.copy()
    xn[where] = np.nan
    got = _strain(eng, xn, y, lat, lon)
    tens = O.flowmap_gradient(xn, y, lat, lon)
    touched = np.isnan(tens[:6]).any(axis=0)
    if where == (17, 30):
        bad = np.zeros(x.shape, bool)
        bad[where] = True
        arms = dilate(bad, 2) & ((np.arange(x.shape[0]) == where[0])[:, None] | (np.arange(x.shape[1]) == where[1])[None, :])
        arms[where] = False
        assert np.array_equal(touched, arms) and touched.sum() == 8
    else:
        assert touched.sum() == 8 and touched[0, 0] and touched[1, 0] and touched[3, 0] and touched[1, -2] and not touched[4, 0]
    for k in PLANES:
        assert np.array_equal(np.isnan(got[k]), touched), k
        assert np.array_equal(got[k][~touched], clean[k][~touched]), k
        assert not np.isnan(clean[k]).any()


# ------------------------------------------------------------------------------------------ batch, names, optional planes
@pytest.mark.parametrize("dtype,cast", [(np.float32, True), (np.float64, True), (np.float64, False)])
def test_batch_equals_single_calls_and_optional_planes(eng, dtype, cast):
    x, y, lat, lon = (a.astype(dtype) for a in FIELDS["perturbed_37x64"])
    xs = np.stack([x, x + dtype(0.25) * np.sin(np.deg2rad(y)).astype(dtype), np.roll(x, 3, axis=1)])
    ys = np.stack([y, np.roll(y, 5, axis=1), y * dtype(0.9)])
    dlat, dlon = float(lat[1] - lat[0]), float(lon[1] - lon[0])
    res = eng.strain(xs, ys, lat, dlat, dlon, fd_fp32_cast=cast)
    assert eng.last_strain_kernel() == KERNELS[(dtype, cast)]
    assert set(res) == set(PLANES) and all(tuple(res[k].shape) == xs.shape for k in PLANES)
    for m in range(3):
        one = eng.strain(xs[m], ys[m], lat, dlat, dlon, fd_fp32_cast=cast)
        assert eng.last_strain_kernel() == KERNELS[(dtype, cast)]
        for k in PLANES:
            assert tuple(one[k].shape) == x.shape and np.array_equal(_np(res[k][m]), _np(one[k]), equal_nan=True), (m, k)
    # planes that are not asked for are not computed; the others do not change
    part = eng.strain(xs, ys, lat, dlat, dlon, fd_fp32_cast=cast, want=("s2", "e_lat"))
    assert set(part) == {"s2", "e_lat"}
    assert np.array_equal(_np(part["s2"]), _np(res["s2"])) and np.array_equal(_np(part["e_lat"]), _np(res["e_lat"]))
    with pytest.raises(ValueError, match="want"):
        eng.strain(xs, ys, lat, dlat, dlon, want=("s1", "s3"))
    with pytest.raises(ValueError):
        eng.strain(xs[:, :4], ys[:, :4], lat[:4], dlat, dlon)      # fewer than 5 rows


# ------------------------------------------------------------------------------------------ one gradient core
# rows: the stencil minimum; a row that is both "first two" and "last two"; one row past the 16-row tile; one past the 20-row
# strip of the marching kernel; two ragged tiles.  widths: narrower than the halo wrap; around the 64-column tile; one even width
# past the 124 columns a marching wave writes and one beyond it.
CORE_ROWS = (5, 6, 17, 21, 37)
CORE_WIDTHS = (5, 63, 64, 65, 126, 130)


def _sigma_route_name(call, dtype, cast=True, march=None):
    """The name tests/kernel_routes.py gives the sigma route of this call, dtype and ``set_sigma_march`` setting."""
    from tests import kernel_routes as KR
    setters = {} if march is None else {"set_sigma_march": march}
    names = [n for n, r in KR.ROUTES.items() if n.startswith("sigma") and r["call"] == call and r["dtype"] == np.dtype(dtype).name
             and r["setters"] == setters and (r["dtype"] == "float32" or r["fd_fp32_cast"] == cast)]
    assert len(names) == 1, names
    return names[0]


def test_sigma_and_strain_share_one_gradient_core(eng):
    """What follows from sigma.hip and strain.hip taking the six derivatives and the Gram eigenvalue from one header, bit for bit
    (``equal_nan``), on smooth random perturbations of seed grids that reach within half a cell of both poles, and on one with a
    NaN departure point in the corner of a tile:

      * float64, both values of ``fd_fp32_cast``: ``strain``'s s1 is ``sigma(tensor_layout="physical")`` and plane 0 of
        ``sigma_batch``; plane 1 of a two-plane batch is the single call on that plane, for ``sigma_batch`` and for ``strain``;
      * float32, every width: batched ``strain`` is the single calls, ``want=("s1",)`` gives the full call's s1;
      * float32, even widths from 64: the marching kernel is the LDS-tile kernel in both layouts, and ``sigma_batch`` is ``sigma``
        plane by plane under both;
      * every call reports the kernel ``KERNELS`` and the route table name."""
    eq = lambda a, b: np.array_equal(_np(a), _np(b), equal_nan=True)
    f32 = np.float32
    try:
        for ny, nx, nan in [(ny, nx, False) for ny in CORE_ROWS for nx in CORE_WIDTHS] + [(21, 130, True)]:
            x, y, lat, lon = S.perturbed_seed_grid(ny, nx, seed=1000 * ny + nx, lat_edge=89.0)
            x2, y2, _, _ = S.perturbed_seed_grid(ny, nx, seed=1000 * ny + nx + 1, lat_edge=89.0)
            dlat, dlon = float(lat[1] - lat[0]), float(lon[1] - lon[0])
            assert 90.0 - lat[-1] < 0.5 * dlat and lat[0] + 90.0 < 0.5 * dlat
            if nan:
                x[16, 64] = np.nan          # first row and first column of a tile: its stencil arms reach into three others
            xs, ys = np.stack([x, x2]), np.stack([y, y2])
            at = f"{ny} x {nx}" + (" with a NaN" if nan else "")
            # ---- float64
            for cast in (True, False):
                kw = dict(fd_fp32_cast=cast)
                st = eng.strain(x, y, lat, dlat, dlon, **kw)
                assert eng.last_strain_kernel() == KERNELS[(np.float64, cast)]
                assert bool(np.isnan(_np(st["s1"])).any()) == nan, at
                sg = eng.sigma(x, y, lat, dlat, dlon, tensor_layout="physical", **kw)
                assert eng.last_sigma_kernel() == _sigma_route_name("sigma", np.float64, cast)
                sb = eng.sigma_batch(xs, ys, lat, dlat, dlon, tensor_layout="physical", **kw)
                assert eng.last_sigma_kernel() == _sigma_route_name("batch", np.float64, cast)
                assert eq(st["s1"], sg) and eq(st["s1"], sb[0]), (at, cast)
                assert eq(sb[1], eng.sigma(x2, y2, lat, dlat, dlon, tensor_layout="physical", **kw)), (at, cast)
                stb, st2 = eng.strain(xs, ys, lat, dlat, dlon, **kw), eng.strain(x2, y2, lat, dlat, dlon, **kw)
                assert all(eq(stb[k][0], st[k]) and eq(stb[k][1], st2[k]) for k in PLANES), (at, cast)
            # ---- float32
            lat32, planes32 = lat.astype(f32), [(x.astype(f32), y.astype(f32)), (x2.astype(f32), y2.astype(f32))]
            xs32, ys32 = xs.astype(f32), ys.astype(f32)
            stb = eng.strain(xs32, ys32, lat32, dlat, dlon)
            assert eng.last_strain_kernel() == KERNELS[(f32, True)]
            for m, (xm, ym) in enumerate(planes32):
                one = eng.strain(xm, ym, lat32, dlat, dlon)
                only = eng.strain(xm, ym, lat32, dlat, dlon, want=("s1",))
                assert eng.last_strain_kernel() == KERNELS[(f32, True)]
                assert all(eq(stb[k][m], one[k]) for k in PLANES) and set(only) == {"s1"} and eq(only["s1"], one["s1"]), (at, m)
            if nx % 2 or nx < 64:
                continue
            for layout in ("reference", "physical"):
                sg = {}
                for march in (1, 0):
                    eng.set_sigma_march(march)
                    sg[march] = [eng.sigma(xm, ym, lat32, dlat, dlon, tensor_layout=layout) for xm, ym in planes32]
                    assert eng.last_sigma_kernel() == _sigma_route_name("sigma", f32, march=march)
                    sb = eng.sigma_batch(xs32, ys32, lat32, dlat, dlon, tensor_layout=layout)
                    assert eng.last_sigma_kernel() == _sigma_route_name("batch", f32, march=march)
                    assert eq(sb[0], sg[march][0]) and eq(sb[1], sg[march][1]), (at, layout, march)
                assert eq(sg[1][0], sg[0][0]) and eq(sg[1][1], sg[0][1]), (at, layout)
    finally:
        eng.set_sigma_march(-1)


# ------------------------------------------------------------------------------------------ float32
def _errors(s1, s2, ex, ey, truth):
    """Errors of a float32 answer against the float64 one: s1 relative, s2 on the scale of s1, the sine of the direction's
    angle to v1 on the cells with s2 / s1 <= 0.99."""
    r1, r2, v1 = truth
    gap = r2 / r1 <= 0.99
    f = lambda a: np.asarray(a, dtype=np.float64)
    return np.abs(f(s1) / r1 - 1), np.abs(f(s2) - r2) / r1, S.sine_of_angle(f(ex), f(ey), v1)[gap]


def _oracle32(O, x32, y32, lat32, lon32, **kw):
    """The float32 oracle: numpy float32 trig and stencil, LAPACK's float32 SVD (the direction's sign does not enter)."""
    tens = O.flowmap_gradient(x32, y32, lat32, lon32, **kw)
    assert tens.dtype == np.float32
    s1, s2, v1 = S.svd_reference(tens)
    return s1, s2, v1[..., 0], v1[..., 1]


def _band32(label, got, o32, truth):
    """tests/_fullsize.py::band with its default multipliers; the floors are the float32 oracle's own figures (so they never
    lift a bound above the multiple of the oracle's error)."""
    for k, eg, eo in zip(("s1", "s2", "direction"), _errors(*got, truth), _errors(*o32, truth)):
        floors = (float(np.median(eo)), float(np.percentile(eo, 99)), float(eo.max()))
        band(eg, eo, f"{label} {k}", *floors)


@pytest.mark.parametrize("name", list(FIELDS))
def test_float32_in_the_float32_oracles_band(eng, O, name):
    x, y, lat, lon = FIELDS[name]
    x32, y32, lat32, lon32 = (a.astype(np.float32) for a in (x, y, lat, lon))
    got = _strain(eng, x32, y32, lat32, lon32)
    assert eng.last_strain_kernel() == "strain_kernel_f32"
    assert all(got[k].dtype == np.float32 and np.isfinite(got[k]).all() for k in PLANES)
    ex, ey = got["e_lon"].astype(np.float64), got["e_lat"].astype(np.float64)
    assert np.abs(np.hypot(ex, ey) - 1).max() <= 2 * np.finfo(np.float32).eps and S.sign_convention_holds(ex, ey)
    # the float64 answer on the same (float32-valued) inputs, clean float64 stencil
    c64 = lambda a: a.astype(np.float64)
    truth = S.svd_reference(O.flowmap_gradient(c64(x32), c64(y32), c64(lat32), c64(lon32), fd_fp32_cast=False))
    _band32(name, tuple(got[k] for k in PLANES), _oracle32(O, x32, y32, lat32, lon32), truth)


def test_float32_full_size_4096(eng, O):
    """4096 x 4096 seeds, departure fields from config 3's advect (order 1, 96 steps, the kernel BASELINE configs[2] runs --
    its positions have their own oracle tests in tests/test_gpu_fullsize_c345.py).  The strain of two row windows -- the first
    34 rows with the two one-sided ones, the last 34 with theirs -- x 64 columns is compared with the oracle on the window + the
    2-seed halo (as tests/_fullsize.py::oracle_window frames it: global spacing, halo ring dropped), float32 inside the float32
    oracle's band around the float64 answer."""
    u, v, lat, lon = flows.era5_like(nt=97)
    slat, slon = flows.seed_grid(4096, 4096, lat, lon)
    f = eng.prepare_field(u, v, lat, lon, 1)
    res = eng.lcs_strain(f, slat, slon, -900.0, 96, SETTLS_order=4, interp_order=1, cyclic_xboundary=True)
    assert eng.last_advect_kernel() == "advect_lds2_kernel<4, true, 0>", eng.last_advect_kernel()
    assert eng.last_strain_kernel() == "strain_kernel_f32"
    assert all(tuple(res[k].shape) == (1, 4096, 4096) for k in PLANES + ("x_dep", "y_dep"))
    ny = slat.size
    c0, c1 = 2000, 2064
    dl = dict(dlat=slat[1] - slat[0], dlon=slon[1] - slon[0])
    for label, (ra, rb), keep in (("first rows", (0, 36), slice(0, 34)), ("last rows", (ny - 36, ny), slice(2, 36))):
        xw, yw = (_np(res[k][0, ra:rb, c0 - 2:c1 + 2]) for k in ("x_dep", "y_dep"))
        got = tuple(_np(res[k][0, ra:rb, c0:c1])[keep] for k in PLANES)
        assert all(np.isfinite(g).all() for g in got)
        cut = lambda a: a[keep, 2:-2]
        o32 = tuple(cut(a) for a in _oracle32(O, xw, yw, slat[ra:rb], slon[c0 - 2:c1 + 2], **dl))
        c64 = lambda a: a.astype(np.float64)
        t64 = S.svd_reference(O.flowmap_gradient(c64(xw), c64(yw), c64(slat[ra:rb]), c64(slon[c0 - 2:c1 + 2]), fd_fp32_cast=False,
                                                 dlat=float(dl["dlat"]), dlon=float(dl["dlon"])))
        _band32(f"4096^2 {label}", got, o32, tuple(cut(a) for a in t64))


# ------------------------------------------------------------------------------------------ memory groups
@pytest.mark.parametrize("cyclic", [True, False])
def test_memory_capped_groups_give_the_bits_of_one_group(eng, cyclic):
    """tests/test_series_gpu.py's test of this name for ``lcs_strain``: 5 windows of its diverging wind (non-cyclic: the last
    two leave the box) in groups of 1 and of 2 against one group, all six outputs bit for bit; a window holds three planes more
    than a window of ``lcs_series`` (8 / 12 instead of 5 / 9)."""
    u, v, lat, lon = _diverging_wind(np.float32)
    f = eng.prepare_field(u, v, lat, lon, 3)
    kw = dict(SETTLS_order=2, interp_order=3, cyclic_xboundary=cyclic)
    whole = eng.lcs_strain(f, lat, lon, 3600.0, 20, 5, t0=0, t0_stride=2, **kw)
    per = (8 if cyclic else 12) * lat.size * lon.size * 4
    assert eng.series_group(np.float32, lat.size * lon.size, 5, cyclic, 3) == 5
    try:
        for g in (1, 2):
            eng.SERIES_MEM_CAP = g * per
            assert eng.series_group(np.float32, lat.size * lon.size, 5, cyclic, 3) == g
            part = eng.lcs_strain(f, lat, lon, 3600.0, 20, 5, t0=0, t0_stride=2, **kw)
            for k in PLANES + ("x_dep", "y_dep"):
                assert np.array_equal(_np(whole[k]), _np(part[k]), equal_nan=True), (g, k)
    finally:
        del eng.SERIES_MEM_CAP


# ------------------------------------------------------------------------------------------ the drop-in contract
def _dataset():
    u, v, lat, lon = flows.config1()
    times = pd.date_range("2000-01-01", periods=u.shape[0], freq="6h").values
    coords = {"latitude": lat, "longitude": lon, "time": times}
    U = labelled.DataArray(u.transpose(1, 2, 0), ["latitude", "longitude", "time"], coords, name="u")
    V = labelled.DataArray(v.transpose(1, 2, 0), ["latitude", "longitude", "time"], coords, name="v")
    return labelled.Dataset({"u": U, "v": V}), times, lat, lon


def _slice(ds, a, b):
    return labelled.Dataset({k: ds[k].isel(time=slice(a, b)) for k in ("u", "v")})


GLOBAL = dict(isglobal=True, interp_to_common_grid=False, truncation=None, verbose=False)


def test_dropin_whole_record_against_the_golden_departure_field(O):
    from LagrangianCoherence.LCS.LCS import LCS
    ds, times, lat, lon = _dataset()
    s1, s2, direction = LCS(timestep=-6 * 3600, SETTLS_order=4).strain(ds, **GLOBAL)
    assert s1.dims == s2.dims == ("time", "latitude", "longitude") and s1.shape == s2.shape == (1, lat.size, lon.size)
    assert direction.dims == ("component", "time", "latitude", "longitude") and direction.shape == (2, 1, lat.size, lon.size)
    assert list(direction.coords["component"]) == ["east", "north"]
    for a in (s1, s2, direction):
        assert a.coords["time"][0] == times[0]                  # backward: the record's first time (LCS.py:158)
        assert np.array_equal(a.coords["latitude"], lat) and np.array_equal(a.coords["longitude"], lon)
    r1, r2, v1 = S.svd_reference(O.flowmap_gradient(*S.golden("g1_bwd_k4_o3"), lat, lon))
    # the engine's departure points sit within 1e-9 degrees of the golden ones: the tolerance the drop-in tests give sigma
    np.testing.assert_allclose(s1.values[0], r1, rtol=1e-7)
    assert np.all(np.abs(s2.values[0] - r2) <= 1e-7 * r1)
    np.testing.assert_allclose(np.hypot(direction.values[0, 0], direction.values[1, 0]), 1.0, rtol=0, atol=1e-12)
    fwd = LCS(timestep=6 * 3600, SETTLS_order=4).strain(ds, **GLOBAL)
    assert fwd[0].coords["time"][0] == times[-1]


def test_dropin_windows_equal_the_per_window_calls_bit_for_bit():
    """float64 at order 1 on the 89-row grid: under the threshold from which ``series``' docstring allows the pack of a window to
    differ from the record's in its last bits."""
    from LagrangianCoherence.LCS.LCS import LCS
    ds, times, lat, lon = _dataset()
    window, stride = 4, 2
    ctor = dict(timestep=-6 * 3600, SETTLS_order=4, return_dpts=True)
    call = dict(GLOBAL, traj_interp_order=1)
    out = LCS(**ctor).strain(ds, window=window, stride=stride, **call)
    n = (times.size - window) // stride + 1
    assert len(out) == 5 and out[0].shape == (n, lat.size, lon.size) and out[0].values.dtype == np.float64
    assert np.array_equal(out[0].coords["time"], times[np.arange(n) * stride])
    for w in range(n):
        one = LCS(**ctor).strain(_slice(ds, w * stride, w * stride + window), **call)
        assert one[0].coords["time"][0] == out[0].coords["time"][w]
        for a, b in zip(out, one):
            ax = a.dims.index("time")
            assert np.array_equal(np.take(a.values, w, axis=ax), np.take(b.values, 0, axis=ax), equal_nan=True), (w, a.dims)
    sig, xs, ys = LCS(**ctor).series(ds, window=window, stride=stride, **call)
    assert np.array_equal(out[3].values, xs.values) and np.array_equal(out[4].values, ys.values)
    assert np.array_equal(out[3].coords["time"], xs.coords["time"])
