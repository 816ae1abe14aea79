"""The Gram and strain steps of csrc/flowmap_gradient.h (gram_eigen, stretch_of) and the float32 closed form of csrc/sigma.hip
driven into their rule branches on the GPU, through every kernel that carries them:

(a) ``lc_aux_gradient`` on the designed cells of tests/jacobians.py -- ill-conditioned, near-isotropic, exactly isotropic,
    collapsed, rank-one, seam, wide-angle, tiny-offset and non-finite cells -- against the longdouble judge of that module (one
    Hestenes rotation, none of the kernel's formulas after the derivatives), which tests/test_jacobians.py holds to a 50-digit
    fixture;
(b) ``lc_strain``, ``lc_flowmap_gradient`` and every sigma route of tests/kernel_routes.py on three degenerate departure fields
    of a global 21 x 64 grid: every parcel at one point, and flow maps that keep only the latitude or only the longitude.

The expected value never comes from the engine.  The error measure E of (a) is tests/lavd.py's: 8 x the largest difference, on
a class of cells, between the numpy restatement in the kernel's dtype (tests/aux_gradient.py) and the judge on the same inputs,
4 eps x the scale where that difference is 0; per class and per output, fixed before the device is asked."""
import numpy as np
import pytest

from tests import aux_gradient as AG
from tests import jacobians as JC
from tests import kernel_routes as KR

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
AUX_KERNEL = {np.dtype(np.float32): "aux_gradient_kernel_f32", np.dtype(np.float64): "aux_gradient_kernel<double>"}
NO_DIRECTION = ("near_isotropic",)            # the classes whose direction is ill-conditioned by design: never compared
MEASURES = ("s1", "sigma_physical", "sigma_reference", "s2", "direction", "residual", "unit")


@pytest.fixture(scope="module")
def eng():
    from lagrangiancoherence_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _np(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------ (a) the auxiliary-grid carrier
def _aux(eng, t, planes=None, sep_lat=None, sep_lon=None, want=JC.OUTS, layout="physical"):
    got = eng.aux_gradient(t.planes if planes is None else planes, t.seed_lat, t.sep_lat if sep_lat is None else sep_lat,
                           t.sep_lon if sep_lon is None else sep_lon, want=want, tensor_layout=layout)
    assert eng.last_aux_kernel() == AUX_KERNEL[t.dtype]
    out = {k: _np(v) for k, v in got.items()}
    assert all(v.dtype == t.dtype and v.shape == t.cls.shape for v in out.values())
    return out


_REFS = {}


def _refs(dtype):
    """The judge (both layouts, and its derivatives) and the restatement in the kernel's dtype, rounded to it, once per dtype."""
    dtype = np.dtype(dtype)
    if dtype not in _REFS:
        t = JC.table(dtype)
        a = (t.planes, t.seed_lat, t.sep_lat, t.sep_lon)
        rest = AG.restatement(*a, dtype.type)
        rest = {k: np.asarray(rest[k]).astype(dtype) for k in ("s1", "s2", "e_lon", "e_lat")}
        rest["sigma_reference"] = np.asarray(AG.restatement(*a, dtype.type, "reference")["sigma"]).astype(dtype)
        rest["sigma"] = rest["s1"]
        _REFS[dtype] = dict(judge=JC.judge(*a), sigma_reference=JC.judge(*a, "reference")["sigma"], d=JC.derivatives(*a), rest=rest)
    return _REFS[dtype]


def _errors(v, ref):
    """Per cell, each measure of MEASURES for the outputs ``v`` (s1, s2, e_lon, e_lat, sigma = the physical layout's,
    sigma_reference) against the judge: absolute differences; the sine of the direction error x the spectral gap; the
    eigen-residual || C e - s1^2 e || over the judge's s1^2 (C from the judge's derivatives; 0 where F = 0); | |e| - 1 |."""
    L = np.longdouble
    j = ref["judge"]
    s1, ex, ey = (np.asarray(v[k]).astype(L) for k in ("s1", "e_lon", "e_lat"))
    with np.errstate(invalid="ignore", divide="ignore"):
        res = np.where(j["s1"] > 0, JC.residual(ref["d"], ex, ey, s1) / j["s1"] ** 2, L(0))
    return dict(s1=np.abs(s1 - j["s1"]), sigma_physical=np.abs(np.asarray(v["sigma"]).astype(L) - j["s1"]),
                sigma_reference=np.abs(np.asarray(v["sigma_reference"]).astype(L) - ref["sigma_reference"]),
                s2=np.abs(np.asarray(v["s2"]).astype(L) - j["s2"]), direction=JC.sine(ex, ey, j["e_lon"], j["e_lat"]) * j["gap"],
                residual=res, unit=np.abs(np.hypot(ex, ey) - 1))


def _bounds(dtype):
    """E[class][measure] from the restatement and the judge alone."""
    t, ref = JC.table(dtype), _refs(dtype)
    own = _errors(ref["rest"], ref)
    cls = JC.judged_class(t.cls)
    E = {}
    for c in sorted(set(cls.ravel())):
        m = cls == c
        scale = float(ref["judge"]["s1"][m].max())                   # s1, s2 and sigma are judged on the scale of s1
        E[c] = {k: JC.error_measure(own[k][m], np.zeros(m.sum()), dtype, 1.0 if k in ("direction", "residual", "unit") else scale)
                for k in MEASURES}
    return cls, E


@pytest.mark.parametrize("dtype", DTYPES)
def test_aux_gradient_on_the_designed_cells(eng, dtype):
    """Every finite class against the judge, per class and per output within E; the direction on every class but
    near_isotropic (which the exactly isotropic cell is measured with), the eigen-residual, | |e| - 1 |, the sign convention
    and s1 >= s2 >= 0 on every cell.  Then the exact rules: collapsed cells give sigma = s1 = s2 = 0 and (1, 0); E == W gives s2 = 0 and (0, 1),
    N == S gives s2 = 0 and (1, 0); the exactly isotropic cell gives s1 == s2 and (1, 0) in float64; the wrapped and the
    unwrapped seam cell agree within the sum of their E.

    Measured on an MI355X (this test's own prints), the largest device error of a class in units of its E:
    float64: 0.125 for every class and output that has an error at all -- the device's float64 results are the numpy
    restatement's, bit for bit, so its error is the restatement's own, an eighth of E (generic: s1 6.1e-14 of E 4.9e-13, s2
    3.3e-14 of 2.7e-13, direction 4.1e-14 of 3.3e-13, residual 1.2e-13 of 9.7e-13; near_isotropic s1 6.4e-16 of 5.1e-15; seam s1
    2.3e-14 of 1.8e-13; tiny s1 1.0e-15 of 8.2e-15; wide s1 1.4e-16 of 1.1e-15); rank_one_ew s2 and direction 2.4e-20 of 1.9e-19:
    the device's exact 0 against the judge's cos(pi / 2).
    float32: between 0.09 and 0.13 (generic: s1 2.3e-5 of 1.8e-4, s2 1.2e-5 of 9.4e-5, direction 1.9e-5 of 1.5e-4, residual 4.6e-5
    of 3.7e-4, unit 2.9e-8 of 2.3e-7; near_isotropic s1 1.2e-6 of 9.9e-6; seam s1 2.9e-4 of 2.3e-3; tiny s1 1.1e-6 of 8.5e-6; wide
    s1 7.9e-8 of 9.2e-7; rank_one_ew s1 6.8e-8 of 6.2e-7).  collapsed: 0 in every output, both dtypes.
    The seam twins differ by 2.9e-4 in s1 in float32 (2 E = 4.6e-3) and by 1.6e-13 in float64 (2 E = 3.6e-13)."""
    t, ref = JC.table(dtype), _refs(dtype)
    got = _aux(eng, t)
    for layout in ("reference", "physical"):
        alone = _aux(eng, t, want=("sigma",), layout=layout)
        every = _aux(eng, t, layout=layout)
        assert np.array_equal(alone["sigma"], every["sigma"]), layout
        assert all(np.array_equal(every[k], got[k]) for k in ("s1", "s2", "e_lon", "e_lat")), layout
        if layout == "reference":
            got["sigma_reference"] = alone["sigma"]
        else:
            assert np.array_equal(alone["sigma"], got["s1"]) and np.array_equal(got["sigma"], got["s1"])
    assert all(np.isfinite(v).all() for v in got.values())
    cls, E = _bounds(dtype)
    err = _errors(got, ref)
    name = np.dtype(dtype).name
    failures = []
    for c in sorted(E):
        m = cls == c
        line = []
        for k in MEASURES:
            if k == "direction" and c in NO_DIRECTION:
                line.append("direction not compared")
                continue
            worst, bound = float(err[k][m].max()), E[c][k]
            line.append(f"{k} {worst:.2e} / E {bound:.2e}" + (f" = {worst / bound:.2f}" if bound > 0 else ""))
            if not worst <= bound:
                failures.append((c, k, worst, bound))
        print(f"{name} {c} ({m.sum()} cells): " + "; ".join(line))
    assert not failures, failures
    ex, ey = got["e_lon"].astype(np.float64), got["e_lat"].astype(np.float64)
    assert JC.sign_convention_holds(ex, ey)
    assert np.all(got["s1"] >= got["s2"]) and np.all(got["s2"] >= 0)
    # the exact rules
    m = t.cls == "collapsed"
    for k, v in (("sigma", 0), ("sigma_reference", 0), ("s1", 0), ("s2", 0), ("e_lon", 1), ("e_lat", 0)):
        assert np.all(got[k][m] == v), k
    for c, e in (("rank_one_ew", (0, 1)), ("rank_one_ns", (1, 0))):
        m = t.cls == c
        assert np.all(got["s2"][m] == 0) and np.all(got["e_lon"][m] == e[0]) and np.all(got["e_lat"][m] == e[1]), c
        assert np.all(got["s1"][m] > 0.5)
    if dtype == np.float64:
        r, k = t.index["isotropic_exact"]
        assert got["s1"][r, k] == got["s2"][r, k] > 0.9 and (got["e_lon"][r, k], got["e_lat"][r, k]) == (1.0, 0.0)
    # the seam twins: the same two points, one longitude written 360 degrees apart
    (r1, k1), (r2, k2) = t.index["seam_wrapped"], t.index["seam_unwrapped"]
    for k, out in (("s1", "s1"), ("s2", "s2"), ("sigma_physical", "sigma"), ("sigma_reference", "sigma_reference")):
        d = abs(np.longdouble(got[out][r1, k1]) - np.longdouble(got[out][r2, k2]))
        print(f"{name} seam twins {k}: differ by {float(d):.2e}, 2 E = {2 * E['seam'][k]:.2e}")
        assert d <= 2 * E["seam"][k], k
    d = JC.sine(got["e_lon"][r1, k1], got["e_lat"][r1, k1], got["e_lon"][r2, k2], got["e_lat"][r2, k2]) * ref["judge"]["gap"][r1, k1]
    assert d <= 2 * E["seam"]["direction"]


@pytest.mark.parametrize("dtype", DTYPES)
def test_aux_gradient_nonfinite_cells(eng, dtype):
    """NaN in each of the eight planes in turn, +inf and -inf in one: NaN in every output of that cell, in both layouts; a NaN
    separation: NaN in its row or column.  Every other cell keeps the bits of the run without the poison."""
    t = JC.table(dtype)
    base = {lay: _aux(eng, t, layout=lay) for lay in ("physical", "reference")}
    for label, key, (row, col), value in JC.poisons(t):
        planes, sl, so = {k: v.copy() for k, v in t.planes.items()}, t.sep_lat.copy(), t.sep_lon.copy()
        hit = np.zeros(t.cls.shape, bool)
        if key == "sep_lat":
            sl[row], hit[row, :] = value, True
        elif key == "sep_lon":
            so[col], hit[:, col] = value, True
        else:
            planes[key][row, col], hit[row, col] = value, True
        for lay in ("physical", "reference"):
            got = _aux(eng, t, planes, sl, so, layout=lay)
            for o in JC.OUTS:
                assert np.isnan(got[o][hit]).all(), (label, lay, o)
                assert np.array_equal(got[o][~hit], base[lay][o][~hit]), (label, lay, o)


# ------------------------------------------------------------------ (b) the stencil carriers
FIELDS = ("collapsed", "meridional", "zonal")
DIRECTION = {"meridional": (0, 1), "zonal": (1, 0), "collapsed": (1, 0)}
_ORACLE = {}


def _oracle_reduced(field, arith, cast):
    """The judge's reduction (both layouts) of the oracle's tensor of a field: ``arith`` float64 on the float64 field,
    ``f32in64`` float64 arithmetic on the field rounded to float32, ``float32`` the oracle in float32."""
    key = (field, arith, cast)
    if key not in _ORACLE:
        from oracle import lcs_oracle as O
        dt = np.float64 if arith == "float64" else np.float32
        (x, y), (lat, lon) = JC.stencil_field(field, dt), JC.stencil_grid(dt)
        if arith == "f32in64":
            x, y, lat, lon = (a.astype(np.float64) for a in (x, y, lat, lon))
        tens = O.flowmap_gradient(x, y, lat, lon, fd_fp32_cast=cast)
        _ORACLE[key] = {lay: JC.hestenes(tens[:6], lay) for lay in ("physical", "reference")}
    return _ORACLE[key]


def _against_oracle(got, field, layout, dtype, cast, tol, label, key="sigma"):
    """float64: relative to the oracle within the route's tolerance of tests/kernel_routes.py.  float32: the sigma routes' band
    (tests/test_kernel_routes_gpu.py): the error against float64 arithmetic on the float32 inputs, over the largest value, within
    4 x the float32 oracle's own + 1e-6."""
    got = np.asarray(got).astype(np.float64)
    assert np.isfinite(got).all(), label
    if np.dtype(dtype) == np.float64:
        ref = _oracle_reduced(field, "float64", cast)[layout][key].astype(np.float64)
        err = float((np.abs(got - ref) / ref).max())
        print(f"{label}: relative error {err:.2e} (bound {tol:.0e})")
        assert err <= tol, label
        return
    ref = _oracle_reduced(field, "f32in64", cast)[layout][key].astype(np.float64)
    o32 = _oracle_reduced(field, "float32", cast)[layout][key].astype(np.float64)
    scale = np.abs(ref).max()
    e_gpu, e_or = float(np.abs(got - ref).max() / scale), float(np.abs(o32 - ref).max() / scale)
    print(f"{label}: error {e_gpu:.2e}, the float32 oracle's own {e_or:.2e}")
    assert e_gpu <= 4 * e_or + 1e-6, label


def _grid_args(dtype):
    lat, lon = JC.stencil_grid(dtype)
    return lat, float(lat[1] - lat[0]), float(lon[1] - lon[0])


STRAIN = [("strain_kernel_f32", np.float32, True, None), ("strain_kernel<double, float>", np.float64, True, "sigma64"),
          ("strain_kernel<double, double>", np.float64, False, "sigma64_nocast")]


@pytest.mark.parametrize("kernel,dtype,cast,tol", STRAIN, ids=[s[0] for s in STRAIN])
def test_strain_on_degenerate_fields(eng, kernel, dtype, cast, tol):
    """collapsed: s1 = s2 = 0 and (1, 0) exactly (the stencil differences bitwise equal numbers).  meridional: s2 == 0 and
    (0, 1); zonal: s2 == 0 and (1, 0); s1 of both against the oracle's tensor reduced by the judge.
    Measured on an MI355X: float32 9.1e-7 (meridional) and 1.3e-6 (zonal) of the largest s1, the float32 oracle's own 1.3e-6 and
    2.6e-6; float64 with the cast 1.1e-16 and 2.1e-16 relative (bound 1e-7), without it 6.7e-16 and 8.6e-16 (bound 1e-9)."""
    lat, dlat, dlon = _grid_args(dtype)
    for field in FIELDS:
        x, y = JC.stencil_field(field, dtype)
        got = {k: _np(v) for k, v in eng.strain(x, y, lat, dlat, dlon, fd_fp32_cast=cast).items()}
        assert eng.last_strain_kernel() == kernel
        assert all(v.dtype == dtype and v.shape == (21, 64) for v in got.values())
        assert np.all(got["s2"] == 0), field
        assert np.all(got["e_lon"] == DIRECTION[field][0]) and np.all(got["e_lat"] == DIRECTION[field][1]), field
        if field == "collapsed":
            assert np.all(got["s1"] == 0)
        else:
            assert np.all(got["s1"] > 0.2)
            _against_oracle(got["s1"], field, "physical", dtype, cast, KR.TOL[tol] if tol else None, f"{kernel} {field} s1", key="s1")
    # the three fields as the members of one call
    xs, ys = (np.stack(a) for a in zip(*(JC.stencil_field(f, dtype) for f in FIELDS)))
    both = {k: _np(v) for k, v in eng.strain(xs, ys, lat, dlat, dlon, fd_fp32_cast=cast).items()}
    for i, field in enumerate(FIELDS):
        one = {k: _np(v) for k, v in eng.strain(*JC.stencil_field(field, dtype), lat, dlat, dlon, fd_fp32_cast=cast).items()}
        assert all(np.array_equal(both[k][i], one[k]) for k in one), field


SIGMA = [n for n in KR.ROUTES if n.startswith("sigma")]


@pytest.mark.parametrize("name", SIGMA)
def test_sigma_routes_on_degenerate_fields(eng, name):
    """Every sigma route of tests/kernel_routes.py, forced as tests/test_kernel_routes_gpu.py forces it, in both tensor
    layouts.  collapsed: sigma exactly 0 (the tensor route: its six derivative planes exactly 0).  meridional / zonal: sigma
    against the oracle's tensor reduced by the judge, within the route's tolerance; the tensor route: the derivatives along the
    direction the flow map forgets exactly 0, and the judge's reduction of the device's tensor against the oracle's.
    Measured on an MI355X: the four float32 sigma kernels 7.6e-7 to 1.2e-6 of the largest sigma (the float32 oracle's own 1.0e-6
    to 2.6e-6), the float32 tensor 1.0e-6 to 2.5e-6; float64 with the cast 1.1e-16 to 2.1e-16 relative (bound 1e-7), without it
    6.7e-16 to 1.0e-15 (bound 1e-9); a batch kernel gives its single-call kernel's figures."""
    from tests.test_kernel_routes_gpu import _Setters
    r = KR.ROUTES[name]
    dtype, cast = np.dtype(r["dtype"]).type, r["fd_fp32_cast"]
    assert 64 in r["widths"]
    tol = KR.TOL[r["tol"]] if dtype == np.float64 else None
    lat, dlat, dlon = _grid_args(dtype)
    fields = {f: JC.stencil_field(f, dtype) for f in FIELDS}
    for layout in ("reference", "physical"):
        with _Setters(eng, r["setters"]):
            if r["call"] == "batch":
                xs, ys = (np.stack(a) for a in zip(*(fields[f] for f in FIELDS)))
                out = _np(eng.sigma_batch(xs, ys, lat, dlat, dlon, fd_fp32_cast=cast, tensor_layout=layout))
                got = dict(zip(FIELDS, out))
            elif r["call"] == "sigma":
                got = {f: _np(eng.sigma(*fields[f], lat, dlat, dlon, fd_fp32_cast=cast, tensor_layout=layout)) for f in FIELDS}
            else:
                got = {f: _np(eng.flowmap_gradient(*fields[f], lat, dlat, dlon, fd_fp32_cast=cast)) for f in FIELDS}
            eng.synchronize()
            assert eng.last_sigma_kernel() == name, eng.last_sigma_kernel()
        if r["call"] == "tensor":
            assert all(v.shape == (9, 21, 64) and v.dtype == dtype for v in got.values())
            assert np.all(got["collapsed"] == 0)
            assert np.all(got["meridional"][[0, 2, 4]] == 0) and np.all(got["zonal"][[1, 3, 5]] == 0)
            assert np.all(got["meridional"][6:] == 0) and np.all(got["zonal"][6:] == 0)
            for f in ("meridional", "zonal"):
                red = JC.hestenes(got[f][:6], layout)
                _against_oracle(red["sigma"], f, layout, dtype, cast, tol, f"{name} {f} {layout}")
            continue
        assert all(v.shape == (21, 64) and v.dtype == dtype for v in got.values())
        assert np.all(got["collapsed"] == 0), layout
        for f in ("meridional", "zonal"):
            _against_oracle(got[f], f, layout, dtype, cast, tol, f"{name} {f} {layout}")


def test_march_and_tile_float32_routes_agree_bit_for_bit(eng):
    """The marching kernel's stated contract (csrc/sigma.hip): the arithmetic of sigma_kernel_f32, bit for bit -- on the
    degenerate fields as well, single calls and batches, both layouts."""
    from tests.test_kernel_routes_gpu import _Setters
    lat, dlat, dlon = _grid_args(np.float32)
    xs, ys = (np.stack(a) for a in zip(*(JC.stencil_field(f, np.float32) for f in FIELDS)))
    for layout in ("reference", "physical"):
        out = {}
        for march in (0, 1):
            with _Setters(eng, {"set_sigma_march": march}):
                one = [_np(eng.sigma(xs[i], ys[i], lat, dlat, dlon, tensor_layout=layout)) for i in range(len(FIELDS))]
                assert eng.last_sigma_kernel() == ("sigma_march_kernel_f32" if march else "sigma_kernel_f32")
                many = _np(eng.sigma_batch(xs, ys, lat, dlat, dlon, tensor_layout=layout))
                assert eng.last_sigma_kernel() == ("sigma_march_batch_kernel_f32" if march else "sigma_batch_kernel_f32")
            out[march] = (np.stack(one), many)
        assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]), layout
        assert np.array_equal(out[0][0], out[0][1]), layout
