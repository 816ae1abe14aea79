"""Every case of tests/ridge_chain.py on the GPU: gauss_kernel against scipy.ndimage.gaussian_filter, index_derivative_kernel
against the oracle's numba restatement bit for bit, ridge_kernel against numpy.linalg.eig per point, and the drop-in
find_ridges_spherical_hessian that strings them against the oracle -- at the sizes where each kernel takes another path: many
folds of the reflection, an axis of one node, radius 0 and GAUSS_MAX_RADIUS, the 5 x 5 grid, element counts past each
launcher's grid cap, dgeev's special rows, non-finite inputs, unsorted coordinates.

Inputs are seeded and built once per case; each reference is computed once and shared.  Every buffer the module's engine
allocates starts as NaN, so an element no kernel wrote fails the comparison.  Each case prints its measured error beside its
bound before asserting (pytest -s).

Largest figures seen on an MI355X: none recorded yet (see the change description).
"""
import functools

import numpy as np
import pytest

from oracle import lcs_oracle as O
from oracle import ridges_oracle as RO
from tests import ridge_chain as RC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from lagrangiancoherence_amd.engine import Engine
    e = Engine(0)
    e._poison = True          # Engine._empty: NaN instead of whatever the caching allocator hands back
    yield e
    e.close()


def _np(t):
    return t.detach().cpu().numpy()


def _id(c):
    return "x".join(map(str, c))


# ------------------------------------------------------------------ lc_gaussian_filter
@functools.lru_cache(maxsize=None)
def _gauss_ref(ny, nx, sigma, dtype, nonfinite=False):
    from scipy.ndimage import gaussian_filter
    a = RC.gauss_input(ny, nx, dtype, nonfinite)
    ref = gaussian_filter(a, sigma=sigma)
    a.setflags(write=False)
    ref.setflags(write=False)
    return a, ref


def _check_gauss(eng, case, nonfinite=False):
    ny, nx, sigma, dtype = case
    a, ref = _gauss_ref(ny, nx, sigma, dtype, nonfinite)
    got = _np(eng.gaussian_filter(a.copy(), sigma))
    assert got.dtype == ref.dtype == np.dtype(dtype) and got.shape == ref.shape
    # the non-finite footprint is scipy's exactly: NaN, inf and the sign of inf
    assert np.array_equal(np.isnan(got), np.isnan(ref)), case
    assert np.array_equal(np.isinf(got), np.isinf(ref)) and np.array_equal(got[np.isinf(ref)], ref[np.isinf(ref)]), case
    assert nonfinite == (not np.isfinite(ref).all())
    ok = np.isfinite(ref)
    err, bound = float(np.abs(got[ok].astype(np.float64) - ref[ok]).max()), RC.gauss_bound(a, sigma)
    print(f"RIDGECHAIN gauss {_id(case)}{' nonfinite' if nonfinite else ''} radius {RC.gauss_radius(sigma)}: "
          f"max|got - scipy| = {err:.3e}  bound {bound:.3e}  ({err / bound:.2f})")
    if RC.gauss_radius(sigma) == 0:
        assert np.array_equal(got, a) and np.array_equal(ref, a), case
    assert err <= bound, (case, err, bound)


@pytest.mark.parametrize("case", RC.GAUSS_CASES, ids=_id)
def test_gaussian_filter_vs_scipy_at_the_edges(eng, case):
    _check_gauss(eng, case)


@pytest.mark.parametrize("case", RC.GAUSS_NONFINITE, ids=_id)
def test_gaussian_filter_nonfinite_footprint_is_scipys(eng, case):
    _check_gauss(eng, case, nonfinite=True)


def test_gaussian_filter_refusals_leave_the_engine_usable(eng):
    case = RC.GAUSS_CASES[0]
    a, _ = _gauss_ref(*case)
    for sigma in RC.GAUSS_REFUSALS:
        with pytest.raises(ValueError, match="lc_gaussian_filter"):
            eng.gaussian_filter(a.copy(), sigma)
        _check_gauss(eng, case)                      # the next valid call on the same engine


# ------------------------------------------------------------------ lc_fourth_order_derivative
DERIV = [(ny, nx, dt) for ny, nx in RC.DERIV_CASES for dt in RC.DERIV_DTYPES]


def _check_deriv(eng, ny, nx, dtype, nonfinite):
    a = RC.deriv_input(ny, nx, dtype, nonfinite)
    for dim in (0, 1):
        for isglobal in (True, False):
            got = _np(eng.index_derivative(a, dim, isglobal))
            with np.errstate(invalid="ignore"):
                ref = O.fourth_order_derivative(a, dim=dim, isglobal=isglobal)
            assert got.dtype == ref.dtype == np.dtype(dtype)
            what = (ny, nx, dtype, dim, isglobal)
            if nonfinite:
                assert np.isnan(ref).any() and np.isinf(ref).any(), what
                assert np.array_equal(got, ref, equal_nan=True), what                # (array_equal on inf compares the sign)
                assert np.array_equal(np.signbit(got[np.isinf(ref)]), np.signbit(ref[np.isinf(ref)])), what
                print(f"RIDGECHAIN deriv {what}: {int(np.isnan(ref).sum())} NaN, {int(np.isinf(ref).sum())} inf, equal")
            else:
                bad = int((got != ref).sum())
                print(f"RIDGECHAIN deriv {what}: {bad} of {ref.size} elements differ")
                assert np.isfinite(ref).all() and np.array_equal(got, ref), what


@pytest.mark.parametrize("ny,nx,dtype", DERIV, ids=[_id(c) for c in DERIV])
def test_fourth_order_derivative_bit_for_bit(eng, ny, nx, dtype):
    _check_deriv(eng, ny, nx, dtype, False)


@pytest.mark.parametrize("dtype", RC.DERIV_DTYPES)
def test_fourth_order_derivative_nonfinite_footprint(eng, dtype):
    _check_deriv(eng, *RC.DERIV_NONFINITE, dtype, True)


def test_fourth_order_derivative_refusals_leave_the_engine_usable(eng):
    for ny, nx, dim in RC.DERIV_REFUSALS:
        with pytest.raises(ValueError, match="too small|Dim must be either 0 or 1"):
            eng.index_derivative(RC.deriv_input(ny, nx, "float64"), dim, True)
        _check_deriv(eng, 5, 5, "float64", False)


# ------------------------------------------------------------------ lc_ridge_classify
@functools.lru_cache(maxsize=None)
def _ridge(n, tol=RC.RIDGE_TOL):
    c = RC.ridge_case(n, tol=tol)
    ref = RC.ridge_reference(c["a"], c["b"], c["d"], c["gx"], c["gy"], tol)
    for v in list(ref) + [c[k] for k in "a b d gx gy".split()]:
        v.setflags(write=False)
    return c, ref


def _check_classify(eng, n, tol):
    c, (m_ref, em_ref, dt_ref, row) = _ridge(n, tol)
    args = [c[k].copy() for k in "a b d gx gy".split()]
    mask, eigmin, dt, vec = (_np(t) for t in eng.ridge_classify(*args, tol, return_eigvec=True))
    assert vec.shape == (2, n)
    if n >= 60000:                                    # every dgeev branch, in what the GPU sees
        ac, bc, dc = (np.where(np.isfinite(v), v, 0.0) for v in (c["a"], c["b"], c["d"]))
        assert min(RC.branch_counts(ac, bc, dc)) > 100
    border = RC.borderline(dt_ref, tol, RC.RIDGE_BORDER, c["exact"])
    assert border.mean() <= RC.BORDER_SHARE           # before anything is excluded
    nz = em_ref != 0
    e_em = float(np.abs(eigmin[nz] / em_ref[nz] - 1).max())
    e_vec = float(np.abs(vec - row.T).max())                                        # both planes, in full
    fin = np.isfinite(dt_ref)
    scale = max(1.0, float(np.abs(dt_ref[fin]).max()))
    e_dt = float(np.abs(dt[fin] - dt_ref[fin]).max()) / scale
    print(f"RIDGECHAIN classify n={n} tol={tol}: eigmin rel {e_em:.2e} / 2e-15, vector {e_vec:.2e} / 5e-15, dt {e_dt:.2e} / 5e-15, "
          f"{int(border.sum())} borderline, {int((mask[~border] != m_ref[~border]).sum())} masks differ")
    # the device's double sqrt/divide can differ from the host's in the last bit
    np.testing.assert_allclose(eigmin, em_ref, rtol=2e-15, atol=0)
    np.testing.assert_allclose(vec, row.T, rtol=0, atol=5e-15)                      # tools.py:107, the ROW of V
    with np.errstate(invalid="ignore"):
        np.testing.assert_allclose(dt, dt_ref, rtol=0, atol=5e-15 * scale, equal_nan=True)
    assert np.array_equal(mask[~border], m_ref[~border])
    assert set(np.unique(mask)) <= {0.0, 1.0} and 0 < mask.sum() < n
    for name, i in c["special"].items():              # one by one: never borderline, so exactly
        what = (name, i, c["a"][i], c["b"][i], c["d"][i], c["gx"][i], c["gy"][i])
        assert not border[i] or i in c["exact"], what
        assert mask[i] == m_ref[i], what + (mask[i], m_ref[i], dt[i], dt_ref[i])
        assert eigmin[i] == pytest.approx(em_ref[i], rel=2e-15, abs=0), what
        assert np.abs(vec[:, i] - row[i]).max() <= 5e-15, what + (vec[:, i], row[i])
        assert (np.isnan(dt[i]) and np.isnan(dt_ref[i])) or dt[i] == dt_ref[i] or abs(dt[i] - dt_ref[i]) <= 5e-15 * scale, what
    for i in c["exact"]:
        assert dt[i] == dt_ref[i]
    assert mask[13] == (1.0 if em_ref[13] < 0 else 0.0)
    return mask, eigmin, dt


@pytest.mark.parametrize("n", RC.RIDGE_N)
def test_ridge_classify_vs_numpy_eig_at_every_size(eng, n):
    mask, eigmin, dt = _check_classify(eng, n, RC.RIDGE_TOL)
    # return_eigvec=False (eigvec_out NULL in the kernel): the same three arrays, bit for bit
    c, _ = _ridge(n)
    three = eng.ridge_classify(*(c[k].copy() for k in "a b d gx gy".split()), RC.RIDGE_TOL)
    assert len(three) == 3
    for got, want in zip(three, (mask, eigmin, dt)):
        assert np.array_equal(_np(got), want, equal_nan=True)


def test_ridge_classify_null_outputs_through_the_c_abi(eng):
    """lc_ridge_classify with dt_out and eigvec_out NULL: the same mask and eigmin, bit for bit."""
    from lagrangiancoherence_amd import _capi
    n = RC.RIDGE_N[1]
    c, _ = _ridge(n)
    t = [eng.to_device(c[k].copy(), np.float64) for k in "a b d gx gy".split()]
    full = eng.ridge_classify(*t, RC.RIDGE_TOL, return_eigvec=True)
    mask, eigmin = eng._empty((n,), np.float64), eng._empty((n,), np.float64)
    eng._use_current_stream()
    _capi.check(eng.lib.lc_ridge_classify(eng.ctx, *(eng._ptr(a) for a in t), n, float(RC.RIDGE_TOL), eng._ptr(mask), eng._ptr(eigmin),
                                          None, None), eng.lib)
    assert np.array_equal(_np(mask), _np(full[0])) and np.array_equal(_np(eigmin), _np(full[1]))


def test_ridge_classify_with_a_zero_tolerance(eng):
    _check_classify(eng, RC.RIDGE_N_TOL0, 0.0)


# ------------------------------------------------------------------ find_ridges_spherical_hessian on the device
@functools.lru_cache(maxsize=None)
def _chain_ref(name):
    case = RC.CHAIN_CASES[name]
    _, _, _, f, lat, lon = RC.chain_input(case)
    return RO.find_ridges_spherical_hessian(f, lat, lon, sigma=case["sigma"], tolerance_threshold=RC.CHAIN_TOL, isglobal=case["isglobal"])


@functools.lru_cache(maxsize=None)
def _chain_got(name):
    from LagrangianCoherence.LCS.tools import find_ridges_spherical_hessian
    from tests import labelled
    case = RC.CHAIN_CASES[name]
    v, lat, lon, _, _, _ = RC.chain_input(case)
    da = labelled.DataArray(v, case["dims"], {"latitude": lat, "longitude": lon}, name="ftle")
    return find_ridges_spherical_hessian(da, sigma=case["sigma"], tolerance_threshold=RC.CHAIN_TOL, isglobal=case["isglobal"])


def _ll(da):
    """values as (latitude, longitude)"""
    return da.values if da.dims == RC.LL else da.values.T


@pytest.mark.parametrize("name", list(RC.CHAIN_CASES))
def test_find_ridges_chain_vs_oracle(name):
    case = RC.CHAIN_CASES[name]
    ridges, eigmin = _chain_got(name)
    m_ref, e_ref, dt_ref = _chain_ref(name)
    _, _, _, f, lat, lon = RC.chain_input(case)
    for o in (ridges, eigmin):                        # the input's dimension order, the sorted coordinates
        assert o.dims == case["dims"] and o.shape == tuple({"latitude": case["ny"], "longitude": case["nx"]}[d] for d in case["dims"])
        assert np.array_equal(o.coords["latitude"], lat) and np.array_equal(o.coords["longitude"], lon)
    border = RC.borderline(dt_ref, RC.CHAIN_TOL, RC.CHAIN_BORDER_REL * RC.CHAIN_TOL)
    assert border.mean() <= RC.BORDER_SHARE
    nz = e_ref != 0
    err = float(np.abs(_ll(eigmin)[nz] / e_ref[nz] - 1).max()) if nz.any() else 0.0
    print(f"RIDGECHAIN chain {name}: eigmin rel {err:.2e} / 1e-12, {int(border.sum())} borderline, "
          f"{int((_ll(ridges)[~border] != m_ref[~border]).sum())} masks differ, {int(m_ref.sum())} ridge points of {m_ref.size}")
    np.testing.assert_allclose(_ll(eigmin), e_ref, rtol=1e-12, atol=1e-25)
    assert np.array_equal(_ll(ridges)[~border], m_ref[~border])
    if case["ny"] > 7:
        assert 0 < ridges.values.sum() < ridges.values.size


@pytest.mark.parametrize("g", ["global", "regional"])
def test_sigma_variants_that_skip_the_filter_equal_sigma_none(g):
    names = [n for n in RC.CHAIN_CASES if n.startswith("sigma") and n.endswith("-" + g)]
    assert [RC.CHAIN_CASES[n]["sigma"] for n in names] == list(RC.SIGMA_VARIANTS) and RC.CHAIN_CASES[names[0]]["sigma"] is None
    none = _chain_got(names[0])
    smoothed = 0
    for n, s in zip(names, RC.SIGMA_VARIANTS):
        got = _chain_got(n)
        same = all(np.array_equal(x.values, y.values, equal_nan=True) for x, y in zip(got, none))
        assert same == (not RC.smooths(s)), (n, s)
        smoothed += not same
    assert smoothed == 2
