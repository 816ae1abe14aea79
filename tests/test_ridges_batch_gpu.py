"""The stacked ridge extraction on the GPU (``gauss_planes_kernel``, ``hessian_ridge_kernel``; ``lc_ridges_batch``,
``Engine.ridges_batch``, the N-D form of ``tools.find_ridges_spherical_hessian``), every case of tests/ridges_batch.py:

  * equality with the per-plane route: the stacked call against a loop of the 2-D ``find_ridges_spherical_hessian`` over the
    same planes, ``numpy.array_equal`` with NaNs in the same places on all six outputs -- both are the same arithmetic, so
    there is no tolerance -- on 5 x 5, 6 x 9, one tile, one pixel more than a tile both ways and a ragged multi-tile grid, one
    and three planes, cyclic and regional, every sigma variant and the driver's 1.2;
  * the oracle as a second anchor, per plane, with the border rule of tests/test_ridges.py;
  * seams and isolation: a NaN on a corner four tiles share and infs on both sides of the wrapped seam, a plane of NaN between
    two others, a leading dimension of length one;
  * the kernel names through ``last_ridges_kernel``, dimension order and coordinates of labelled records;
  * chaining on the device: ``Engine.lcs_series`` -> ``ridges_batch`` -> ``filter_components`` without a host copy against the
    same chain through host arrays plane by plane.

Every buffer the engine allocates starts as NaN, so an element no kernel wrote fails the comparison.  The per-plane results and
the oracle's are computed once per plane and shared.

Largest figures seen on an MI355X: every bit-for-bit comparison held; against the oracle eigmin off by at most 6.7e-16 relative
(bound 1e-12), no borderline point and no differing mask in any of the 180 planes; the whole module in under 4 s.
"""
import functools

import numpy as np
import pytest

from oracle import ridges_oracle as RO
from tests import labelled
from tests import ridge_chain as RC
from tests import ridges_batch as RB

pytestmark = pytest.mark.gpu

TLL = ("time", "latitude", "longitude")
NAMES = ("ridges", "eigmin", "dt", "eigvectors", "gradient", "angle")


@pytest.fixture(scope="module", autouse=True)
def eng():
    """The drop-in's own engine (the one ``tools`` uses), with poisoned allocations for this module."""
    from lagrangiancoherence_amd.dropin import get_engine
    e = get_engine()
    before, e._poison = e._poison, True       # Engine._empty: NaN instead of whatever the caching allocator hands back
    yield e
    e._poison = before


def _find(da, **kw):
    from LagrangianCoherence.LCS.tools import find_ridges_spherical_hessian
    return find_ridges_spherical_hessian(da, tolerance_threshold=RB.TOL, return_eigvectors=True, **kw)


def _da(values, dims, lat, lon, **coords):
    return labelled.DataArray(values, dims, {"latitude": lat, "longitude": lon, **coords}, name="ftle")


def _frozen(arrays):
    for a in arrays:
        a.setflags(write=False)
    return tuple(arrays)


@functools.lru_cache(maxsize=None)
def per_plane(ny, nx, m, isglobal, si):
    """Today's 2-D route on plane m: the six outputs as (latitude, longitude) / (2, latitude, longitude) arrays."""
    lat, lon = RB.grid(ny, nx)
    out = _find(_da(RB.plane(ny, nx, m), TLL[1:], lat, lon), sigma=RB.SIGMAS[si], isglobal=isglobal)
    return _frozen([o.values for o in out])


@functools.lru_cache(maxsize=None)
def stacked(ny, nx, n, isglobal, si):
    """The stacked call on planes 0 .. n-1 as a (time, latitude, longitude) record: six arrays with time (after the label
    dimension, where there is one) leading."""
    v, lat, lon = RB.stack(ny, nx, n)
    out = _find(_da(v, TLL, lat, lon, time=np.arange(n)), sigma=RB.SIGMAS[si], isglobal=isglobal)
    assert [o.dims for o in out] == [TLL, TLL, TLL, ("eigvectors",) + TLL, ("elements",) + TLL, TLL]
    return _frozen([o.values for o in out])


def _assert_same(got, want, what):
    assert got.dtype == want.dtype == np.float64 and got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    assert np.array_equal(got, want, equal_nan=True), (what, int((~np.isclose(got, want, rtol=0, atol=0, equal_nan=True)).sum()))


# ------------------------------------------------------------------ equality with the per-plane route
@pytest.mark.parametrize("case", RB.CASES, ids=RB.case_id)
def test_stacked_call_equals_the_per_plane_route_bit_for_bit(eng, case):
    ny, nx, n, g, si = case
    got = stacked(*case)
    smooth = RC.smooths(RB.SIGMAS[si])
    for m in range(n):
        want = per_plane(ny, nx, m, g, si)
        for name, a, b in zip(NAMES, got, want):
            _assert_same(a[:, m] if a.ndim == 4 else a[m], b, (RB.case_id(case), name, m))
    assert set(np.unique(got[0])) == {0.0, 1.0}, RB.case_id(case)           # the mask has both values
    if not smooth:                                                          # the variants that skip the filter: sigma None's bits
        none = stacked(ny, nx, n, g, 0)
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(got, none))


@pytest.mark.parametrize("si", range(len(RB.SIGMAS)), ids=lambda i: f"sigma{i}_{type(RB.SIGMAS[i]).__name__}_{RB.SIGMAS[i]}")
def test_kernel_names(eng, si):
    v, lat, lon = RB.stack(*RB.SHAPES[3], 3)
    smooth = RC.smooths(RB.SIGMAS[si])
    res = eng.ridges_batch(v, lat, lon, sigma=RB.SIGMAS[si] if smooth else None, tolerance=RB.TOL, isglobal=True)
    assert eng.last_ridges_kernel() == ("gauss_planes_kernel+hessian_ridge_kernel" if smooth else "hessian_ridge_kernel")
    assert set(res) == {"mask", "eigmin"} and all(t.is_cuda and tuple(t.shape) == v.shape for t in res.values())
    # ... and through the drop-in: the N-D form launches them, the 2-D form does not
    _find(_da(v, TLL, lat, lon, time=np.arange(3)), sigma=RB.SIGMAS[si], isglobal=True)
    assert eng.last_ridges_kernel() == ("gauss_planes_kernel+hessian_ridge_kernel" if smooth else "hessian_ridge_kernel")


# ------------------------------------------------------------------ the oracle, as a second anchor
@functools.lru_cache(maxsize=None)
def oracle_plane(ny, nx, m, isglobal, si):
    return _frozen(list(RO.find_ridges_spherical_hessian(RB.plane(ny, nx, m), *RB.grid(ny, nx), sigma=RB.SIGMAS[si],
                                                         tolerance_threshold=RB.TOL, isglobal=isglobal)))


@pytest.mark.parametrize("case", [c for c in RB.CASES if c[2] == max(RB.MEMBERS)], ids=RB.case_id)
def test_stacked_call_vs_oracle_per_plane(case):
    ny, nx, n, g, si = case
    ridges, eigmin = stacked(*case)[:2]
    for m in range(n):
        m_ref, e_ref, dt_ref = oracle_plane(ny, nx, m, g, si)
        border = RC.borderline(dt_ref, RB.TOL, RC.CHAIN_BORDER_REL * RB.TOL)
        assert border.mean() <= RC.BORDER_SHARE
        nz = e_ref != 0
        err = float(np.abs(eigmin[m][nz] / e_ref[nz] - 1).max()) if nz.any() else 0.0
        print(f"RIDGESBATCH {RB.case_id(case)} plane {m}: eigmin rel {err:.2e} / 1e-12, {int(border.sum())} borderline, "
              f"{int((ridges[m][~border] != m_ref[~border]).sum())} masks differ, {int(m_ref.sum())} ridge points of {m_ref.size}")
        np.testing.assert_allclose(eigmin[m], e_ref, rtol=1e-12, atol=1e-25)
        assert np.array_equal(ridges[m][~border], m_ref[~border])


# ------------------------------------------------------------------ seams and isolation
@pytest.mark.parametrize("isglobal", RB.GLOBAL)
@pytest.mark.parametrize("sigma", [None, 0.5, 1.2])
def test_nonfinite_values_on_tile_corners_and_the_wrapped_seam(isglobal, sigma):
    ny, nx = RB.SHAPES[-1]
    v, lat, lon = RB.stack(ny, nx, 3)
    p = RB.seam_points(ny, nx)
    v[0][p["nan"]] = np.nan
    v[1][p["inf_east"]] = np.inf
    v[2][p["inf_west"]] = -np.inf
    v[2][p["nan"][0] - 1, p["nan"][1] - 1] = np.nan                           # the last point of the tile before the corner
    got = _find(_da(v, TLL, lat, lon, time=np.arange(3)), sigma=sigma, isglobal=isglobal)
    touched = 0
    for m in range(3):
        want = _find(_da(v[m], TLL[1:], lat, lon), sigma=sigma, isglobal=isglobal)
        clean = per_plane(ny, nx, m, isglobal, RB.SIGMAS.index(sigma))
        for name, a, b, c in zip(NAMES, got, want, clean):
            _assert_same(a.values[:, m] if a.values.ndim == 4 else a.values[m], b.values, (name, m, isglobal, sigma))
            touched += not np.array_equal(b.values, c, equal_nan=True)
    assert touched >= 9                                                     # the planted values reached the outputs they were compared on


@pytest.mark.parametrize("sigma", [None, 1.2])
def test_a_plane_of_nan_leaves_its_neighbours_alone(eng, sigma):
    ny, nx = RB.SHAPES[3]
    v, lat, lon = RB.stack(ny, nx, 3)
    v[1] = np.nan
    want = ("mask", "eigmin", "dt", "eigvec", "grad")
    res = eng.ridges_batch(v, lat, lon, sigma=sigma, tolerance=RB.TOL, isglobal=True, want=want)
    for m in (0, 2):
        solo = eng.ridges_batch(v[m], lat, lon, sigma=sigma, tolerance=RB.TOL, isglobal=True, want=want)
        for k in want:
            a, b = res[k][m].cpu().numpy(), solo[k].cpu().numpy()
            assert np.isfinite(b).any(), k
            _assert_same(a, b, (k, m, sigma))
    assert np.isnan(res["dt"][1].cpu().numpy()).all() and np.isnan(res["grad"][1].cpu().numpy()).all()
    assert not res["eigmin"][1].cpu().numpy().any()                         # a Hessian of NaN is cleaned to zero (tools.py:92-93)


@pytest.mark.parametrize("isglobal", RB.GLOBAL)
def test_a_leading_dimension_of_length_one_equals_the_2d_call(isglobal):
    ny, nx = RB.SHAPES[-1]
    lat, lon = RB.grid(ny, nx)
    got = _find(_da(RB.plane(ny, nx, 1)[None], TLL, lat, lon, time=np.array([7.0])), sigma=1.2, isglobal=isglobal)
    want = per_plane(ny, nx, 1, isglobal, RB.SIGMAS.index(1.2))
    for name, a, b in zip(NAMES, got, want):
        assert a.values.shape == ((2, 1, ny, nx) if a.values.ndim == 4 else (1, ny, nx))
        _assert_same(a.values[:, 0] if a.values.ndim == 4 else a.values[0], b, (name, isglobal))


# ------------------------------------------------------------------ dimension order and coordinates
@pytest.mark.parametrize("dims", [TLL, ("latitude", "time", "longitude")])
def test_dimension_order_and_coordinates(dims):
    """A record with descending latitudes and rolled longitudes: the results come back in its dimension order, with sorted
    latitude / longitude and its own time coordinate, and hold what the sorted stack gives."""
    ny, nx, n = *RB.SHAPES[3], 3
    v, lat, lon = RB.stack(ny, nx, n)
    times = np.array(["2000-01-01T00", "2000-01-01T06", "2000-01-01T12"], dtype="datetime64[h]")
    stored = _da(np.roll(v[:, ::-1], 9, axis=2), TLL, lat[::-1].copy(), np.roll(lon, 9), time=times).transpose(*dims)
    out = _find(stored, sigma=0.5, isglobal=True)
    ref = stacked(ny, nx, n, True, RB.SIGMAS.index(0.5))
    for name, o, r in zip(NAMES, out, ref):
        lead = tuple(d for d in o.dims if d in ("eigvectors", "elements"))
        assert o.dims == lead + dims, name
        assert np.array_equal(o.coords["latitude"], lat) and np.array_equal(o.coords["longitude"], lon), name
        assert np.array_equal(o.coords["time"], times) and o.name == "ftle"
        _assert_same(o.transpose(*lead, *TLL).values, r, name)


# ------------------------------------------------------------------ chaining on the device
def test_series_to_ridges_to_filter_without_a_host_copy(eng):
    torch = eng.torch
    ny, nx, nt, n = 23, 31, 12, 3
    lat, lon = np.linspace(-70.0, 70.0, ny), -180.0 + 360.0 / nx * np.arange(nx)
    LON, LAT = np.meshgrid(np.deg2rad(lon), np.deg2rad(lat))
    t = np.arange(nt)[:, None, None]
    u = 25.0 * np.cos(LAT) * (1 + 0.5 * np.sin(2 * LON + 0.3 * t))
    v = 12.0 * np.sin(3 * LON - 0.2 * t) * np.cos(LAT) ** 2
    field = eng.prepare_field(u, v, lat, lon, 1)
    sig = eng.lcs_series(field, lat, lon, 3600.0, 6, n, t0=0, t0_stride=2, SETTLS_order=1, interp_order=1)["sigma"]
    assert sig.is_cuda and tuple(sig.shape) == (n, ny, nx) and sig.dtype == torch.float64
    crit, thr = ["area", "mean_intensity"], [3, float(sig.mean())]
    res = eng.ridges_batch(sig, lat, lon, sigma=1.2, tolerance=RB.TOL, isglobal=True)
    kept = eng.filter_components(res["mask"], sig, crit, thr, connectivity=2, cyclic=True)
    assert kept.is_cuda and tuple(kept.shape) == (n, ny, nx)
    host = sig.cpu().numpy()
    for m in range(n):
        ridges = _find(_da(host[m], TLL[1:], lat, lon), sigma=1.2, isglobal=True)[0].values
        _assert_same(res["mask"][m].cpu().numpy(), ridges, ("mask", m))
        want = eng.filter_components(ridges, host[m], crit, thr, connectivity=2, cyclic=True).cpu().numpy()
        _assert_same(kept[m].cpu().numpy(), want, ("filtered", m))
    n_kept, n_ridge = int((kept != 0).sum()), int((res["mask"] != 0).sum())
    print(f"RIDGESBATCH chain: {n_ridge} ridge points of {n * ny * nx}, {n_kept} kept by the filter")
    assert 0 < n_kept <= n_ridge < n * ny * nx
