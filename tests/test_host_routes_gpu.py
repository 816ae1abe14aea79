"""The one-call host routes against the engine's route, bit for bit, on a field smaller than some kernels' tiles.

``lcs_host`` (``lc_lcs_host``: upload, pack, advect, smoothing, sigma and download in one C call) must give exactly what
``Engine.prepare_field`` + ``Engine.lcs`` (advect, smoothing, sigma, call by call) give on the same arrays: both describe the
same wind, images and options to the same kernels.  Every run is on a 24 x 40 field with 33 x 47 seeds -- no axis a
multiple of any tile, the field smaller than some tiles, so direct and LDS kernel families are both reached.  float64 at
this size keeps the reference's operation order on the host route (``LC_F64_AUTO``): the engine's field is prepared with
``fuse_levels=False``.  The 41-level runs compare the pipelined form of the route with its serial form, whole series and
sub-range; ``lcs_global_host`` without regridding and truncation is compared with ``lcs_host`` on the same arrays."""
import numpy as np
import pytest

from lagrangiancoherence_amd import flows

pytestmark = pytest.mark.gpu
DT = -900.0


@pytest.fixture(scope="module")
def eng():
    from lagrangiancoherence_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _wind(nt, dtype, ny=24, nx=40):
    u, v, lat, lon = flows.era5_like(nt=nt, ny=ny, nx=nx)
    slat, slon = flows.seed_grid(33, 47, lat, lon)
    return tuple(np.ascontiguousarray(a, dtype=dtype) for a in (u, v, lat, lon, slat, slon))


@pytest.fixture(scope="module")
def fields(eng):
    """The engine's packed field of a (dtype, order), prepared once."""
    made = {}

    def get(dtype, order):
        if (dtype, order) not in made:
            u, v, lat, lon, _, _ = _wind(5, dtype)
            made[dtype, order] = eng.prepare_field(u, v, lat, lon, order, fuse_levels=None if dtype == np.float32 else False)
        return made[dtype, order]
    return get


def _same(eng, fields, dtype, order, K, boundary, traj=False, gauss=None):
    from lagrangiancoherence_amd.engine import lcs_host
    u, v, lat, lon, slat, slon = _wind(5, dtype)
    kw = dict(SETTLS_order=K, interp_order=order, cyclic_xboundary=boundary == "cyclic",
              noncyclic_clamp=None if boundary == "cyclic" else boundary, gauss_sigma=gauss, return_traj=traj)
    out = lcs_host(u, v, lat, lon, DT, seed_lat=slat, seed_lon=slon, **kw)
    r = eng.lcs(fields(dtype, order), slat, slon, DT, **kw)
    for k in ("x_dep", "y_dep", "sigma") + (("traj_x", "traj_y") if traj else ()):
        got, want = out[k], r[k].cpu().numpy()
        assert got.dtype == want.dtype == dtype and got.shape == want.shape
        assert np.array_equal(got, want, equal_nan=True), (k, int((got != want).sum()), float(np.nanmax(np.abs(got - want))))
    assert np.isfinite(out["x_dep"]).all() and np.isfinite(out["sigma"]).any()


@pytest.mark.parametrize("boundary", ["cyclic", "pointwise"])
@pytest.mark.parametrize("K", [0, 4])
@pytest.mark.parametrize("order", [1, 3])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_lcs_host_is_the_engine_route_bit_for_bit(eng, fields, dtype, order, K, boundary):
    _same(eng, fields, dtype, order, K, boundary)


def test_lcs_host_under_the_references_outer_clamp(eng, fields):
    _same(eng, fields, np.float64, 1, 4, "reference_outer")


def test_lcs_host_with_trajectories(eng, fields):
    _same(eng, fields, np.float32, 3, 4, "cyclic", traj=True)


def test_lcs_host_with_smoothing(eng, fields):
    _same(eng, fields, np.float64, 3, 4, "cyclic", gauss=1.5)


@pytest.mark.parametrize("dtype,order", [(np.float32, 1), (np.float64, 3)])
def test_pipelined_form_is_the_serial_form(dtype, order):
    """41 levels: three level chunks travel while the one before is packed and advected; the sub-range moves its own levels."""
    from lagrangiancoherence_amd.engine import lcs_host
    u, v, lat, lon, slat, slon = _wind(41, dtype)
    kw = dict(SETTLS_order=4, interp_order=order, cyclic_xboundary=True, seed_lat=slat, seed_lon=slon, float64_fidelity="fast")
    for sub in ({}, dict(t0=3, nsteps=35)):
        a = lcs_host(u, v, lat, lon, DT, **kw, **sub)
        b = lcs_host(u, v, lat, lon, DT, pipeline=False, **kw, **sub)
        for k in ("x_dep", "y_dep", "sigma"):
            assert a[k].dtype == dtype and np.array_equal(a[k], b[k], equal_nan=True), (sub, k)
        assert np.isfinite(a["x_dep"]).all()


def test_lcs_global_host_without_preprocessing_is_lcs_host():
    from lagrangiancoherence_amd.engine import lcs_global_host, lcs_host
    u, v, lat, lon = (np.ascontiguousarray(a, dtype=np.float64) for a in flows.era5_like(nt=5, ny=45, nx=90))
    g = lcs_global_host(u, v, lat, lon, DT, SETTLS_order=4, interp_order=3, interp_to_common_grid=False, truncation=None)
    h = lcs_host(u, v, lat, lon, DT, SETTLS_order=4, interp_order=3, cyclic_xboundary=True)
    assert np.array_equal(g["latitude"], lat) and np.array_equal(g["longitude"], lon)
    for k in ("x_dep", "y_dep", "sigma"):
        assert g[k].dtype == np.float64 and np.array_equal(g[k], h[k], equal_nan=True), k
    assert np.isfinite(g["x_dep"]).all()
