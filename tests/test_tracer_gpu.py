"""Scalar tracers sampled along the engine's trajectories (lc_tracer_sample, Engine.advect_tracer, the drop-in's
``parcel_propagation(..., C=)``) on the MI355X.

Expected values come from the existing oracle: the trajectories of ``O.parcel_propagation(return_traj=True)`` (or the
GPU's own trajectories, to judge the sampler on its own) followed by ``O.xr_map_coordinates`` per level."""
import numpy as np
import pandas as pd
import pytest

from lagrangiancoherence_amd import dropin, flows
from oracle import lcs_oracle as O
from tests import labelled

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from lagrangiancoherence_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _np(t):
    return t.cpu().numpy()


def _tracer(u, v, lat):
    """A smooth tracer on the wind's grid (a column-water-vapour-like field: magnitude + latitude profile)."""
    return np.hypot(u, v) + 20.0 * np.cos(np.deg2rad(np.asarray(lat, np.float64)))[None, :, None]


def _oracle_levels(c, lat, lon, tx, ty, t0, order):
    return np.stack([O.xr_map_coordinates(c[t0 + i], lat, lon, tx[i], ty[i], order=order) for i in range(tx.shape[0])])


def _mean_within_one_ulp(mean, per_level):
    ref = per_level.astype(np.float64).mean(axis=0).astype(mean.dtype)
    assert np.all(np.abs(mean.astype(np.float64) - ref) <= np.spacing(np.abs(ref)).astype(np.float64)), \
        np.abs(mean.astype(np.float64) - ref).max()


CFG1 = flows.config1()


# ------------------------------------------------------------------ 1, 5, 9: the sampler on the GPU's own trajectories
@pytest.mark.parametrize("dtype,order", [(np.float64, o) for o in (1, 2, 3, 4, 5)] + [(np.float32, 1), (np.float32, 3)])
@pytest.mark.parametrize("cyclic", [True, False])
@pytest.mark.parametrize("sign", [-1, 1])
def test_sampler_on_own_trajectories_vs_oracle(eng, dtype, order, cyclic, sign):
    u, v, lat, lon = CFG1
    c64 = _tracer(u, v, lat)
    cmax = np.abs(c64).max()
    field = eng.prepare_field(u.astype(dtype), v.astype(dtype), lat.astype(dtype), lon.astype(dtype), order)
    tr = eng.prepare_tracer(c64.astype(dtype), None, lat.astype(dtype), lon.astype(dtype), order, dtype=field.dtype)
    for K in (0, 4):
        for slat, slon in ((lat, lon), flows.seed_grid(150, 300, lat, lon)):
            r = eng.advect_tracer(field, tr, slat.astype(dtype), slon.astype(dtype), sign * 6 * 3600.0, SETTLS_order=K,
                                  interp_order=order, cyclic_xboundary=cyclic, return_traj=True, tracer_traj=True)
            assert eng.last_tracer_kernel() == f"tracer_kernel<{np.dtype(dtype).name.replace('float32', 'float').replace('float64', 'double')}, {order}>"
            tx, ty, cg, mean = _np(r["traj_x"]), _np(r["traj_y"]), _np(r["c"]), _np(r["mean"])
            assert r["c2"] is None and r["mean2"] is None and cg.shape == tx.shape == (8, len(slat), len(slon))
            assert np.array_equal(_np(r["x"]), tx[-1]) and np.array_equal(_np(r["y"]), ty[-1])
            if dtype == np.float64:
                want = _oracle_levels(c64, lat, lon, tx, ty, 0, order)
                assert np.abs(cg - want).max() <= 1e-12 * cmax, (K, np.abs(cg - want).max())
            else:
                # judged against the float64 answer on the same positions, inside the float32 oracle's own error there
                want = _oracle_levels(c64, lat, lon, tx.astype(np.float64), ty.astype(np.float64), 0, order)
                o32 = _oracle_levels(c64.astype(np.float32), lat.astype(np.float32), lon.astype(np.float32), tx, ty, 0, order)
                e_gpu = np.abs(cg - want).max()
                e_or = np.abs(o32 - want).max()
                print(f"float32 order {order} K={K} seeds {len(slat)}x{len(slon)}: max err {e_gpu:.3e} "
                      f"(float32 oracle's own {e_or:.3e}, max|C| {cmax:.1f})")
                assert e_gpu <= 4 * e_or + 1e-6 * cmax, (K, e_gpu, e_or)
            _mean_within_one_ulp(mean, cg)


# ------------------------------------------------------------------ 2: end to end against the oracle
@pytest.mark.parametrize("order", [1, 3])
def test_end_to_end_config1_vs_oracle(eng, order):
    u, v, lat, lon = CFG1
    c = _tracer(u, v, lat)
    field = eng.prepare_field(u, v, lat, lon, order, fuse_levels=False)        # numpy / scipy's operation order
    tr = eng.prepare_tracer(c, None, lat, lon, order)
    r = eng.advect_tracer(field, tr, lat, lon, -6 * 3600.0, SETTLS_order=4, interp_order=order, cyclic_xboundary=True,
                          tracer_traj=True)
    tx, ty = O.parcel_propagation(u, v, lat, lon, timestep=-6 * 3600.0, SETTLS_order=4, interp_order=order,
                                  cyclic_xboundary=True, return_traj=True)
    want = _oracle_levels(c, lat, lon, tx, ty, 0, order)
    tol = 1e-10 * (c.max() - c.min())
    assert np.abs(_np(r["c"]) - want).max() <= tol
    assert np.abs(_np(r["mean"]) - want.mean(axis=0)).max() <= tol


# ------------------------------------------------------------------ 3: positions unchanged by the tracer
def _same_positions(eng, field, tr, slat, slon, order, K, ts):
    base = eng.advect(field, slat, slon, ts, K, order, True)
    k_plain = eng.last_advect_kernel()
    r = eng.advect_tracer(field, tr, slat, slon, ts, K, order, True)
    k_tracer = eng.last_advect_kernel()
    assert eng.torch.equal(r["x"], base[0]) and eng.torch.equal(r["y"], base[1])
    del base
    bt = eng.advect(field, slat, slon, ts, K, order, True, return_traj=True)
    k_traj = eng.last_advect_kernel()
    rt = eng.advect_tracer(field, tr, slat, slon, ts, K, order, True, return_traj=True)
    assert eng.last_advect_kernel() == k_traj
    for a, b in zip(("x", "y", "traj_x", "traj_y"), bt):
        assert eng.torch.equal(rt[a], b), a
    return k_plain, k_tracer, k_traj


def test_positions_bit_identical_with_tracer_c3_shape(eng):
    torch = eng.torch
    u, v, lat, lon = flows.era5_like_on_device(torch, eng.device, nt=9)
    slat, slon = flows.seed_grid(4096, 4096, lat, lon)
    field = eng.prepare_field(u, v, lat, lon, 1)
    tr = eng.prepare_tracer(torch.hypot(u, v), None, lat, lon, 1, dtype=field.dtype)
    names = _same_positions(eng, field, tr, slat.astype(np.float32), slon.astype(np.float32), 1, 4, -900.0)
    # the plain call's kernel (BASELINE configs[2]: two seeds per lane); the tracer call's ring needs trajectories stored
    assert names[0] == "advect_lds2_kernel<4, true, 0>", names
    assert names[1] == names[2], names


def test_positions_bit_identical_with_tracer_c2_shape(eng):
    torch = eng.torch
    u, v, lat, lon = flows.config2_on_device(torch, eng.device, n=1024, nt=9)
    field = eng.prepare_field(u, v, lat, lon, 1)
    tr = eng.prepare_tracer(torch.hypot(u, v), None, lat, lon, 1, dtype=field.dtype)
    names = _same_positions(eng, field, tr, lat, lon, 1, 4, -3600.0)
    assert names[1] == names[2], names


# ------------------------------------------------------------------ 4: chunked ring vs whole series
@pytest.mark.parametrize("dtype,order", [(np.float64, 3), (np.float32, 1)])
def test_ring_chunks_equal_the_whole_series(eng, dtype, order):
    u, v, lat, lon = (a.astype(dtype) for a in CFG1)
    c = _tracer(u, v, lat).astype(dtype)
    field = eng.prepare_field(u, v, lat, lon, order)
    tr = eng.prepare_tracer(c, 2 * c + 1, lat, lon, order)
    whole = eng.advect_tracer(field, tr, lat, lon, -3600.0, 2, order, True)
    assert whole["x"].shape == (89, 180)
    for steps in (1, 2, 3):            # ring of steps + 1 entries: chunks of 1, 2 and 3 steps over the 7
        ring = (steps + 1) * 2 * 89 * 180 * np.dtype(dtype).itemsize
        r = eng.advect_tracer(field, tr, lat, lon, -3600.0, 2, order, True, ring_bytes=ring)
        for k in ("x", "y", "mean", "mean2"):
            assert eng.torch.equal(r[k], whole[k]), (steps, k)
    full = eng.advect_tracer(field, tr, lat, lon, -3600.0, 2, order, True, tracer_traj=True)
    assert eng.torch.equal(full["mean"], whole["mean"]) and eng.torch.equal(full["mean2"], whole["mean2"])
    _mean_within_one_ulp(_np(full["mean2"]), _np(full["c2"]))


# ------------------------------------------------------------------ 6: two tracers in one call
@pytest.mark.parametrize("dtype,order", [(np.float64, 1), (np.float64, 3), (np.float32, 1), (np.float32, 3), (np.float64, 5)])
def test_two_tracers_equal_two_single_calls(eng, dtype, order):
    u, v, lat, lon = (a.astype(dtype) for a in CFG1)
    c1 = _tracer(u, v, lat).astype(dtype)
    c2 = (np.sin(np.deg2rad(lon))[None, None, :] * u).astype(dtype)
    field = eng.prepare_field(u, v, lat, lon, order)
    both = eng.advect_tracer(field, eng.prepare_tracer(c1, c2, lat, lon, order), lat, lon, 3600.0, 1, order, False,
                             tracer_traj=True)
    one = eng.advect_tracer(field, eng.prepare_tracer(c1, None, lat, lon, order), lat, lon, 3600.0, 1, order, False,
                            tracer_traj=True)
    two = eng.advect_tracer(field, eng.prepare_tracer(c2, None, lat, lon, order), lat, lon, 3600.0, 1, order, False,
                            tracer_traj=True)
    t = eng.torch
    assert t.equal(both["c"], one["c"]) and t.equal(both["mean"], one["mean"])
    assert t.equal(both["c2"], two["c"]) and t.equal(both["mean2"], two["mean"])


# ------------------------------------------------------------------ 7: row sharding
@pytest.mark.parametrize("order", [1, 3])
def test_row_blocks_equal_the_whole_grid(eng, order):
    u, v, lat, lon = CFG1
    c = _tracer(u, v, lat)
    field = eng.prepare_field(u, v, lat, lon, order)
    tr = eng.prepare_tracer(c, None, lat, lon, order)
    whole = eng.advect_tracer(field, tr, lat, lon, -3600.0, 2, order, True, return_traj=True, tracer_traj=True)
    for a, b in ((0, 10), (1, 40), (40, 86), (79, 89)):          # both poles' rows, and blocks that cut into them
        tx = whole["traj_x"][:, a:b].contiguous()
        ty = whole["traj_y"][:, a:b].contiguous()
        (cb, _), (mb, _) = eng.sample_tracer(tr, tx, ty, 0, order, row0=a, ny_global=89, mean_count=8)
        assert eng.torch.equal(cb, whole["c"][:, a:b]) and eng.torch.equal(mb, whole["mean"][a:b]), (a, b)
        # and through advect_tracer on the row block itself (cyclic: no flag all-reduce needed)
        r = eng.advect_tracer(field, tr, lat[a:b], lon, -3600.0, 2, order, True, row0=a, ny_global=89)
        assert eng.torch.equal(r["mean"], whole["mean"][a:b]), (a, b)


# ------------------------------------------------------------------ 8: the drop-in
@pytest.mark.parametrize("timestep", [-6 * 3600, 6 * 3600])
def test_dropin_parcel_propagation_with_tracer(timestep):
    u, v, lat, lon = CFG1
    c = _tracer(u, v, lat)
    times = pd.date_range("2000-01-01", periods=u.shape[0], freq="6h").values
    coords = {"latitude": lat, "longitude": lon, "time": times}
    U = labelled.DataArray(u.transpose(1, 2, 0), ["latitude", "longitude", "time"], coords, name="u")
    V = labelled.DataArray(v.transpose(1, 2, 0), ["latitude", "longitude", "time"], coords, name="v")
    Cl = labelled.DataArray(c, ["time", "latitude", "longitude"], coords, name="tcwv")
    kw = dict(timestep=timestep, propdim="time", SETTLS_order=4, cyclic_xboundary=True, verbose=False, interp_order=3)
    x0, y0 = dropin.parcel_propagation(U, V, return_traj=True, **kw)
    x, y, cs = dropin.parcel_propagation(U, V, return_traj=True, C=Cl, **kw)
    assert np.array_equal(x.values, x0.values) and np.array_equal(y.values, y0.values)
    assert cs.dims == x.dims and np.array_equal(cs.coords["time"], x.coords["time"])
    want = _oracle_levels(c, lat, lon, x.values, y.values, 0, 3)
    assert np.abs(cs.values - want).max() <= 1e-12 * np.abs(c).max()
    tx, ty = O.parcel_propagation(u, v, lat, lon, timestep=timestep, SETTLS_order=4, interp_order=3, cyclic_xboundary=True,
                                  return_traj=True)
    assert np.abs(cs.values - _oracle_levels(c, lat, lon, tx, ty, 0, 3)).max() <= 1e-10 * (c.max() - c.min())
    xl, yl, cl = dropin.parcel_propagation(U, V, C=Cl, **kw)
    assert np.array_equal(xl.values, x.values[-1]) and np.array_equal(cl.values, cs.values[-1])
    assert cl.coords["time"] == xl.coords["time"]


# ------------------------------------------------------------------ 10: memory cap at full C3 size
def test_c3_mean_only_stays_under_the_ring_cap(eng):
    torch = eng.torch
    u, v, lat, lon = flows.era5_like_on_device(torch, eng.device, nt=97)
    slat, slon = (a.astype(np.float32) for a in flows.seed_grid(4096, 4096, lat, lon))
    field = eng.prepare_field(u, v, lat, lon, 1)
    cd = torch.hypot(u, v)
    tr = eng.prepare_tracer(cd, None, lat, lon, 1, dtype=field.dtype)
    n = 4096 * 4096
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated(eng.device)
    torch.cuda.reset_peak_memory_stats(eng.device)
    r = eng.advect_tracer(field, tr, slat, slon, -900.0, 4, 1, True)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated(eng.device) - base
    # the documented cap: the ring, plus x, y and the mean (4 bytes each) and the float64 sums (8) per seed, and the
    # seed coordinates on the device
    cap = eng.TRACER_RING_BYTES + n * (3 * 4 + 8) + (4096 + 4096) * 4
    print(f"C3 mean-only: peak extra {extra / 2**30:.3f} GiB, cap {cap / 2**30:.3f} GiB "
          f"(the whole series would be {97 * 2 * 4 * n / 2**30:.1f} GiB of positions)")
    assert extra <= cap, (extra, cap)
    mean = r["mean"]
    # seeded rows (both poles' and a few inside) against the oracle on the GPU's positions of the same rows
    rng = np.random.default_rng(20261016)
    ch = _np(cd).astype(np.float64)
    lat64, lon64 = lat.astype(np.float64), lon.astype(np.float64)
    for a in (0, 4095, *rng.integers(1, 4095, 3)):
        a = int(a)
        rb = eng.advect_tracer(field, tr, slat[a:a + 1], slon, -900.0, 4, 1, True, row0=a, ny_global=4096,
                               return_traj=True, tracer_traj=True)
        assert torch.equal(rb["mean"][0], mean[a]), a
        tx, ty, cg = _np(rb["traj_x"])[:, 0], _np(rb["traj_y"])[:, 0], _np(rb["c"])[:, 0]
        cols = np.sort(rng.choice(4096, 256, replace=False))
        # O.xr_map_coordinates classifies pole rows by the index of the rows it is given: a pole row alone is one
        # (order 1, 'constant'), an interior row is handed as the middle one of three copies ('wrap')
        pole = a < 1 or a >= 4095
        for i in range(97):
            px, py = tx[i, cols].astype(np.float64)[None], ty[i, cols].astype(np.float64)[None]
            if pole:
                want = O.xr_map_coordinates(ch[i], lat64, lon64, px, py, order=1)[0]
            else:
                want = O.xr_map_coordinates(ch[i], lat64, lon64, np.repeat(px, 3, 0), np.repeat(py, 3, 0), order=1)[1]
            err = np.abs(cg[i, cols] - want).max()
            assert err <= 1e-5 * np.abs(ch[i]).max(), (a, i, err)
