"""The out-of-tile path of the two-seed order-1 kernel's iterations (advect_lds2_kernel, tall patches and whole-line
stores): a sample whose window leaves the wave's 16 x 8-node tile is gathered from global memory -- at the common path's
tap when its window origin lies in [1, n - 2] on both axes, through the whole exact sequence (clamps, scipy's wrap map)
otherwise.  A seed's bits must not depend on which of the three served it, so every call here is made on the two-seed
kernel (``set_lds_tiles(1)``, the kernel's name is the witness) and must equal, bit for bit, the same call on the
direct-gather kernel (``set_lds_tiles(0)``: the exact sequence for every sample) and on the one-seed tile kernel
(``set_lds_tiles(2)``: one seed per lane, another tile per wave).

The 48 x 96-node, 41-level field of tests/test_gpu_level_grading_matrix.py (3.75 degrees a cell, longitudes -180 ... 176.25,
latitudes -88.125 ... 88.125).  A wave of the two-seed kernel holds 8 columns x 16 rows of seeds, lane = column + 8 row, the
lane's second seed 8 rows further down; its tile holds the window origins of 15 x 7 nodes around the centre seed.  Seed grids:
  dense       328 x 136 seeds spanning the field: what the flow stretches leaves the tile, the rest does not;
  sparse_lat  16 rows 0.6 cells apart (9 node rows) x 136 columns: rows 0-1 (first seeds) and 14-15 (second seeds, other
              lanes) start outside the tile -- out-of-tile seeds in disjoint lanes;
  sparse_lon  8 columns 2.5 cells apart (17.5 nodes) x 16 rows: the end columns start outside, both seeds of a lane;
  edges       window origins 0 and n - 2 on each axis (and the cells beyond n - 1 that the cyclic wrap serves), one seed
              column exactly on -180;
  nan         `edges` continued from its own positions with one latitude made NaN.
The sparse grids and `edges` are row windows of a taller global grid, so that none of their rows is a pole row."""
import numpy as np
import pytest
import torch

from lagrangiancoherence_amd import flows
from tests.test_gpu_level_grading_matrix import BOUNDARIES, DT, NT, NX, NY, tall_instance

pytestmark = pytest.mark.gpu

CELL = 3.75
LAT0, LON0 = -88.125, -180.0           # node (0, 0)
ONE_SEED, DIRECT = "advect_lds_kernel<1, ", "advect_kernel_f32"      # (families: the instance is the call's K and boundary)


def _grids(lat, lon):
    f = np.float32
    dense = flows.seed_grid(NY, NX, lat, lon)
    cols = dense[1]
    sparse_lat = ((LAT0 + CELL * (20.0 + 0.6 * np.arange(16))).astype(f), cols)
    sparse_lon = ((LAT0 + CELL * (22.0 + 0.25 * np.arange(16))).astype(f), (LON0 + CELL * (30.2 + 2.5 * np.arange(8))).astype(f))
    # latitudes: cells 0, 1, n - 3, n - 2 (four offsets each) and mid-latitudes between them; longitudes: exactly -180, cells 0,
    # 1, n - 2, n - 1 (beyond the last node: the cyclic wrap's) and the middle
    ey = [0.0, 0.3, 0.6, 0.9, 1.0, 1.2, 1.5, 1.9, 14.1, 18.4, 23.5, 23.7, 28.2, 32.6, 40.3, 44.2, 44.6, 44.9, 45.0, 45.3, 45.7, 45.99, 46.2, 46.9]
    ex = [0.0, 0.05, 0.3, 0.6, 0.95, 1.0, 1.4, 47.5, 93.2, 93.9, 94.0, 94.3, 94.7, 94.99, 95.0, 95.5]
    edges = ((LAT0 + CELL * np.array(ey)).astype(f), (LON0 + CELL * np.array(ex)).astype(f))
    assert edges[1][0] == f(-180.0)
    return {"dense": dense, "sparse_lat": sparse_lat, "sparse_lon": sparse_lon, "edges": edges}


class Case:
    def __init__(self, eng, f, grids):
        self.eng, self.f, self.grids = eng, f, grids

    def three_ways(self, grid, K, boundary, want=None, equal_nan=False, **kw):
        """The call on the two-seed kernel, equal to the direct-gather and the one-seed kernels' bit for bit."""
        eng = self.eng
        slat, slon = self.grids[grid]
        if grid != "dense":     # a row window of a taller grid: no pole rows
            kw.update(row0=1, ny_global=len(slat) + 2)
        names = {1: want or tall_instance(K, boundary == "cyclic"), 0: DIRECT, 2: ONE_SEED}
        got = {}
        try:
            for mode in (1, 0, 2):
                eng.set_lds_tiles(mode)
                got[mode] = eng.advect(self.f, slat, slon, DT, SETTLS_order=K, interp_order=1, **BOUNDARIES[boundary], **kw)
                name = eng.last_advect_kernel()
                assert name == names[1] if mode == 1 else name.startswith(names[mode]), (grid, K, boundary, mode, name)
        finally:
            eng.set_lds_tiles(-1)
        for mode in (0, 2):
            for a, b in zip(got[1], got[mode]):
                if equal_nan:       # NaN where the other has NaN, then torch.equal on the rest
                    assert torch.equal(torch.isnan(a), torch.isnan(b)), (grid, K, boundary, mode)
                    a, b = torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0)
                assert torch.equal(a, b), (grid, K, boundary, mode)
        return got[1]


@pytest.fixture(scope="module")
def case():
    from lagrangiancoherence_amd.engine import Engine
    u, v, lat, lon = flows.era5_like(nt=NT, ny=48, nx=96)
    assert abs(float(lat[0]) - LAT0) < 1e-4 and float(lon[0]) == LON0 and abs(float(lat[1] - lat[0]) - CELL) < 1e-4
    eng = Engine(0)
    yield Case(eng, eng.prepare_field(u, v, lat, lon, 1), _grids(lat, lon))
    eng.close()


@pytest.mark.parametrize("boundary", ["cyclic", "pointwise"])
@pytest.mark.parametrize("K", [4, 1])
@pytest.mark.parametrize("grid", ["dense", "sparse_lat", "sparse_lon", "edges"])
def test_out_of_tile_samples_equal_the_other_kernels(case, grid, K, boundary):
    x, y = case.three_ways(grid, K, boundary)
    assert bool(torch.isfinite(x).all()) and bool(torch.isfinite(y).all())


@pytest.mark.parametrize("boundary", ["cyclic", "pointwise"])
@pytest.mark.parametrize("K", [4, 1])
def test_a_nan_seed_equals_the_other_kernels(case, K, boundary):
    """Continued from the positions after 7 levels with one latitude NaN.  A NaN coordinate converts to index 0, so every
    iteration's window test fails for it and the exact sequence clamps the latitude first (Q8); what the sample at a NaN
    fraction makes of the longitude is the reference's business -- here it has to be the same in all three kernels, NaN for
    NaN (``equal_nan``: torch.equal on the NaN masks and on everything else), and no other seed may be touched by it."""
    eng = case.eng
    slat, slon = case.grids["edges"]
    kw = dict(row0=1, ny_global=len(slat) + 2, **BOUNDARIES[boundary])
    eng.set_lds_tiles(0)
    try:
        xa, ya = eng.advect(case.f, slat, slon, DT, SETTLS_order=K, interp_order=1, nsteps=7, **kw)
        xw, yw = eng.advect(case.f, slat, slon, DT, SETTLS_order=K, interp_order=1, **kw)       # the same seeds without the NaN
    finally:
        eng.set_lds_tiles(-1)
    ya = ya.clone()
    ya[11, 7] = float("nan")
    x, y = case.three_ways("edges", K, boundary, equal_nan=True, t0=7, nsteps=NT - 1 - 7, start=(xa, ya))
    others = torch.ones_like(x, dtype=torch.bool)
    others[11, 7] = False
    assert torch.equal(x[others], xw[others]) and torch.equal(y[others], yw[others])
    assert bool(torch.isfinite(y).all()) and float(y.min()) >= float(slat.min()) - 1e-3     # Q8: the latitude is clamped, never NaN


@pytest.mark.parametrize("K", [4, 1])
def test_whole_line_stores_take_the_same_path(case, K):
    """With trajectories the two-seed kernel runs its PATCH_LINES form (136 columns: whole-line stores), same iterations."""
    out = case.three_ways("dense", K, "cyclic", want="advect_lds2_kernel<%d, true, 2>" % (4 if K == 4 else -1), return_traj=True)
    assert len(out) == 4 and tuple(out[2].shape) == (NT, NY, NX)
