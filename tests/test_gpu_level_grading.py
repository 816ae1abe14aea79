"""Graded level counts on the device (lc_ctx_set_level_grading): the two-seed order-1 kernel takes each workgroup's levels
from its dispatch position -- some ranges empty, some one level long, some longer than a chunk -- and the positions are
those of one launch and of uniform chunks, bit for bit.  A 48 x 96-node float32 field with 41 levels, 200 x 136 seeds: no
multiple of the 8 x 64-seed workgroup patch, pole rows present, 68 tiles in a grid of 72 blocks, three launches of 14
levels (tests/c/level_grading_test.cpp checks that this very plan has empty and one-level ranges)."""
import pytest
import torch

from lagrangiancoherence_amd import flows

pytestmark = pytest.mark.gpu

NT, DT = 42, -3600.0
KW = dict(SETTLS_order=4, interp_order=1)


@pytest.fixture(scope="module")
def setup():
    from lagrangiancoherence_amd.engine import Engine
    eng = Engine(0)
    u, v, lat, lon = flows.era5_like(nt=NT, ny=48, nx=96)
    slat, slon = flows.seed_grid(200, 136, lat, lon)
    f = eng.prepare_field(u, v, lat, lon, 1)
    eng.set_lds_tiles(1)        # the two-seed kernel whatever the size
    yield eng, f, slat, slon
    eng.close()


def _reset(eng):
    eng.set_level_chunk(-1)
    eng.set_level_grading(0, -1, -1)


@pytest.mark.parametrize("boundary", [dict(cyclic_xboundary=True), dict(cyclic_xboundary=False, noncyclic_clamp="pointwise")],
                         ids=["cyclic", "pointwise"])
def test_graded_launches_equal_one_launch_and_uniform_chunks(setup, boundary):
    eng, f, slat, slon = setup
    try:
        eng.set_level_chunk(0)
        x0, y0 = eng.advect(f, slat, slon, DT, **KW, **boundary)
        assert eng.last_advect_launches() == 1
        eng.set_level_chunk(13)
        x13, y13 = eng.advect(f, slat, slon, DT, **KW, **boundary)
        assert eng.last_advect_launches() == 4
        assert torch.equal(x13, x0) and torch.equal(y13, y0)
        eng.set_level_chunk(-1)
        for zone, depth in ((8, 14), (1000, 14), (8, 5), (8, 1)):
            eng.set_level_grading(14, zone, depth)
            assert eng.level_grading == (14, zone, depth)
            x, y = eng.advect(f, slat, slon, DT, **KW, **boundary)
            assert eng.last_advect_launches() == 3, (zone, depth)
            assert eng.last_advect_kernel() == "advect_lds2_kernel<4, %s, 0>" % ("true" if boundary["cyclic_xboundary"] else "false")
            assert torch.equal(x, x0) and torch.equal(y, y0), (zone, depth)
            assert torch.equal(x, x13) and torch.equal(y, y13), (zone, depth)
    finally:
        _reset(eng)


def test_graded_continuation_from_given_positions_in_place(setup):
    """lc_advect_from: a range that begins at the call's first level starts from x_start -- also in a later launch (its
    earlier ranges were empty), and also when x_start is x_out."""
    eng, f, slat, slon = setup
    try:
        eng.set_level_chunk(0)
        xa, ya = eng.advect(f, slat, slon, DT, nsteps=7, **KW)
        xw, yw = eng.advect(f, slat, slon, DT, t0=7, nsteps=NT - 1 - 7, start=(xa, ya), **KW)
        xf, yf = eng.advect(f, slat, slon, DT, **KW)
        assert torch.equal(xw, xf) and torch.equal(yw, yf)
        eng.set_level_chunk(-1)
        eng.set_level_grading(12, 8, 12)
        xg, yg = eng.advect(f, slat, slon, DT, t0=7, nsteps=NT - 1 - 7, start=(xa, ya), **KW)
        assert eng.last_advect_launches() == 3
        assert torch.equal(xg, xw) and torch.equal(yg, yw)
        xi, yi = xa.clone(), ya.clone()
        eng.advect(f, slat, slon, DT, t0=7, nsteps=NT - 1 - 7, start=(xi, yi), out=(xi, yi), **KW)
        assert eng.last_advect_launches() == 3
        assert torch.equal(xi, xw) and torch.equal(yi, yw)
    finally:
        _reset(eng)


def test_calls_that_do_not_qualify_make_the_launches_they_made_before(setup):
    eng, f, slat, slon = setup
    try:
        made = {}
        for grading in ((0, -1, 0), (14, 8, 14)):       # off; forced
            eng.set_level_grading(*grading)
            eng.set_level_chunk(-1)
            out = eng.advect(f, slat, slon, DT, return_traj=True, **KW)          # trajectories: uniform chunks
            made[grading, "traj"] = (eng.last_advect_launches(), eng.last_advect_kernel(), [t.clone() for t in out])
            eng.advect(f, slat, slon, DT, cyclic_xboundary=False, **KW)          # the reference's outer clamp: its fixed chunks
            made[grading, "outer"] = (eng.last_advect_launches(), eng.last_advect_kernel())
            eng.set_level_chunk(13)                                               # an explicit level chunk is the A/B switch
            eng.advect(f, slat, slon, DT, **KW)
            made[grading, "explicit"] = (eng.last_advect_launches(), eng.last_advect_kernel())
        off, on = (0, -1, 0), (14, 8, 14)
        assert made[off, "traj"][0] == made[on, "traj"][0] == 1                   # 27 200 seeds: one launch by size
        assert made[off, "traj"][1] == made[on, "traj"][1]
        for a, b in zip(made[off, "traj"][2], made[on, "traj"][2]):
            assert torch.equal(a, b)
        assert made[off, "outer"] == made[on, "outer"]
        assert made[off, "explicit"] == made[on, "explicit"] == (4, "advect_lds2_kernel<4, true, 0>")
        with pytest.raises(ValueError):
            eng.set_level_grading(-1, 8, 8)
    finally:
        _reset(eng)
