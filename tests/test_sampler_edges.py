"""The sampler's edge battery (tests/sampler_edges.py) and the oracle on it.  No GPU, no build.

What the GPU tests rely on is proved here first: every battery position is a float32 number whose index coordinate is exact,
the oracle (scipy through ``O.xr_map_coordinates``) is finite and decides every jump the same way in float32 and float64
there, the constant rows are 0 exactly outside the field and nowhere else, and the generic grid's neighbours do straddle its
jumps."""
import re
import os

import numpy as np
import pytest

from oracle import lcs_oracle as O
from tests import sampler_edges as SE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_battery_is_the_40_by_40_cross_product_on_the_jumps():
    for n in (SE.NY_F, SE.NX_F):
        c = SE.axis_coords(n)
        s = n - 1
        assert c.size == 40 and np.signbit(c[1]) and c[1] == 0
        assert {0, 0.125, -0.125, 0.5, 1, 1.5, 2, 2.5, s - 0.5, s - 0.125, s, s + 0.125, s + 0.5, n, n + 0.5} <= set(c)
        for k in (-3, -2, -1, 2, 3, 1000):
            assert {k * s - 0.125, k * s, k * s + 0.125, k * s + 0.5} <= set(c)
        assert np.array_equal(c * 8, np.round(c * 8))               # multiples of 1/8: p = min + 8 c is an integer
        half = c[(c % 1) == 0.5]
        assert half.size >= 10 and (half < 0).any() and (half > s).any()      # an even order's window moves here
    cy, cx = SE.battery_coords()
    assert cy.size == 1600 and len(set(zip(cy.tolist(), cx.tolist()))) == 39 * 39        # 0 and -0.0 are one number
    assert SE.inside().mean() == pytest.approx(121 / 1600)


@pytest.mark.parametrize("order", SE.ORDERS)
def test_dyadic_positions_are_float32_numbers_with_exact_index_coordinates(order):
    lat, lon = SE.dyadic_grid()
    cy, cx = SE.battery_coords()
    for shift in (0.0, 0.125 * (SE.NT - 1)):
        px, py = SE.battery(order, shift)
        assert px.shape == py.shape == (2 * order + 3, 1600) and SE.pole_mask(order).sum() == 2 * order
        assert np.array_equal(px.astype(np.float32).astype(np.float64), px) and np.array_equal(py.astype(np.float32).astype(np.float64), py)
        # numpy's order (the oracle, the float64 kernel) in both dtypes, and the float32 kernel's (p - min) * sx
        for dt in (np.float64, np.float32):
            x, y, la, lo = (a.astype(dt) for a in (px, py, lat, lon))
            assert np.array_equal(SE.NX_F * (x - lo.min()) / (lo.max() - lo.min()), np.tile(cx + shift, (len(x), 1)))
            assert np.array_equal(SE.NY_F * (y - la.min()) / (la.max() - la.min()), np.tile(cy + shift, (len(y), 1)))
        sx = np.float32(SE.NX_F / 256.0)
        assert np.array_equal((px.astype(np.float32) - np.float32(lon[0])) * sx, np.tile(cx + shift, (len(px), 1)))


@pytest.mark.parametrize("order", SE.ORDERS)
def test_the_oracle_on_the_dyadic_battery(order):
    """The oracle alone: finite in both dtypes; the constant rows are exactly 0 outside ``[0, s]^2`` and non-zero inside (at
    least 5 % of a row is inside); no interior-row sample is exactly 0; and the float32 oracle decides no jump the other way:
    it stays within the rounding of its float32 result (half an ulp of |value| < 8: 4.8e-7; a side flip is O(1))."""
    lat, lon = SE.dyadic_grid()
    u, _ = SE.dyadic_field()
    px, py = SE.battery(order)
    pole, inside = SE.pole_mask(order), SE.inside()
    assert inside.mean() >= 0.05
    f32 = u[SE.LEVEL].astype(np.float32)
    o64 = O.xr_map_coordinates(f32.astype(np.float64), lat, lon, px, py, order=order)
    o32 = O.xr_map_coordinates(f32, lat.astype(np.float32), lon.astype(np.float32), px.astype(np.float32), py.astype(np.float32), order=order)
    assert o32.dtype == np.float32 and o64.dtype == np.float64
    for o in (o64, o32, O.xr_map_coordinates(u[SE.LEVEL], lat, lon, px, py, order=order)):
        assert np.isfinite(o).all()
        assert np.all(o[pole][:, ~inside] == 0) and np.all(o[pole][:, inside] != 0)
        assert np.all(o[~pole] != 0)
    assert np.abs(o64).max() < 8
    err = np.abs(o32.astype(np.float64) - o64).max()
    print(f"order {order}: float32 oracle within {err:.2e} of the float64 one on the battery")
    assert err <= 4.8e-7


def test_the_dyadic_battery_crosses_every_jump_of_the_index_map():
    """On a wrap row the sample at ``c = k s + 0.125`` is next to node 0 and the one at ``k s - 0.125`` next to node s: white
    noise tells them apart, so a period of ``n`` instead of ``n - 1``, or ``>=`` for ``>``, shows as an O(1) error."""
    lat, lon = SE.dyadic_grid()
    u, _ = SE.dyadic_field()
    f = u[SE.LEVEL]
    px, py = SE.battery(1)
    o = O.xr_map_coordinates(f, lat, lon, px, py, order=1)[2].reshape(40, 40)      # an interior row, [cy index, cx index]
    cy, cx = SE.axis_coords(SE.NY_F), SE.axis_coords(SE.NX_F)
    iy = int(np.flatnonzero(cy == 1.0)[0])
    s = SE.NX_F - 1
    for k in (-3, -2, -1, 1, 2, 3, 1000):
        at, lo, hi = (int(np.flatnonzero(cx == v)[0]) for v in (k * s, k * s - 0.125, k * s + 0.125))
        # scipy's map: identity on [0, s], so c = s is node s; c = k s is sent to s for k < 0 (c += s (|k| + 1)), to 0 for k > 1
        want = f[1, s] if k <= 1 else f[1, 0]
        assert o[iy, at] == want, k
        assert o[iy, lo] == 0.875 * f[1, s] + 0.125 * f[1, s - 1], k
        assert o[iy, hi] == 0.875 * f[1, 0] + 0.125 * f[1, 1], k
    assert o[iy, int(np.flatnonzero(cx == 0.0)[0])] == f[1, 0]


@pytest.mark.parametrize("order", SE.GENERIC_ORDERS)
def test_generic_grid_neighbours_straddle_the_jumps(order):
    lat, lon = SE.generic_grid()
    u, _ = SE.generic_field()
    px, py, axis = SE.generic_points(order)
    assert px.shape == (2 * order + 3, 2 * 28 * SE.N_PARTNERS) and (axis == 0).sum() == (axis == 1).sum()
    for coord in (lat, lon):
        e = SE.edge_positions(coord).reshape(4, 7)
        assert e[3, 0] == coord.min()
        assert np.all(np.diff(e[:, [6, 4, 2, 0, 1, 3, 5]], axis=1) > 0)           # -1e-9, -2, -1 ulp, p, +1, +2 ulp, +1e-9
        c = coord.size * (e[:3, 0] - coord.min()) / (coord.max() - coord.min())
        assert np.abs(c - np.array([-1, 1, 2]) * (coord.size - 1)).max() < 1e-10
    o = O.xr_map_coordinates(u[SE.LEVEL], lat, lon, px, py, order=order)
    assert np.isfinite(o).all()
    # [axis, centre, offset, partner] on an interior row: the sample 1e-9 degrees below a jump and the one above differ by O(1)
    w = o[order + 1].reshape(2, 4, 7, SE.N_PARTNERS)
    jump = np.abs(w[:, :, 5] - w[:, :, 6]).max(axis=-1)
    assert np.all(jump > 0.1), jump
    # a constant row: 0 outside, so 0 at both sides of k = -1 and 2, on one side of c = s and of p = min
    z = (o[0].reshape(2, 4, 7, SE.N_PARTNERS) == 0).all(axis=-1)
    assert z[:, 0].all() and z[:, 2].all() and not z[:, 1, 6].any() and z[:, 1, 5].all() and z[:, 3, 6].all() and not z[:, 3, 5].any()
    assert not z[:, 3, 0].any()                                                     # p = min itself is inside


def test_the_sizes_restate_the_kernels_constants():
    with open(os.path.join(ROOT, "lagrangiancoherence_amd", "csrc", "advect.hip")) as fh:
        code = fh.read()
    assert re.search(r"constexpr int TRACER_DEPTH = %d;" % SE.TRACER_DEPTH, code)
    assert "(n + 255) / 256 < %d ? (n + 255) / 256 : %d" % (SE.SAMPLE_GRID_CAP, SE.SAMPLE_GRID_CAP) in code
    # the ring's loads are clamped to the last entry, the first fill and every refill: an unclamped one reads past the
    # trajectory into slots that are never sampled, so no value can show it (and no test may wait for a fault): pinned as text
    walk = code[code.index("void tracer_walk("):code.index("void __launch_bounds__(256) tracer_kernel(")]
    assert "const int last = n_levels - 1;" in walk
    assert "(size_t)(d < last ? d : last) * n + i" in walk
    assert "(size_t)(j + TRACER_DEPTH < last ? j + TRACER_DEPTH : last) * n + i" in walk
    assert len(re.findall(r"\bp[xy]\[", walk)) == 4 and len(re.findall(r"\bp[xy]\[e\]", walk)) == 4
    assert SE.STRIDE_POSITIONS > SE.SAMPLE_GRID_CAP * SE.SAMPLE_BLOCK and SE.STRIDE_POSITIONS % SE.SAMPLE_BLOCK
    d = SE.TRACER_DEPTH
    assert {1, d - 1, d, d + 1, 2 * d - 1, 2 * d + 1} <= set(SE.RING_LEVELS) and max(SE.RING_LEVELS) <= SE.NT
