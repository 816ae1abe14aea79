"""Edge battery for the point sampler: ``sample<T, ORDER, WRAP, RAW>`` (``locate`` + ``fetch`` in ``csrc/advect.hip``) under
``lc_sample`` / ``lc_sample_raw``, ``lc_tracer_sample`` and the drop-in's ``tools.xr_map_coordinates``.

Plain data and helpers, imported by ``test_sampler_edges.py`` (the battery and the oracle on it, no GPU) and
``test_sampler_edges_gpu.py`` (the kernels against the oracle on it).

The sampler restates LCS/tools.py:11-41: an index map scaled by ``n`` instead of ``n - 1`` (Q2), scipy's ``'wrap'`` with period
``n - 1`` on interior seed rows, and order 1 with ``'constant'`` (exactly 0 outside ``[0, n - 1]``) on the first and last
``interp_order`` seed rows.  That map jumps: on wrap rows from the last node to node 0 as ``c`` passes ``n - 1`` (and every
``k (n - 1)``), on constant rows to 0 at ``c < 0`` and ``c > n - 1``, and even orders move their window at half-integers.  The
battery puts samples ON those jumps and next to them.

**Dyadic grid** (``dyadic_grid``): 16 x 32 nodes over spans of 128 and 256 degrees, so ``c = (p - min) / 8`` exactly, in
float64 and in float32, under numpy's operation order ``n * (p - min) / span`` and under the float32 kernel's
``(p - min) * sx`` alike; every battery position ``p = min + 8 c`` is a float32 number.  float32 is therefore tested on the
edges themselves, nothing left out.  The field is N(0, 1) white noise: a sample taken one node off is wrong by O(1).

**Generic grid** (``generic_grid``): config 1's 89 x 180 nodes (spans 176 and 358: not dyadic), float64 only.  The positions
whose index coordinate is ``k (n - 1)`` up to rounding, and ``p = min``, with their neighbours at 1 and 2 ulp and at 1e-9
degrees: the float64 kernel keeps numpy's operation order in the index map, so it must land on the oracle's side of every jump.
"""
import numpy as np

ORDERS = (1, 2, 3, 4, 5)
NY_F, NX_F, NT = 16, 32, 9
LEVEL = 2                       # the level the single-level tests sample
K_PERIODS = (-3, -2, -1, 2, 3, 1000)

# float64 tolerances, the project's own for an N(0, 1) field: 5e-13 at orders 1 and 3 (test_tools_helpers_vs_scipy_and_oracle),
# 20 * tol of test_general_spline_orders_vs_scipy_and_oracle at orders 2 (tol 1e-12) and 4, 5 (tol 5e-11)
TOL64 = {1: 5e-13, 3: 5e-13, 2: 2e-11, 4: 1e-9, 5: 1e-9}


def seed_rows(order):
    """Seed rows of a battery call: ``order`` pole rows at either end and 3 interior rows."""
    return 2 * order + 3


def pole_mask(order, rows=None):
    rows = seed_rows(order) if rows is None else rows
    i = np.arange(rows)
    return (i < order) | (i >= rows - order)


# ------------------------------------------------------------------ the dyadic grid
def dyadic_grid():
    return np.linspace(-64.0, 64.0, NY_F), np.linspace(-128.0, 128.0, NX_F)


def dyadic_field(seed=20261019):
    """``(u, v)``, each ``(NT, NY_F, NX_F)`` float64 N(0, 1) white noise."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((NT, NY_F, NX_F)), rng.standard_normal((NT, NY_F, NX_F))


def axis_coords(n):
    """The 40 index coordinates of one axis of ``n`` nodes (``s = n - 1``, the wrap period and the last node)."""
    s = float(n - 1)
    c = [0.0, -0.0, 0.125, -0.125, 0.5, 1.0, 1.5, 2.0, 2.5, s - 0.5, s - 0.125, s, s + 0.125, s + 0.5, float(n), n + 0.5]
    for k in K_PERIODS:
        c += [k * s - 0.125, k * s, k * s + 0.125, k * s + 0.5]
    return np.array(c, dtype=np.float64)


def battery_coords():
    """``(cy, cx)`` of the 1600 battery columns: the full cross product of the two axes' coordinates."""
    cy, cx = np.meshgrid(axis_coords(NY_F), axis_coords(NX_F), indexing="ij")
    return cy.ravel(), cx.ravel()


def battery(order, shift=0.0):
    """``(px, py)`` in degrees, ``(seed_rows(order), 1600)`` float64: the battery on every seed row, moved by ``shift`` index
    units on both axes (a multiple of 0.125 keeps every position a float32 number)."""
    lat, lon = dyadic_grid()
    cy, cx = battery_coords()
    py = lat[0] + 8.0 * (cy + shift)
    px = lon[0] + 8.0 * (cx + shift)
    rows = seed_rows(order)
    return np.tile(px, (rows, 1)), np.tile(py, (rows, 1))


def inside():
    """The battery columns inside ``[0, s]^2``: where a constant row samples the field, not 0."""
    cy, cx = battery_coords()
    return (cy >= 0) & (cy <= NY_F - 1) & (cx >= 0) & (cx <= NX_F - 1)


def f32_bound(err_oracle32, field_max):
    """The bound of test_sampler_on_own_trajectories_vs_oracle for a float32 sample judged against the float64 oracle:
    four times the float32 oracle's own maximum error on the same positions plus 1e-6 of the field's magnitude."""
    return 4.0 * err_oracle32 + 1e-6 * field_max


# ------------------------------------------------------------------ the generic grid
GENERIC_ORDERS = (1, 3, 4)
GENERIC_NT = 3
OFFSETS = ("0", "+1ulp", "-1ulp", "+2ulp", "-2ulp", "+1e-9", "-1e-9")
N_PARTNERS = 8


def generic_grid():
    from lagrangiancoherence_amd import flows
    _, _, lat, lon = flows.config1()
    lat, lon = np.asarray(lat, np.float64), np.asarray(lon, np.float64)
    assert lat.shape == (89,) and lon.shape == (180,)
    return lat, lon


def generic_field(seed=20261020):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((GENERIC_NT, 89, 180)), rng.standard_normal((GENERIC_NT, 89, 180))


def _neighbours(p):
    up1, dn1 = np.nextafter(p, np.inf), np.nextafter(p, -np.inf)
    return np.array([p, up1, dn1, np.nextafter(up1, np.inf), np.nextafter(dn1, -np.inf), p + 1e-9, p - 1e-9])


def edge_positions(coord):
    """The 28 positions of one axis: ``p_k = min + k s span / n`` for k in -1, 1, 2 and ``p = min``, each with OFFSETS."""
    n = coord.size
    lo = coord.min()
    span = coord.max() - lo
    centres = [lo + k * (n - 1) * span / n for k in (-1, 1, 2)] + [lo]
    return np.concatenate([_neighbours(np.float64(p)) for p in centres])


def generic_points(order, seed=7):
    """``(px, py, axis)``, positions ``(seed_rows(order), 448)``: every edge position of one axis crossed with 8 generic positions
    (inside the field, off the nodes) on the other; ``axis`` is 0 where the edge is in y, 1 where it is in x.  Column
    ``(28 * a + 7 * c + o) * 8 + j``: axis a, centre c (k = -1, 1, 2, then min), offset OFFSETS[o], partner j."""
    lat, lon = generic_grid()
    rng = np.random.default_rng(seed)

    def partners(coord):
        n = coord.size
        return coord.min() + rng.uniform(0.3, n - 1.3, N_PARTNERS) * (coord.max() - coord.min()) / n

    ey, ex = edge_positions(lat), edge_positions(lon)
    py = np.concatenate([np.repeat(ey, N_PARTNERS), np.tile(partners(lat), ex.size)])
    px = np.concatenate([np.tile(partners(lon), ey.size), np.repeat(ex, N_PARTNERS)])
    axis = np.concatenate([np.zeros(ey.size * N_PARTNERS, int), np.ones(ex.size * N_PARTNERS, int)])
    rows = seed_rows(order)
    return np.tile(px, (rows, 1)), np.tile(py, (rows, 1)), axis


# ------------------------------------------------------------------ sizes of the grid-stride and ring tests
SAMPLE_GRID_CAP = 8192          # sample_impl: at most this many workgroups ...
SAMPLE_BLOCK = 256              # ... of this many threads; beyond, sample_kernel's loop iterates
STRIDE_POSITIONS = SAMPLE_GRID_CAP * SAMPLE_BLOCK + 257
TRACER_DEPTH = 4                # tracer_walk's register ring
RING_LEVELS = (1, 2, 3, 4, 5, 7, 9)
