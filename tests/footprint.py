"""The footprint fold restated in numpy (include/lcs_hip.h, "footprints"), and the records the tests bin.

The restatement is the judge of ``lc_footprint_update``: the float64 index map, ``np.rint``, ``np.add.at`` into int64.  Every
output is an integer sum, so the tests ask for equality.  Nothing here touches the engine."""
import numpy as np

Q_MAX = 1 << 20
PLANES = ("hits", "mass", "csum", "chits")


class Grid:
    """A target grid: the centres of its first and last cell, its shape, whether its columns wrap."""

    def __init__(self, lat, lon, cyclic=False):
        self.lat, self.lon, self.cyclic = np.asarray(lat, np.float64), np.asarray(lon, np.float64), bool(cyclic)
        self.ny_t, self.nx_t = self.lat.size, self.lon.size
        self.lat0, self.lat1, self.lon0, self.lon1 = (float(v) for v in (self.lat[0], self.lat[-1], self.lon[0], self.lon[-1]))
        self.inv_dy = np.float64(self.ny_t - 1) / (np.float64(self.lat1) - np.float64(self.lat0))
        self.inv_dx = np.float64(self.nx_t - 1) / (np.float64(self.lon1) - np.float64(self.lon0))

    @property
    def shape(self):
        return self.ny_t, self.nx_t


GRID_2X2 = Grid([-10.0, 10.0], [0.0, 20.0])
GRID_CYCLIC = Grid(np.linspace(-90.0, 90.0, 19), np.linspace(-180.0, 170.0, 36), cyclic=True)
GRID_REGIONAL = Grid(np.linspace(-30.0, 6.0, 37), np.linspace(-70.0, -31.0, 40))
GRID_HALF = Grid(np.linspace(-45.0, 45.0, 181), np.linspace(-180.0, 179.5, 720), cyclic=True)      # 0.5 degrees from -180
GRIDS = {"2x2": GRID_2X2, "cyclic": GRID_CYCLIC, "regional": GRID_REGIONAL}


def cells(x, y, g: Grid):
    """``(valid, row, col)`` of positions in degrees (any float dtype: widened first); row and col are 0 where not valid."""
    with np.errstate(invalid="ignore", over="ignore"):
        fy = (np.asarray(y).astype(np.float64) - g.lat0) * g.inv_dy + 0.5
        fx = (np.asarray(x).astype(np.float64) - g.lon0) * g.inv_dx + 0.5
        ok = (fy >= 0.0) & (fy < float(g.ny_t))
        ok &= (np.abs(fx) < 2.0 ** 31) if g.cyclic else ((fx >= 0.0) & (fx < float(g.nx_t)))
    row = np.floor(np.where(ok, fy, 0.0)).astype(np.int64)
    col = np.floor(np.where(ok, fx, 0.0)).astype(np.int64)
    if g.cyclic:
        col = np.mod(col, g.nx_t)                                           # floored
    return ok, row, col


def half_weights(n_levels, level0, final):
    """h per entry of a block: 0 for the skipped entry 0 of a continued block, 1 at the record's two ends, else 2."""
    h = np.full(n_levels, 2, np.int64)
    h[0] = 1 if level0 == 0 else 0
    if final:
        h[-1] = 1
    return h


def new_acc(g: Grid, with_c=False):
    acc = {k: np.zeros(g.shape, np.int64) for k in (PLANES if with_c else PLANES[:2])}
    acc.update({k: None for k in PLANES if k not in acc})
    acc["stats"] = np.zeros(4, np.int64)
    return acc


def fold(tx, ty, g: Grid, level0=0, final=True, q=None, c=None, c_scale=None, acc=None):
    """One block added into ``acc`` (created when None): the dict of int64 planes and ``stats``."""
    tx, ty = np.asarray(tx), np.asarray(ty)
    n_levels = tx.shape[0]
    acc = new_acc(g, c is not None) if acc is None else acc
    qq = np.ones(tx.shape[1:], np.int64) if q is None else np.asarray(q).astype(np.int64)
    h = half_weights(n_levels, level0, final).reshape((n_levels,) + (1,) * (tx.ndim - 1))
    h = np.broadcast_to(h, tx.shape) * (qq > 0)                              # a parcel with q == 0 counts nowhere
    ok, row, col = cells(tx, ty, g)
    acc["stats"][0] += h[~ok].sum()
    ok = ok & (h > 0)
    flat = (row * g.nx_t + col)[ok]
    np.add.at(acc["hits"].reshape(-1), flat, h[ok])
    np.add.at(acc["mass"].reshape(-1), flat, (h * qq)[ok])
    if c is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            v = np.rint(np.asarray(c).astype(np.float64) * np.float64(c_scale))
            good = np.abs(v) <= 2.0 ** 31                                    # NaN and inf fail
        acc["stats"][1] += h[ok & ~good].sum()
        use = ok & good
        flat = (row * g.nx_t + col)[use]
        np.add.at(acc["csum"].reshape(-1), flat, (h * np.where(good, v, 0.0).astype(np.int64))[use])
        np.add.at(acc["chits"].reshape(-1), flat, h[use])
    return acc


def fold_in_blocks(tx, ty, g, block, q=None, c=None, c_scale=None):
    steps = tx.shape[0] - 1
    acc = None
    for lo in range(0, steps, block):
        hi = min(lo + block, steps)
        acc = fold(tx[lo:hi + 1], ty[lo:hi + 1], g, lo, hi == steps, q, None if c is None else c[lo:hi + 1], c_scale, acc)
    return acc


def same(a, b):
    """Two accumulator dicts hold the same planes with the same integers."""
    return all((a[k] is None) == (b[k] is None) and (a[k] is None or np.array_equal(a[k], b[k])) for k in PLANES + ("stats",))


def conserved(acc, levels, q, shape):
    """sum(hits) + stats[0] == 2 (levels - 1) #{q > 0} over a whole record."""
    counted = int(np.prod(shape)) if q is None else int((np.asarray(q) > 0).sum())
    return int(acc["hits"].sum()) + int(acc["stats"][0]) == 2 * (levels - 1) * counted


# ------------------------------------------------------------------ records
def weights_case(shape, seed=3):
    """Integer weights with zeros, the two ends of the range and small values."""
    rng = np.random.default_rng(seed)
    q = rng.integers(0, Q_MAX + 1, size=shape, dtype=np.int64)
    q[rng.random(shape) < 0.25] = 0
    q.reshape(-1)[::7] = Q_MAX
    q.reshape(-1)[3::11] = 1
    if q.size > 1:
        q.reshape(-1)[1] = 0
    return q.astype(np.int32)


def mixed_case(n_levels, shape, dtype, g: Grid, seed=0):
    """Positions all over the grid and around it -- cell edges, the seam, half a cell beyond the last column, rows and columns
    outside, NaN, +-inf, 1e30 -- and values with non-finite ones and ones beyond 2^31 / c_scale.  Returns (tx, ty, c, c_scale)."""
    rng = np.random.default_rng(seed + 17 * n_levels + shape[0] * 131 + shape[1])
    full = (n_levels,) + tuple(shape)
    dy, dx = (g.lat1 - g.lat0) / (g.ny_t - 1), (g.lon1 - g.lon0) / (g.nx_t - 1)
    ty = rng.uniform(g.lat0 - 1.5 * dy, g.lat1 + 1.5 * dy, full)
    tx = rng.uniform(g.lon0 - 2.5 * dx, g.lon1 + 2.5 * dx, full)
    pick = lambda p: rng.random(full) < p
    # exactly on cell edges (centres +- half a cell), both axes
    m = pick(0.15)
    ty[m] = (g.lat0 + (rng.integers(-1, g.ny_t + 1, full) - 0.5) * dy)[m]
    m = pick(0.15)
    tx[m] = (g.lon0 + (rng.integers(-1, g.nx_t + 1, full) - 0.5) * dx)[m]
    m = pick(0.05)
    tx[m] = g.lon1 + 0.5 * dx                                                # wraps to column 0 on a cyclic grid, else outside
    m = pick(0.05)
    tx[m] = (tx + 360.0 * rng.integers(-2, 3, full))[m]                      # other turns of the circle
    for bad in (np.nan, np.inf, -np.inf, 1e30, -1e30):
        tx[pick(0.01)] = bad
        ty[pick(0.01)] = bad
    c = rng.normal(0.0, 40.0, full)
    c_scale = 2.0 ** 24
    c[pick(0.02)] = np.nan
    c[pick(0.01)] = np.inf
    c[pick(0.02)] = 2.0 ** 7 + 1.0                                           # beyond 2^31 / c_scale
    c[pick(0.02)] = -(2.0 ** 7)                                              # exactly -2^31: counts
    m = pick(0.05)
    c[m] = ((rng.integers(-50, 50, full) + 0.5) / c_scale)[m]                # ties: rint rounds them to even
    return tx.astype(dtype), ty.astype(dtype), c.astype(dtype), c_scale


def one_cell_case(n_levels, shape, dtype, g: Grid):
    """Every parcel in one cell at every level, the largest value that counts: maximal contention, the largest sums."""
    full = (n_levels,) + tuple(shape)
    tx = np.full(full, g.lon0 + (g.lon1 - g.lon0) / (g.nx_t - 1) * (g.nx_t // 2), dtype)
    ty = np.full(full, g.lat0 + (g.lat1 - g.lat0) / (g.ny_t - 1) * (g.ny_t // 3), dtype)
    c = np.full(full, -128.0, dtype)
    return tx, ty, c, 2.0 ** 24


def jump_case(n_levels, shape, dtype, g: Grid):
    """Parcels that jump across the whole grid at each level, each its own way: no window holds them."""
    full = (n_levels,) + tuple(shape)
    j, r, k = np.meshgrid(np.arange(n_levels), np.arange(shape[0]), np.arange(shape[1]), indexing="ij")
    row = (j * 7 + r * 5 + k * 3) % g.ny_t
    col = (j * 11 + r * 3 + k * 13) % g.nx_t
    ty = g.lat0 + (g.lat1 - g.lat0) / (g.ny_t - 1) * row
    tx = g.lon0 + (g.lon1 - g.lon0) / (g.nx_t - 1) * col
    c = ((j + r - k) % 9 - 4).astype(np.float64)
    assert ty.shape == full
    return tx.astype(dtype), ty.astype(dtype), c.astype(dtype), 2.0 ** 20


def drift_case(n_levels, shape, dtype, g: Grid):
    """A compact patch that drifts slowly (and, on a cyclic grid, across the seam): it never leaves a window."""
    dy, dx = (g.lat1 - g.lat0) / (g.ny_t - 1), (g.lon1 - g.lon0) / (g.nx_t - 1)
    j, r, k = np.meshgrid(np.arange(n_levels), np.arange(shape[0]), np.arange(shape[1]), indexing="ij")
    ty = g.lat0 + dy * (g.ny_t / 2 + 0.02 * r + 0.1 * j)
    tx = (g.lon1 - 2 * dx if g.cyclic else g.lon0 + dx * (g.nx_t / 3)) + dx * (0.01 * k + 0.3 * j)
    c = 0.25 * j + 0.001 * k
    return tx.astype(dtype), ty.astype(dtype), c.astype(dtype), 2.0 ** 16


def edge_case(dtype):
    """On GRID_HALF every ``k 0.5 - 0.25`` is a cell edge, exact in float32, and inv_dx is exactly 2: the entry belongs to the
    upper cell.  Steps across the seam, and ``lon1 + 0.25``, which wraps to column 0.  One parcel per column edge, three levels."""
    g = GRID_HALF
    k = np.arange(-2, g.nx_t + 3)
    x = k * 0.5 - 0.25 - 180.0
    rows = np.arange(k.size) % g.ny_t
    y = g.lat0 + rows * 0.5 - 0.25                                           # the lower edge of row `rows`: belongs to it
    tx = np.stack([x, x + 360.0, x[::-1]])[:, None, :]
    ty = np.stack([y, y, y + 0.5])[:, None, :]
    return tx.astype(dtype), ty.astype(dtype)


KINDS = {"mixed": mixed_case, "one_cell": one_cell_case, "jump": jump_case, "drift": drift_case}
