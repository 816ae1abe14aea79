"""Case tables of the stacked ridge extraction (``lc_ridges_batch``, ``Engine.ridges_batch``, the N-D form of
``tools.find_ridges_spherical_hessian``).

Plain data and numpy input builders, imported by ``test_ridges_batch.py`` (no GPU: the cases' own promises under the oracle,
the C ABI's refusals, the intake) and ``test_ridges_batch_gpu.py`` (every case on the GPU against the per-plane route, bit for
bit, and against the oracle).  No torch, no engine.

- ``TILE``: the tile of ``hessian_ridge_kernel`` (rows, columns), read back from the source by the CPU test.
- ``SHAPES``: ``(ny, nx)``: 5 x 5 (every row and column is an edge rule), 6 x 9, one tile exactly, one pixel more than a tile
  in both directions, a ragged multi-tile grid (3 tiles + 3 rows by 2 tiles + 5 columns).
- ``MEMBERS``, ``GLOBAL``, ``SIGMAS`` (``tests/ridge_chain.py::SIGMA_VARIANTS`` and 1.2, the driver's value).
- ``stack(ny, nx, n)``: ``n`` planes of ``tests/ridge_chain.py::chain_input``'s field, each with its own phase, so no two planes
  are equal and the mask of every stack has both values.
"""
import numpy as np

from tests import ridge_chain as RC

TILE = (16, 64)
SHAPES = ((5, 5), (6, 9), TILE, (TILE[0] + 1, TILE[1] + 1), (3 * TILE[0] + 3, 2 * TILE[1] + 5))
MEMBERS = (1, 3)
GLOBAL = (True, False)
SIGMAS = RC.SIGMA_VARIANTS + (1.2,)
TOL = RC.CHAIN_TOL

CASES = tuple((ny, nx, n, g, si) for ny, nx in SHAPES for n in MEMBERS for g in GLOBAL for si in range(len(SIGMAS)))


def case_id(c):
    ny, nx, n, g, si = c
    s = SIGMAS[si]
    return f"{ny}x{nx}-n{n}-{'global' if g else 'regional'}-sigma{si}_{type(s).__name__}_{s}"


def grid(ny, nx):
    """Ascending coordinates: a band of latitudes, a whole circle of longitudes (the wrap of ``isglobal`` closes on itself)."""
    return np.linspace(-60.0, 60.0, ny), -180.0 + (360.0 / nx) * np.arange(nx)


def plane(ny, nx, m):
    """Plane ``m`` of a stack: chain_input's meandering ridge and ripple, three times as high and shifted in longitude with ``m``,
    in a shallow trough along the equator (positive curvature away from the ridge: the mask has both values even on the 5 x 5 grid
    under the widest smoothing)."""
    lat, lon = grid(ny, nx)
    LON, LAT = np.meshgrid(lon, lat)
    return 3.0 * (np.exp(-((LAT - 5 - 8 * np.sin(np.deg2rad(2 * LON + 40 * m))) / 10.0) ** 2) * (1 + 0.2 * np.cos(np.deg2rad(3 * LON)))
                  + 0.05 * np.sin(np.deg2rad(5 * LON + 25 * m)) * np.cos(np.deg2rad(4 * LAT))
                  + 0.8 * (LAT / 60.0) ** 2 * (1 + 0.5 * np.sin(np.deg2rad(LON + 30 * m))))


def stack(ny, nx, n):
    """``(values (n, ny, nx), lat, lon)``, fresh arrays."""
    lat, lon = grid(ny, nx)
    return np.stack([plane(ny, nx, m) for m in range(n)]), lat, lon


def seam_points(ny, nx):
    """Where the seam test plants its non-finite values in a grid of several tiles: a NaN on the corner where four tiles
    meet, an inf on the last column (the western neighbour of column 0 under the cyclic wrap) and one on column 0."""
    assert ny > TILE[0] + 4 and nx > TILE[1] + 4
    return dict(nan=(TILE[0], TILE[1]), inf_east=(ny // 2, nx - 1), inf_west=(3, 0))
