"""TEST SUPPORT -- the host restatement of the distance transform (csrc/distance.hip, Engine.distance_transform,
tools.distance_to_ridges) and the masks the tests transform.

- ``brute``: for every pixel the minimum, over ALL foreground pixels, of ``(dr * sy) ** 2 + (dc * sx) ** 2`` evaluated by numpy
  in float64, one rounding per operation -- then the smallest linear index among the minima, then the square root.  Chunked
  over pixels so that no temporary passes about 100 MB.  ``cyclic``: ``dc = min(|c - c'|, nx - |c - c'|)``.  ``max_distance``:
  ``+inf`` and index -1 where the distance is larger.  A plane without foreground is ``+inf`` and -1 everywhere.
- ``scipy_edt``: ``scipy.ndimage.distance_transform_edt(~foreground, sampling=...)``; for ``cyclic`` the middle third of the
  transform of the plane tiled three times along x.  (scipy's own ``return_indices`` breaks ties another way than by the
  smallest index, so indices are compared with ``brute`` only.)
- ``CASES`` / ``mask_of``: the planes of tests/test_distance_gpu.py, by name.
"""
from __future__ import annotations

import numpy as np

from tests.components import foreground

SEED = 20261019
SAMPLINGS = [(2.0, 0.5), (0.25, 0.3125), (1.0, 0.7)]
CHUNK_ELEMS = 3_000_000          # pixels x foreground pixels of one chunk: four float64 temporaries of it are 96 MB


def cost_of(dr, dc, sampling=(1.0, 1.0)):
    """The cost the kernels minimise, from integer offsets (arrays or scalars): float64, every operation rounded once."""
    y = np.abs(np.asarray(dr)).astype(np.float64) * np.float64(sampling[0])
    x = np.abs(np.asarray(dc)).astype(np.float64) * np.float64(sampling[1])
    return y * y + x * x


def brute(mask, cyclic=False, sampling=(1.0, 1.0), max_distance=None):
    """``(dist float64, nearest int32)`` of one plane."""
    fg = foreground(mask)
    ny, nx = fg.shape
    dist = np.full(ny * nx, np.inf)
    nearest = np.full(ny * nx, -1, dtype=np.int32)
    idx = np.flatnonzero(fg)                      # ascending: argmin's first minimum is the smallest linear index
    if idx.size:
        fr, fc = np.divmod(idx, nx)
        step = max(1, CHUNK_ELEMS // idx.size)
        for p0 in range(0, ny * nx, step):
            r, c = np.divmod(np.arange(p0, min(p0 + step, ny * nx)), nx)
            dc = np.abs(c[:, None] - fc[None, :])
            if cyclic:
                dc = np.minimum(dc, nx - dc)
            cost = cost_of(r[:, None] - fr[None, :], dc, sampling)
            k = np.argmin(cost, axis=1)
            dist[p0:p0 + r.size] = np.sqrt(cost[np.arange(r.size), k])
            nearest[p0:p0 + r.size] = idx[k]
    if max_distance is not None:
        far = ~(dist <= max_distance)
        dist[far], nearest[far] = np.inf, -1
    return dist.reshape(ny, nx), nearest.reshape(ny, nx)


def scipy_edt(mask, cyclic=False, sampling=(1.0, 1.0)):
    from scipy import ndimage
    fg = foreground(mask)
    if not cyclic:
        return ndimage.distance_transform_edt(~fg, sampling=sampling)
    nx = fg.shape[1]
    return ndimage.distance_transform_edt(~np.tile(fg, (1, 3)), sampling=sampling)[:, nx:2 * nx].copy()


# ------------------------------------------------------------------ the planes
def random(ny, nx, density, salt=0):
    """A random plane of that density; a draw without a pixel gets one."""
    rng = np.random.default_rng([SEED, ny, nx, int(round(density * 1000)), salt])
    m = (rng.random((ny, nx)) < density).astype(np.float64)
    if not m.any():
        m[rng.integers(ny), rng.integers(nx)] = 1
    return m


def _pixels(ny, nx, *at):
    m = np.zeros((ny, nx))
    for r, c in at:
        m[r, c] = 1
    return m


def _nan_negative(ny, nx):
    m = random(ny, nx, 0.05, salt=1)
    rng = np.random.default_rng([SEED, 7])
    m[rng.random((ny, nx)) < 0.3] = np.nan          # background, also where a pixel was drawn
    m[rng.random((ny, nx)) < 0.03] = -2.5           # foreground
    return m


def _full_row(ny, nx, r):
    m = np.zeros((ny, nx))
    m[r] = 1
    return m


def _full_column(ny, nx, c):
    m = np.zeros((ny, nx))
    m[:, c] = 1
    return m


SMALL = {   # compared with scipy and with the brute-force oracle
    "1x1-foreground": lambda: np.ones((1, 1)),
    "1x37": lambda: random(1, 37, 0.1),
    "37x1": lambda: random(37, 1, 0.1),
    "foreground-67x130": lambda: np.ones((67, 130)),
    "corners-67x130": lambda: _pixels(67, 130, (0, 0), (0, 129), (66, 0), (66, 129)),
    "one-pixel-67x130": lambda: _pixels(67, 130, (66, 0)),
    **{f"random-{ny}x{nx}-{d}": (lambda ny=ny, nx=nx, d=d: random(ny, nx, d))
       for ny, nx in ((67, 130), (130, 67)) for d in (0.002, 0.02, 0.2)},
    "row-67x130": lambda: _full_row(67, 130, 40),             # every column holds one pixel
    "column-67x130": lambda: _full_column(67, 130, 77),       # every other column holds none
    "two-rows-130x67": lambda: np.maximum(_full_row(130, 67, 3), _full_row(130, 67, 100)),   # up / down ties across segments
    "pair-in-a-row": lambda: _pixels(67, 130, (30, 20), (30, 101)),          # equidistant along a whole column
    "pair-in-a-column": lambda: _pixels(67, 130, (10, 64), (55, 64)),        # equidistant along a whole row (odd offset: none)
    "pair-in-a-column-even": lambda: _pixels(67, 130, (10, 64), (56, 64)),   # row 33 is equidistant: the tie goes up
    "nan-negative": lambda: _nan_negative(67, 130),
}
EMPTY = {   # our own rule: +inf, nearest -1
    "1x1-background": lambda: np.zeros((1, 1)),
    "background-67x130": lambda: np.zeros((67, 130)),
}
LARGE = {   # compared with scipy only: several row segments, more columns than one pass of a workgroup
    "random-515x513-0.02": lambda: random(515, 513, 0.02),
}
CYCLIC = {
    "cyclic-20x13": lambda: random(20, 13, 0.05),
    "cyclic-20x12": lambda: random(20, 12, 0.05),
    "cyclic-67x130-0.02": lambda: random(67, 130, 0.02, salt=3),
    "cyclic-column-0": lambda: _full_column(20, 13, 0),
}
CASES = {**SMALL, **EMPTY, **LARGE, **CYCLIC}


def mask_of(name, dtype=np.float64):
    return CASES[name]().astype(dtype)
