"""TEST SUPPORT -- the host restatement of the great-circle distance to the nearest ridge pixel (csrc/sphere_distance.hip,
Engine.sphere_distance, tools.distance_to_ridges(metric='sphere')).

- ``tables`` / ``unit_vectors``: ``cos`` and ``sin`` of the coordinates by numpy, and the nodes' unit vectors ``X = cl cx``,
  ``Y = cl sx``, ``Z = sl``, float64, one rounding per product.
- ``brute``: for every pixel the minimum, over ALL foreground pixels in ascending linear index, of the squared chord
  ``((dX dX + dY dY) + dZ dZ)`` evaluated by numpy in float64, one rounding per operation; ``argmin``'s first minimum is the
  smallest linear index; ``dist = 2 radius arcsin(min(1, sqrt(cost) / 2))``.  Chunked over pixels so that no temporary passes
  about 100 MB.  ``max_distance``: ``+inf`` and index -1 where ``cost > fl(c c)``, ``c = 2 sin(max_distance / (2 radius))``; a
  bound of ``pi radius`` or more is none.  A plane without foreground is ``+inf`` and -1 everywhere.
- ``haversine_min``: the textbook haversine formula from the coordinates themselves, minimised over the foreground pixels: what
  the chord form is measured against.
- ``GRID``: the global grid of the tests.  The planes are those of tests/distance.py (``DT.mask_of``).
"""
from __future__ import annotations

import numpy as np

from tests.components import foreground

RADIUS = 6371000.0
CHUNK_ELEMS = 3_000_000          # pixels x foreground pixels of one chunk: four float64 temporaries of it are 96 MB


def GRID(ny, nx):
    return np.linspace(-89.75, 89.75, ny), np.linspace(-180, 180, nx, endpoint=False)


def tables(lat, lon):
    y, x = np.asarray(lat, dtype=np.float64) * np.pi / 180, np.asarray(lon, dtype=np.float64) * np.pi / 180
    return np.cos(y), np.sin(y), np.cos(x), np.sin(x)


def unit_vectors(lat, lon):
    """``(X, Y, Z)`` of every node, each ``(ny * nx,)``."""
    cl, sl, cx, sx = tables(lat, lon)
    X, Y = cl[:, None] * cx[None, :], cl[:, None] * sx[None, :]
    return X.ravel(), Y.ravel(), np.broadcast_to(sl[:, None], X.shape).ravel().copy()


def cost_of(P, Q):
    """The cost the kernels minimise, between two tuples of broadcastable ``(X, Y, Z)``: float64, every operation rounded once."""
    dx, dy, dz = P[0] - Q[0], P[1] - Q[1], P[2] - Q[2]
    return (dx * dx + dy * dy) + dz * dz


def chord2_of(max_distance, radius=RADIUS):
    """``fl(c c)``, ``c = 2 sin(max_distance / (2 radius))``; None where the bound is none."""
    if max_distance is None or max_distance >= np.pi * radius:
        return None
    c = np.float64(2.0) * np.sin(np.float64(max_distance) / (np.float64(2.0) * np.float64(radius)))
    return c * c


def dist_of(cost, radius=RADIUS):
    return 2.0 * radius * np.arcsin(np.minimum(1.0, np.sqrt(cost) / 2.0))


def brute(mask, lat, lon, max_distance=None, radius=RADIUS):
    """``(dist float64, nearest int32, cost float64)`` of one plane."""
    fg = foreground(mask)
    ny, nx = fg.shape
    cost = np.full(ny * nx, np.inf)
    nearest = np.full(ny * nx, -1, dtype=np.int32)
    idx = np.flatnonzero(fg)                      # ascending: argmin's first minimum is the smallest linear index
    if idx.size:
        X, Y, Z = unit_vectors(lat, lon)
        Q = (X[idx][None, :], Y[idx][None, :], Z[idx][None, :])
        step = max(1, CHUNK_ELEMS // idx.size)
        for p0 in range(0, ny * nx, step):
            p = slice(p0, min(p0 + step, ny * nx))
            c = cost_of((X[p, None], Y[p, None], Z[p, None]), Q)
            k = np.argmin(c, axis=1)
            cost[p] = c[np.arange(k.size), k]
            nearest[p] = idx[k]
    bound = chord2_of(max_distance, radius)
    if bound is not None:
        far = ~(cost <= bound)
        cost[far], nearest[far] = np.inf, -1
    with np.errstate(invalid="ignore"):
        dist = np.where(np.isinf(cost), np.inf, dist_of(np.where(np.isinf(cost), 0.0, cost), radius))
    return dist.reshape(ny, nx), nearest.reshape(ny, nx), cost.reshape(ny, nx)


def haversine_min(mask, lat, lon, radius=RADIUS):
    """The smallest, over the foreground pixels, of ``2 radius arcsin(sqrt(sin^2(dphi / 2) + cos phi1 cos phi2 sin^2(dlambda / 2)))``."""
    fg = foreground(mask)
    ny, nx = fg.shape
    phi, lam = np.deg2rad(np.asarray(lat, dtype=np.float64)), np.deg2rad(np.asarray(lon, dtype=np.float64))
    P, L = np.broadcast_to(phi[:, None], (ny, nx)).ravel(), np.broadcast_to(lam[None, :], (ny, nx)).ravel()
    idx = np.flatnonzero(fg)
    out = np.full(ny * nx, np.inf)
    step = max(1, CHUNK_ELEMS // max(1, idx.size))
    for p0 in range(0, ny * nx if idx.size else 0, step):
        p = slice(p0, min(p0 + step, ny * nx))
        h = np.sin((P[p, None] - P[idx][None, :]) / 2) ** 2 + np.cos(P[p, None]) * np.cos(P[idx][None, :]) * np.sin((L[p, None] - L[idx][None, :]) / 2) ** 2
        out[p] = (2.0 * radius * np.arcsin(np.sqrt(np.minimum(1.0, h)))).min(axis=1)
    return out.reshape(ny, nx)


def tie_grid():
    """A grid and a mask on which the costs of a whole column against two pixels are bit-equal: longitudes -180 and 180 are one
    meridian whose sines differ in sign only, and column 65 is longitude 0 (``sx == 0``)."""
    lat, lon = np.linspace(-10, 10, 5), np.linspace(-180, 180, 131)
    mask = np.zeros((5, 131))
    mask[2, 0] = mask[2, 130] = 1
    return mask, lat, lon
