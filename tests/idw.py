"""TEST SUPPORT -- the host restatement of inverse-distance weighting on the sphere (csrc/idw.hip, Engine.idw_interp,
tools.Inverse_weighted_interpolation, tools.xr_idx_interp).

- ``unit``: a point in degrees as the unit vector ``X = cos lat cos lon``, ``Y = cos lat sin lon``, ``Z = sin lat`` with numpy's
  cos / sin of ``degrees * pi / 180``, float64, one rounding per product; ``grid=True``: from the row / column tables.  A point
  with a coordinate that is not finite or ``|lat| > 90`` is NaN: it is left out of everything.
- ``costs``: the squared chord ``((dX dX + dY dY) + dZ dZ)`` of every (target, source) pair, numpy float64, one rounding per
  operation -- bit for bit what the kernel forms, so that ``cost == 0`` and ``cost <= max_chord2`` decide identically.
- ``weights``: ``d = (2 radius) arcsin(min(1, sqrt(cost) / 2))`` and ``w = 1 / (d d)``, ``1 / d`` or ``1 / d**p`` for ``p`` 2, 1 or
  anything else.
- ``oracle``: per plane and target ``u = fsum(w z) / fsum(w)`` over the contributing sources with ``math.fsum`` (the exact sum
  of the rounded terms, rounded once); the mean of the values of the sources of cost 0 where there are any (``weight = +inf``);
  NaN and ``weight = 0`` without a contributing source.  ``count``: the sources within reach whose coordinates are valid,
  whatever their values are.  Beside them what the tolerance is made of: ``n``, the contributing sources of every plane and
  target, and ``scale = fsum(w |z|) / fsum(w)``.
- ``bound_u`` / ``bound_w``: the tolerance of tests/test_idw_gpu.py,
      |u - u_oracle| <= (n + K) eps64 scale      (+ half a float32 ulp of |u_oracle| for float32 values)
      |W - W_oracle| <= (n + K) eps64 W_oracle
  ``n eps64`` is the textbook bound for a sum of ``n`` rounded terms, numerator and denominator alike.  ``K`` covers the device's
  asin, pow and division against numpy's and is measured, not guessed: with a single source the returned ``sum(w)`` is the
  device's weight itself; ``E`` is the largest distance in ulp between that weight and numpy's over all single-source pairs of
  tests/test_idw_gpu.py (n_tgt 1, 255, 256, 257, 700; the grid and the scattered form) and the powers 1, 2 and 3.5, and
  ``K = 8 (E + 1)``: one weight enters both sums, which gives ``2 E``; the factor 4 covers the product, the quotient and headroom.
- ``haversine``: the textbook ``2 R arctan2(sqrt(a), sqrt(1 - a))``, what the chord form is measured against, and
  ``reference_formula``: ``sum(z / d^2) / sum(1 / d^2)`` with it, what LCS/tools.py:285-299 means.
"""
from __future__ import annotations

import math

import numpy as np

RADIUS = 6371000.0
EPS64 = float(np.finfo(np.float64).eps)
# E, measured on one MI355X (gfx950; the device library's asin, pow and division against numpy 2.2's on x86-64) over the 2 938
# single-source pairs of tests/test_idw_gpu.py per power: 2 ulp for power 1 (asin and one division), 5 ulp for power 2 (the
# square doubles the distance's error), 9 ulp for power 3.5 (pow multiplies it by 3.5 and adds its own); the means are 0.4 to
# 0.6 ulp.  test_the_single_source_weight_is_within_E_ulp_of_numpys measures it again on every run.
E = 9
K = 8 * (E + 1)  # 80


def unit(lon, lat, grid=False):
    lon, lat = np.asarray(lon, dtype=np.float64), np.asarray(lat, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        y, x = lat * np.pi / 180, lon * np.pi / 180
        cl, sl, cx, sx = np.cos(y), np.sin(y), np.cos(x), np.sin(x)
        bad_lat, bad_lon = ~(np.isfinite(lat) & (np.abs(lat) <= 90.0)), ~np.isfinite(lon)
    if grid:
        X, Y, Z = cl[:, None] * cx[None, :], cl[:, None] * sx[None, :], np.broadcast_to(sl[:, None], (lat.size, lon.size))
        bad = bad_lat[:, None] | bad_lon[None, :]
    else:
        X, Y, Z, bad = cl * cx, cl * sx, sl, bad_lat | bad_lon
    return tuple(np.where(bad, np.nan, v).reshape(-1) for v in (X, Y, Z))


def costs(tgt, src):
    """``(n_tgt, n_src)``: NaN where either point is left out."""
    dx, dy, dz = (t[:, None] - s[None, :] for t, s in zip(tgt, src))
    return (dx * dx + dy * dy) + dz * dz


def chord2_of(max_distance, radius=RADIUS):
    """``fl(c c)``, ``c = 2 sin(max_distance / (2 radius))``; None where the bound is none."""
    if max_distance is None or max_distance >= np.pi * radius:
        return None
    c = np.float64(2.0) * np.sin(np.float64(max_distance) / (np.float64(2.0) * np.float64(radius)))
    return c * c


def distances(cost, radius=RADIUS):
    return (2.0 * radius) * np.arcsin(np.minimum(1.0, np.sqrt(cost) / 2.0))


def weights(cost, p, radius=RADIUS):
    d = distances(cost, radius)
    with np.errstate(divide="ignore"):
        return 1.0 / (d * d) if p == 2 else 1.0 / d if p == 1 else 1.0 / np.power(d, np.float64(p))


def oracle(src_lon, src_lat, z, tgt_lon, tgt_lat, grid=False, p=2, radius=RADIUS, max_distance=None):
    """A dict of ``u`` (in ``z``'s dtype), ``u64`` (before that rounding), ``weight``, ``n``, ``scale`` -- each ``(n_planes,
    n_tgt)``, or ``(n_tgt,)`` for one-dimensional ``z`` -- and ``count`` ``(n_tgt,)`` int32."""
    z = np.asarray(z)
    dtype = z.dtype if z.dtype in (np.float32, np.float64) else np.dtype(np.float64)
    planes = z.astype(np.float64).reshape(-1, z.shape[-1])
    cost = costs(unit(tgt_lon, tgt_lat, grid), unit(src_lon, src_lat))
    bound = chord2_of(max_distance, radius)
    with np.errstate(invalid="ignore"):
        reach = ~np.isnan(cost) if bound is None else cost <= bound
    w = weights(np.where(reach & (cost > 0), cost, 1.0), p, radius)
    n_tgt = cost.shape[0]
    u = np.full((planes.shape[0], n_tgt), np.nan)
    weight, scale = np.zeros_like(u), np.full_like(u, np.nan)
    n = np.zeros(u.shape, dtype=np.int64)
    for q, zq in enumerate(planes):
        has = ~np.isnan(zq)
        for i in range(n_tgt):
            use = reach[i] & has
            hit = use & (cost[i] == 0)
            if hit.any():
                v = zq[hit]
                u[q, i], weight[q, i], n[q, i] = math.fsum(v) / v.size, np.inf, v.size
                scale[q, i] = math.fsum(np.abs(v)) / v.size
            elif use.any():
                wi, v = w[i][use], zq[use]
                den = math.fsum(wi)
                u[q, i], weight[q, i], n[q, i] = math.fsum(wi * v) / den, den, v.size
                scale[q, i] = math.fsum(wi * np.abs(v)) / den
    out = {"u": u.astype(dtype), "u64": u, "weight": weight, "n": n, "scale": scale}
    if z.ndim == 1:
        out = {k: v[0] for k, v in out.items()}
    out["count"] = reach.sum(axis=1).astype(np.int32)
    return out


def bound_u(o, dtype):
    """The largest ``|u - u_oracle|`` the tolerance allows, per plane and target (NaN where the oracle is NaN)."""
    b = (o["n"] + K) * EPS64 * o["scale"]
    if np.dtype(dtype) == np.float32:
        with np.errstate(invalid="ignore"):
            b = b + 0.5 * np.spacing(np.abs(o["u64"]).astype(np.float32)).astype(np.float64)
    return b


def bound_w(o):
    """The largest ``|W - W_oracle|`` the tolerance allows where ``W_oracle`` is finite and not 0."""
    return (o["n"] + K) * EPS64 * o["weight"]


def ulps(got, want):
    """``|got - want|`` in units of the spacing of ``want``."""
    return np.abs(got - want) / np.spacing(np.abs(want))


def haversine(lon1, lat1, lon2, lat2, radius=RADIUS):
    rad = math.pi / 180
    dlon, dlat = (lon2 - lon1) * rad, (lat2 - lat1) * rad
    a = math.sin(dlat / 2) ** 2 + math.cos(lat1 * rad) * math.cos(lat2 * rad) * math.sin(dlon / 2) ** 2
    return 2 * radius * math.atan2(math.sqrt(a), math.sqrt(max(0.0, 1 - a)))


def reference_formula(x, y, z, xi, yi, radius=6378.1):
    """What LCS/tools.py:285-299 means, with the textbook haversine in the place of its own: a plain double loop."""
    out = []
    for p in range(len(xi)):
        d = [haversine(x[s], y[s], xi[p], yi[p], radius) for s in range(len(x))]
        out.append(math.fsum(z[s] / d[s] ** 2 for s in range(len(x))) / math.fsum(1 / d[s] ** 2 for s in range(len(x))))
    return np.array(out)


# ------------------------------------------------------------------ the points of the tests
def scattered(n, seed, lat_max=89.0):
    """``n`` seeded points, uniform on the sphere between the latitudes ``+-lat_max``: ``(lon, lat)`` in degrees."""
    rng = np.random.default_rng(seed)
    lon = rng.uniform(-180.0, 180.0, n)
    lat = np.degrees(np.arcsin(rng.uniform(-np.sin(np.radians(lat_max)), np.sin(np.radians(lat_max)), n)))
    return lon, lat


def values(n_planes, n, seed, dtype=np.float64):
    """Seeded values of both signs and a few orders of magnitude, ``(n,)`` for ``n_planes`` None."""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n_planes or 1, n)) * 10.0 ** rng.integers(-2, 3, size=(n_planes or 1, 1)) + rng.normal(size=(n_planes or 1, 1))
    return (v if n_planes else v[0]).astype(dtype)


def grid_of(n_tgt):
    """``(lon (nx,), lat (ny,))`` of a regular grid of exactly ``n_tgt`` nodes (or one row of them where ``n_tgt`` is prime)."""
    ny = max(d for d in range(1, int(math.isqrt(n_tgt)) + 1) if n_tgt % d == 0)
    nx = n_tgt // ny
    return np.linspace(-180.0, 180.0, nx, endpoint=False) + 0.25, np.linspace(-80.0, 80.0, ny) if ny > 1 else np.array([12.5])
