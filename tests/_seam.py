"""The oracle's cyclic loop restated (oracle/lcs_oracle.py parcel_propagation, LCS/trajectory.py:80-126) so that a test
can look inside a time level: how close a parcel comes to the hard-coded +-180 wrap (Q7) at any update, and what a
kernel that leaves the in-level wrap to its next sample's window test would compute (the mutant).

On a field whose longitudes do not start at -180 (0 ... 360, say) the reference still wraps at +-180: a parcel that passes
180 is rewritten to a negative longitude and its next sample goes through scipy's ``wrap`` map about two cells away from
where the unwrapped longitude would have sampled.  ``propagate`` with ``defer=False`` is the oracle bit for bit (the same
calls in the same order); with ``defer=True`` it skips the clamp after an update that is not the level's last whenever
the unclamped position's index lies in [1, n - 1) on both axes, which is what the float32 LDS-tile kernels' window test
accepts (csrc/advect.hip, DEFER_X)."""
import functools

import numpy as np

from lagrangiancoherence_amd import flows
from oracle import lcs_oracle as O
from tests import kernel_routes as KR

NEAR_SEAM = 1e-2       # degrees: 30 x the float32 oracle's largest distance from the float64 answer on the route table's flow


def propagate(u, v, lat, lon, slat, slon, timestep, K, order, t0, nsteps, defer=False):
    """Cyclic parcel propagation.  Returns ``(traj_x, traj_y, seam)``: the stored levels ``(nsteps + 1, ny, nx)`` and each
    seed's smallest distance from +-180 over every update (the Euler step and each SETTLS iteration), before the clamp."""
    u, v, lat, lon, slat, slon = (np.asarray(a) for a in (u, v, lat, lon, slat, slon))
    conv_y = 180 / (O.EARTH_R * np.pi)
    conv_x = 180 / (np.pi * O.EARTH_R * np.abs(np.cos(slat * np.pi / 180)))
    conv_x = np.broadcast_to(conv_x[:, None], (slat.size, slon.size))
    y_min, y_max, x_min, x_max = lat.min(), lat.max(), lon.min(), lon.max()
    px, py = np.meshgrid(slon, slat)
    tx, ty = [px], [py]
    seam = np.full(px.shape, np.inf)

    def interp(F, x, y):
        return O.xr_map_coordinates(F, lat, lon, x, y, order=order)

    def clamp(x, y, last):
        nonlocal seam
        x64 = np.asarray(x, dtype=np.float64)
        seam = np.minimum(seam, np.minimum(np.abs(x64 - 180.0), np.abs(x64 + 180.0)))
        cx, cy = O._clamp(x, y, x_min, x_max, y_min, y_max, True, None)
        if not defer or last:
            return cx, cy
        ix = lon.shape[0] * (x - x_min) / (x_max - x_min)
        iy = lat.shape[0] * (y - y_min) / (y_max - y_min)
        skip = (ix >= 1) & (ix < lon.shape[0] - 1) & (iy >= 1) & (iy < lat.shape[0] - 1)
        return np.where(skip, x, cx), np.where(skip, y, cy)

    for t in range(t0, t0 + nsteps):
        va = interp(v[t], px, py)
        ua = interp(u[t], px, py)
        py = py + timestep * conv_y * va
        px = px + timestep * conv_x * ua
        px, py = clamp(px, py, K == 0)
        for k in range(K):
            v_t, v_tp = interp(v[t], px, py), interp(v[t + 1], px, py)
            u_t, u_tp = interp(u[t], px, py), interp(u[t + 1], px, py)
            py = py + 0.5 * timestep * conv_y * (va + 2 * v_t - v_tp)
            px = px + 0.5 * timestep * conv_x * (ua + 2 * u_t - u_tp)
            px, py = clamp(px, py, k == K - 1)
        tx.append(px)
        ty.append(py)
    return np.stack(tx), np.stack(ty), seam


def crossed(traj_x):
    """Seeds whose longitude jumps by more than 180 degrees between two stored levels: they crossed +-180."""
    return (np.abs(np.diff(np.asarray(traj_x, dtype=np.float64), axis=0)) > 180.0).any(axis=0)


# ------------------------------------------------------------------ the route table's inputs, per longitude grid
@functools.lru_cache(maxsize=None)
def flow64():
    f = KR.FLOW
    u, v, lat, lon = flows.era5_like(nt=f["nt"], ny=f["ny"], nx=f["nx"], dtype=np.float64, dt_seconds=f["dt_seconds"])
    return u * f["scale"], v * f["scale"], lat, lon


@functools.lru_cache(maxsize=None)
def inputs(kind, grid="m180"):
    """(u, v, lat, lon, seed_lat, seed_lon) as the engine gets them, and as the oracle gets them for the float64 answer:
    the flow's winds on its longitudes plus ``KR.GRIDS[grid]``, the seeds spanning the shifted coordinates."""
    u, v, lat, lon = flow64()
    if KR.GRIDS[grid]:
        lon = lon + KR.GRIDS[grid]
    f32 = np.float32
    if kind == "float32":
        u, v, lat, lon = (a.astype(f32) for a in (u, v, lat, lon))
    elif kind == "f64_wind_f32":
        u, v = u.astype(f32), v.astype(f32)
    slat, slon = flows.seed_grid(*KR.SEEDS, lat, lon)
    return u, v, lat, lon, slat, slon


@functools.lru_cache(maxsize=None)
def restated(kind, order, K, dt, t0, grid, arith="float64", defer=False):
    """``propagate`` on the route inputs of (kind, grid) in `arith` arithmetic."""
    a = inputs(kind, grid)
    if arith == "float64" and kind == "float32":
        a = tuple(q.astype(np.float64) for q in a)
    return propagate(*a, dt, K, order, t0, KR.NSTEPS, defer=defer)


def near_seam(kind, order, K, dt, t0, grid):
    """Seeds whose float64 oracle position comes within NEAR_SEAM of +-180 at any update: float32 and float64 can wrap
    such a parcel on different iterations and then sample two cells apart, so they are left out of float32 statistics."""
    return restated(kind, order, K, dt, t0, grid)[2] < NEAR_SEAM
