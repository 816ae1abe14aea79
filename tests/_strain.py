"""Helpers of the strain tests (tests/test_strain_host.py, tests/test_strain_gpu.py): the 3 x 2 flow-map Jacobian from the
oracle's deformation tensor, its SVD with numpy (the expected value of every strain test), and the closed form the HIP kernel
implements, stated in numpy."""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def golden(name):
    """(x_dep, y_dep) of a committed config 1 fixture."""
    g = np.load(os.path.join(GOLD, name + ".npz"))
    return g["x_dep"], g["y_dep"]


def jacobian(tens):
    """F = [[dXdx, dXdy], [dYdx, dYdy], [dZdx, dZdy]] per cell, shape (ny, nx, 3, 2), from the oracle's (9, ny, nx) tensor."""
    a, b, c, d, e, f = (np.asarray(tens[i]) for i in range(6))
    return np.stack([np.stack([a, b], -1), np.stack([c, d], -1), np.stack([e, f], -1)], -2)


def svd_reference(tens):
    """(s1, s2, v1) of F with numpy.linalg.svd: singular values (ny, nx) and the leading right singular vector (ny, nx, 2)
    as (east, north), its sign as LAPACK left it."""
    F = jacobian(tens)
    _, s, vt = np.linalg.svd(F, full_matrices=False)
    return s[..., 0], s[..., 1], vt[..., 0, :]


def gram(tens):
    """p, q, r of C = F^T F = [[p, r], [r, q]] in float64."""
    a, b, c, d, e, f = (np.asarray(tens[i], dtype=np.float64) for i in range(6))
    return a * a + c * c + e * e, b * b + d * d + f * f, a * b + c * d + e * f


def closed_form(tens):
    """The kernel's formulas in float64: (s1, s2, e_lon, e_lat)."""
    a, b, c, d, e, f = (np.asarray(tens[i], dtype=np.float64) for i in range(6))
    p, q, r = gram(tens)
    dpq = p - q
    disc = np.sqrt(dpq * dpq + 4.0 * r * r)
    lam = 0.5 * ((p + q) + disc)
    s1 = np.sqrt(lam)
    cx, cy, cz = c * f - e * d, e * b - a * f, a * d - c * b        # col1 x col2
    area = np.sqrt(cx * cx + cy * cy + cz * cz)
    with np.errstate(invalid="ignore", divide="ignore"):
        s2 = np.where(s1 == 0, 0.0, area / s1)
        vx = np.where(p >= q, lam - q, r)
        vy = np.where(p >= q, r, lam - p)
        n = np.sqrt(vx * vx + vy * vy)
        ex, ey = vx / n, vy / n
    flip = (ex < 0) | ((ex == 0) & (ey < 0))
    ex, ey = np.where(flip, -ex, ex), np.where(flip, -ey, ey)
    iso = n == 0
    return s1, s2, np.where(iso, 1.0, ex), np.where(iso, 0.0, ey)


def eigen_residual(tens, ex, ey, lam):
    """|| C e - lam e || per cell, C from the tensor."""
    p, q, r = gram(tens)
    return np.hypot(p * ex + r * ey - lam * ex, r * ex + q * ey - lam * ey)


def sine_of_angle(ex, ey, v1):
    """|sin| of the angle between (ex, ey) and v1 (..., 2): the 2-D cross product of two unit vectors."""
    return np.abs(ex * v1[..., 1] - ey * v1[..., 0])


def sign_convention_holds(ex, ey):
    return bool(np.all((ex > 0) | ((ex == 0) & (ey > 0))))


def perturbed_seed_grid(ny=37, nx=64, seed=7, dtype=np.float64, lat_edge=70.0):
    """A seed grid (odd tile remainder in both directions; rows from -lat_edge to lat_edge) and a smooth random perturbation of
    it as departure points."""
    rng = np.random.default_rng(seed)
    lat = np.linspace(-lat_edge, lat_edge, ny)
    lon = -180.0 + 360.0 / nx * np.arange(nx)
    yy, xx = np.meshgrid(np.deg2rad(lat), np.deg2rad(lon), indexing="ij")
    x, y = xx * 0, yy * 0
    for _ in range(6):
        k, l = rng.integers(1, 4, 2)
        ax, ay, px, py = rng.uniform(-1, 1, 4)
        x += 4.0 * ax * np.sin(k * xx + 6.28 * px) * np.cos(l * yy)
        y += 3.0 * ay * np.cos(k * xx + 6.28 * py) * np.sin(l * yy + 1.0)
    return (lon[None, :] + x).astype(dtype), (lat[:, None] + y).astype(dtype), lat.astype(dtype), lon.astype(dtype)
