"""Helpers of the auxiliary-grid tests (tests/test_aux_gradient.py, tests/test_aux_gradient_gpu.py): the formulas of
csrc/aux_gradient.hip stated in numpy for any dtype (float32 / float64 as the kernels run them, ``np.longdouble`` as the
reference the tests judge by), the naive Cartesian difference the half-angle form replaces, an analytic smooth map, and the
eight departure planes of an auxiliary grid from the CPU oracle.  No expected value here comes from the engine."""
import numpy as np

R_EARTH = 6371000
PLANES = ("x_e", "y_e", "x_w", "y_w", "x_n", "y_n", "x_s", "y_s")


def _chord(xp, yp, xm, ym, T):
    """P+ - P- on the reference's sphere (LCS/LCS.py:195-199) from half-sums and half-differences of the angles, in T."""
    k = T(np.pi) / T(180)
    r2 = T(2) * T(R_EARTH)
    am = ((yp + ym) * T(0.5) - T(90)) * k
    da = ((yp - ym) * T(0.5)) * k
    lm = ((xp + xm) * T(0.5)) * k
    dl = ((xp - xm) * T(0.5)) * k
    sa, ca, sda, cda = np.sin(am), np.cos(am), np.sin(da), np.cos(da)
    sl, cl, sdl, cdl = np.sin(lm), np.cos(lm), np.sin(dl), np.cos(dl)
    A, B = ca * sda, sa * cda
    dX = r2 * ((A * cl) * cdl - (B * sl) * sdl)
    dY = r2 * ((A * sl) * cdl + (B * cl) * sdl)
    dZ = -(r2 * (sa * sda))
    return dX, dY, dZ


def _metric(seed_lat, sep_lat, sep_lon, T):
    k = T(np.pi) / T(180)
    R = T(R_EARTH)
    dx = ((k * sep_lon[None, :]) * R) * np.cos(seed_lat * k)[:, None]
    dy = ((k * sep_lat) * R)[:, None]
    return dx, dy


def derivatives(planes, seed_lat, sep_lat, sep_lon, T):
    """(dXdx, dXdy, dYdx, dYdy, dZdx, dZdy) in T from the eight planes (a mapping by PLANES' names), each (..., ny, nx)."""
    p = {k: np.asarray(planes[k]).astype(T) for k in PLANES}
    seed_lat, sep_lat, sep_lon = (np.asarray(a).astype(T) for a in (seed_lat, sep_lat, sep_lon))
    with np.errstate(invalid="ignore"):
        ex, ey, ez = _chord(p["x_e"], p["y_e"], p["x_w"], p["y_w"], T)
        nx_, ny_, nz_ = _chord(p["x_n"], p["y_n"], p["x_s"], p["y_s"], T)
        dx, dy = _metric(seed_lat, sep_lat, sep_lon, T)
        return ex / dx, nx_ / dy, ey / dx, ny_ / dy, ez / dx, nz_ / dy


def naive_derivatives(planes, seed_lat, sep_lat, sep_lon, T):
    """The same six derivatives as differences of X, Y, Z of the two points, each evaluated in T: what cancels."""
    p = {k: np.asarray(planes[k]).astype(T) for k in PLANES}
    seed_lat, sep_lat, sep_lon = (np.asarray(a).astype(T) for a in (seed_lat, sep_lat, sep_lon))
    k, R = T(np.pi) / T(180), T(R_EARTH)

    def xyz(x, y):
        a, l = (y - T(90)) * k, x * k
        return (R * np.sin(a)) * np.cos(l), (R * np.sin(a)) * np.sin(l), R * np.cos(a)
    e, w, n, s = xyz(p["x_e"], p["y_e"]), xyz(p["x_w"], p["y_w"]), xyz(p["x_n"], p["y_n"]), xyz(p["x_s"], p["y_s"])
    dx, dy = _metric(seed_lat, sep_lat, sep_lon, T)
    return tuple(v for i in range(3) for v in ((e[i] - w[i]) / dx, (n[i] - s[i]) / dy))


def closed_form(d, W=np.float64, layout="physical"):
    """The Gram and strain steps of csrc/flowmap_gradient.h in W on the six derivatives: dict of sigma (in ``layout``), s1, s2,
    e_lon, e_lat, lam (the larger eigenvalue of the physical F^T F) and p, q, r."""
    a, b, c, dd, e, f = (np.asarray(v).astype(W) for v in d)
    with np.errstate(invalid="ignore", divide="ignore"):
        p, q, r = a * a + c * c + e * e, b * b + dd * dd + f * f, a * b + c * dd + e * f
        dpq = p - q
        lam = W(0.5) * ((p + q) + np.sqrt(dpq * dpq + W(4) * r * r))
        s1 = np.sqrt(lam)
        cx, cy, cz = c * f - e * dd, e * b - a * f, a * dd - c * b
        s2 = np.where(s1 == 0, W(0), np.sqrt(cx * cx + cy * cy + cz * cz) / s1)
        vx, vy = np.where(p >= q, lam - q, r), np.where(p >= q, r, lam - p)
        n = np.sqrt(vx * vx + vy * vy)
        ex, ey = vx / n, vy / n
        flip = (ex < 0) | ((ex == 0) & (ey < 0))
        ex, ey = np.where(flip, -ex, ex), np.where(flip, -ey, ey)
        ex, ey = np.where(n == 0, W(1), ex), np.where(n == 0, W(0), ey)
        if layout == "physical":
            sigma = s1
        else:       # the reference's row-major 3 x 3 reshape (LCS/LCS.py:153): rows (a, b, c), (d, e, f)
            P, Q, Rr = a * a + b * b + c * c, dd * dd + e * e + f * f, a * dd + b * e + c * f
            sigma = np.sqrt(W(0.5) * ((P + Q) + np.sqrt((P - Q) * (P - Q) + W(4) * Rr * Rr)))
    return dict(sigma=sigma, s1=s1, s2=s2, e_lon=ex, e_lat=ey, lam=lam, p=p, q=q, r=r)


def restatement(planes, seed_lat, sep_lat, sep_lon, T, layout="physical"):
    """What the kernel computes, in numpy: the derivatives in T (float32 / float64), the Gram and strain steps in float64 --
    or everything in T for ``np.longdouble``, the reference."""
    W = np.longdouble if T is np.longdouble else np.float64
    return closed_form(derivatives(planes, seed_lat, sep_lat, sep_lon, T), W, layout)


def naive(planes, seed_lat, sep_lat, sep_lon, T, layout="physical"):
    return closed_form(naive_derivatives(planes, seed_lat, sep_lat, sep_lon, T), np.float64, layout)


# ------------------------------------------------------------------ maps
def smooth_map(x, y):
    """x' = x + 20 sin(2y) + 5 cos(3x), y' = 0.8 y + 4 sin(x) (degrees), in longdouble."""
    x, y = np.asarray(x, dtype=np.longdouble), np.asarray(y, dtype=np.longdouble)
    k = np.longdouble(np.pi) / 180
    return x + 20 * np.sin(2 * y * k) + 5 * np.cos(3 * x * k), 0.8 * y + 4 * np.sin(x * k) + 0 * x


def identity_map(x, y):
    x, y = np.asarray(x, dtype=np.longdouble), np.asarray(y, dtype=np.longdouble)
    return x + 0 * y, y + 0 * x


def planes_of_map(fmap, seed_lat, seed_lon, seeds, dtype):
    """The eight departure planes of ``fmap`` on the auxiliary grid ``seeds`` (Engine.aux_seeds), rounded to ``dtype``."""
    la, lo = np.asarray(seed_lat)[:, None], np.asarray(seed_lon)[None, :]
    pts = {"e": (seeds.lon_e[None, :], la), "w": (seeds.lon_w[None, :], la), "n": (lo, seeds.lat_n[:, None]),
           "s": (lo, seeds.lat_s[:, None])}
    out = {}
    for d, (x, y) in pts.items():
        fx, fy = fmap(x, y)
        out["x_" + d], out["y_" + d] = np.ascontiguousarray(fx.astype(dtype)), np.ascontiguousarray(fy.astype(dtype))
    return out


def aux_planes_from_oracle(O, u, v, lat, lon, seed_lat, seed_lon, seeds, **kw):
    """The eight departure planes from four runs of the oracle's parcel_propagation, one per shifted seed grid."""
    grids = {"e": (seed_lat, seeds.lon_e), "w": (seed_lat, seeds.lon_w), "n": (seeds.lat_n, seed_lon), "s": (seeds.lat_s, seed_lon)}
    out = {}
    for d, (la, lo) in grids.items():
        out["x_" + d], out["y_" + d] = O.parcel_propagation(u, v, lat, lon, seed_lat=la, seed_lon=lo, **kw)
    return out


def global_grid(ny, nx, dtype=np.float64, lat_edge=89.75):
    """Latitudes out to +-lat_edge, longitudes from -180, and a box that leaves every seed +- 0.5 degree inside."""
    lat = np.linspace(-lat_edge, lat_edge, ny).astype(dtype)
    lon = (-180.0 + 360.0 / nx * np.arange(nx)).astype(dtype)
    return lat, lon, (-90.0, 90.0, -180.5, 180.5)
