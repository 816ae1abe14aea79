"""TEST SUPPORT -- the host restatement of the spherical ridge properties (csrc/components.hip: lc_component_sphere_sums;
Engine.sphere_cell_tables / component_sphere_props / filter_components(metric='sphere'); tools.ridge_properties and
filter_ridges(metric='sphere')) in numpy, the coordinates the tests use, and the error bounds the tests assert.

- ``cell_tables``: the separable cell areas, edge by edge in a python loop.
- ``tables``: the six tables the device reads, as the engine forms them.
- ``sums``: per label the root, the pixel count, the eleven sums W | M1 | M2 | S and ``sum |term|`` of each, the extrema.  The
  terms are formed with the device's operations in the device's order (every product and difference rounded once to float64:
  numpy's element-wise loops fuse nothing), so they are the device's terms bit for bit; each SUM is ``math.fsum`` of them, the
  correctly rounded sum -- the reference's own error is then one rounding, not a second arbitrary summation order.
- ``props``: the properties from those sums by the documented formulas, the eigen-decomposition by ``numpy.linalg.eigh``.
- ``bounds``: see its docstring.
- ``filtered``: the mask with the labels that fail a threshold on the sphere replaced by ``fill``.
"""
from __future__ import annotations

import math

import numpy as np

from tests import components as CO

EPS = 2.0 ** -53
SOLVE = 64          # the eigen-solvers' error: SOLVE * EPS * trace(C), see bounds()
NAMES = ("W", "M1x", "M1y", "M1z", "M2xx", "M2xy", "M2xz", "M2yy", "M2yz", "M2zz", "S")


# ------------------------------------------------------------------ coordinates
def coordinates(shape, variant="uniform"):
    """``(lat, lon)`` of a case of shape (ny, nx).  ``uniform``: lat = linspace(-78, 81, ny), lon = -180 + 360 arange(nx) / nx.
    ``gauss``: latitudes bunched towards the equator like Gaussian ones (not uniform), the same longitudes.  ``global``: lat =
    linspace(-90, 90, ny): the outer band edges would lie beyond the poles and are clipped there."""
    ny, nx = shape
    lon = -180.0 + 360.0 * np.arange(nx) / nx
    if variant == "uniform":
        lat = np.linspace(-78.0, 81.0, ny)
    elif variant == "gauss":
        lat = np.degrees(np.arcsin(np.linspace(-0.97, 0.985, ny))) if ny > 1 else np.array([3.0])
    elif variant == "global":
        lat = np.linspace(-90.0, 90.0, ny)
    else:
        raise ValueError(variant)
    return lat, lon


def cell_tables(lat, lon, cyclic=False):
    lat, lon = np.asarray(lat, dtype=np.float64), np.asarray(lon, dtype=np.float64)

    def edges(x, first, last):
        e = [x[0] - first / 2]
        for k in range(1, x.size):
            e.append((x[k - 1] + x[k]) / 2)
        e.append(x[-1] + last / 2)
        return np.array(e)
    ey = np.minimum(np.maximum(edges(lat, lat[1] - lat[0], lat[-1] - lat[-2]), -90.0), 90.0)
    sy = np.sin(ey * np.pi / 180)
    gap = lon[0] + 360.0 - lon[-1]
    ex = edges(lon, gap, gap) if cyclic else edges(lon, lon[1] - lon[0], lon[-1] - lon[-2])
    return (np.array([sy[k + 1] - sy[k] for k in range(lat.size)]),
            np.array([(ex[k + 1] - ex[k]) * np.pi / 180 for k in range(lon.size)]))


def tables(lat, lon, cyclic=False):
    """cos lat, sin lat, row weight, cos lon, sin lon, column weight."""
    y, x = np.asarray(lat, dtype=np.float64) * np.pi / 180, np.asarray(lon, dtype=np.float64) * np.pi / 180
    rw, cw = cell_tables(lat, lon, cyclic)
    return np.cos(y), np.sin(y), rw, np.cos(x), np.sin(x), cw


# ------------------------------------------------------------------ sums
def sums(labels, n, lat, lon, intensity=None, cyclic=False):
    """Labels 1 .. n of one plane (a label without a pixel: count 0, root -1, sums 0, NaN extrema).  dict: ``root`` (n,),
    ``count`` (n,), ``sums`` (11, n) in the order of NAMES, ``abs`` (11, n) the sums of the terms' magnitudes, ``max``, ``min``
    (n,) with an intensity (row 10 of both is 0 without one)."""
    labels = np.asarray(labels)
    nx = labels.shape[1]
    cl, sl, rw, cx, sx, cw = tables(lat, lon, cyclic)
    flat = labels.ravel()
    order = np.argsort(flat, kind="stable")
    bounds = np.searchsorted(flat[order], np.arange(1, n + 2))
    count = np.diff(bounds)
    idx = order[bounds[0]:bounds[n]]                   # the measured pixels, by label and then in raster order
    start = bounds[:-1] - bounds[0]
    root = np.where(count > 0, order[np.minimum(bounds[:-1], flat.size - 1)], -1).astype(np.int32)
    root_of_pixel = np.repeat(root, count)
    r, c = np.divmod(idx, nx)
    rr, rc = np.divmod(root_of_pixel, nx)
    dx = cl[r] * cx[c] - cl[rr] * cx[rc]
    dy = cl[r] * sx[c] - cl[rr] * sx[rc]
    dz = sl[r] - sl[rr]
    w = rw[r] * cw[c]
    wx, wy, wz = w * dx, w * dy, w * dz
    terms = [w, wx, wy, wz, wx * dx, wx * dy, wx * dz, wy * dy, wy * dz, wz * dz]
    if intensity is not None:
        v = np.asarray(intensity, dtype=np.float64).ravel()[idx]
        terms.append(w * v)
    else:
        terms.append(np.zeros_like(w))
    T = np.stack(terms)                                # (11, pixels)
    out = dict(root=root, count=count.astype(np.int64), sums=np.zeros((11, n)), abs=np.zeros((11, n)))
    one, two = count == 1, count == 2                  # one addition at most: any order gives the correctly rounded sum
    out["sums"][:, one], out["abs"][:, one] = T[:, start[one]], np.abs(T[:, start[one]])
    out["sums"][:, two] = T[:, start[two]] + T[:, start[two] + 1]
    out["abs"][:, two] = np.abs(T[:, start[two]]) + np.abs(T[:, start[two] + 1])
    for k in np.flatnonzero(count >= 3):
        seg = slice(start[k], start[k] + count[k])
        for j in range(11):
            out["sums"][j, k], out["abs"][j, k] = math.fsum(T[j, seg]), math.fsum(np.abs(T[j, seg]))      # a NaN term gives NaN
    if intensity is not None:
        out["max"], out["min"] = np.full(n, np.nan), np.full(n, np.nan)
        some = count > 0
        if some.any():                                 # the segments of the labels that have pixels follow one another
            out["max"][some] = np.maximum.reduceat(v, start[some])      # np.maximum / np.minimum hand a NaN on
            out["min"][some] = np.minimum.reduceat(v, start[some])
    return out


# ------------------------------------------------------------------ properties
def props(s, lat, lon, radius=6371000.0, with_intensity=True):
    """The properties of every label of ``sums``' result; labels without a pixel: area 0, NaN elsewhere.  Also ``e`` (n, 3)
    descending, ``trace``, ``C`` (n, 3, 3), ``m`` (n, 3), ``c`` (n, 3) the centroid before it is normalised, ``rho`` = |c|, ``h``
    its horizontal part and ``tangent`` the length of the major eigenvector's part in the tangent plane at the centroid."""
    cl, sl, _, cx, sx, _ = tables(lat, lon)
    n, nx = s["count"].size, cx.size
    some = s["count"] > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        S = np.where(some, s["sums"], np.nan)
        W = S[0]
        m = S[1:4] / W                                                         # (3, n)
        C = np.empty((n, 3, 3))
        for q, (i, j) in enumerate([(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]):
            C[:, i, j] = C[:, j, i] = S[4 + q] / W - m[i] * m[j]
        ok = np.isfinite(C).all(axis=(1, 2))
        e, vec = np.full((n, 3), np.nan), np.full((n, 3, 3), np.nan)
        if ok.any():
            e[ok], vec[ok] = np.linalg.eigh(C[ok])                             # ascending
        e1, e2, v = e[:, 2], e[:, 1], vec[:, :, 2]
        r2 = radius * radius
        rr, rc = np.divmod(np.maximum(s["root"], 0), nx)
        c = np.stack([cl[rr] * cx[rc], cl[rr] * sx[rc], sl[rr]]) + m          # (3, n)
        h, rho = np.sqrt(c[0] * c[0] + c[1] * c[1]), np.sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2])
        there = rho >= 1e-6                                                    # False on NaN
        phi, lam = np.where(there, np.arctan2(c[2], h), np.nan), np.where(there, np.arctan2(c[1], c[0]), np.nan)
        ve = v[:, 1] * np.cos(lam) - v[:, 0] * np.sin(lam)
        vn = v[:, 2] * np.cos(phi) - np.sin(phi) * (v[:, 0] * np.cos(lam) + v[:, 1] * np.sin(lam))
        t = np.degrees(np.arctan2(vn, ve))
        t = np.where(t > 90.0, t - 180.0, np.where(t <= -90.0, t + 180.0, t))
        out = dict(area=np.where(some, r2 * W, 0.0),
                   major_axis_length=4.0 * radius * np.sqrt(np.maximum(e1, 0.0)),
                   minor_axis_length=4.0 * radius * np.sqrt(np.maximum(e2, 0.0)),
                   centroid_latitude=np.degrees(phi), centroid_longitude=np.degrees(lam),
                   orientation=np.where(e1 > 0.0, t, np.nan),
                   mean_intensity=S[10] / W if with_intensity else np.full(n, np.nan),
                   total_intensity=r2 * S[10] if with_intensity else np.full(n, np.nan),
                   e=e[:, ::-1], C=C, m=m.T, c=c.T, rho=rho, h=h, trace=C[:, 0, 0] + C[:, 1, 1] + C[:, 2, 2], tangent=np.hypot(ve, vn))
    return out


def angle_difference(a, b, period):
    """|a - b| as angles of that period (degrees)."""
    return np.abs((np.asarray(a) - np.asarray(b) + period / 2) % period - period / 2)


def bounds(s, p, radius=6371000.0):
    """Bounds on |device - restatement|, per label, derived from the arithmetic alone; u = 2^-53, n = the label's pixel count.

    ``sums`` (11, n): n u sum|term|.  The device adds the label's n terms (bit for bit the restatement's) in some order: the
    standard bound is (n - 1) u sum|term|; the restatement's own sum is correctly rounded: u |sum| <= u sum|term| more.

    With A1_i = sum|w d_i| / W >= |m_i| and A2_ij = sum|w d_i d_j| / W >= |M2_ij / W| (the weights are positive):
    ``m``   bm_i = (2 n + 4) u A1_i: the two sums of the quotient contribute n u A1_i each, the divisions of both sides u |m_i|.
    ``C``   bC_ij = (2 n + 4) u A2_ij + |m_i| bm_j + |m_j| bm_i + bm_i bm_j + 4 u (A2_ij + |m_i m_j|): the quotient as above, the
            product of the two means, and the product's and the difference's roundings on both sides.
    ``e``   be = |bC|_F + SOLVE u (trace C + |bC|_F): Weyl's inequality for the perturbation, plus the solvers (cyclic Jacobi
            there, LAPACK here), each backward stable with an error of a small multiple of u |C|; |C| <= trace C + |bC|_F.
    axis lengths  4 R (sqrt(e + be) - sqrt(max(e - be, 0))) + 8 u L: the square root is monotone; three more roundings a side.
    ``area`` (n + 4) u area; ``total_intensity`` (n + 4) u R^2 sum|w v|; ``mean_intensity`` (2 n + 4) u sum|w v| / W.
    centroid  bc = |(bm_i + 2 u)_i| (the sum n(root) + m rounds once more, and the device may fuse the root's product into it);
            the direction moves by at most asin(bc / rho) <= 1.01 bc / rho (asserted small by the tests on the reference);
            latitude: that angle, longitude: 1.01 bc / h, each plus 16 u |angle| for atan2, the square roots and the degrees.
    ``orientation``  with E = |bC|_F + 2 SOLVE u (trace C + |bC|_F) and gap = e1 - e2: the major eigenvector turns by at most
            2 E / gap (Davis-Kahan, sin theta <= E / (gap - E), for E <= gap / 4, which the tests assert on the reference); the
            (east, north) basis turns with the centroid by at most the sum of its two angle bounds, counted twice; evaluating
            the two projections and atan2 costs at most 32 u / t, t the length of the eigenvector's tangential part."""
    n = s["count"].astype(np.float64)
    W = s["sums"][0]
    with np.errstate(invalid="ignore", divide="ignore"):
        out = {"sums": n * EPS * s["abs"]}
        A1 = s["abs"][1:4] / W                                         # (3, n)
        A2 = np.empty((3, 3, n.size))
        for q, (i, j) in enumerate([(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]):
            A2[i, j] = A2[j, i] = s["abs"][4 + q] / W
        m = np.abs(p["m"].T)                                           # (3, n)
        bm = (2 * n + 4) * EPS * A1
        bC = np.empty((3, 3, n.size))
        for i in range(3):
            for j in range(3):
                bC[i, j] = (2 * n + 4) * EPS * A2[i, j] + m[i] * bm[j] + m[j] * bm[i] + bm[i] * bm[j] + 4 * EPS * (A2[i, j] + m[i] * m[j])
        EF = np.sqrt((bC ** 2).sum(axis=(0, 1)))
        solve = SOLVE * EPS * (p["trace"] + EF)
        be = EF + solve
        out.update(m=bm, C=bC, e=be)
        for name, col in (("major_axis_length", 0), ("minor_axis_length", 1)):
            e = p["e"][:, col]
            out[name] = 4 * radius * (np.sqrt(e + be) - np.sqrt(np.maximum(e - be, 0))) + 8 * EPS * p[name]
        out["area"] = (n + 4) * EPS * p["area"]
        out["total_intensity"] = (n + 4) * EPS * radius * radius * s["abs"][10]
        out["mean_intensity"] = (2 * n + 4) * EPS * s["abs"][10] / W
        bc = np.sqrt(((bm + 2 * EPS) ** 2).sum(axis=0))
        turn_lat, turn_lon = 1.01 * bc / p["rho"], 1.01 * bc / p["h"]
        out["centroid_turn"] = bc / p["rho"]
        out["centroid_latitude"] = np.degrees(turn_lat) + 16 * EPS * np.abs(p["centroid_latitude"])
        out["centroid_longitude"] = np.degrees(turn_lon) + 16 * EPS * np.abs(p["centroid_longitude"])
        E = EF + 2 * solve
        gap = p["e"][:, 0] - p["e"][:, 1]
        out["E_over_gap"] = E / gap
        out["orientation"] = np.degrees(2 * E / gap + 2 * (turn_lat + turn_lon) + 32 * EPS / p["tangent"])
    return out


# ------------------------------------------------------------------ the filter
def filtered(mask, intensity, criteria, thresholds, lat, lon, connectivity=2, cyclic=False, fill=0.0, radius=6371000.0):
    mask = np.asarray(mask)
    lab, n = CO.label(mask, connectivity, cyclic)
    s = sums(lab, n, lat, lon, intensity, cyclic)
    p = props(s, lat, lon, radius)
    p["max_intensity"], p["min_intensity"] = s["max"], s["min"]
    keep = np.ones(n, bool)
    for k, th in zip(criteria, thresholds):
        with np.errstate(invalid="ignore"):
            keep &= p[k] >= th
    table = np.concatenate([[False], keep])
    return np.where(table[lab], mask, np.asarray(fill, dtype=mask.dtype))
