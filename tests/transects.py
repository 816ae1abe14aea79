"""TEST SUPPORT -- the host restatement of great-circle transects across ridge lines (csrc/transects.hip,
Engine.ridge_transects, tools.ridge_transects): the definition of include/lcs_hip.h written point by point in numpy and plain
Python floats (IEEE float64, one rounding per operation, nothing fused), and the bounds of tests/test_transects_gpu.py.

- ``tables``: numpy's cos / sin of ``degrees * pi / 180`` (``Engine.sphere_tables``); ``unit``: ``p = (cl cx, cl sx, sl)``.
- ``offsets``: ``s_k = k spacing``, ``k = -K .. K``, ``K = floor(half_width / spacing)``, with ``cos(s_k / R)``, ``sin(s_k / R)``.
- ``normals``: per point of every line the tangent from the chord ``p_b - p_a`` (``a``, ``b`` the points ``smooth`` before and
  after, clamped on an open line, wrapped on a ring with ``smooth`` capped at ``(count - 1) // 2``) made perpendicular to
  ``p_i`` and normalised, the left normal ``n = p_i x t``, its east / north components against the point's own column, the
  ``orient`` flip.  NaN where ``a == b`` or the tangent has no length.
- ``positions``: ``q = cos(s_k / R) p + sin(s_k / R) n``, latitude ``atan2(q_z, sqrt(q_x q_x + q_y q_y))``, longitude
  ``atan2(q_y, q_x)``, in degrees (times ``180 / pi``), wrapped into ``[lon[0], lon[0] + 360)`` with ``cyclic``.
- ``cells`` / ``interpolate``: the cell of a position by exact comparisons in the ascending coordinates, bilinear weights in
  float64 or the nearer node (ties to the lower index); beside every value ``sum |w_c v_c|``, what its tolerance is made of.
- ``composite``: per line and offset ``math.fsum`` of the finite values over their number.

The bounds:
- ``NORMAL_TOL = 16 eps64`` on every component of the normal and of the tangent.  Up to the unit tangent both sides perform the
  same IEEE operations on the same table entries (subtractions, products, one correctly rounded square root), so they cannot
  differ there; from the unit tangent on there are one division, a cross product (three roundings per component) and a
  component against east / north (five roundings): nine roundings of at most eps64 / 2 each on quantities bounded by 1, 4.5
  eps64; 16 leaves a factor of 3.5.  ``HEADING_TOL``: the heading is numpy's ``arctan2`` of the tangent's two components on
  both sides; two components within ``NORMAL_TOL`` of a unit vector turn it by at most ``2 NORMAL_TOL`` radians, to which the
  rounding of ``arctan2``, of the conversion and of ``mod`` adds at most 4 spacings of 360.
- ``POSITION_BOUND = 8 (E + 1) eps64`` radians on the great-circle separation of the device's position from the oracle's and on
  their latitude difference.  ``E`` is the largest distance in ulp between the device's ``atan2(...) (180 / pi)`` and numpy's on
  the same arguments: the arguments are formed from the device's own normals with the operations above, so nothing else
  differs.  A latitude is at most pi / 2 (one ulp: eps64 radians), a longitude at most pi (2 eps64): E ulp in each separate the
  positions by at most sqrt(5) E eps64; the two conversions to degrees add an ulp each; 8 covers both with a factor of 2.
- values: ``4 eps sum |w_c v_c|`` in the field's dtype against ``interpolate`` evaluated at the device's own positions;
  ``nearest`` bit for bit.  ``line_mean``: ``(n + 2) eps sum |v| / n`` against ``composite`` of the device's own values.
"""
from __future__ import annotations

import math

import numpy as np

from tests import lines as L

RADIUS = 6371000.0
EPS64 = float(np.finfo(np.float64).eps)
DEG = 180.0 / np.pi
NORMAL_TOL = 16 * EPS64
HEADING_TOL = float(np.degrees(2 * NORMAL_TOL) + 4 * np.spacing(360.0))
# E, measured on one MI355X (gfx950; the device library's atan2 against numpy 2.2's on x86-64) over the 143 133 evaluations of
# tests/test_transects_gpu.py's cases in the three orientations (every latitude, and every longitude the wrap left alone): 2 ulp
# for the latitudes and 2 ulp for the longitudes.  test_the_devices_atan2_is_within_E_ulp_of_numpys measures it again on every
# run and prints it (-s).
E = 2
POSITION_BOUND = 8 * (E + 1) * EPS64      # radians
ORIENTS = ("left", "north", "east")
METHODS = ("linear", "nearest")


def tables(lat, lon):
    lat, lon = np.asarray(lat, dtype=np.float64), np.asarray(lon, dtype=np.float64)
    y, x = lat * np.pi / 180, lon * np.pi / 180
    return np.cos(y), np.sin(y), np.cos(x), np.sin(x)


def unit(tab, pixel, nx):
    """``(X, Y, Z)`` of pixels (any shape): one rounded product each."""
    cl, sl, cx, sx = tab
    pixel = np.asarray(pixel, dtype=np.int64)
    r, c = pixel // nx, pixel % nx
    return cl[r] * cx[c], cl[r] * sx[c], sl[r]


def offsets(half_width, spacing, radius=RADIUS):
    K = int(math.floor(float(half_width) / float(spacing)))
    s = np.arange(-K, K + 1, dtype=np.float64) * np.float64(spacing)
    return K, s, np.cos(s / np.float64(radius)), np.sin(s / np.float64(radius))


def chord_ends(j, count, closed, smooth):
    """The positions ``(a, b)`` within the line of the chord's ends for its point ``j``."""
    if closed:
        m = min(smooth, (count - 1) // 2)
        return (j - m) % count, (j + m) % count
    return max(j - smooth, 0), min(j + smooth, count - 1)


def normals(trace, lat, lon, smooth=3, orient="left"):
    """``(n_points, 7)``: n_x, n_y, n_z, n_east, n_north, t_east, t_north, NaN for a point without a tangent.  ``trace``: the
    ``offset``, ``count``, ``closed`` of every line and the ``pixel`` of every point (tests/lines.py's trace or the device's)."""
    cl, sl, cx, sx = (t.tolist() for t in tables(lat, lon))
    nx_ = len(cx)
    pixel = [int(p) for p in trace["pixel"]]
    out = np.full((len(pixel), 7), np.nan)

    def vec(p):
        r, c = divmod(p, nx_)
        return cl[r] * cx[c], cl[r] * sx[c], sl[r]
    for off, cnt, closed in zip(trace["offset"], trace["count"], trace["closed"]):
        off, cnt = int(off), int(cnt)
        for j in range(cnt):
            a, b = chord_ends(j, cnt, bool(closed), smooth)
            if a == b:
                continue
            i = off + j
            (px, py, pz), (ax, ay, az), (bx, by, bz) = vec(pixel[i]), vec(pixel[off + a]), vec(pixel[off + b])
            dx, dy, dz = bx - ax, by - ay, bz - az
            dot = (dx * px + dy * py) + dz * pz
            tx, ty, tz = dx - dot * px, dy - dot * py, dz - dot * pz
            ln = math.sqrt((tx * tx + ty * ty) + tz * tz)
            if not ln > 0.0:
                continue
            tx, ty, tz = tx / ln, ty / ln, tz / ln
            n = [py * tz - pz * ty, pz * tx - px * tz, px * ty - py * tx]
            r, c = divmod(pixel[i], nx_)
            ux, uy = -(sl[r] * cx[c]), -(sl[r] * sx[c])
            ne, nn = cx[c] * n[1] - sx[c] * n[0], (ux * n[0] + uy * n[1]) + cl[r] * n[2]
            te, tn = cx[c] * ty - sx[c] * tx, (ux * tx + uy * ty) + cl[r] * tz
            flip = (orient == "north" and (nn < 0 or (nn == 0 and ne < 0))) or (orient == "east" and (ne < 0 or (ne == 0 and nn < 0)))
            if flip:
                n, ne, nn = [-v for v in n], -ne, -nn
            out[i] = (*n, ne, nn, te, tn)
    return out


def heading(te, tn):
    with np.errstate(invalid="ignore"):
        h = np.mod(np.degrees(np.arctan2(te, tn)), 360.0)
        return np.where(h >= 360.0, 0.0, h)            # a tiny negative angle rounds up to 360 itself


def heading_difference(a, b):
    """``|a - b|`` of two headings in degrees, on the circle (0 and 360 are one direction)."""
    with np.errstate(invalid="ignore"):
        d = np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))
        return np.minimum(d, 360.0 - d)


def raw_positions(normal, pixel, lat, lon, cos_off, sin_off):
    """``(latitude, longitude, q)`` before any wrap, ``(n_points, M)`` each (``q`` a tuple of three)."""
    px, py, pz = (v[:, None] for v in unit(tables(lat, lon), pixel, len(lon)))
    c, s = np.asarray(cos_off)[None, :], np.asarray(sin_off)[None, :]
    n = np.asarray(normal, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        qx, qy, qz = c * px + s * n[:, 0:1], c * py + s * n[:, 1:2], c * pz + s * n[:, 2:3]
        return np.arctan2(qz, np.sqrt(qx * qx + qy * qy)) * DEG, np.arctan2(qy, qx) * DEG, (qx, qy, qz)


def wrap(x, x0):
    with np.errstate(invalid="ignore"):
        x = x - np.floor((x - x0) / 360.0) * 360.0
        x = np.where(x < x0, x + 360.0, x)
        return np.where(x >= x0 + 360.0, x - 360.0, x)


def positions(normal, pixel, lat, lon, cos_off, sin_off, cyclic=False):
    y, x, _ = raw_positions(normal, pixel, lat, lon, cos_off, sin_off)
    return y, wrap(x, np.float64(lon[0])) if cyclic else x


def cells(y, x, lat, lon, cyclic=False):
    """Of positions of any shape: ``inside`` and, where inside, the rows ``j0``, ``j1``, the columns ``i0``, ``i1`` and the four
    coordinates ``ya``, ``yb``, ``xa``, ``xb`` of the cell (``xb = lon[0] + 360`` in the seam cell)."""
    lat, lon = np.asarray(lat, dtype=np.float64), np.asarray(lon, dtype=np.float64)
    ny, nx = lat.size, lon.size
    with np.errstate(invalid="ignore"):
        ok = (y >= lat[0]) & (y <= lat[-1]) & (x >= lon[0])
    ys, xs = np.where(ok, y, lat[0]), np.where(ok, x, lon[0])
    j0 = np.searchsorted(lat, ys, side="right") - 1
    j1 = np.minimum(j0 + 1, ny - 1)
    i0 = np.searchsorted(lon, xs, side="right") - 1
    last = i0 == nx - 1
    i1 = np.where(last, 0 if cyclic else nx - 1, np.minimum(i0 + 1, nx - 1))
    xa = lon[i0]
    xb = np.where(last, lon[0] + 360.0 if cyclic else lon[-1], lon[i1])
    inside = ok & np.where(last, xs < xb if cyclic else xs <= xa, True)
    return {"inside": inside, "j0": j0, "j1": j1, "i0": i0, "i1": i1, "ya": lat[j0], "yb": lat[j1], "xa": xa, "xb": xb}


def nearest_nodes(y, x, cell):
    """The rows and columns ``method='nearest'`` reads."""
    with np.errstate(invalid="ignore"):
        j = np.where(y - cell["ya"] > cell["yb"] - y, cell["j1"], cell["j0"])
        i = np.where(x - cell["xa"] > cell["xb"] - x, cell["i1"], cell["i0"])
    return j, i


def interpolate(planes, plane_of_point, y, x, lat, lon, cyclic=False, method="linear"):
    """``planes`` ``(n_planes, ny, nx)`` of one field, positions ``(n_points, M)``: ``(values, scale)`` in float64 before the
    rounding to the field's dtype, ``scale = sum |w_c v_c|`` (``|v|`` for nearest)."""
    planes = np.asarray(planes)
    f = planes.astype(np.float64)
    cell = cells(y, x, lat, lon, cyclic)
    m = np.broadcast_to(np.asarray(plane_of_point, dtype=np.int64)[:, None], y.shape)
    inside = cell["inside"]
    with np.errstate(invalid="ignore", divide="ignore"):
        if method == "nearest":
            j, i = nearest_nodes(y, x, cell)
            v = f[m, j, i]
            return np.where(inside, v, np.nan), np.where(inside, np.abs(v), np.nan)
        wy = np.where(cell["j1"] != cell["j0"], (y - cell["ya"]) / (cell["yb"] - cell["ya"]), 0.0)
        wx = np.where(cell["i1"] != cell["i0"], (x - cell["xa"]) / (cell["xb"] - cell["xa"]), 0.0)
        w = ((1.0 - wy) * (1.0 - wx), (1.0 - wy) * wx, wy * (1.0 - wx), wy * wx)
        v = (f[m, cell["j0"], cell["i0"]], f[m, cell["j0"], cell["i1"]], f[m, cell["j1"], cell["i0"]], f[m, cell["j1"], cell["i1"]])
        t = [wc * vc for wc, vc in zip(w, v)]
        value = ((t[0] + t[1]) + t[2]) + t[3]
        scale = ((np.abs(t[0]) + np.abs(t[1])) + np.abs(t[2])) + np.abs(t[3])
    return np.where(inside, value, np.nan), np.where(inside, scale, np.nan)


def composite(values, offset, count):
    """``values`` ``(n_points, M)`` of one field: ``(mean, count, scale)`` ``(n_lines, M)`` with ``math.fsum``; ``scale = sum |v|
    / n``."""
    v = np.asarray(values, dtype=np.float64)
    n_lines, M = len(offset), v.shape[1]
    mean, scale = np.full((n_lines, M), np.nan), np.full((n_lines, M), np.nan)
    num = np.zeros((n_lines, M), dtype=np.int32)
    for l, (off, cnt) in enumerate(zip(offset, count)):
        block = v[int(off):int(off) + int(cnt)]
        for k in range(M):
            col = block[:, k]
            col = col[np.isfinite(col)]
            num[l, k] = col.size
            if col.size:
                mean[l, k], scale[l, k] = math.fsum(col) / col.size, math.fsum(np.abs(col)) / col.size
    return mean, num, scale


def oracle(trace, fields, lat, lon, half_width, spacing, smooth=3, orient="left", method="linear", cyclic=False, radius=RADIUS):
    """Everything from the oracle's own normals and positions.  ``fields`` ``(n_fields, n_planes, ny, nx)``."""
    K, s, c_off, s_off = offsets(half_width, spacing, radius)
    nrm = normals(trace, lat, lon, smooth, orient)
    y, x = positions(nrm[:, :3], trace["pixel"], lat, lon, c_off, s_off, cyclic)
    plane_of_point = np.asarray(trace["plane"], dtype=np.int64)[np.asarray(trace["line"], dtype=np.int64)]
    fields = np.asarray(fields)
    vals = [interpolate(f, plane_of_point, y, x, lat, lon, cyclic, method)[0].astype(fields.dtype) for f in fields]
    return {"K": K, "offset": s, "cos_off": c_off, "sin_off": s_off, "normal": nrm, "latitude": y, "longitude": x,
            "values": np.stack(vals) if vals else np.zeros((0, *y.shape), dtype=fields.dtype), "plane_of_point": plane_of_point}


def separation(lat1, lon1, lat2, lon2):
    """Great-circle separation in radians of positions in degrees, by the haversine formula (well conditioned near 0)."""
    rad = np.pi / 180
    with np.errstate(invalid="ignore"):
        a = np.sin((lat2 - lat1) * rad / 2) ** 2 + np.cos(lat1 * rad) * np.cos(lat2 * rad) * np.sin((lon2 - lon1) * rad / 2) ** 2
        return 2 * np.arctan2(np.sqrt(a), np.sqrt(np.maximum(0.0, 1 - a)))


def haversine(lon1, lat1, lon2, lat2, radius=RADIUS):
    rad = math.pi / 180
    dlon, dlat = (lon2 - lon1) * rad, (lat2 - lat1) * rad
    a = math.sin(dlat / 2) ** 2 + math.cos(lat1 * rad) * math.cos(lat2 * rad) * math.sin(dlon / 2) ** 2
    return 2 * radius * math.atan2(math.sqrt(a), math.sqrt(max(0.0, 1 - a)))


def ambiguous(y, x, lat, lon, cyclic=False, method="linear", bound=POSITION_BOUND):
    """Positions within ``bound`` (radians on the sphere) of where the cell, or the nearest node, changes: a node's latitude or
    longitude (the domain's edges among them, and ``lon[0] + 360`` with ``cyclic``), and for ``nearest`` the midpoints."""
    lat, lon = np.asarray(lat, dtype=np.float64), np.asarray(lon, dtype=np.float64)
    ys, xs = lat, np.append(lon, lon[0] + 360.0) if cyclic else lon
    if method == "nearest":
        ys, xs = np.sort(np.concatenate([ys, (ys[1:] + ys[:-1]) / 2])), np.sort(np.concatenate([xs, (xs[1:] + xs[:-1]) / 2]))
    tol = np.degrees(bound)
    with np.errstate(invalid="ignore"):
        near_y = np.abs(y[..., None] - ys).min(-1) <= 2 * tol
        tol_x = 2 * tol / np.maximum(np.cos(np.radians(y)), 1e-300)
        near_x = np.abs(x[..., None] - xs).min(-1) <= tol_x
    return near_y | near_x | np.isnan(y) | np.isnan(x)


def ulps(got, want):
    """``|got - want|`` in units of the spacing of ``want``."""
    return np.abs(got - want) / np.spacing(np.abs(want))


# ------------------------------------------------------------------ the masks, grids and fields of the tests
def line_mask(ny, nx, n):
    """A serpentine of exactly ``n`` points in a ``ny x nx`` plane: rows 0, 2, 4, ... joined alternately at their ends, cut off
    after ``n`` pixels -- one open line (``n >= 2``) or a lone pixel."""
    m = np.zeros((ny, nx))
    r, c, step = 0, 0, 1
    for _ in range(n):
        assert r < ny
        m[r, c] = 1
        if 0 <= c + step < nx and not (m[r, c + step]):
            c += step
        elif r % 2 == 0:
            r += 1
        else:
            r, step = r + 1, -step
    return m


def ring_mask(ny=12, nx=16):
    m = np.zeros((ny, nx))
    m[2, 3:11] = m[8, 3:11] = m[2:9, 3] = m[2:9, 10] = 1
    return m


def junction_mask(ny=12, nx=16):
    m = np.zeros((ny, nx))
    m[5, 1:14] = 1
    m[1:11, 7] = 1
    return m


def regional_grid(ny, nx):
    return L.grid(ny, nx)


def gaussian_like_grid(ny, nx):
    """Ascending, non-uniform latitudes (the roots of a Legendre polynomial) and uniform longitudes."""
    lat = np.degrees(np.arcsin(np.polynomial.legendre.leggauss(ny)[0]))
    return np.sort(lat), np.linspace(0.0, 360.0, nx, endpoint=False)


def fields_of(n_fields, shape, seed, dtype=np.float64, nan_nodes=0):
    """Seeded smooth-ish fields ``(n_fields, *shape)`` of both signs and different magnitudes, with ``nan_nodes`` NaN nodes each."""
    rng = np.random.default_rng([20261021, seed])
    f = rng.normal(size=(n_fields, *shape)) * 10.0 ** rng.integers(-2, 3, size=(n_fields,) + (1,) * len(shape))
    for k in range(n_fields):
        flat = f[k].reshape(-1)
        flat[rng.choice(flat.size, size=nan_nodes, replace=False)] = np.nan
    return f.astype(dtype)


def _seam_mask(ny=20, nx=32):
    m = np.zeros((ny, nx))
    m[6, :5] = m[6, -4:] = 1            # a row across the seam
    m[10:17, 1] = 1                     # a meridional line next to it: its transects cross the seam
    m[9:16, nx - 2] = 1
    return m


def _edge_mask(ny=20, nx=32):
    m = np.zeros((ny, nx))
    m[1, 1:-1] = m[-2, 1:-1] = m[1:-1, 1] = m[1:-1, -2] = 1      # a ring one pixel inside the border: it looks out over all four edges
    return m


def _pole_mask(ny=19, nx=36):
    m = np.zeros((ny, nx))
    m[ny - 2, 3:12] = 1                 # along the last parallel before the north pole row
    m[1, 20:30] = 1                     # and the first after the south pole row
    m[10:17, 16] = 1                    # a meridional line clear of the equator row, whose transects would follow a node's latitude
    return m


def _shapes(ny=16, nx=24):
    ring, junction = ring_mask(ny, nx), junction_mask(ny, nx)
    junction[13, 20] = 1                # a lone pixel
    return np.stack([ring, junction, line_mask(ny, nx, 40)])


def _cyclic_grid(ny, nx, start=0.0):
    return np.linspace(-78.0, 81.0, ny), np.linspace(start, start + 360.0, nx, endpoint=False)


def _polar_grid(ny, nx):
    return np.linspace(-90.0, 90.0, ny), np.linspace(-180.0, 180.0, nx, endpoint=False)


def _case(mask, grid, cyclic=False, half_width=500e3, spacing=25e3, smooth=3, n_fields=1, dtype=np.float64, nan_nodes=0, seed=0):
    lat, lon = grid
    return dict(mask=mask, lat=lat, lon=lon, cyclic=cyclic, half_width=half_width, spacing=spacing, smooth=smooth, n_fields=n_fields,
                dtype=dtype, nan_nodes=nan_nodes, seed=seed)


SMOOTH = 3
LENGTHS_FIXED = (1, 2, 3, 2 * SMOOTH, 2 * SMOOTH + 1)


def cases(threads=256, chunk=256):
    """name -> case.  ``threads`` and ``chunk`` are csrc/transects.hip's TR_THREADS and TR_CHUNK: the long lines sit around them
    (with one offset a composite workgroup adds ``chunk`` points per pass, and ``n_points * M`` is the line's length)."""
    out = {}
    lengths = sorted(set(LENGTHS_FIXED + (chunk - 1, chunk, chunk + 1, threads - 1, threads, threads + 1, 2 * chunk + 1)))
    for n in lengths:
        for M, (hw, sp) in ((1, (0.0, 200e3)), (3, (200e3, 200e3))):
            out[f"line-{n}-M{M}"] = _case(line_mask(40, 64, n), regional_grid(40, 64), half_width=hw, spacing=sp, seed=n)
    out["shapes-3d-f32x5-M41"] = _case(_shapes(), regional_grid(16, 24), n_fields=5, dtype=np.float32, seed=1)
    out["shapes-3d-f64x1-nan"] = _case(_shapes(), regional_grid(16, 24), nan_nodes=30, seed=2)
    out["ring-junction-2d-f64x5"] = _case(np.maximum(ring_mask(), np.roll(junction_mask(), 0)), regional_grid(12, 16), n_fields=5, seed=3)
    out["ring-2d-f32x1-nan"] = _case(ring_mask(), regional_grid(12, 16), dtype=np.float32, nan_nodes=12, seed=4)
    out["seam"] = _case(_seam_mask(), _cyclic_grid(20, 32, start=-180.0), cyclic=True, half_width=1500e3, spacing=100e3, n_fields=2, seed=5)
    out["seam-lon0-20"] = _case(_seam_mask(), _cyclic_grid(20, 32, start=20.0), cyclic=True, half_width=1500e3, spacing=100e3, seed=6)
    out["edges"] = _case(_edge_mask(), regional_grid(20, 32), half_width=1000e3, spacing=100e3, seed=7)
    out["pole"] = _case(_pole_mask(), _polar_grid(19, 36), cyclic=True, half_width=2500e3, spacing=125e3, n_fields=2, seed=8)
    out["pole-not-cyclic"] = _case(_pole_mask(), _polar_grid(19, 36), half_width=2500e3, spacing=125e3, seed=9)
    out["gaussian-latitudes"] = _case(np.maximum(ring_mask(40, 64), junction_mask(40, 64)), gaussian_like_grid(40, 64), cyclic=True,
                                      n_fields=2, dtype=np.float32, seed=10)
    return out


def case_fields(case):
    """``(n_fields, n_planes, ny, nx)``."""
    m = case["mask"]
    shape = m.shape if m.ndim == 3 else (1, *m.shape)
    return fields_of(case["n_fields"], shape, case["seed"], case["dtype"], case["nan_nodes"])


def case_trace(case):
    m = case["mask"]
    t = L.trace_planes(m if m.ndim == 3 else m[None], case["cyclic"], metric="sphere", lat=case["lat"], lon=case["lon"])
    return t


def on_a_grid_line(normal, K):
    """Samples that lie on a node's latitude or longitude by construction: offset 0 (the point is a node) and the transects of
    points whose normal has no east component (the transect follows the point's meridian) -- ``(n_points, M)``."""
    mask = np.zeros((normal.shape[0], 2 * K + 1), dtype=bool)
    mask[:, K] = True
    mask |= (np.abs(normal[:, 3]) <= NORMAL_TOL)[:, None]
    return mask
