"""Designed cells for the Gram and strain steps (csrc/flowmap_gradient.h: gram_eigen, stretch_of) and an independent judge.

Used by tests/test_jacobians.py (CPU), tests/test_jacobians_gpu.py and tests/golden/make_jacobians_mp.py (the 50-digit
fixture).  No expected value here comes from the engine.

**The case table** (:func:`table`): one ``(ny, nx)`` plane of auxiliary-grid cells per dtype.  A cell has a name, a class, a
seed ``(lat, lon)``, the offsets ``d_ew`` / ``d_ns`` of its east-west and north-south parcel pairs, and its eight departure
values.  A designed cell takes a tangent Jacobian ``J = R(alpha) diag(1, +-1/ratio) R(beta)^T`` (east, north components; the
minus sign is the reflection, det < 0) and puts the parcels at ``E/W = seed +- o_ew J[:, 0]``, ``N/S = seed +- d_ns J[:, 1]``,
the east component divided by ``cos(lat)``; the stretching direction is ``(cos beta, sin beta)``.  ``seed_lat`` and ``sep_lat
= 2 d_ns`` belong to a row and ``sep_lon = 2 d_ew`` to a column (lc_aux_gradient's arguments).  The east-west pair's seeds are
``d_ew`` degrees of longitude from the centre, ``o_ew = d_ew cos(lat)`` on the sphere, so with that offset the metric is the
nominal one in every cell and one column serves every latitude: a row is a ``(seed latitude, d_ns)`` pair, a column group a
``d_ew``, and a cell takes the next free column of its group in its row.  Slots no cell takes hold a ``collapsed`` cell at the
row's seed.

Classes (the class column decides what a test asserts about a cell; nothing is decided from the data):

``generic``          ratio 1.5, 1e3, 1e6 x beta 0, +-0.3, pi/4, +-1.2, pi/2, alpha and the reflection varied with them, at the
                     seeds (0, 0), (10, 20), (60, 179.9), (+-85, ..) and (+-89.75, ..).  beta = -1.2 gives r < 0 with p < q,
                     the vx < 0 flip; beta = 0 / pi/2 lie on the two sides of p >= q.
                     The designed ratio has to survive as s1 / s2 of the rounded planes within a factor 2
                     (tests/test_jacobians.py), which sets the offsets at the high latitudes (``OFFSETS``): a pair whose
                     longitudes differ by w radians has a chord that leaves the tangent vector by w^2 / 6, so the
                     north-south pair (d_ns / cos(lat) of longitude) wants a small d_ns there, and float32 rounds a latitude
                     near 90 to 3.8e-6 degrees, so the east-west pair (d_ew cos(lat) of latitude) wants a large d_ew.
                     float64 carries all three ratios at every seed.  float32 drops ratio 1e6 everywhere (ulp(60) / 2 =
                     1.9e-6 degrees against d / 1e6) and at +-89.75 takes ratio 30 in the place of 1e3: there the two
                     demands leave 6e-4 of s1 as the least error of s2, which 1e-3 does not survive.
``near_isotropic``   ratio 1, 1 + 1e-9, 1 + 1e-4: the direction is ill-conditioned by design (never compared).
``isotropic_exact``  the identity at (0, 0): in float64 p == q and r == 0 bitwise, and the kernels must return (s, s, 1, 0).
                     Not so in float32 (the device's float32 sines are not numpy's).  Its errors are measured with the
                     near_isotropic cells (:func:`judged_class`).
``collapsed``        all four parcels at one point: the half-differences are 0 in every arithmetic, F = 0.
``rank_one_ew`` / ``rank_one_ns``   E == W / N == S: one column of F is exactly 0.
``seam``             at (60, 179.95): x_e wrapped to -179.8, its twin unwrapped, and the four longitudes shifted by +3960
                     degrees (a mean of 72.3 rad: the |a| >= 64 library branch of the float32 mean angle) and by +3420 (a mean
                     of 3600 degrees, 62.8 rad: just inside the polynomial's).
``wide``             half-differences of 30, 50, 89 degrees in longitude, latitude and both (either side of the pi/4 switch
                     of the float32 half-angle sine).
``tiny``             d = 1e-4 degrees (float32) / 1e-9 (float64).
``nonfinite``        not cells of the plane: :func:`poisons` lists the NaN / inf runs, each on a copy of the plane.

**The judge** (:func:`judge`): ``np.longdouble``.  After the six derivatives it uses none of the kernel's formulas: one
Hestenes rotation of F's two columns by theta = atan2(2 r, p - q) / 2, s1 and s2 the norms of the rotated columns, the
direction (cos theta, sin theta) in the project's sign convention; the reference layout's sigma the same on the rows
(a, b, c), (d, e, f).  No ``p q - r^2`` and no ``(p + q) - disc``.
The six derivatives (:func:`derivatives`) are the half-angle chords of ``tests.aux_gradient.derivatives``, with every sine and
cosine taken after an exact reduction of the angle in degrees (:func:`sincos_deg`).  ``tests.aux_gradient.derivatives`` in
longdouble multiplies the degrees by k first, and a cosine next to one of its zeros (the metric's cos(89.75 k), the seam's
sin(179.95 k), 69 rad of the shifted seam cells) then carries the rounding of that product tan(angle) x angle times over: 17
eps at 85 degrees, 205 eps at 89.75, 280 eps on the seam cells, measured against the 50-digit fixture, where the fixture's
test allows 8.  tests/test_jacobians.py holds the two derivative steps to each other within that amplification.
"""
import os
from collections import namedtuple

import numpy as np

from tests import aux_gradient as AG

GOLD = os.path.join(os.path.dirname(__file__), "golden", "jacobians_mp.npz")
OUTS = ("sigma", "s1", "s2", "e_lon", "e_lat")
FINITE_CLASSES = ("generic", "near_isotropic", "isotropic_exact", "collapsed", "rank_one_ew", "rank_one_ns", "seam", "wide", "tiny")

D0 = 0.05                                              # degrees: the offset of every cell that names no other
D_TINY = {np.dtype(np.float32): 1e-4, np.dtype(np.float64): 1e-9}
SEEDS = {"eq": (0.0, 0.0), "mid": (10.0, 20.0), "n60": (60.0, 179.9), "n85": (85.0, 40.0), "s85": (-85.0, -30.0),
         "n8975": (89.75, 100.0), "s8975": (-89.75, -100.0)}
BETAS = (0.0, 0.3, -0.3, np.pi / 4, 1.2, -1.2, np.pi / 2)
RATIOS = (1.5, 1e3, 1e6)
# (d_ns, d_ew) of the generic, collapsed and rank-one cells at the high-latitude seeds (the docstring's generic row); D0 elsewhere
OFFSETS = {np.dtype(np.float64): {"n85": (0.005, D0), "s85": (0.005, D0), "n8975": (1e-4, D0), "s8975": (1e-4, D0)},
           np.dtype(np.float32): {"n85": (D0, 0.5), "s85": (D0, 0.5), "n8975": (0.01, 2.0), "s8975": (0.01, 2.0)}}

Cell = namedtuple("Cell", "name cls lat lon d_ns d_ew values ratio beta")          # values: the eight planes' entries, PLANES' order
Table = namedtuple("Table", "dtype cells index planes seed_lat sep_lat sep_lon cls names")


def rot(t):
    return np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]])


def jacobian(alpha, beta, ratio, reflect=False):
    return rot(alpha) @ np.diag([1.0, (-1.0 if reflect else 1.0) / ratio]) @ rot(beta).T


def _designed(name, cls, seed, d_ns, d_ew, J, ratio=None, beta=None, shift=0.0, wrap_e=False):
    lat, lon = seed
    c = np.cos(np.deg2rad(lat))
    x_e, y_e = lon + (d_ew * c) * J[0, 0] / c, lat + (d_ew * c) * J[1, 0]      # the pair's offset on the sphere: d_ew cos(lat)
    x_w, y_w = lon - (d_ew * c) * J[0, 0] / c, lat - (d_ew * c) * J[1, 0]
    x_n, y_n = lon + d_ns * J[0, 1] / c, lat + d_ns * J[1, 1]
    x_s, y_s = lon - d_ns * J[0, 1] / c, lat - d_ns * J[1, 1]
    if wrap_e:
        assert x_e > 180.0
        x_e -= 360.0
    v = (x_e + shift, y_e, x_w + shift, y_w, x_n + shift, y_n, x_s + shift, y_s)
    return Cell(name, cls, lat, lon, d_ns, d_ew, v, ratio, beta)


def cells(dtype):
    """The designed cells of a dtype, in table order."""
    dtype = np.dtype(dtype)
    out = []
    for sname, seed in SEEDS.items():
        pole = abs(seed[0]) > 89
        d_ns, d_ew = OFFSETS[dtype].get(sname, (D0, D0))
        for i, ratio in enumerate(RATIOS):
            if dtype == np.float32 and ratio == 1e6:
                continue                                 # does not survive there (the docstring's generic row)
            if dtype == np.float32 and pole and ratio == 1e3:
                ratio = 30.0
            for j, beta in enumerate(BETAS):
                J = jacobian(0.4 + 0.9 * (i + 3 * j), beta, ratio, reflect=(i + j) % 2 == 1)
                out.append(_designed(f"generic_{sname}_r{ratio:g}_b{j}", "generic", seed, d_ns, d_ew, J, ratio, beta))
    for sname in ("mid", "n60", "s85"):
        for i, ratio in enumerate((1.0, 1.0 + 1e-9, 1.0 + 1e-4)):
            for j, beta in enumerate((0.3, 1.2)):
                J = jacobian(0.7 + i + 2 * j, beta, ratio, reflect=(i + j) % 2 == 1)
                out.append(_designed(f"near_isotropic_{sname}_{i}_b{j}", "near_isotropic", SEEDS[sname],
                                     *OFFSETS[dtype].get(sname, (D0, D0)), J, ratio, beta))
    out.append(_designed("isotropic_exact", "isotropic_exact", SEEDS["eq"], D0, D0, np.eye(2), 1.0, None))
    Z = np.zeros((2, 2))
    for sname, seed in SEEDS.items():
        out.append(_designed(f"collapsed_{sname}", "collapsed", seed, *OFFSETS[dtype].get(sname, (D0, D0)), Z))
    for sname in ("eq", "mid", "n60", "s85"):
        d_ns, d_ew = OFFSETS[dtype].get(sname, (D0, D0))
        for j, beta in enumerate((0.3, -1.2)):
            J = jacobian(0.5 + j, beta, 1.5, reflect=j == 1)
            out.append(_designed(f"rank_one_ew_{sname}_{j}", "rank_one_ew", SEEDS[sname], d_ns, d_ew, J * np.array([0.0, 1.0])))
            out.append(_designed(f"rank_one_ns_{sname}_{j}", "rank_one_ns", SEEDS[sname], d_ns, d_ew, J * np.array([1.0, 0.0])))
    seam = (60.0, 179.95)
    Js = 5.0 * jacobian(0.2, 0.3, 1.5)                  # x_e = 179.95 + 0.05 * 4.9 = 180.2 -> -179.8
    out.append(_designed("seam_wrapped", "seam", seam, D0, D0, Js, wrap_e=True))
    out.append(_designed("seam_unwrapped", "seam", seam, D0, D0, Js))
    out.append(_designed("seam_plus3960", "seam", seam, D0, D0, Js, shift=3960.0))
    out.append(_designed("seam_plus3420", "seam", seam, D0, D0, Js, shift=3420.0))
    for wn in (30.0, 50.0, 89.0):                        # latitude pairs at the equator: y_n, y_s = +-wn
        for we in (30.0, 50.0, 89.0):
            out.append(_designed(f"wide_ns{wn:g}_ew{we:g}", "wide", SEEDS["eq"], wn, we, np.eye(2)))
    for we in (30.0, 50.0, 89.0):                        # longitude pairs alone, off the equator, a sheared J
        out.append(_designed(f"wide_mid_ew{we:g}", "wide", SEEDS["mid"], D0, we, np.array([[1.0, 0.4], [0.0, 0.8]])))
    dt = D_TINY[dtype]
    for sname in ("eq", "mid", "n60", "s85"):
        for j, (ratio, beta) in enumerate(((1.5, 0.3), (1e3, -1.2), (1.5, np.pi / 2))):
            J = jacobian(0.9 + j, beta, ratio, reflect=j == 2)
            out.append(_designed(f"tiny_{sname}_{j}", "tiny", SEEDS[sname], dt, dt, J, ratio, beta))
    return out


_TABLES = {}


def table(dtype) -> Table:
    """The plane of a dtype: cells laid out as the module docstring says, the planes rounded to the dtype."""
    dtype = np.dtype(dtype)
    if dtype in _TABLES:
        return _TABLES[dtype]
    cs = cells(dtype)
    rows, groups = [], {}
    for c in cs:
        if (c.lat, c.d_ns) not in rows:
            rows.append((c.lat, c.d_ns))
    for key in rows:
        for d_ew in sorted({c.d_ew for c in cs}):
            n = sum(1 for c in cs if (c.lat, c.d_ns) == key and c.d_ew == d_ew)
            groups[d_ew] = max(groups.get(d_ew, 0), n)
    col0, start = {}, 0
    for d_ew in sorted(groups):
        col0[d_ew] = start
        start += groups[d_ew]
    ny, nx = len(rows), start
    sep_lon = np.concatenate([np.full(groups[d], 2 * d) for d in sorted(groups)])
    seed_lat, sep_lat = np.array([r[0] for r in rows]), np.array([2 * r[1] for r in rows])
    vals = np.empty((8, ny, nx))
    cls = np.full((ny, nx), "collapsed", dtype=object)
    names = np.full((ny, nx), "", dtype=object)
    for r, (lat, _) in enumerate(rows):                  # every slot starts as a collapsed cell at the row's seed, longitude 0
        vals[0::2, r, :], vals[1::2, r, :] = 0.0, lat
        names[r, :] = [f"fill_{r}_{c}" for c in range(nx)]
    used, index = {}, {}
    for c in cs:
        r = rows.index((c.lat, c.d_ns))
        k = used.get((r, c.d_ew), 0)
        used[(r, c.d_ew)] = k + 1
        col = col0[c.d_ew] + k
        vals[:, r, col], cls[r, col], names[r, col] = c.values, c.cls, c.name
        index[c.name] = (r, col)
    planes = {k: np.ascontiguousarray(vals[i].astype(dtype)) for i, k in enumerate(AG.PLANES)}
    t = Table(dtype, cs, index, planes, seed_lat.astype(dtype), sep_lat.astype(dtype), sep_lon.astype(dtype), cls, names)
    _TABLES[dtype] = t
    return t


def judged_class(cls):
    """The class a cell's errors are measured in: ``isotropic_exact`` is one cell, and the largest difference "on a class" of one
    cell is that cell's luck (0.3 ulp of s1 in float64), so it shares ``near_isotropic``'s E, in both dtypes; its exact rules are
    asserted on it alone."""
    cls = np.asarray(cls, dtype=object).copy()
    cls[cls == "isotropic_exact"] = "near_isotropic"
    return cls


def poisons(t: Table):
    """The ``nonfinite`` runs: ``(label, plane name or "sep_lat" / "sep_lon", (row, col), value)``; row or col is None for a
    separation.  The poisoned cells are generic cells spread over the rows; the separations a row and a column with cells of
    several classes."""
    gen = [t.index[c.name] for c in t.cells if c.cls == "generic"]
    out = []
    for i, k in enumerate(AG.PLANES):
        out.append((f"nan_{k}", k, gen[(11 * i + 2) % len(gen)], np.nan))
    out.append(("posinf_x_w", "x_w", gen[5], np.inf))
    out.append(("neginf_y_n", "y_n", gen[len(gen) - 3], -np.inf))
    out.append(("nan_sep_lat", "sep_lat", (t.index["seam_wrapped"][0], None), np.nan))
    out.append(("nan_sep_lon", "sep_lon", (None, 3), np.nan))
    return out


# ------------------------------------------------------------------ the judge
def hestenes(d, layout="physical") -> dict:
    """sigma (in ``layout``), s1, s2, e_lon, e_lat and gap = 1 - (s2 / s1)^2 of the six derivatives, in longdouble, by one
    Hestenes rotation of two vectors: the columns (a, c, e), (b, d, f) of F, and for the reference layout's sigma the rows
    (a, b, c), (d, e, f) of the reference's reshape."""
    L = np.longdouble
    a, b, c, dd, e, f = (np.asarray(v).astype(L) for v in d)

    def rotate(u, v):
        with np.errstate(invalid="ignore"):
            p, q, r = sum(x * x for x in u), sum(x * x for x in v), sum(x * y for x, y in zip(u, v))
            th = L(0.5) * np.arctan2(L(2) * r, p - q)
            cs, sn = np.cos(th), np.sin(th)
            big = np.sqrt(sum((cs * x + sn * y) ** 2 for x, y in zip(u, v)))
            small = np.sqrt(sum((cs * y - sn * x) ** 2 for x, y in zip(u, v)))
        return big, small, cs, sn
    s1, s2, ex, ey = rotate((a, c, e), (b, dd, f))
    flip = (ex < 0) | ((ex == 0) & (ey < 0))
    ex, ey = np.where(flip, -ex, ex), np.where(flip, -ey, ey)
    sigma = s1 if layout == "physical" else rotate((a, b, c), (dd, e, f))[0]
    with np.errstate(invalid="ignore", divide="ignore"):
        gap = np.where(s1 > 0, 1 - (s2 / s1) ** 2, L(0))
    return dict(sigma=sigma, s1=s1, s2=s2, e_lon=ex, e_lat=ey, gap=gap)


PI_MINUS_PI64 = np.longdouble("1.224646799147353177226065928e-16")        # pi - the float64 pi, to longdouble's precision


def sincos_deg(deg):
    """sin and cos of ``deg k``, k = (float64 pi) / 180, in longdouble to a few eps *relative*, zeros' neighbourhoods included.
    ``deg`` (float32 / float64 values, or exact sums and differences of two) = 90 m + rem exactly, |rem| <= 45, and 90 k is pi/2
    less half of PI_MINUS_PI64: the angle is m pi/2 + (rem k - m (pi - pi64) / 2), the bracket small and relatively exact."""
    L = np.longdouble
    deg = np.asarray(deg, dtype=L)
    with np.errstate(invalid="ignore"):
        m = np.rint(deg / L(90))
        phi = (deg - L(90) * m) * (L(np.pi) / L(180)) - m * (PI_MINUS_PI64 / L(2))
        s, c = np.sin(phi), np.cos(phi)
        quad = np.mod(m, 4)
    sn = np.where(quad == 0, s, np.where(quad == 1, c, np.where(quad == 2, -s, -c)))
    cs = np.where(quad == 0, c, np.where(quad == 1, -s, np.where(quad == 2, -c, s)))
    return np.where(np.isfinite(deg), sn, L(np.nan)), np.where(np.isfinite(deg), cs, L(np.nan))


def derivatives(planes, seed_lat, sep_lat, sep_lon):
    """(dXdx, dXdy, dYdx, dYdy, dZdx, dZdy) of the eight planes in longdouble: the half-angle chords of csrc/aux_gradient.hip's
    header over the metric, the angles reduced in degrees (the half-sums and half-differences of two float64 are exact in
    longdouble's 64 bits)."""
    L = np.longdouble
    p = {k: np.asarray(planes[k]).astype(L) for k in AG.PLANES}
    seed_lat, sep_lat, sep_lon = (np.asarray(a).astype(L) for a in (seed_lat, sep_lat, sep_lon))
    k, R = L(np.pi) / L(180), L(AG.R_EARTH)

    def chord(xp, yp, xm, ym):
        sa, ca = sincos_deg((yp + ym) * L(0.5) - L(90))
        sda, cda = sincos_deg((yp - ym) * L(0.5))
        sl, cl = sincos_deg((xp + xm) * L(0.5))
        sdl, cdl = sincos_deg((xp - xm) * L(0.5))
        A, B = ca * sda, sa * cda
        return 2 * R * (A * cl * cdl - B * sl * sdl), 2 * R * (A * sl * cdl + B * cl * sdl), -2 * R * sa * sda
    with np.errstate(invalid="ignore"):
        ex, ey, ez = chord(p["x_e"], p["y_e"], p["x_w"], p["y_w"])
        nx_, ny_, nz_ = chord(p["x_n"], p["y_n"], p["x_s"], p["y_s"])
        dx = (k * sep_lon[None, :] * R) * sincos_deg(seed_lat)[1][:, None]
        dy = (k * sep_lat * R)[:, None]
        return ex / dx, nx_ / dy, ey / dx, ny_ / dy, ez / dx, nz_ / dy


def judge(planes, seed_lat, sep_lat, sep_lon, layout="physical") -> dict:
    return hestenes(derivatives(planes, seed_lat, sep_lat, sep_lon), layout)


def sine(ex, ey, jx, jy):
    """|sin| of the angle between the unit vectors (ex, ey) and (jx, jy), in longdouble."""
    L = np.longdouble
    return np.abs(np.asarray(ex).astype(L) * np.asarray(jy).astype(L) - np.asarray(ey).astype(L) * np.asarray(jx).astype(L))


def residual(d, ex, ey, s1):
    """|| C e - s1^2 e || with C = F^T F of the six derivatives ``d``, in longdouble."""
    L = np.longdouble
    a, b, c, dd, e, f = (np.asarray(v).astype(L) for v in d)
    ex, ey, lam = np.asarray(ex).astype(L), np.asarray(ey).astype(L), np.asarray(s1).astype(L) ** 2
    p, q, r = a * a + c * c + e * e, b * b + dd * dd + f * f, a * b + c * dd + e * f
    return np.hypot(p * ex + r * ey - lam * ex, r * ex + q * ey - lam * ey)


def sign_convention_holds(ex, ey):
    return bool(np.all((ex > 0) | ((ex == 0) & (ey > 0))))


def error_measure(in_dtype, judged, dtype, scale) -> float:
    """tests/lavd.py's rule: 8 x the largest difference between the restatement in the kernel's dtype and the judge on the same
    inputs; 4 eps x the scale where that difference is 0."""
    from tests.lavd import error_measure as E
    return E(in_dtype, judged, dtype, scale)


# ------------------------------------------------------------------ the fixture
MP_KEYS = ("s1", "s2", "e_lon", "e_lat", "sigma_reference")


def load_mp(dtype) -> dict:
    """The 50-digit values of tests/golden/jacobians_mp.npz for a dtype's plane, hi + lo summed in longdouble."""
    z = np.load(GOLD)
    tag = "f32" if np.dtype(dtype) == np.float32 else "f64"
    return {k: z[f"{tag}_{k}_hi"].astype(np.longdouble) + z[f"{tag}_{k}_lo"].astype(np.longdouble) for k in MP_KEYS}


# ------------------------------------------------------------------ the stencil carriers' fields
def stencil_grid(dtype=np.float64):
    """The global 21 x 64 seed grid of the stencil carriers: latitudes +-80, longitudes at 360 / 64 from -180."""
    lat = np.linspace(-80.0, 80.0, 21).astype(dtype)
    lon = (-180.0 + 360.0 / 64 * np.arange(64)).astype(dtype)
    return lat, lon


def stencil_field(name, dtype=np.float64):
    """(x_dep, y_dep) of ``collapsed`` (every parcel at (7, 3)), ``meridional`` (x_dep = 7, y_dep = seed latitude) or ``zonal``
    (x_dep = seed longitude, y_dep = 3)."""
    lat, lon = stencil_grid(dtype)
    ones = np.ones((lat.size, lon.size), dtype=dtype)
    x = ones * lon[None, :] if name == "zonal" else ones * dtype(7)
    y = ones * lat[:, None] if name == "meridional" else ones * dtype(3)
    assert name in ("collapsed", "meridional", "zonal")
    return np.ascontiguousarray(x), np.ascontiguousarray(y)
