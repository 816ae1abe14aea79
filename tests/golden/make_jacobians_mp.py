"""Write ``tests/golden/jacobians_mp.npz``: both stretch factors, the stretching direction and the reference layout's sigma of
every cell of the case planes of tests/jacobians.py, computed with mpmath at 50 significant digits.

    python tests/golden/make_jacobians_mp.py

Run on the planes as the kernels are given them: rounded to float32 (keys ``f32_*``) and to float64 (``f64_*``), with the
rounded ``seed_lat``, ``sep_lat`` and ``sep_lon``.  Written from the definitions of include/lcs_hip.h and csrc/aux_gradient.hip's
header, not from any float code:

* a departure point (x, y) in degrees lies at X = R sin a cos l, Y = R sin a sin l, Z = R cos a with a = (y - 90) k, l = x k,
  k = pi / 180 with the float64 pi (the kernels' and the tests' constant: every arithmetic of the project forms k from it, so
  it is part of the definition, not an error);
* the six derivatives are the plain differences (P_e - P_w) / (k sep_lon R cos(k seed_lat)) and (P_n - P_s) / (k sep_lat R) --
  at 50 digits the difference of two points a nanodegree apart keeps 35 of them, so no half-angle form is needed;
* s1 >= s2 are the square roots of the eigenvalues of F^T F = [[p, r], [r, q]]: lam1 = ((p + q) + sqrt((p - q)^2 + 4 r^2)) / 2,
  s2 = sqrt(p q - r^2) / s1 (0 where s1 is 0; at 50 digits the cancellation of a ratio of 1e6 costs 12 of them);
* the direction is (cos t, sin t), t = atan2(2 r, p - q) / 2, with e_lon > 0, or e_lon == 0 and e_lat > 0; (1, 0) where p == q
  and r == 0;
* sigma of the reference layout is sqrt(lam1) of the Gram matrix of the rows (a, b, c), (d, e, f).

Each value is stored as a float64 pair ``_hi`` + ``_lo`` (106 bits: more than a longdouble holds).  The archive is written with
fixed timestamps and without compression: two runs give the same bytes.  A few seconds on one core.
"""
import io
import os
import sys
import zipfile

import numpy as np
from mpmath import mp, mpf

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import jacobians as JC            # noqa: E402
from tests.aux_gradient import PLANES, R_EARTH  # noqa: E402

DIGITS = 50


def cell(v, seed_lat, sep_lat, sep_lon):
    """(s1, s2, e_lon, e_lat, sigma_reference) of one cell; ``v`` the eight plane values in PLANES' order, everything mpf."""
    k = mpf(float(np.pi)) / 180
    R = mpf(R_EARTH)

    def xyz(x, y):
        a, l = (y - 90) * k, x * k
        return R * mp.sin(a) * mp.cos(l), R * mp.sin(a) * mp.sin(l), R * mp.cos(a)
    e, w, n, s = xyz(v[0], v[1]), xyz(v[2], v[3]), xyz(v[4], v[5]), xyz(v[6], v[7])
    dx, dy = k * sep_lon * R * mp.cos(seed_lat * k), k * sep_lat * R
    a, c, ee = ((e[i] - w[i]) / dx for i in range(3))
    b, d, f = ((n[i] - s[i]) / dy for i in range(3))

    def eig(u, v_):
        p, q, r = sum(x * x for x in u), sum(x * x for x in v_), sum(x * y for x, y in zip(u, v_))
        lam = ((p + q) + mp.sqrt((p - q) ** 2 + 4 * r * r)) / 2
        return p, q, r, mp.sqrt(lam)
    p, q, r, s1 = eig((a, c, ee), (b, d, f))
    det = p * q - r * r
    s2 = mpf(0) if s1 == 0 else mp.sqrt(det if det > 0 else mpf(0)) / s1
    if p == q and r == 0:
        ex, ey = mpf(1), mpf(0)
    else:
        t = mp.atan2(2 * r, p - q) / 2
        ex, ey = mp.cos(t), mp.sin(t)
        if p < q and r == 0:
            ex, ey = mpf(0), mpf(1)             # t = +-pi / 2 exactly: no cos(pi / 2) left over from the 50-digit pi
        if ex < 0 or (ex == 0 and ey < 0):
            ex, ey = -ex, -ey
    return s1, s2, ex, ey, eig((a, b, c), (d, ee, f))[3]


def hi_lo(x):
    hi = float(x)
    return hi, float(x - mpf(hi))


def write_npz(path, arrays):
    """An .npz numpy.load reads, with nothing in it that changes from run to run."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), version=(1, 0))
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


if __name__ == "__main__":
    mp.dps = DIGITS
    arrays = {}
    for tag, dtype in (("f32", np.float32), ("f64", np.float64)):
        t = JC.table(dtype)
        ny, nx = t.cls.shape
        out = np.zeros((len(JC.MP_KEYS), 2, ny, nx))
        for r in range(ny):
            for c in range(nx):
                v = [mpf(float(t.planes[k][r, c])) for k in PLANES]
                vals = cell(v, mpf(float(t.seed_lat[r])), mpf(float(t.sep_lat[r])), mpf(float(t.sep_lon[c])))
                for i, x in enumerate(vals):
                    out[i, :, r, c] = hi_lo(x)
        for i, key in enumerate(JC.MP_KEYS):
            arrays[f"{tag}_{key}_hi"], arrays[f"{tag}_{key}_lo"] = out[i, 0], out[i, 1]
        print(tag, (ny, nx), flush=True)
    write_npz(JC.GOLD, arrays)
    print(JC.GOLD, os.path.getsize(JC.GOLD), "bytes")
