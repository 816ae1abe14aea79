"""Write ``tests/golden/trunc_operators_mp.npz``: the per-zonal-wavenumber truncation operators ``P[m]`` (row 0 = north) of
``lc_spectral_truncate`` computed with mpmath at 40 significant digits and stored rounded to float64.

    python tests/golden/make_trunc_operators_mp.py

Written from the published statement (oracle/preprocess_oracle.py's docstring; Swarztrauber 1979), not from the float64 code:

* regular grid, theta_i = i pi / N, N = nlat - 1.  A zonal Fourier coefficient g of wavenumber m, known on the rows, is
  interpolated by a cosine series (m even: g(theta) = sum''_{k=0..N} b_k cos k theta, b_k = (2/N) sum''_i g_i cos(k i pi / N),
  the double prime halving the first and the last term) or a sine series (m odd: g(theta) = sum_{k=1..N-1} b_k sin k theta,
  b_k = (2/N) sum_{i=1..N-1} g_i sin(k i pi / N)); a^m_n = integral_0^pi g(theta) Pbar^m_n(cos theta) sin(theta) dtheta for
  m <= n <= T; the result is sum_n a^m_n Pbar^m_n(cos theta_i).  P[m][i][j] is the result at row i for g = e_j.
* Gaussian grid of nlat rows, x_i the roots of P_nlat (north first), w_i its weights:
  P[m][i][j] = sum_{n=m..T} Pbar^m_n(x_i) Pbar^m_n(x_j) w_j.

The integrals are taken by Gauss-Legendre quadrature in x = cos(theta), with nodes Newton-refined in the working precision.
cos(k theta) Pbar^m_n (m even) and sin(k theta) Pbar^m_n (m odd: sin(theta)^(m+1) U_{k-1}(x) q_{n-m}(x), m + 1 even) are
polynomials in x of degree k + n <= N + T, so the rule with Q = N + T + 2 nodes (exact to degree 2 Q - 1) has no quadrature
error at all; what is left is 40-digit rounding.  Pbar^m_n comes from the three-term recurrence in mpf and is checked below
against the closed form (Rodrigues' formula differentiated term by term) before anything is written.

The archive is written with fixed timestamps and without compression: two runs give the same bytes.  About a minute on one core.
"""
import io
import os
import zipfile

import numpy as np
from mpmath import mp, mpf

HERE = os.path.dirname(os.path.abspath(__file__))
DIGITS = 40
REGULAR = ((5, 4), (9, 8), (17, 7), (33, 16))       # (nlat, T)
GAUSSIAN = ((8, 7), (16, 5), (32, 16))


def pbar(m, nmax, xs):
    """Pbar^m_n(x), n = m..nmax, with integral_{-1}^{1} Pbar^2 dx = 1: out[n - m][q], mpf."""
    out = [[None] * len(xs) for _ in range(nmax - m + 1)]
    for q, x in enumerate(xs):
        s = mp.sqrt(1 - x * x) if abs(x) < 1 else mpf(0)
        p = mp.sqrt(mpf(1) / 2)
        for k in range(1, m + 1):
            p = -mp.sqrt(mpf(2 * k + 1) / (2 * k)) * s * p
        out[0][q] = p
        if nmax > m:
            out[1][q] = mp.sqrt(mpf(2 * m + 3)) * x * p
        for n in range(m + 2, nmax + 1):
            a = mp.sqrt(mpf(4 * n * n - 1) / (n * n - m * m))
            b = mp.sqrt(mpf((n - 1) ** 2 - m * m) / (4 * (n - 1) ** 2 - 1))
            out[n - m][q] = a * (x * out[n - m - 1][q] - b * out[n - m - 2][q])
    return out


def gauss_legendre(n):
    """Roots of P_n, descending (north first), and weights 2 / ((1 - x^2) P_n'(x)^2), to the working precision."""
    xs, ws = [], []
    for i in range(n):
        x = mp.cos(mp.pi * (i + mpf(3) / 4) / (n + mpf(1) / 2))
        for _ in range(200):
            p1, p2 = mpf(1), mpf(0)
            for j in range(1, n + 1):
                p1, p2 = ((2 * j - 1) * x * p1 - (j - 1) * p2) / j, p1
            dp = n * (x * p1 - p2) / (x * x - 1)
            dx = p1 / dp
            x -= dx
            if abs(dx) < mpf(10) ** (-(DIGITS - 3)):
                break
        else:
            raise RuntimeError("Newton did not converge")
        p1, p2 = mpf(1), mpf(0)
        for j in range(1, n + 1):
            p1, p2 = ((2 * j - 1) * x * p1 - (j - 1) * p2) / j, p1
        dp = n * (x * p1 - p2) / (x * x - 1)
        xs.append(x)
        ws.append(2 / ((1 - x * x) * dp * dp))
    assert all(a > b for a, b in zip(xs, xs[1:])) and abs(sum(ws) - 2) < mpf(10) ** (-(DIGITS - 5))
    return xs, ws


def regular(nlat, T):
    """P[m][i][j] on the equally spaced grid."""
    N = nlat - 1
    xg = [mp.cos(i * mp.pi / N) for i in range(nlat)]
    xg[0], xg[N] = mpf(1), mpf(-1)
    xq, wq = gauss_legendre(N + T + 2)
    tq = [mp.acos(x) for x in xq]
    ops = []
    for m in range(T + 1):
        even = m % 2 == 0
        ks = range(0, N + 1) if even else range(1, N)
        Sg, Sq = pbar(m, T, xg), pbar(m, T, xq)
        Pm = [[mpf(0)] * nlat for _ in range(nlat)]
        for k in ks:
            basis = [mp.cos(k * t) if even else mp.sin(k * t) for t in tq]
            # the interpolant's k-th coefficient as a function of the row values
            bk = [mpf(2) / N * (mp.cos(mpf(k * j) * mp.pi / N) if even else mp.sin(mpf(k * j) * mp.pi / N)) for j in range(nlat)]
            if even:
                bk[0] /= 2
                bk[N] /= 2
                if k == 0 or k == N:
                    bk = [b / 2 for b in bk]
            for a in range(T - m + 1):
                integral = sum(Sq[a][q] * wq[q] * basis[q] for q in range(len(xq)))
                for i in range(nlat):
                    c = Sg[a][i] * integral
                    row = Pm[i]
                    for j in range(nlat):
                        row[j] += c * bk[j]
        ops.append(Pm)
    return ops


def gaussian(nlat, T):
    xs, ws = gauss_legendre(nlat)
    ops = []
    for m in range(T + 1):
        S = pbar(m, T, xs)
        ops.append([[sum(S[a][i] * S[a][j] for a in range(T - m + 1)) * ws[j] for j in range(nlat)] for i in range(nlat)])
    return ops


def to_float64(ops):
    return np.array([[[float(v) for v in row] for row in Pm] for Pm in ops], dtype=np.float64)


def check_pbar_against_rodrigues():
    """The recurrence against the closed form: P^m_n = (-1)^m (1 - x^2)^(m/2) d^m/dx^m P_n with
    P_n = 2^-n sum_k (-1)^k C(n, k) C(2n - 2k, n) x^(n - 2k), normalised by sqrt((2n + 1)/2 (n - m)!/(n + m)!)."""
    xs = [mpf(-9) / 10, mpf(-1) / 3, mpf(0), mpf(1) / 7, mpf(99) / 100]
    worst = mpf(0)
    for m in (0, 1, 2, 5, 16):
        got = pbar(m, 16, xs)
        for n in range(m, 17):
            norm = mp.sqrt(mpf(2 * n + 1) / 2 * mp.factorial(n - m) / mp.factorial(n + m))
            for q, x in enumerate(xs):
                d = sum((-1) ** k * mp.binomial(n, k) * mp.binomial(2 * n - 2 * k, n) * mp.factorial(n - 2 * k) / mp.factorial(n - 2 * k - m)
                        * x ** (n - 2 * k - m) for k in range((n - m) // 2 + 1)) / mpf(2) ** n
                worst = max(worst, abs(got[n - m][q] - norm * (-1) ** m * (1 - x * x) ** (mpf(m) / 2) * d))
    assert worst < mpf(10) ** (-(DIGITS - 8)), worst
    return worst


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
    print("Pbar recurrence against the closed form: max difference", mp.nstr(check_pbar_against_rodrigues(), 3))
    arrays = {}
    for nlat, T in REGULAR:
        arrays[f"regular_{nlat}_{T}"] = to_float64(regular(nlat, T))
        print("regular", nlat, T, flush=True)
    for nlat, T in GAUSSIAN:
        arrays[f"gaussian_{nlat}_{T}"] = to_float64(gaussian(nlat, T))
        print("gaussian", nlat, T, flush=True)
    out = os.path.join(HERE, "trunc_operators_mp.npz")
    write_npz(out, arrays)
    print(out, os.path.getsize(out), "bytes")
