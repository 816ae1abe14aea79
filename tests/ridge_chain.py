"""Case tables of the ridge chain: the three kernels that turn an FTLE field into ridges, and the drop-in that strings them.

Plain data and numpy input builders, imported by ``test_ridge_chain.py`` (completeness and the cases' own promises, no GPU)
and ``test_ridge_chain_gpu.py`` (every case on the GPU against scipy, numpy and the oracle).  No torch, no engine.

- ``KERNELS``: kernel name -> source file, the C entry point that launches it, the ``Engine`` method, its case table here.
- ``GAUSS_CASES``: ``(ny, nx, sigma, dtype)`` for ``lc_gaussian_filter``; ``GAUSS_NONFINITE`` the same with a NaN at an interior
  node and an inf at a corner; ``GAUSS_REFUSALS`` the sigmas the entry point refuses before any launch.
- ``DERIV_CASES``: ``(ny, nx)`` for ``lc_fourth_order_derivative``, each run for both ``dim``, both ``isglobal``, both dtypes;
  ``DERIV_NONFINITE`` the grid that also runs with a NaN and an inf; ``DERIV_REFUSALS`` ``(ny, nx, dim)``.
- ``RIDGE_N``: matrix counts for ``lc_ridge_classify``; ``ridge_case`` builds the inputs: ``ridge_inputs`` rows, then the
  ``SPECIAL_ROWS`` and the gradient specials at the tail (past the grid cap at the largest count).
- ``CHAIN_CASES``: inputs of ``find_ridges_spherical_hessian``; ``chain_input`` builds one.

Every builder is seeded and returns fresh arrays; the references are computed by the tests, once per case.
"""
import numpy as np

KERNELS = {
    "gauss_kernel": dict(file="api.hip", entry="lc_gaussian_filter", engine="gaussian_filter", cases="GAUSS_CASES"),
    "index_derivative_kernel": dict(file="sigma.hip", entry="lc_fourth_order_derivative", engine="index_derivative", cases="DERIV_CASES"),
    "ridge_kernel": dict(file="ridges.hip", entry="lc_ridge_classify", engine="ridge_classify", cases="RIDGE_N"),
}
# the files whose every __global__ kernel must be in KERNELS, and the one kernel of sigma.hip that belongs to the chain (its
# other kernels are the sigma dispatcher's: tests/kernel_routes.py)
WHOLE_FILES = ("api.hip", "ridges.hip")
SHARED_FILES = {"sigma.hip": ("index_derivative_kernel",)}

BLOCK = 256

# ------------------------------------------------------------------ lc_gaussian_filter
_GAUSS_SHAPES = (
    (3, 7, 2.0),          # radius 8 > 2 n on both axes: reflect_index folds several times
    (2, 5, 3.0),          # radius 12
    (1, 9, 1.0),          # an axis of one node (reflect_index's n == 1)
    (9, 1, 1.0),
    (37, 53, 0.1),        # radius 0: the input, bit for bit
    (37, 53, 0.624),      # int(4 sigma + 0.5): 2.996 -> 2
    (37, 53, 0.625),      # 3.0 -> 3
    (5, 5, 64.0),         # radius 256 = GAUSS_MAX_RADIUS, accepted; 51 folds
    (300, 7, 64.0),
    (1030, 1021, 2.0),    # 1,051,630 elements: past 4096 blocks of 256, both axes ragged against 256
)
GAUSS_CASES = tuple(s + ("float64",) for s in _GAUSS_SHAPES) + tuple(_GAUSS_SHAPES[i] + ("float32",) for i in (0, 2, 5, 9))
GAUSS_NONFINITE = ((37, 53, 2.0, "float64"), (37, 53, 1.5, "float32"))
GAUSS_REFUSALS = (64.2, 0.0, -1.0)      # radius 257; scipy would return the input; scipy would raise


def gauss_radius(sigma):
    return int(4.0 * sigma + 0.5)        # scipy: int(truncate * sd + 0.5)


def gauss_input(ny, nx, dtype, nonfinite=False):
    a = np.random.default_rng([7, ny, nx]).standard_normal((ny, nx)).astype(dtype)
    if nonfinite:
        a[ny // 2, nx // 2] = np.nan
        a[0, nx - 1] = np.inf
    return a


def gauss_bound(a, sigma):
    """max |device - scipy| over the finite reference values.

    float64: (6 r + 12) eps64 max|a| -- the weights (a sequential normalising sum against numpy's pairwise one, exp, the
    divide) and r + 1 accumulated products per pass over two passes.  float32: two float32 stores of half an ulp each; the
    double accumulation between them is the float64 bound, far below."""
    scale = float(np.abs(a[np.isfinite(a)]).max())
    if a.dtype == np.float32:
        return 2.0 * float(np.finfo(np.float32).eps) * scale
    return (6 * gauss_radius(sigma) + 12) * float(np.finfo(np.float64).eps) * scale


def reflect_index(i, n):
    """api.hip's reflect_index, restated: scipy 'reflect' (d c b a | a b c d | d c b a) at any distance."""
    i = np.asarray(i)
    if n == 1:
        return np.zeros_like(i)
    period = 2 * n
    i = np.mod(i, period)                # (C's % and the `i < 0` correction)
    return np.where(i < n, i, period - 1 - i)


def reflect_single_fold(i, n):
    """What reflect_index would be with one fold and nothing else: right up to a distance of n, outside the array beyond
    (gauss_restated reads NaN there, where the device would read whatever lies next to the array)."""
    i = np.asarray(i)
    i = np.where(i < 0, -1 - i, i)
    return np.where(i >= n, 2 * n - 1 - i, i)


def _take(src, idx, axis):
    inside = (idx >= 0) & (idx < src.shape[axis])
    out = np.take(src, np.where(inside, idx, 0), axis=axis)
    out[(slice(None),) * axis + (~inside,)] = np.nan
    return out


def gauss_restated(a, sigma, reflect=reflect_index):
    """lc_gaussian_filter on the host: the weights as the entry point builds them, gauss_kernel's summation order."""
    r = gauss_radius(sigma)
    phi = [np.exp(-0.5 / (sigma * sigma) * float(k) * k) for k in range(-r, r + 1)]
    total = 0.0
    for p in phi:
        total += p
    w = [phi[k + r] / total for k in range(r + 1)]
    out = a
    for axis in (0, 1):
        n = out.shape[axis]
        idx = np.arange(n)
        src = out.astype(np.float64)
        acc = src * w[0]
        for j in range(r, 0, -1):
            acc = acc + (_take(src, reflect(idx - j, n), axis) + _take(src, reflect(idx + j, n), axis)) * w[j]
        out = acc.astype(a.dtype)
    return out


# ------------------------------------------------------------------ lc_fourth_order_derivative
DERIV_CASES = ((5, 5), (5, 6), (6, 5), (29, 40), (257, 255), (1449, 1448))    # the last: 2,098,152 elements, past 8192 x 256
DERIV_NONFINITE = (29, 40)             # NaN at (2, 2), inf at (0, nx - 1), once per (dim, isglobal)
DERIV_REFUSALS = ((4, 9, 0), (9, 4, 0), (9, 9, 2))
DERIV_DTYPES = ("float32", "float64")


def deriv_input(ny, nx, dtype, nonfinite=False):
    """1e6 * standard normal, cast to float32 and then to the case's dtype: float32 differences that round."""
    a = (1e6 * np.random.default_rng([12, ny, nx]).standard_normal((ny, nx))).astype(np.float32).astype(dtype)
    if nonfinite:
        a[2, 2] = np.nan
        a[0, nx - 1] = np.inf
    return a


# ------------------------------------------------------------------ lc_ridge_classify
def ridge_inputs(n=120000, seed=0):
    rng = np.random.default_rng(seed)
    a = rng.standard_normal(n) * 10.0 ** rng.integers(-20, 3, n)
    b = rng.standard_normal(n) * 10.0 ** rng.integers(-22, 3, n)
    d = rng.standard_normal(n) * 10.0 ** rng.integers(-20, 3, n)
    a[:100] = d[:100]
    b[100:200] = 0
    a[200:300] = 0
    d[300:400] = -a[300:400]
    d[600:700] = 0
    a[700:800] = 0
    d[700:800] = 0
    a[2000:3000] = d[2000:3000] * (1 + 1e-16 * rng.integers(-5, 5, 1000))
    a[5000:60000] *= 1e-10      # realistic Hessian magnitudes (FTLE per metre^2)
    b[5000:60000] *= 1e-10
    d[5000:60000] *= 1e-10
    return a, b, d


ULP = float(np.finfo(np.float64).eps)


def branch_counts(a, b, d):
    """How many matrices take (dlanv2's almost-equal branch with b != 0, dlahqr's first deflation test, neither): the
    criterion of tests/test_ridges.py, more than 100 of each."""
    p, ab = 0.5 * (a - d), np.abs(b)
    with np.errstate(all="ignore"):
        z0 = (p / np.maximum(np.abs(p), ab)) * p + (ab / np.maximum(np.abs(p), ab)) * ab
    almost, defl = (z0 < 4 * ULP) & (b != 0), ab <= ULP * (np.abs(a) + np.abs(d))
    return int(almost.sum()), int(defl.sum()), int((~almost & ~defl).sum())


MAGNITUDES = (1.0, 1e-10, 1e-300)      # 1e-300: below 2^-459, where dgeev scales the matrix before it does anything else


def _special_rows():
    """(name, a, b, d): the ties, the zero matrix, the diagonal and the anti-diagonal, equal diagonals, and |b| one ulp
    either side of dlahqr's first deflation test |b| <= ulp (|a| + |d|), each with both signs of a and of b."""
    rows = [("zero", 0.0, 0.0, 0.0)]
    for m in MAGNITUDES:
        for sa in (1.0, -1.0):
            a = sa * m
            rows.append((f"a,0,a a={a:g}", a, 0.0, a))                   # w0 == w1: the first index, as np.argmin
            rows.append((f"a,0,-a a={a:g}", a, 0.0, -a))                 # |w0| == |w1|, opposite signs: first, as np.argmax(abs)
        for sb in (1.0, -1.0):
            rows.append((f"0,b,0 b={sb * m:g}", 0.0, sb * m, 0.0))       # |w0| == |w1| again, through dlanv2
        for sa in (1.0, -1.0):
            for sb in (1.0, -1.0):
                a, b = sa * m, sb * m
                rows.append((f"a,b,a a={a:g} b={b:g}", a, b, a))         # a == d, b != 0
                d = -0.5 * a
                thr = ULP * (abs(a) + abs(d))
                rows.append((f"a,b,d |b| above ulp(|a|+|d|) a={a:g} sb={sb:g}", a, sb * float(np.nextafter(thr, np.inf)), d))
                rows.append((f"a,b,d |b| below ulp(|a|+|d|) a={a:g} sb={sb:g}", a, sb * float(np.nextafter(thr, 0.0)), d))
    return tuple(rows)


SPECIAL_ROWS = _special_rows()

RIDGE_TOL = 0.3
# (name, (a, b, d), gx, gy); gx = None: chosen from numpy.linalg.eig's row so that dt is the `dt` named
GRAD_SPECIALS = (
    ("gx=inf on a zero of the row, eigmin<0", (-1.0, 0.0, -2.0), np.inf, 0.25),     # row (0, 1): 0 * inf = NaN, flagged
    ("gy=inf on a zero of the row, eigmin>0", (1.0, 0.0, 2.0), 0.25, np.inf),       # row (1, 0): NaN, but eigmin > 0
    ("gx=-inf, no zero in the row", (-2.0, 1.0, -1.0), -np.inf, 0.25),              # dt = +-inf: not a ridge
    ("gy=NaN", (-2.0, 1.0, -1.0), 0.25, np.nan),                                    # flagged
    ("dt==tol", (-2.0, 0.0, -1.0), None, 0.5),
    ("dt==nextafter(tol)", (-2.0, 0.0, -1.0), None, 0.5),
)
RIDGE_N = (257, 60000, 4096 * 256 + 257)
RIDGE_N_TOL0 = 60000        # tol = 0 is run once, at this size
RIDGE_SEEDS = {257: 5, 60000: 3, 4096 * 256 + 257: 6}
RIDGE_BORDER = 1e-12        # |(|dt| - tol)| below which the mask is not compared (tests/test_ridges.py)
BORDER_SHARE = 1e-3         # ... and the largest share of points that may lie there


def _eig_rows(a, b, d):
    w, V = np.linalg.eig(np.stack([np.stack([a, b], -1), np.stack([b, d], -1)], -2))
    n = np.arange(a.size)
    return w, V[n, np.argmin(w, axis=1), :]                                          # tools.py:107, the ROW of V


def ridge_case(n, tol=RIDGE_TOL):
    """dict(a, b, d, gx, gy, tol, special: name -> index, exact: indices whose mask is compared whatever their dt).

    Rows 0 .. n - K - 1: ridge_inputs (of at least 3000 rows: it writes rows 2000 .. 2999), standard normal gradients, the
    non-finite entries of the existing classify test at rows 10 .. 13.  The last K rows: SPECIAL_ROWS, then GRAD_SPECIALS."""
    seed = RIDGE_SEEDS[n]
    a, b, d = (v[:n].copy() for v in ridge_inputs(max(n, 3000), seed))
    rng = np.random.default_rng(seed + 1)
    gx, gy = rng.standard_normal(n), rng.standard_normal(n)
    a[10], b[11], d[12] = np.inf, np.nan, -np.inf                                    # cleaned to 0 (tools.py:92-93)
    gx[13] = np.nan                                                                  # a NaN gradient flags the point
    k = len(SPECIAL_ROWS) + len(GRAD_SPECIALS)
    assert n >= k + 100
    special, exact = {}, []
    for i, (name, sa, sb, sd) in enumerate(SPECIAL_ROWS, n - k):
        a[i], b[i], d[i] = sa, sb, sd
        special[name] = i
    for i, (name, (sa, sb, sd), sgx, sgy) in enumerate(GRAD_SPECIALS, n - len(GRAD_SPECIALS)):
        a[i], b[i], d[i], gy[i] = sa, sb, sd, sgy
        if sgx is None:
            _, row = _eig_rows(a[i:i + 1], b[i:i + 1], d[i:i + 1])
            assert row[0, 0] == 1.0 and row[0, 1] == 0.0, row                        # so that dt is gx itself
            sgx = tol if name == "dt==tol" else float(np.nextafter(tol, np.inf))
            exact.append(i)
        gx[i] = sgx
        special[name] = i
    return dict(a=a, b=b, d=d, gx=gx, gy=gy, tol=tol, special=special, exact=tuple(exact))


def ridge_reference(a, b, d, gx, gy, tol):
    """(mask, eigmin, dt, row) as tools.find_ridges_spherical_hessian computes them per point with numpy.linalg.eig."""
    ac, bc, dc = (np.where(np.isfinite(v), v, 0.0) for v in (a, b, d))
    w, row = _eig_rows(ac, bc, dc)
    with np.errstate(invalid="ignore"):
        dt = row[:, 0] * gx + row[:, 1] * gy                                         # tools.py:115
        em = w[np.arange(a.size), np.argmax(np.abs(w), axis=1)]                      # tools.py:118
        m = np.where(np.abs(dt) <= tol, dt, 0)
        m = np.where(np.abs(dt) > tol, m, 1)
        m = np.where(np.sign(em) == -1, m, 0)
    return m, em, dt, row


def borderline(dt, tol, window, exact=()):
    """Points whose mask is not compared: |dt| within `window` of tol, but for the rows built to sit there exactly."""
    with np.errstate(invalid="ignore"):
        out = np.abs(np.abs(dt) - tol) < window
    flat = out.reshape(-1)
    for i in exact:
        flat[i] = False
    return out


# ------------------------------------------------------------------ find_ridges_spherical_hessian
LL, LON_LAT = ("latitude", "longitude"), ("longitude", "latitude")
CHAIN_TOL = 0.0005e-3       # the reference's default
CHAIN_BORDER_REL = 1e-9     # |(|dt| - tol)| < 1e-9 tol is not compared (tests/test_ridges.py)
SIGMA_VARIANTS = (None, 0, 0.5, np.float64(0.5), np.float32(0.5))


def smooths(sigma):
    """The reference's rule (tools.py:74-75) with scipy's own guard: numpy.float64 is a float, numpy.float32 is not."""
    return isinstance(sigma, (float, int)) and sigma > 1e-15


def _chain_cases():
    base = dict(ny=41, nx=72, lat_desc=False, roll=0, dims=LL, sigma=0.5)
    cases = {}

    def add(name, **kw):
        for g in (True, False):
            cases[f"{name}-{'global' if g else 'regional'}"] = dict(base, isglobal=g, **kw)
    add("lat_descending", lat_desc=True)
    add("lon_rolled_17", roll=17)
    add("dims_lat_lon")
    add("dims_lon_lat_descending_rolled", dims=LON_LAT, lat_desc=True, roll=17)
    add("narrower_than_the_radius", ny=7, nx=12, sigma=3.0)
    for i, s in enumerate(SIGMA_VARIANTS):
        add(f"sigma{i}_{type(s).__name__}_{s}", sigma=s)
    return cases


CHAIN_CASES = _chain_cases()


def chain_input(case):
    """(values in the case's dims, lat, lon as stored; values (lat, lon) sorted, lat sorted, lon sorted)."""
    ny, nx = case["ny"], case["nx"]
    lat = np.linspace(-60.0, 60.0, ny)
    lon = -180.0 + (360.0 / nx) * np.arange(nx)
    LON, LAT = np.meshgrid(lon, lat)
    f = (np.exp(-((LAT - 5 - 8 * np.sin(np.deg2rad(2 * LON))) / 10.0) ** 2) * (1 + 0.2 * np.cos(np.deg2rad(3 * LON)))
         + 0.05 * np.sin(np.deg2rad(5 * LON)) * np.cos(np.deg2rad(4 * LAT)))
    v, slat, slon = f, lat, lon
    if case["lat_desc"]:
        v, slat = v[::-1], slat[::-1]
    if case["roll"]:
        v, slon = np.roll(v, case["roll"], axis=1), np.roll(slon, case["roll"])
    if case["dims"] == LON_LAT:
        v = v.T
    return np.ascontiguousarray(v), slat.copy(), slon.copy(), f, lat, lon
