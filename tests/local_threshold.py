"""TEST SUPPORT -- the host restatement of the local threshold (csrc/threshold.hip, Engine.local_threshold,
tools.threshold_local / above_local_threshold), the scipy reference, the tolerance and the cases the tests run.

- ``smooth`` / ``threshold``: numpy in the device's summation order -- per axis, latitude first: the weights of
  ``gauss_fill_weights`` (``exp(-0.5 / sigma^2 * k^2)``, summed from ``-r`` to ``r`` one by one, then divided), the sample index
  folded by scipy's 'reflect' rule (periodically along longitude with ``cyclic``) at any distance, the centre first and then
  ``acc += (lo + hi) * w[j]`` from ``j = r`` down to 1; an axis with ``sigma <= 1e-15`` is not filtered.  (The device fuses the
  multiply and the add; numpy rounds twice: the tolerance covers it.)
- ``scipy_threshold``: ``scipy.ndimage.gaussian_filter(f, sigma, mode='reflect')``, ``mode=['reflect', 'wrap']`` for cyclic,
  minus offset, plane by plane: what ``skimage.filters.threshold_local(f, block_size, offset=offset)`` documents for
  ``method='gaussian'`` with ``sigma = (block_size - 1) / 6``.
- ``atol``: ``8 (2 r + 2) 2^-53 max|f|`` -- each pass is a convex sum of ``2 r + 1`` products, there are two passes, two
  implementations, and last-bit freedom in the weights.  Derived, not measured.
- ``CASES``: the smallest shapes that cross every boundary of the kernel, stated with the tile constants below (read from
  threshold.hip by tests/test_local_threshold.py, so the table cannot drift from the kernel).
"""
from __future__ import annotations

import functools

import numpy as np

SEED = 20261019
TL_THREADS = 256      # threads of a workgroup
TL_RUN = 256          # outputs along the axis per workgroup
TL_LINES = 8          # neighbouring lines per workgroup
TL_PITCH = 768        # TL_RUN + 2 * 256: samples of one staged line at the largest radius
MAX_RADIUS = 256
SKIP_SIGMA = 1e-15
BOTH, ONLY_Y, ONLY_X = "gauss_line_kernel<0>+gauss_line_kernel<1>", "gauss_line_kernel<0>", "gauss_line_kernel<1>"


def sigma_of(block):
    """skimage: sigma = (block_size - 1) / 6 per axis; ``block`` an odd int or a (latitude, longitude) pair."""
    by, bx = (block, block) if np.ndim(block) == 0 else block
    return (by - 1) / 6.0, (bx - 1) / 6.0


def radius(sigma):
    return int(4.0 * sigma + 0.5)


def weights(sigma):
    r = radius(sigma)
    phi = [float(np.exp(np.float64(-0.5 / (sigma * sigma) * float(k) * k))) for k in range(-r, r + 1)]
    s = 0.0
    for p in phi:
        s += p
    return np.array([phi[k + r] / s for k in range(r + 1)])


def fold(q, n, periodic=False):
    """Where sample ``q`` (any integer array) of a line of ``n`` lies: scipy 'reflect' (d c b a | a b c d | d c b a) or periodic."""
    q = np.asarray(q, dtype=np.int64)
    if periodic:
        return q % n
    i = q % (2 * n)
    return np.where(i < n, i, 2 * n - 1 - i)


def smooth_axis(f, sigma, axis, periodic=False):
    """One pass over float64 ``f`` (..., ny, nx) along ``axis`` (-2 or -1), in the device's order."""
    if sigma <= SKIP_SIGMA:
        return f
    w = weights(sigma)
    n = f.shape[axis]
    at = np.arange(n)
    acc = f * w[0]
    for j in range(len(w) - 1, 0, -1):
        acc = acc + (np.take(f, fold(at - j, n, periodic), axis=axis) + np.take(f, fold(at + j, n, periodic), axis=axis)) * w[j]
    return acc


def smooth(f, sigma, cyclic=False):
    sy, sx = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (2,))
    with np.errstate(invalid="ignore"):
        return smooth_axis(smooth_axis(np.asarray(f, dtype=np.float64), float(sy), -2), float(sx), -1, cyclic)


def threshold(f, sigma, offset=0.0, cyclic=False):
    with np.errstate(invalid="ignore"):
        return smooth(f, sigma, cyclic) - np.float64(offset)


def scipy_threshold(f, sigma, offset=0.0, cyclic=False):
    from scipy import ndimage
    f = np.asarray(f, dtype=np.float64)
    sy, sx = np.broadcast_to(np.asarray(sigma, dtype=np.float64), (2,))
    planes = f.reshape((-1,) + f.shape[-2:])
    mode = ["reflect", "wrap"] if cyclic else "reflect"
    with np.errstate(invalid="ignore"):
        out = np.stack([ndimage.gaussian_filter(p, (sy, sx), mode=mode) for p in planes]) - np.float64(offset)
    return out.reshape(f.shape)


def atol(f, sigma):
    """8 (2 r + 2) 2^-53 max|f| with r the larger radius of the two axes and the maximum over the finite values."""
    f = np.asarray(f, dtype=np.float64)
    r = max(radius(float(s)) if s > SKIP_SIGMA else 0 for s in np.broadcast_to(np.asarray(sigma, dtype=np.float64), (2,)))
    return 8.0 * (2 * r + 2) * 2.0 ** -53 * float(np.abs(f[np.isfinite(f)]).max())


# ------------------------------------------------------------------ the fields
def field(shape, salt=0):
    """Smoothed noise about 1.5 with a standard deviation near 1: the look of an FTLE plane, every plane drawn on its own."""
    from scipy import ndimage
    rng = np.random.default_rng([SEED, *shape, salt])
    noise = rng.standard_normal(shape)
    planes = noise.reshape((-1,) + tuple(shape[-2:]))
    out = np.stack([ndimage.gaussian_filter(p, 1.5, mode="wrap") for p in planes]).reshape(shape)
    return 1.5 + 5.0 * out          # (white noise smoothed at sigma 1.5 has a standard deviation near 0.19)


# name -> (shape, block, offset, cyclic, kernels): what the case crosses is stated with the tile constants
CASES = {
    # radius 4 exceeds the plane: the index folds repeatedly; one workgroup, most of its lines and outputs past the edge
    "1x1-b7": ((1, 1), 7, 0.25, False, BOTH),
    "1x9-b7": ((1, 9), 7, 0.25, False, BOTH),
    "9x1-b7": ((9, 1), 7, 0.25, False, BOTH),
    # radius 200 on 9 x 11: about 18 folds along longitude, 22 along latitude
    "9x11-b301": ((9, 11), 301, -0.8, False, BOTH),
    "9x11-b301-cyclic": ((9, 11), 301, -0.8, True, BOTH),
    # one run + 1 on both axes (a second workgroup with one output), one bundle + 1 line
    f"{TL_RUN + 1}x{TL_RUN + 1}-b7": ((TL_RUN + 1, TL_RUN + 1), 7, 0.1, False, BOTH),
    f"{TL_RUN + 1}x{TL_RUN + 1}-b61": ((TL_RUN + 1, TL_RUN + 1), 61, 0.1, False, BOTH),
    # a ragged edge is walked for 1, 2, 4 or 8 outputs per thread: 257 and 523 leave 1 and 11 rows to the last run (1 output)
    # and 1 and 3 lines to the last bundle (1 and 4); 298 leaves 42 rows (2) and 2 lines (2); 363 leaves 107 rows (4) and 3
    # lines (4); 9 x 11 is 9 rows (1) and one full line more (1)
    f"{TL_RUN + 42}x20-b7": ((TL_RUN + 42, 20), 7, 0.1, False, BOTH),
    f"{TL_RUN + 107}x20-b61": ((TL_RUN + 107, 20), 61, 0.1, True, BOTH),
    # the driver's parameters on a ragged plane of more than two runs each way (2 * 256 + 11 and + 19; neither a multiple of
    # the bundle of 8), three planes
    "3x523x531-b301": ((3, 2 * TL_RUN + 11, 2 * TL_RUN + 19), 301, -0.8, False, BOTH),
    "3x523x531-b301-cyclic": ((3, 2 * TL_RUN + 11, 2 * TL_RUN + 19), 301, -0.8, True, BOTH),
    # a block of 1 is sigma 0: scipy skips that axis
    "20x23-b1x7": ((20, 23), (1, 7), 0.25, False, ONLY_X),
    "20x23-b7x1": ((20, 23), (7, 1), 0.25, False, ONLY_Y),
    "20x23-b7x31": ((20, 23), (7, 31), 0.25, True, BOTH),
    "20x23-b1x1": ((20, 23), (1, 1), 0.25, False, ONLY_X),
}
MASK_CASES = [k for k in CASES if CASES[k][1] != (1, 1)]   # (f > f - offset is decided by the offset alone)


@functools.lru_cache(maxsize=None)
def case(name):
    """``(f, sigma, offset, cyclic, kernels, scipy's threshold, atol)`` of a case; computed once, read-only."""
    shape, block, offset, cyclic, kernels = CASES[name]
    f = field(shape)
    sigma = sigma_of(block)
    ref = scipy_threshold(f, sigma, offset, cyclic)
    f.setflags(write=False)
    ref.setflags(write=False)
    return f, sigma, offset, cyclic, kernels, ref, atol(f, sigma)


def undecided(f, ref, tol):
    """Pixels whose comparison with scipy's own threshold an error of ``tol`` could turn."""
    return np.abs(np.asarray(f, dtype=np.float64) - ref) <= tol


def with_nan_and_inf(shape=(20, 23)):
    f = field(shape, salt=5).copy()
    f[3, 4] = np.nan
    f[15, 19] = np.inf
    return f
