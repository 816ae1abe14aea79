"""TEST SUPPORT -- the host restatement of the component filter (csrc/components.hip, Engine.label_components /
component_props / filter_components, tools.filter_ridges) in numpy and scipy, and the masks the tests label.

- ``label``: ``scipy.ndimage.label`` with ``generate_binary_structure(2, connectivity)`` on the foreground (``!= 0`` and not
  NaN); with ``cyclic`` the components that touch across the seam are merged by a small union-find and renumbered by their
  first pixel in raster order.
- ``sums``: per component the root (first pixel), the area, the five integer sums about the root pixel and the sum, maximum
  and minimum of an intensity -- python integers and numpy reductions, nothing clever.
- ``props``: mean, centroid, the eigenvalues l1 >= l2 of the inertia tensor per pixel and the axis lengths 4 sqrt(l), from
  two-pass CENTRED moments in float64 (the mean first, then the squares of the differences): another route to the same
  numbers than the shifted-sum formula the engine uses.
- ``filtered``: the mask with the components that fail a threshold replaced by ``fill``.
- ``CASES`` / ``mask_of``: the planes of tests/test_components_gpu.py, by name.
"""
from __future__ import annotations

import numpy as np

SEED = 20261018
PROPS = ("area", "mean_intensity", "max_intensity", "min_intensity", "major_axis_length", "minor_axis_length")


def foreground(mask):
    mask = np.asarray(mask)
    return (mask != 0) & ~np.isnan(mask.astype(np.float64))


def label(mask, connectivity=2, cyclic=False):
    """``(labels int32, count)`` of one plane."""
    from scipy import ndimage
    fg = foreground(mask)
    lab, n = ndimage.label(fg, structure=ndimage.generate_binary_structure(2, connectivity))
    lab = lab.astype(np.int32)
    if not cyclic or n == 0:
        return lab, int(n)
    ny, nx = fg.shape
    parent = list(range(n + 1))

    def find(i):
        while parent[i] != i:
            i = parent[i]
        return i
    for r in range(ny):
        if not lab[r, 0]:
            continue
        for rr in ((r - 1, r, r + 1) if connectivity == 2 else (r,)):
            if 0 <= rr < ny and lab[rr, nx - 1]:
                a, b = find(lab[r, 0]), find(lab[rr, nx - 1])
                if a != b:
                    parent[max(a, b)] = min(a, b)
    # scipy's labels are in the order of the first pixels, and a merged set keeps its smallest label: ranking the surviving
    # roots renumbers by first pixel
    roots = sorted({find(i) for i in range(1, n + 1)})
    rank = {r: k + 1 for k, r in enumerate(roots)}
    table = np.zeros(n + 1, dtype=np.int32)
    for i in range(1, n + 1):
        table[i] = rank[find(i)]
    return table[lab], len(roots)


def _offsets(idx, root, nx, cyclic):
    r, c = np.divmod(idx, nx)
    rr, rc = divmod(int(root), nx)
    dr, dc = r - rr, c - rc
    if cyclic:
        dc = np.where(dc >= nx - nx // 2, dc - nx, np.where(dc < -(nx // 2), dc + nx, dc))
    return dr.astype(np.int64), dc.astype(np.int64)


def sums(labels, n, intensity=None, cyclic=False):
    """dict of arrays of length ``n``: root, area, moments (5, n) as int64, and sum / max / min / abs_sum with an intensity."""
    labels = np.asarray(labels)
    nx = labels.shape[1]
    flat = labels.ravel()
    order = np.argsort(flat, kind="stable")
    bounds = np.searchsorted(flat[order], np.arange(1, n + 2))
    out = dict(root=np.zeros(n, np.int32), area=np.zeros(n, np.int64), moments=np.zeros((5, n), np.int64))
    if intensity is not None:
        v_all = np.asarray(intensity, dtype=np.float64).ravel()
        out.update({k: np.zeros(n) for k in ("sum", "max", "min", "abs_sum")})
    for k in range(n):
        idx = order[bounds[k]:bounds[k + 1]]          # ascending: stable sort of the raster order
        dr, dc = _offsets(idx, idx[0], nx, cyclic)
        out["root"][k], out["area"][k] = idx[0], idx.size
        out["moments"][:, k] = [dr.sum(), dc.sum(), (dr * dr).sum(), (dr * dc).sum(), (dc * dc).sum()]
        if intensity is not None:
            v = v_all[idx]
            out["sum"][k], out["abs_sum"][k] = v.sum(), np.abs(v).sum()
            out["max"][k], out["min"][k] = (np.nan, np.nan) if np.isnan(v).any() else (v.max(), v.min())
    out["order"], out["bounds"] = order, bounds
    return out


def props(labels, n, intensity=None, cyclic=False):
    """Properties of the ``n`` components of one plane: dict of float64 arrays of length ``n`` (area int64, centroid (n, 2)),
    with ``l1`` >= ``l2`` the eigenvalues the axis lengths are 4 sqrt of."""
    labels = np.asarray(labels)
    nx = labels.shape[1]
    s = sums(labels, n, intensity, cyclic)
    out = dict(area=s["area"].copy(), centroid=np.zeros((n, 2)), l1=np.zeros(n), l2=np.zeros(n))
    for k in range(n):
        idx = s["order"][s["bounds"][k]:s["bounds"][k + 1]]
        dr, dc = (d.astype(np.float64) for d in _offsets(idx, idx[0], nx, cyclic))
        mr, mc = dr.mean(), dc.mean()
        a, b, c = ((dr - mr) ** 2).mean(), ((dr - mr) * (dc - mc)).mean(), ((dc - mc) ** 2).mean()
        rad = np.sqrt(((a - c) / 2) ** 2 + b * b)
        out["l1"][k], out["l2"][k] = (a + c) / 2 + rad, (a + c) / 2 - rad
        rr, rc = divmod(int(idx[0]), nx)
        out["centroid"][k] = rr + mr, (rc + mc) % nx if cyclic else rc + mc
    out["major_axis_length"] = 4 * np.sqrt(out["l1"])
    out["minor_axis_length"] = 4 * np.sqrt(np.maximum(out["l2"], 0))
    if intensity is not None:
        with np.errstate(invalid="ignore"):
            out["mean_intensity"] = s["sum"] / s["area"]
        out["max_intensity"], out["min_intensity"], out["abs_sum"] = s["max"], s["min"], s["abs_sum"]
    return out


def filtered(mask, intensity, criteria, thresholds, connectivity=2, cyclic=False, fill=0.0):
    mask = np.asarray(mask)
    lab, n = label(mask, connectivity, cyclic)
    p = props(lab, n, intensity, cyclic)
    keep = np.ones(n, bool)
    for k, th in zip(criteria, thresholds):
        with np.errstate(invalid="ignore"):
            keep &= p[k] >= th
    table = np.concatenate([[False], keep])
    return np.where(table[lab], mask, np.asarray(fill, dtype=mask.dtype))


# ------------------------------------------------------------------ the planes
def _random(ny, nx, density, salt=0):
    rng = np.random.default_rng([SEED, ny, nx, int(density * 100), salt])
    return (rng.random((ny, nx)) < density).astype(np.float64)


def _checkerboard(ny, nx):
    return ((np.add.outer(np.arange(ny), np.arange(nx)) % 2) == 0).astype(np.float64)


def _serpentine(ny, nx):
    """One pixel wide, back and forth over the whole plane: full rows 0, 2, 4, ..., joined at alternating ends."""
    m = np.zeros((ny, nx))
    m[0::2] = 1
    for i, r in enumerate(range(1, ny, 2)):
        m[r, nx - 1 if i % 2 == 0 else 0] = 1
    return m


def _comb(ny, nx):
    """Vertical teeth in every other column, joined only along the last row."""
    m = np.zeros((ny, nx))
    m[:, 0::2] = 1
    m[ny - 1] = 1
    return m


def _seam(ny, nx):
    """Pieces that meet only across the seam: a straight pair, two diagonal pairs, a bar around it, and bystanders."""
    m = np.zeros((ny, nx))
    m[1, 0] = m[1, nx - 1] = 1                      # straight
    m[4, 0] = m[5, nx - 1] = 1                      # column 0 above
    m[9, 0] = m[8, nx - 1] = 1                      # column 0 below
    m[12, :3] = m[12, nx - 4:] = 1                  # a bar around the seam
    m[15, 5:9] = 1
    m[ny - 1, 0] = m[ny - 2, nx - 1] = 1
    m[0, nx - 1] = 1                                # touches (1, 0) across the seam by a corner
    return m


def _nan_negative(ny, nx):
    m = _random(ny, nx, 0.3, salt=1)
    rng = np.random.default_rng([SEED, 7])
    m[rng.random((ny, nx)) < 0.2] = np.nan          # background
    m[rng.random((ny, nx)) < 0.2] = -2.5            # foreground
    return m


CASES = {
    "1x1": lambda: np.ones((1, 1)),
    "1x1-empty": lambda: np.zeros((1, 1)),
    "1x17": lambda: _random(1, 17, 0.6),
    "17x1": lambda: _random(17, 1, 0.6),
    "2x2": lambda: np.array([[1.0, 0.0], [0.0, 1.0]]),
    "33x65": lambda: _random(33, 65, 0.5),
    "67x130": lambda: _random(67, 130, 0.5),
    "background": lambda: np.zeros((33, 65)),
    "foreground": lambda: np.ones((33, 65)),
    "checkerboard-96x130": lambda: _checkerboard(96, 130),
    "serpentine-67x130": lambda: _serpentine(67, 130),
    "comb-67x130": lambda: _comb(67, 130),
    "random-0.1": lambda: _random(67, 130, 0.1),
    "random-0.41": lambda: _random(67, 130, 0.41),
    "random-0.59": lambda: _random(67, 130, 0.59),
    "random-0.9": lambda: _random(67, 130, 0.9),
    "nan-negative": lambda: _nan_negative(33, 65),
    # more tiles than one pass of the tile scan takes (256 tiles of 1024 pixels): its carry from pass to pass
    "checkerboard-515x513": lambda: _checkerboard(515, 513),
}
SEAM_CASES = {
    "seam-20x13": lambda: _seam(20, 13),
    "seam-20x12": lambda: _seam(20, 12),
    "seam-random-0.41": lambda: _random(67, 130, 0.41, salt=2),
    "seam-random-0.59": lambda: _random(33, 65, 0.59, salt=2),
    "seam-one-column": lambda: _random(17, 1, 0.6),
    "seam-two-columns": lambda: _random(17, 2, 0.5),
}


def mask_of(name, dtype=np.float64):
    return {**CASES, **SEAM_CASES}[name]().astype(dtype)


def intensity_of(shape, dtype=np.float64, salt=0):
    return np.random.default_rng([SEED, 99, salt, *shape]).random(shape).astype(dtype)
