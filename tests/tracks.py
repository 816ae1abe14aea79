"""TEST SUPPORT -- the host restatement of ridge tracking (csrc/tracks.hip, Engine.label_tracks / track_spans / filter_tracks,
tools.track_ridges / persistent_ridges) in numpy and scipy, and the records the tests label.  No torch.

- ``edges``: the linked pairs of include/lcs_hip.h's definition as two index arrays, from shifted slices of the record (the
  column shift a ``numpy.roll``, i.e. modulo ``nx``, with ``cyclic``): in-plane neighbours under ``connectivity``, and the
  voxels of adjacent planes at most ``reach`` apart in row and column.
- ``label``: ``scipy.sparse.csgraph.connected_components`` of that graph, renumbered in the order of each component's first
  voxel in raster order.
- ``spans``: first / last / duration / volume per track with ``np.minimum.at``, ``np.maximum.at`` and ``np.bincount``.
- ``filtered`` / ``tracked``: what Engine.filter_tracks / tools.persistent_ridges and tools.track_ridges return.
- ``structure``: the 3 x 3 x 3 structure with which ``scipy.ndimage.label`` is the same relation (reach 0 or 1, not cyclic).
- the seeded and hand-made records of tests/test_tracks.py and tests/test_tracks_gpu.py.
"""
from __future__ import annotations

import numpy as np

SEED = 20261020


def foreground(mask):
    mask = np.asarray(mask)
    return (mask != 0) & ~np.isnan(mask.astype(np.float64))


def _pairs(fg, idx, dt, dr, dc, cyclic):
    """Linked pairs (t, r, c) -- (t + dt, r + dr, c + dc) with both ends foreground; dt >= 0."""
    nt, ny, nx = fg.shape
    none = np.zeros(0, np.int64)
    if dt >= nt or abs(dr) >= ny:
        return none, none

    def cut(n, d):   # slices of the source and the target along an axis of length n for the offset d
        return (slice(0, n - d), slice(d, n)) if d >= 0 else (slice(-d, n), slice(0, n + d))
    (ts, tt), (rs, rt) = cut(nt, dt), cut(ny, dr)
    if cyclic:
        a_f, a_i = fg[ts, rs], idx[ts, rs]
        b_f, b_i = np.roll(fg[tt, rt], -dc, axis=2), np.roll(idx[tt, rt], -dc, axis=2)     # [c] = column (c + dc) mod nx
    else:
        if abs(dc) >= nx:
            return none, none
        cs, ct = cut(nx, dc)
        a_f, a_i, b_f, b_i = fg[ts, rs, cs], idx[ts, rs, cs], fg[tt, rt, ct], idx[tt, rt, ct]
    both = a_f & b_f
    return a_i[both], b_i[both]


def edges(fg, connectivity=2, cyclic=False, reach=1):
    fg = np.asarray(fg, bool)
    idx = np.arange(fg.size, dtype=np.int64).reshape(fg.shape)
    offsets = [(0, 0, 1), (0, 1, 0)] + ([(0, 1, 1), (0, 1, -1)] if connectivity == 2 else [])
    offsets += [(1, dr, dc) for dr in range(-reach, reach + 1) for dc in range(-reach, reach + 1)]
    pairs = [_pairs(fg, idx, *o, cyclic) for o in offsets]
    return np.concatenate([p[0] for p in pairs]), np.concatenate([p[1] for p in pairs])


def label(mask, connectivity=2, cyclic=False, reach=1):
    """``(labels int32 shaped like mask, count)`` of a ``(n_times, ny, nx)`` record."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    fg = foreground(mask)
    a, b = edges(fg, connectivity, cyclic, reach)
    graph = coo_matrix((np.ones(a.size, np.int8), (a, b)), shape=(fg.size, fg.size)).tocsr()
    comp = connected_components(graph, directed=False)[1][fg.ravel()]        # of the foreground voxels, in raster order
    out = np.zeros(fg.size, np.int32)
    if comp.size:
        uniq, first = np.unique(comp, return_index=True)                     # first voxel of every component
        rank = np.zeros(comp.max() + 1, np.int32)
        rank[uniq[np.argsort(first, kind="stable")]] = np.arange(1, uniq.size + 1)
        out[fg.ravel()] = rank[comp]
    return out.reshape(fg.shape), int(out.max(initial=0))


def spans(labels, n):
    """dict of arrays of length ``n``: first, last, duration (int32) and volume (int64)."""
    labels = np.asarray(labels)
    t = np.broadcast_to(np.arange(labels.shape[0])[:, None, None], labels.shape)[labels > 0]
    l = labels[labels > 0] - 1
    first, last = np.full(n, labels.shape[0], np.int32), np.full(n, -1, np.int32)
    np.minimum.at(first, l, t)
    np.maximum.at(last, l, t)
    return dict(first=first, last=last, duration=(last - first + 1).astype(np.int32),
                volume=np.bincount(l, minlength=n).astype(np.int64))


def filtered(mask, min_duration=1, min_volume=1, connectivity=2, cyclic=False, reach=1, fill=0.0):
    mask = np.asarray(mask)
    lab, n = label(mask, connectivity, cyclic, reach)
    s = spans(lab, n)
    table = np.concatenate([[False], (s["duration"] >= min_duration) & (s["volume"] >= min_volume)])
    return np.where(table[lab], mask, np.asarray(fill, dtype=mask.dtype))


def tracked(mask, reach=1, connectivity=2, cyclic=False, min_duration=1):
    """``(ids, table)`` of tools.track_ridges on a sorted ``(time, latitude, longitude)`` record (indices only in the table)."""
    lab, n = label(mask, connectivity, cyclic, reach)
    s = spans(lab, n)
    keep = s["duration"] >= min_duration
    new = np.concatenate([[0], np.where(keep, np.cumsum(keep), 0)]).astype(np.int32)
    return new[lab], {k: v[keep] for k, v in s.items()}


def structure(connectivity, reach):
    """scipy.ndimage.label's structure for ``reach`` 0 or 1."""
    from scipy import ndimage
    s = np.zeros((3, 3, 3), bool)
    s[1] = ndimage.generate_binary_structure(2, connectivity)
    if reach == 1:
        s[0] = s[2] = True
    else:
        s[0, 1, 1] = s[2, 1, 1] = True
    return s


# ------------------------------------------------------------------ the records
def random_record(shape, density, salt=0):
    rng = np.random.default_rng([SEED, *shape, int(density * 100), salt])
    return (rng.random(shape) < density).astype(np.float64)


def moving_blob(n_times, ny, nx, step=1, size=2):
    """A ``size`` x ``size`` blob that moves ``step`` columns per plane (wrapping round the plane's end)."""
    m = np.zeros((n_times, ny, nx))
    for t in range(n_times):
        for j in range(size):
            m[t, ny // 2:ny // 2 + size, (3 + t * step + j) % nx] = 1
    return m


def meeting_ridges(n_times=4, ny=5, nx=9):
    """Two ridges, in rows 1 and 3, that a bar in the last plane joins: one track, which carries the label of row 1's ridge."""
    m = np.zeros((n_times, ny, nx))
    m[:, 1, 2:5] = 1
    m[1:, 3, 2:5] = 1          # starts one plane later: its first voxel comes after every voxel of plane 0
    m[-1, 1:4, 4] = 1
    return m


def comb_in_time(n_times, ny, nx):
    """Teeth one pixel wide that run along time, two pixels apart, joined only by the full last plane."""
    m = np.zeros((n_times, ny, nx))
    m[:, 0::2, 0::2] = 1
    m[-1] = 1
    return m


def serpentine_in_time(n_times, ny, nx):
    """One voxel wide through the whole record: row 0 of every even plane, joined to the next even plane through a single voxel
    of the odd plane between them, at alternating ends.  One track at reach 0 and connectivity 1, found through the longest chains."""
    m = np.zeros((n_times, ny, nx))
    m[0::2, 0, :] = 1
    for k, t in enumerate(range(1, n_times, 2)):
        m[t, 0, nx - 1 if k % 2 == 0 else 0] = 1
    return m


def seam_in_time(ny, nx, rows_apart=0):
    """Column 0 of plane 0 and column nx - 1 of plane 1, ``rows_apart`` rows from each other."""
    m = np.zeros((2, ny, nx))
    m[0, 1, 0] = 1
    m[1, 1 + rows_apart, nx - 1] = 1
    return m


def background_forms(shape):
    """NaN and both zeros are background, negative values foreground."""
    m = random_record(shape, 0.3, salt=1)
    rng = np.random.default_rng([SEED, 7, *shape])
    m[rng.random(shape) < 0.2] = np.nan
    m[rng.random(shape) < 0.2] = -2.5
    m[rng.random(shape) < 0.1] = -0.0
    return m
