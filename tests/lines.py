"""TEST SUPPORT -- the host restatement of ridge lines (csrc/lines.hip, Engine.trace_lines, tools.ridge_lines): the definition
of include/lcs_hip.h written as a plain pixel WALK in numpy and Python, not as pointer doubling, and the hand-made masks.

- ``links``: the link byte of every pixel (bit k: linked to the neighbour in direction k = NW, N, NE, E, SE, S, SW, W; an edge
  neighbour links, a corner neighbour only if neither of the two edge neighbours beside it is foreground).
- ``trace``: every line of one plane by walking.  From every node, along every link that leaves it, pixel by pixel through
  the interior pixels to the next node; of the two walks of an open line the one that starts with the smaller dart id
  ``p * 8 + k`` is kept.  What no such walk has visited lies on rings: the first unvisited interior pixel in raster order is a
  ring's first pixel and the walk leaves it by its lower code.  Isolated pixels are lines of one point, keyed ``p * 8``.
  Lines are sorted by key.  Link lengths are ``tests.sphere_distance``'s chord and arc per link, ``distance`` their sequential
  ``numpy.cumsum``.
- ``trace_planes``: the same for a stack, concatenated as ``Engine.trace_lines`` concatenates.
- ``CASES``: the hand-made masks by name, as ``(mask, cyclic)``; ``EXPECT``: what a person reads off them.
"""
from __future__ import annotations

import numpy as np

from tests import sphere_distance as SD
from tests.components import foreground

RADIUS = SD.RADIUS
STEPS = ((-1, -1), (-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1), (0, -1))      # direction codes 0 .. 7
POPCOUNT = np.array([bin(i).count("1") for i in range(256)], dtype=np.int32)


def grid(ny, nx):
    """A regional grid with distinct coordinates for any size, poles and seam avoided."""
    return np.linspace(-60.0, 70.0, ny) if ny > 1 else np.array([12.5]), np.linspace(-170.0, 175.0, nx) if nx > 1 else np.array([33.0])


def links(mask, cyclic=False):
    fg = foreground(np.asarray(mask))
    ny, nx = fg.shape
    pad = np.zeros((ny + 2, nx + 2), dtype=bool)
    pad[1:-1, 1:-1] = fg
    if cyclic:
        pad[1:-1, 0], pad[1:-1, -1] = fg[:, -1], fg[:, 0]
    at = [pad[1 + dr:1 + dr + ny, 1 + dc:1 + dc + nx] for dr, dc in STEPS]
    out = np.zeros((ny, nx), dtype=np.uint8)
    for k in range(8):
        ok = at[k] if k % 2 else at[k] & ~at[(k + 7) % 8] & ~at[(k + 1) % 8]
        out |= (ok & fg).astype(np.uint8) << k
    return out


def neighbour(p, k, ny, nx, cyclic):
    r, c = divmod(p, nx)
    r, c = r + STEPS[k][0], c + STEPS[k][1]
    if cyclic:
        c %= nx
    assert 0 <= r < ny and 0 <= c < nx
    return r * nx + c


def link_lengths(a, b, lat, lon, radius=RADIUS):
    """Great-circle length of the links between the pixel lists ``a`` and ``b``."""
    X, Y, Z = SD.unit_vectors(lat, lon)
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    return SD.dist_of(SD.cost_of((X[a], Y[a], Z[a]), (X[b], Y[b], Z[b])), radius)


def index_length(n_edge, n_diag, sampling=None):
    """``fl(n_edge * sy + fl(n_diag * fl(sqrt(fl(sy * sy + sx * sx)))))``."""
    sy, sx = (np.float64(s) for s in np.broadcast_to(np.asarray(1.0 if sampling is None else sampling, dtype=np.float64), (2,)))
    diag = np.sqrt(sy * sy + sx * sx)
    return np.asarray(n_edge, dtype=np.float64) * sy + np.asarray(n_diag, dtype=np.float64) * diag


def walk(mask, cyclic=False):
    """``[(key, closed, [pixels], [codes of the links between them, the closing one of a ring included])]`` sorted by key, and
    the link bytes."""
    lk = links(mask, cyclic)
    ny, nx = lk.shape
    flat = lk.ravel()
    degree = POPCOUNT[flat]
    fg = foreground(np.asarray(mask)).ravel()
    codes = [[k for k in range(8) if b >> k & 1] for b in range(256)]
    found, visited = [], np.zeros(flat.size, dtype=bool)
    for p in np.flatnonzero(fg & (degree != 2)):
        p = int(p)
        if degree[p] == 0:
            found.append((p * 8, 0, [p], []))
        for k in codes[flat[p]]:
            pixels, steps, cur, d = [p], [], p, k
            while True:
                cur = neighbour(cur, d, ny, nx, cyclic)
                pixels.append(cur)
                steps.append(d)
                if degree[cur] != 2:
                    break
                visited[cur] = True
                a, b = codes[flat[cur]]
                d = a if b == (d + 4) % 8 else b
            if p * 8 + k < cur * 8 + (d + 4) % 8:
                found.append((p * 8 + k, 0, pixels, steps))
    for p in np.flatnonzero(fg & (degree == 2)):
        p = int(p)
        if visited[p]:
            continue
        pixels, steps, cur, d = [], [], p, codes[flat[p]][0]
        while True:
            pixels.append(cur)
            visited[cur] = True
            steps.append(d)
            cur = neighbour(cur, d, ny, nx, cyclic)
            if cur == p:
                break
            a, b = codes[flat[cur]]
            d = a if b == (d + 4) % 8 else b
        found.append((p * 8 + steps[0], 1, pixels, steps))
    found.sort(key=lambda line: line[0])
    return found, lk


LINE_INTS = ("plane", "offset", "count", "closed", "first", "last", "first_degree", "last_degree", "n_edge", "n_diag")
POINT_INTS = ("line", "pixel")


def trace(mask, cyclic=False, metric="sphere", lat=None, lon=None, radius=RADIUS, sampling=None, plane=0, line0=0, offset0=0):
    found, lk = walk(mask, cyclic)
    degree = POPCOUNT[lk.ravel()]
    L = {k: [] for k in LINE_INTS + ("key", "length")}
    P = {k: [] for k in POINT_INTS + ("distance", "step")}
    offset = offset0
    for i, (key, closed, pixels, steps) in enumerate(found):
        corner = np.array([1 - k % 2 for k in steps], dtype=np.int64)
        if metric == "sphere":
            ends = pixels[1:] + ([pixels[0]] if closed else [])
            step = link_lengths(pixels[:len(steps)], ends, lat, lon, radius) if steps else np.zeros(0)
            run = np.cumsum(step)
        else:
            step = index_length(1 - corner, corner, sampling)
            run = index_length(np.cumsum(1 - corner), np.cumsum(corner), sampling)
        n = len(pixels)
        L["plane"].append(plane)
        L["key"].append(key)
        L["offset"].append(offset)
        L["count"].append(n)
        L["closed"].append(closed)
        L["first"].append(pixels[0])
        L["last"].append(pixels[-1])
        L["first_degree"].append(degree[pixels[0]])
        L["last_degree"].append(degree[pixels[-1]])
        L["n_diag"].append(int(corner.sum()))
        L["n_edge"].append(len(steps) - int(corner.sum()))
        L["length"].append(run[-1] if len(steps) else 0.0)
        P["line"] += [line0 + i] * n
        P["pixel"] += pixels
        P["distance"] += [0.0] + list(run[:n - 1])
        P["step"] += [0.0] + list(step[:n - 1])
        offset += n
    out = {k: np.asarray(v, dtype=np.float64 if k == "length" else np.int64) for k, v in L.items()}
    out.update({k: np.asarray(v, dtype=np.float64 if k in ("distance", "step") else np.int64) for k, v in P.items()})
    out["links"] = lk
    return out


def trace_planes(stack, cyclic=False, **kw):
    """A stack ``(n, ny, nx)``: lines ordered by plane, then by number; ``line`` and ``offset`` run through all planes."""
    parts, lines, points = [], 0, 0
    for m, plane in enumerate(np.asarray(stack)):
        t = trace(plane, cyclic, plane=m, line0=lines, offset0=points, **kw)
        lines += t["count"].size
        points += t["pixel"].size
        parts.append(t)
    out = {k: np.concatenate([t[k] for t in parts]) for k in parts[0] if k != "links"}
    out["links"] = np.stack([t["links"] for t in parts])
    return out


def invariants(t):
    """What holds of every trace: every link in exactly one line, the counts add up, the numbering follows the keys."""
    lk = t["links"].reshape(-1, t["links"].shape[-2], t["links"].shape[-1])
    n_links = int(POPCOUNT[lk].sum()) // 2
    assert int((t["count"] - 1 + t["closed"]).sum()) == n_links == int((t["n_edge"] + t["n_diag"]).sum())
    assert np.array_equal(t["offset"], np.cumsum(t["count"]) - t["count"]) and int(t["count"].sum()) == t["pixel"].size
    order = t["plane"] * (8 * lk.shape[1] * lk.shape[2]) + t["key"]
    assert (np.diff(order) > 0).all()
    seen = set()
    for i in range(t["count"].size):
        pix = t["pixel"][t["offset"][i]:t["offset"][i] + t["count"][i]]
        assert (t["line"][t["offset"][i]:t["offset"][i] + t["count"][i]] == i).all()
        pairs = list(zip(pix[:-1], pix[1:])) + ([(pix[-1], pix[0])] if t["closed"][i] else [])
        for a, b in pairs:
            link = (int(t["plane"][i]), min(int(a), int(b)), max(int(a), int(b)))
            assert link not in seen
            seen.add(link)
    assert len(seen) == n_links


# ------------------------------------------------------------------ the hand-made masks
def _of(rows):
    return np.array([[0.0 if ch in ". " else 1.0 for ch in row] for row in rows])


def serpentine(ny=33, nx=65):
    m = np.zeros((ny, nx))
    for r in range(0, ny, 2):
        m[r, :] = 1
        if r + 1 < ny:
            m[r + 1, nx - 1 if (r // 2) % 2 == 0 else 0] = 1
    return m


def spiral(ny=33, nx=65):
    """A rectangular spiral inwards from the corner, its arms one pixel apart."""
    m = np.zeros((ny, nx))
    r, c, d, turns = 0, 0, 0, 0
    m[0, 0] = 1
    while turns < 2:
        dr, dc = ((0, 1), (1, 0), (0, -1), (-1, 0))[d]
        r1, c1, r2, c2 = r + dr, c + dc, r + 2 * dr, c + 2 * dc
        free = 0 <= r1 < ny and 0 <= c1 < nx and m[r1, c1] == 0
        if free and not (0 <= r2 < ny and 0 <= c2 < nx and m[r2, c2] == 1):
            r, c, turns = r1, c1, 0
            m[r, c] = 1
        else:
            d, turns = (d + 1) % 4, turns + 1
    return m


def _frame(ny=6, nx=8):
    m = np.zeros((ny, nx))
    m[0, :] = m[-1, :] = m[:, 0] = m[:, -1] = 1
    return m


def _values():
    m = _of(["##.#",
             ".#.#",
             "...."])
    m[0, 0], m[0, 1], m[1, 1], m[0, 3], m[1, 3] = -2.5, np.nan, -0.0, 7.0, -1.0
    return m


CASES = {
    "1x1-on": (np.ones((1, 1)), False),
    "1x1-off": (np.zeros((1, 1)), False),
    "1x9": (np.ones((1, 9)), False),
    "9x1": (np.ones((9, 1)), False),
    "block-2x2": (_of(["....", ".##.", ".##.", "...."]), False),
    "plus": (_of([".....", "..#..", "..#..", "#####", "..#..", "..#.."]), False),
    "T": (_of(["#####", "..#..", "..#..", "..#.."]), False),
    "Y": (_of(["#...#", ".#.#.", "..#..", "..#..", "..#.."]), False),
    "two-junctions": (_of(["#..#", ".##.", "#..#"]), False),
    "lollipop": (_of([".###.", ".#.#.", ".###.", "..#..", "..#.."]), False),
    "staircase": (_of(["##....", ".##...", "..##..", "...##."]), False),
    "diagonal": (_of(["#....", ".#...", "..#..", "...#.", "....#"]), False),
    "row": (_of([".......", "#######", "......."]), False),
    "row-cyclic": (_of([".......", "#######", "......."]), True),
    "seam-crossing": (_of([".......", "##...##", "......."]), True),
    "nx3-cyclic": (_of(["###", "...", "#.#"]), True),
    "frame": (_frame(), False),
    "full-5x7": (np.ones((5, 7)), False),
    "empty": (np.zeros((4, 6)), False),
    "values": (_values(), False),
    "serpentine": (serpentine(), False),
    "spiral": (spiral(), False),
}

# name -> [(count, closed, first pixel, last pixel, n_edge, n_diag)] in the order of the lines, read off the masks by hand
EXPECT = {
    "1x1-on": [(1, 0, 0, 0, 0, 0)],
    "1x1-off": [],
    "1x9": [(9, 0, 0, 8, 8, 0)],
    "9x1": [(9, 0, 0, 8, 8, 0)],
    "block-2x2": [(4, 1, 5, 9, 4, 0)],                      # leaves (1, 1) eastwards: 5, 6, 10, 9
    "diagonal": [(5, 0, 0, 24, 0, 4)],
    "staircase": [(8, 0, 0, 22, 7, 0)],
    "row": [(7, 0, 7, 13, 6, 0)],
    "row-cyclic": [(7, 1, 7, 13, 7, 0)],                    # leaves (1, 0) by E (3) before W (7): 7, 8, ..., 13
    "seam-crossing": [(4, 0, 8, 12, 3, 0)],                 # ends (1, 1) and (1, 5): 8, 7, 13, 12
    "nx3-cyclic": [(3, 1, 0, 2, 3, 0), (2, 0, 6, 8, 1, 0)], # the ring 0, 1, 2 and the pair (2, 0) - (2, 2) across the seam
    "T": [(3, 0, 0, 2, 2, 0), (3, 0, 2, 4, 2, 0), (4, 0, 2, 17, 3, 0)],
    "frame": [(24, 1, 0, 8, 24, 0)],
    "lollipop": [(9, 0, 12, 12, 8, 0), (3, 0, 12, 22, 2, 0)],   # the loop leaves (2, 2) by E (3) and comes back by W; then the stick
    "empty": [],
}


def random_mask(ny, nx, density, salt=0):
    rng = np.random.default_rng([20261020, ny, nx, int(density * 100), salt])
    return (rng.random((ny, nx)) < density).astype(np.float64)
