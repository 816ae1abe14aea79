"""TEST SUPPORT -- randomised draws for the ridge-mask kernels (csrc/components.hip, csrc/distance.hip, csrc/morphology.hip,
csrc/tracks.hip, csrc/sphere_distance.hip) and the numpy / scipy reference of every draw.  No GPU here: tests/test_mask_draws.py
pins the references and the conditions the draws must meet, tests/test_mask_hypothesis_gpu.py runs the same draws through the
engine.

- ``EDGES``: the plane sides worth drawing on purpose -- 1 .. 5 and ``k - 1, k, k + 1`` around the tile constants, which are read
  out of the ``.hip`` sources (``constants``), so a kernel whose tile changes moves the draws with it.
- ``Plane`` / ``Stack``: one plane is white noise (``components._random``), thresholded smoothed noise (``skeleton._smooth``), all
  background or all foreground, optionally sprinkled with NaN (background) and negative values (foreground; an all-background
  plane gets the NaN only and stays empty); a stack is 1 .. 3 planes of one shape and dtype (1 .. 6 as the record of a track
  draw).  A draw holds parameters only; the arrays are built from them on demand (``Stack.masks``), so a failing draw prints as
  something one can paste back.
- ``ComponentDraw`` / ``DistanceDraw`` / ``ThinDraw`` / ``DilateDraw`` and their strategies, and ``*_reference`` for each, built
  on tests/components.py, tests/distance.py and tests/skeleton.py.
- ``dilate_reference`` / ``scipy_structure``: dilation by any of the 255 structures of ``lc_morph_args.structure``.
- ``TrackDraw``: a record of at most 48 x 80 x 6 with a connectivity, ``cyclic``, a reach of 0 .. 16, a capacity of the spans and
  two quantiles for the lifetime filter; ``tracks_reference`` / ``track_spans_reference`` / ``track_filter_reference`` on
  tests/tracks.py (scipy.sparse.csgraph).  ``TRACK_EXPLICIT``: the plane widths 2 reach, 2 reach + 1 and 2 reach + 2 where the
  cyclic window in time changes its form, records of one voxel below, at and above ``TR_TILE`` and ``TS_TILE``, an empty plane
  between two others, planes smaller than one thread's span of the spans kernel, narrow cyclic records at reach 0.
- ``SphereDistanceDraw``: a stack from three families of shapes (narrow and tall, wide and short -- the long side up to 520 with
  the values around ``SD_THREADS`` and twice it drawn on purpose --, and both sides around the wave), one of five grids
  (``coordinates``), a bound in row steps and a radius; ``sphere_distance_reference`` is tests/sphere_distance.py's brute force.
- the sums on the sphere, over the ``ComponentDraw`` sequence and its cached labels: ``sphere_sums_reference`` (the grid is
  ``sphere_props.coordinates`` in the variant the draw's salt chooses), ``sphere_admitted`` (which labels the direction checks
  admit, on the reference alone) and ``sphere_filter_reference`` (thresholds that the reference's own bounds decide).
- ``Space``: a hypothesis strategy and a plain seeded sampler over the same values, built together by combinators named after
  hypothesis's.  ``each`` runs a body over the draws of a space: by default the sampler's, handed to hypothesis as explicit
  examples, so that the CPU test that checks the conditions and the GPU test see the same draws; with ``LCS_HYP_RANDOM``
  hypothesis's own.

Wall time of the references on one CPU core, whole sequence: tracks 1.3 s with the filter (0.25 s the slowest draw), the
great-circle distance 2.6 s for 102 planes, the sums on the sphere 0.6 s and their filter 0.5 s for 58 draws.
"""
from __future__ import annotations

import dataclasses
import functools
import os
import re
import zlib

import numpy as np
from hypothesis import HealthCheck, Phase, example, given, settings
from hypothesis import strategies as st

from lagrangiancoherence_amd import build
from tests import components as CO
from tests import distance as DT
from tests import skeleton as SK

SEED = 20261020
# Deterministic draws by default (the same examples on every run); LCS_HYP_RANDOM=1 LCS_HYP_SCALE=10 explores.
DERAND = not os.environ.get("LCS_HYP_RANDOM")
SCALE = int(os.environ.get("LCS_HYP_SCALE", "1"))
EXAMPLES = 50
NY_MAX, NX_MAX = 140, 270


# ------------------------------------------------------------------ the tile constants, from the sources
def constants(source, *names):
    src = build._strip_comments(open(os.path.join(build.CSRC, source)).read())
    return {n: int(re.search(r"\b%s = (\d+)\s*[,;]" % n, src).group(1)) for n in names}


CC = constants("components.hip", "CC_THREADS", "CC_ITEMS", "CS_ITEMS")
CC_TILE, CS_TILE = CC["CC_THREADS"] * CC["CC_ITEMS"], CC["CC_THREADS"] * CC["CS_ITEMS"]
DTC = constants("distance.hip", "DT_THREADS", "DT_SEG")
MO = constants("morphology.hip", "MO_HALO", "MO_TW", "MO_TH")
# the halo and twice it, a tile's height alone and with one halo, a row segment, a tile's width alone, with one and with both
# halos (the image in LDS), the columns of one workgroup
TILE_SIDES = sorted({MO["MO_HALO"], 2 * MO["MO_HALO"], MO["MO_TH"], MO["MO_TH"] + MO["MO_HALO"], DTC["DT_SEG"], MO["MO_TW"],
                     MO["MO_TW"] + MO["MO_HALO"], MO["MO_TW"] + 2 * MO["MO_HALO"], DTC["DT_THREADS"]})
EDGES = sorted({1, 2, 3, 4, 5} | {k + d for k in TILE_SIDES for d in (-1, 0, 1)})


# ------------------------------------------------------------------ one description of a set of draws, two ways to draw from it
class Space:
    """A hypothesis strategy and a plain sampler over the same values.  hypothesis explores and shrinks with the strategy; the
    fixed draws of a default run come from the sampler, because what hypothesis generates -- derandomised or seeded alike --
    also depends on the integer constants it finds in whatever project modules happen to be loaded (the engine, other test
    files), so it is not the same under the whole suite, a single file and the CPU test that checks the conditions."""

    def __init__(self, strategy, sample):
        self.strategy, self.sample = strategy, sample


def sampled_from(values):
    values = list(values)
    return Space(st.sampled_from(values), lambda rng: values[int(rng.integers(len(values)))])


def integers(lo, hi):
    return Space(st.integers(lo, hi), lambda rng: int(rng.integers(lo, hi + 1)))


def booleans():
    return Space(st.booleans(), lambda rng: bool(rng.integers(2)))


def just(value):
    return Space(st.just(value), lambda rng: value)


def one_of(*spaces):
    return Space(st.one_of(*[s.strategy for s in spaces]), lambda rng: spaces[int(rng.integers(len(spaces)))].sample(rng))


def tuples(*spaces):
    return Space(st.tuples(*[s.strategy for s in spaces]), lambda rng: tuple(s.sample(rng) for s in spaces))


def tuples_of(space, fewest, most):
    return Space(st.lists(space.strategy, min_size=fewest, max_size=most).map(tuple),
                 lambda rng: tuple(space.sample(rng) for _ in range(int(rng.integers(fewest, most + 1)))))


def builds(cls, **fields):
    return Space(st.builds(cls, **{k: s.strategy for k, s in fields.items()}),
                 lambda rng: cls(**{k: s.sample(rng) for k, s in fields.items()}))


def side(most):
    return one_of(sampled_from([e for e in EDGES if e <= most]), integers(1, most))


# ------------------------------------------------------------------ masks
KINDS = ("background", "foreground", "noise", "smooth")
DENSITIES = (0.02, 0.1, 0.41, 0.59, 0.9)
SPRINKLE = 0.05


@dataclasses.dataclass(frozen=True)
class Plane:
    kind: str
    density: float = 0.41      # of "noise" only
    salt: int = 0
    sprinkle: bool = False

    def mask(self, ny, nx):
        m = {"background": lambda: np.zeros((ny, nx)), "foreground": lambda: np.ones((ny, nx)),
             "noise": lambda: CO._random(ny, nx, self.density, self.salt),
             "smooth": lambda: SK._smooth(ny, nx, salt=self.salt)}[self.kind]()
        if self.sprinkle:
            rng = np.random.default_rng([SEED, self.salt, ny, nx])
            m[rng.random((ny, nx)) < SPRINKLE] = np.nan
            if self.kind != "background":
                m[rng.random((ny, nx)) < SPRINKLE] = -2.5
        return m


@dataclasses.dataclass(frozen=True)
class Stack:
    ny: int
    nx: int
    planes: tuple
    dtype: str = "float64"

    def masks(self):
        """``(n_members, ny, nx)`` in the stack's dtype."""
        return np.stack([p.mask(self.ny, self.nx) for p in self.planes]).astype(self.dtype)


def planes(kinds=KINDS, densities=DENSITIES):
    """``kinds`` and ``densities`` may name an entry more than once: that is its weight."""
    return builds(Plane, kind=sampled_from(kinds), density=sampled_from(densities), salt=integers(0, 2 ** 16), sprinkle=booleans())


def stacks(kinds=KINDS, densities=DENSITIES):
    return builds(Stack, ny=side(NY_MAX), nx=side(NX_MAX), planes=tuples_of(planes(kinds, densities), 1, 3),
                  dtype=sampled_from(["float32", "float64"]))


# ------------------------------------------------------------------ running a body over the draws
def each(name, space, body, explicit=(), examples=EXAMPLES, derandomize=None, scale=None):
    """``body(draw)`` on every explicit draw and on ``examples`` draws of ``space``.  Derandomised, the draws come from the
    space's own sampler, seeded by ``name`` alone, and hypothesis runs them as explicit examples: one sequence per name, the
    same wherever and beside whatever it is asked for.  Otherwise hypothesis generates, and shrinks what fails."""
    def draws(draw):
        body(draw)
    fixed = DERAND if derandomize is None else derandomize
    count = examples * (SCALE if scale is None else scale)
    cases = list(explicit)
    if fixed:
        rng = np.random.default_rng([SEED, zlib.crc32(name.encode())])
        cases += [space.sample(rng) for _ in range(count)]
    for e in reversed(cases):        # the decorator applied last runs first
        draws = example(draw=e)(draws)
    kw = dict(derandomize=True, phases=(Phase.explicit,)) if fixed else {}
    settings(max_examples=count, deadline=None, suppress_health_check=list(HealthCheck), **kw)(given(draw=space.strategy)(draws))()


def collect(name, space, explicit=()):
    """The derandomised draws of a strategy, explicit ones included, whatever the environment asks of the GPU tests."""
    out = []
    each(name, space, out.append, explicit, derandomize=True, scale=1)
    return out


# ------------------------------------------------------------------ components: labels, sums, filter
CAPACITIES = ("largest", "above", "below")        # n_max None; largest count + 2; max(1, smallest non-zero count // 2)
CRITERIA = (("area",), ("max_intensity",), ("area", "max_intensity"))
EPS = 2.0 ** -53


@dataclasses.dataclass(frozen=True)
class ComponentDraw:
    stack: Stack
    connectivity: int = 2
    cyclic: bool = False
    capacity: str = "largest"
    nan_intensity: bool = False
    criteria: tuple = ("area",)
    quantiles: tuple = (0.5, 0.5)      # where in the reference's sorted property values each threshold is taken
    fill: float = 0.0
    salt: int = 0


def component_draws():
    return builds(ComponentDraw, stack=stacks(), connectivity=sampled_from([1, 2]), cyclic=booleans(),
                  capacity=sampled_from(CAPACITIES), nan_intensity=booleans(), criteria=sampled_from(CRITERIA),
                  quantiles=tuples(*[sampled_from([0.0, 0.25, 0.5, 0.75, 1.0])] * 2),
                  fill=sampled_from([0.0, -1.0, float("nan")]), salt=integers(0, 2 ** 16))


def _bg(n=1):
    return (Plane("background"),) * n


# stacks whose planes sit on both sides of the "below" capacity: an empty plane (count 0) beside planes of many components
COMPONENT_EXPLICIT = (
    ComponentDraw(Stack(67, 130, (Plane("noise", 0.41, 1),) + _bg()), 2, False, "below", True, ("area",), (0.5, 0.5), 0.0, 1),
    ComponentDraw(Stack(33, 65, _bg() + (Plane("noise", 0.1, 2), Plane("smooth", salt=3)), "float32"), 1, True, "below", False,
                  ("max_intensity",), (0.25, 0.75), float("nan"), 2),
    ComponentDraw(Stack(49, 113, (Plane("noise", 0.59, 4, True), Plane("background", sprinkle=True), Plane("noise", 0.02, 5))), 1, False,
                  "below", False, ("area", "max_intensity"), (0.75, 0.25), -1.0, 3),
    ComponentDraw(Stack(129, 17, (Plane("noise", 0.9, 6),) + _bg() + (Plane("noise", 0.41, 7, True),), "float32"), 2, True, "below", True,
                  ("area",), (1.0, 0.0), 0.0, 4),
    ComponentDraw(Stack(5, 257, _bg() + (Plane("noise", 0.1, 8),)), 2, True, "below", False, ("area", "max_intensity"), (0.0, 0.5),
                  float("nan"), 5),
    # narrow cyclic planes of sparse noise: much of what joins two pieces there is one diagonal step across the seam, and an
    # area threshold low in the list of areas tells a joined pair from two single pixels
    *[ComponentDraw(Stack(ny, nx, (Plane("noise", density, salt), Plane("noise", 0.1, salt + 1, True)), dtype), 2, True, capacity, False,
                    ("area",), (q, 0.5), 0.0, salt)
      for ny, nx, density, salt, dtype, capacity, q in ((140, 9, 0.1, 11, "float64", "largest", 0.25), (129, 3, 0.41, 12, "float32", "above", 0.5),
                                                       (140, 47, 0.1, 15, "float64", "above", 0.25))],
)


@functools.lru_cache(maxsize=None)
def labels_reference(stack, connectivity, cyclic):
    """``[(labels, count)]`` of every plane, read-only."""
    out = []
    for m in stack.masks():
        lab, n = CO.label(m, connectivity, cyclic)
        lab.setflags(write=False)
        out.append((lab, n))
    return out


def intensity_of(draw):
    """Both signs, in the stack's dtype; with ``nan_intensity`` one NaN somewhere in the stack."""
    s = draw.stack
    v = CO.intensity_of((len(s.planes), s.ny, s.nx), salt=draw.salt) - 0.25
    if draw.nan_intensity:
        v.flat[np.random.default_rng([SEED, draw.salt]).integers(v.size)] = np.nan
    return v.astype(s.dtype)


def capacity_of(draw, counts):
    """``n_max`` as the engine is given it (None: the largest count, read back by the engine)."""
    if draw.capacity == "largest":
        return None
    if draw.capacity == "above":
        return max(counts) + 2
    some = [c for c in counts if c > 0]
    return max(1, min(some) // 2) if some else 1


def straddles(draw):
    """The capacity is below one plane's count and above another's."""
    counts = [n for _, n in labels_reference(draw.stack, draw.connectivity, draw.cyclic)]
    cap = capacity_of(draw, counts)
    return cap is not None and any(c > cap for c in counts) and any(c < cap for c in counts)


def sums_reference(draw):
    """``(intensity, n_max, slots, sums)``: ``n_max`` the argument, ``slots`` the length of the engine's arrays, ``sums`` per plane
    the dict of ``components.sums`` cut to the labels the plane measures (``measured`` of them) and padded to ``slots`` with what
    include/lcs_hip.h promises for entries without a component: area 0, root -1, NaN extrema, sums 0."""
    labelled = labels_reference(draw.stack, draw.connectivity, draw.cyclic)
    counts = [n for _, n in labelled]
    v = intensity_of(draw)
    n_max = capacity_of(draw, counts)
    slots = max(1, max(counts) if n_max is None else n_max)
    out = []
    for (lab, n), vi in zip(labelled, v):
        s = CO.sums(lab, n, vi.astype(np.float64), draw.cyclic)
        k = min(n, slots)
        pad = slots - k
        out.append(dict(measured=k,
                        root=np.concatenate([s["root"][:k], np.full(pad, -1, np.int32)]),
                        area=np.concatenate([s["area"][:k], np.zeros(pad, np.int64)]),
                        moments=np.concatenate([s["moments"][:, :k], np.zeros((5, pad), np.int64)], axis=1),
                        sum=np.concatenate([s["sum"][:k], np.zeros(pad)]),
                        abs_sum=np.concatenate([s["abs_sum"][:k], np.zeros(pad)]),
                        max=np.concatenate([s["max"][:k], np.full(pad, np.nan)]),
                        min=np.concatenate([s["min"][:k], np.full(pad, np.nan)])))
    return v, n_max, slots, out


def filter_reference(draw):
    """``(intensity, thresholds, filtered stack)``: each threshold is one of the reference's own values of its property, over all
    planes, at the drawn quantile -- ``area`` and ``max_intensity`` are exact, so ``>=`` at the value itself is decided."""
    labelled = labels_reference(draw.stack, draw.connectivity, draw.cyclic)
    masks, v = draw.stack.masks(), intensity_of(draw)
    props = [CO.props(lab, n, vi.astype(np.float64), draw.cyclic) for (lab, n), vi in zip(labelled, v)]
    thresholds = []
    for k, q in zip(draw.criteria, draw.quantiles):
        vals = np.concatenate([p[k].astype(np.float64) for p in props])
        vals = np.unique(vals[np.isfinite(vals)])
        thresholds.append(float(vals[int(round(q * (len(vals) - 1)))]) if len(vals) else 1.0)
    want = np.stack([CO.filtered(m, vi.astype(np.float64), draw.criteria, thresholds, draw.connectivity, draw.cyclic, draw.fill)
                     for m, vi in zip(masks, v)])
    return v, thresholds, want


def tiled_label(mask, connectivity):
    """The cyclic labels another way: scipy's label of the plane tiled three times along x, the three copies of every pixel
    taken as one pixel (a bar that crosses the seam but does not close the circle is two pieces inside the middle copy, joined
    only through its neighbours), restricted to the middle copy and renumbered by first pixel."""
    from scipy import ndimage
    fg = CO.foreground(mask)
    nx = fg.shape[1]
    lab, n = ndimage.label(np.tile(fg, (1, 3)), structure=ndimage.generate_binary_structure(2, connectivity))
    parent = np.arange(n + 1)

    def find(i):
        while parent[i] != i:
            i = parent[i]
        return i
    copies = [lab[:, k * nx:(k + 1) * nx][fg] for k in range(3)]
    for a, b in {(int(a), int(b)) for k in (0, 2) for a, b in zip(copies[1], copies[k]) if a != b}:
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    roots = np.array([find(i) for i in range(n + 1)])
    mid = roots[lab[:, nx:2 * nx]]
    _, first = np.unique(mid[fg], return_index=True)            # fg selects in raster order
    order = mid[fg][np.sort(first)]                             # the classes in the order of their first pixels
    table = np.zeros(n + 1, dtype=np.int32)
    table[order] = np.arange(1, len(order) + 1)
    return np.where(fg, table[mid], 0).astype(np.int32), len(order)


# ------------------------------------------------------------------ distance
SAMPLINGS = [(1.0, 1.0)] + DT.SAMPLINGS
BOUNDS = (None, 1, 2.5, 12, 40)           # times the smaller sampling
# distance_to_ridges is fed lines: noise three times as often as each other kind and its two sparse densities twice as often as
# the dense ones, which also keeps the brute-force oracle in reach of more draws
DISTANCE_KINDS = ("background", "noise", "noise", "noise", "foreground", "smooth")
DISTANCE_DENSITIES = (0.02, 0.02, 0.1, 0.1, 0.41, 0.59, 0.9)


@dataclasses.dataclass(frozen=True)
class DistanceDraw:
    stack: Stack
    cyclic: bool = False
    sampling: tuple = (1.0, 1.0)
    bound: float | None = None

    @property
    def max_distance(self):
        return None if self.bound is None else self.bound * min(self.sampling)


def distance_draws():
    return builds(DistanceDraw, stack=stacks(DISTANCE_KINDS, DISTANCE_DENSITIES), cyclic=booleans(), sampling=sampled_from(SAMPLINGS),
                  bound=sampled_from(BOUNDS))


def brute_in_reach(mask):
    return mask.size * int(np.count_nonzero(CO.foreground(mask))) <= DT.CHUNK_ELEMS


def takes_the_brute_path(draw):
    return all(brute_in_reach(m) for m in draw.stack.masks())


def edt_reference(mask, cyclic, sampling, max_distance):
    """scipy's transform with the engine's two own rules applied: ``+inf`` on a plane without foreground and beyond the bound."""
    if not CO.foreground(mask).any():
        return np.full(mask.shape, np.inf)
    d = DT.scipy_edt(mask, cyclic, sampling)
    return d if max_distance is None else np.where(d <= max_distance, d, np.inf)


def nearest_is_a_nearest_pixel(mask, dist, nearest, cyclic, sampling):
    """What is asked of ``nearest`` where the brute-force oracle is out of reach: -1 exactly where the distance is ``+inf``;
    elsewhere a foreground pixel whose cost, in scipy's expression, is the square the distance is the root of."""
    ny, nx = mask.shape
    far = np.isposinf(dist).ravel()
    near = nearest.ravel().astype(np.int64)
    if not np.array_equal(near < 0, far) or (near[far] != -1).any() or (near >= mask.size).any():
        return False
    fg = CO.foreground(mask).ravel()
    r, c = np.divmod(np.flatnonzero(~far), nx)
    fr, fc = np.divmod(near[~far], nx)
    dc = np.abs(c - fc)
    if cyclic:
        dc = np.minimum(dc, nx - dc)
    return bool(fg[near[~far]].all()) and np.array_equal(np.sqrt(DT.cost_of(r - fr, dc, sampling)), dist.ravel()[~far])


def distance_reference(draw):
    """``(dist stack, [nearest or None])``: ``nearest`` from ``distance.brute`` where it is in reach."""
    masks = draw.stack.masks()
    dist = np.stack([edt_reference(m, draw.cyclic, draw.sampling, draw.max_distance) for m in masks])
    nearest = [DT.brute(m, draw.cyclic, draw.sampling, draw.max_distance)[1] if brute_in_reach(m) else None for m in masks]
    return dist, nearest


# ------------------------------------------------------------------ morphology
NEIGHBOURS = ((-1, -1), (-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1), (0, -1))    # bit k of the index: NW N NE E SE S SW W
# thinning is for blobs and bands: smooth planes as often as the three other kinds together
THIN_KINDS = ("smooth", "smooth", "smooth", "noise", "foreground", "background")


def scipy_structure(structure):
    """The 3 x 3 structuring element with which ``scipy.ndimage.binary_dilation`` sets a pixel when a neighbour named in the
    bitmask is set: scipy looks from the set pixel, the bitmask from the pixel to be set, hence the point reflection."""
    s = np.zeros((3, 3), dtype=bool)
    s[1, 1] = True
    for k, (dr, dc) in enumerate(NEIGHBOURS):
        if structure >> k & 1:
            s[1 - dr, 1 - dc] = True
    return s


def dilate_reference(fg, structure, iterations, cyclic):
    """The header's sentence, iterated: a pixel is set when it is, or when a neighbour named in ``structure`` is."""
    fg = np.asarray(fg, dtype=bool)
    for _ in range(iterations):
        fg = fg | ((SK.index(fg, cyclic) & structure) != 0)
    return fg


def mirrored(structure):
    """The structure reflected left to right: NW <-> NE, E <-> W, SE <-> SW."""
    swap = {0: 2, 2: 0, 3: 7, 7: 3, 4: 6, 6: 4, 1: 1, 5: 5}
    return sum(1 << swap[k] for k in range(8) if structure >> k & 1)


@dataclasses.dataclass(frozen=True)
class Table:
    kind: str                  # "shipped", "redrawn" (a shipped table with `entries` codes redrawn), "sparse"
    method: str = "guohall"
    entries: int = 0
    density: float = 0.1       # of "sparse": the probability that an entry is not 0
    salt: int = 0

    def codes(self):
        rng = np.random.default_rng([SEED, self.salt, self.entries])
        if self.kind == "sparse":
            return np.where(rng.random(256) < self.density, rng.integers(1, 4, 256), 0).astype(np.uint8)
        t = SK.table(self.method).copy()
        if self.kind == "redrawn":
            t[rng.choice(256, self.entries, replace=False)] = rng.integers(0, 4, self.entries)
        return t


def tables():
    salt = integers(0, 2 ** 16)
    sparse = builds(Table, kind=just("sparse"), density=sampled_from([0.1, 0.3]), salt=salt)
    # sparse tables twice: they are the ones that reach entries no shipped rule sets, and that act on a plane one pixel wide
    return one_of(builds(Table, kind=just("shipped"), method=sampled_from(SK.METHODS)),
                  builds(Table, kind=just("redrawn"), method=sampled_from(SK.METHODS), entries=integers(1, 16), salt=salt),
                  sparse, sparse)


@dataclasses.dataclass(frozen=True)
class ThinDraw:
    stack: Stack
    table: Table
    cyclic: bool = False
    max_iterations: int | None = None
    per_launch: int | None = None


def thin_draws():
    return builds(ThinDraw, stack=stacks(THIN_KINDS), table=tables(), cyclic=booleans(),
                  max_iterations=sampled_from([None, 1, 2, 5]), per_launch=sampled_from([None, 1, 2, 3, 4]))


def thin_reference(draw):
    codes = draw.table.codes()
    return np.stack([SK.thin(m, codes, draw.cyclic, draw.max_iterations)[0] for m in draw.stack.masks()])


@dataclasses.dataclass(frozen=True)
class DilateDraw:
    stack: Stack
    structure: int
    iterations: int = 1
    cyclic: bool = False
    per_launch: int | None = None


def dilate_draws():
    return builds(DilateDraw, stack=stacks(), structure=integers(1, 255), iterations=integers(1, 12), cyclic=booleans(),
                  per_launch=sampled_from([None, 1, 2, 3, 4, 5, 6, 7, 8]))


# every neighbour alone, on a plane one pixel more than a tile both ways and on a narrow one, cyclic and not, over a launch's
# eight sub-steps and past them
DILATE_EXPLICIT = tuple(DilateDraw(Stack(49, 113, (Plane("noise", 0.02, k),)) if k % 2 else Stack(17, 5, (Plane("noise", 0.1, k),), "float32"),
                                   1 << k, 3 + 2 * k, k % 4 >= 2, None if k < 4 else 3) for k in range(8))


def dilate_draw_reference(draw):
    return np.stack([dilate_reference(CO.foreground(m), draw.structure, draw.iterations, draw.cyclic)
                     for m in draw.stack.masks()]).astype(np.uint8)


# ------------------------------------------------------------------ tracks: labels through time, spans, the lifetime filter
TRC = constants("tracks.hip", "TR_THREADS", "TR_ITEMS", "TS_ITEMS")
TR_TILE, TS_TILE = TRC["TR_THREADS"] * TRC["TR_ITEMS"], TRC["TR_THREADS"] * TRC["TS_ITEMS"]
TRACK_NY_MAX, TRACK_NX_MAX, TRACK_PLANES = 48, 80, 6       # the csgraph oracle at reach 16 stays near 0.03 s a draw
TRACK_EDGES = sorted({1, 2, 3, 4, 5} | {31, 32, 33, 34, 35})         # around twice the largest reach
TRACK_MAX_REACH = 16                                                  # LC_TRACK_MAX_REACH of include/lcs_hip.h
REACHES = (0, 1, 2, 3, 8, 15, 16)
# sparse planes are the ones that tell: a dense plane at a large reach is one track
TRACK_KINDS = ("noise",) * 10 + ("smooth", "background", "foreground")
TRACK_DENSITIES = (0.02,) * 4 + (0.1,) * 4 + (0.41,)


@dataclasses.dataclass(frozen=True)
class TrackDraw:
    stack: Stack                       # the record: its planes are the times
    connectivity: int = 2
    cyclic: bool = False
    reach: int = 1
    capacity: str = "largest"
    quantiles: tuple = (0.5, 0.5)      # where in the reference's sorted durations / volumes min_duration / min_volume are taken
    fill: float = 0.0


def side_of(edges, most):
    return one_of(sampled_from([e for e in edges if e <= most]), integers(1, most))


def track_draws():
    record = builds(Stack, ny=side_of(TRACK_EDGES, TRACK_NY_MAX), nx=side_of(TRACK_EDGES, TRACK_NX_MAX),
                    planes=tuples_of(planes(TRACK_KINDS, TRACK_DENSITIES), 1, TRACK_PLANES), dtype=sampled_from(["float32", "float64"]))
    return builds(TrackDraw, stack=record, connectivity=sampled_from([1, 2]), cyclic=booleans(),
                  reach=one_of(sampled_from(REACHES), integers(0, TRACK_MAX_REACH)), capacity=sampled_from(CAPACITIES),
                  quantiles=tuples(*[sampled_from([0.0, 0.25, 0.5, 0.75, 1.0])] * 2), fill=sampled_from([0.0, -1.0, float("nan")]))


def _sparse(count, salt, densities=(0.1, 0.02)):
    return tuple(Plane("noise", densities[k % len(densities)], salt + k) for k in range(count))


def _window_draws():
    """Independent draws of ``nx`` and ``reach`` almost never meet: the widths 2 reach, 2 reach + 1 and 2 reach + 2, where a
    cyclic window that is "every column once" meets one that "one turn brings into the plane" -- cyclic for four reaches, and,
    for two of them, not cyclic (the window is then cut at both ends of every row)."""
    out, k = [], 0
    for cyclic, reaches in ((True, (1, 2, 8, 16)), (False, (1, 8))):
        for reach in reaches:
            for nx in (2 * reach, 2 * reach + 1, 2 * reach + 2):
                ny = {1: 48, 2: 47, 8: 33, 16: 21}[reach]
                out.append(TrackDraw(Stack(ny, nx, _sparse(2 + k % 2, 20 + k), ("float64", "float32")[k % 2]), 1 + k % 2, cyclic, reach,
                                     CAPACITIES[k % 3], ((0.5, 0.0), (0.0, 0.5), (0.75, 0.25))[k % 3], (0.0, float("nan"), -1.0)[k % 3]))
                k += 1
    return tuple(out)


# records of TR_TILE - 1, TR_TILE, TR_TILE + 1 and TS_TILE - 1, TS_TILE, TS_TILE + 1 voxels.  2047 = 23 x 89 and 2049 = 3 x 683
# have no other factors: these two records are the only ones wider than TRACK_NX_MAX (a row of 683 at reach 2 is cheap).
TRACK_TILE_RECORDS = ((11, 31, 3), (32, 32, 1), (5, 41, 5), (23, 89, 1), (32, 32, 2), (1, 683, 3))
TRACK_EXPLICIT = (
    *_window_draws(),
    *[TrackDraw(Stack(ny, nx, _sparse(nt, 60 + k, (0.1, 0.41)), ("float32", "float64")[k % 2]), 1 + k % 2, k % 3 == 0, (1, 2, 0)[k % 3],
                CAPACITIES[k % 3], (0.5, 0.5), 0.0) for k, (ny, nx, nt) in enumerate(TRACK_TILE_RECORDS)],
    # an empty plane between two others: nothing reaches across it, whatever the reach
    TrackDraw(Stack(33, 35, (Plane("noise", 0.1, 70), Plane("background"), Plane("noise", 0.1, 71))), 2, True, 16, "above", (0.5, 0.0), float("nan")),
    TrackDraw(Stack(5, 34, (Plane("noise", 0.41, 72), Plane("background", sprinkle=True), Plane("noise", 0.41, 73, True)), "float32"), 1, False, 1,
              "below", (0.0, 0.5), 0.0),
    # planes of fewer voxels than one thread of ts_spans_kernel walks (TS_ITEMS): the thread goes on into the next planes on the
    # same label, and what it alone knows of the track's last plane is its running ``tmax = t`` -- without that line no random draw
    # failed, because on a larger plane some other thread starts on the label in the last plane and reports it
    TrackDraw(Stack(1, 1, (Plane("foreground"),) * 6), 1, False, 0, "largest", (0.0, 0.0), 0.0),
    TrackDraw(Stack(1, 3, _sparse(5, 74, (0.9, 0.59)), "float32"), 2, True, 1, "above", (0.5, 0.0), float("nan")),
    TrackDraw(Stack(2, 3, _sparse(4, 75, (0.59, 0.41))), 2, False, 2, "largest", (1.0, 0.0), -1.0),
    # narrow cyclic planes of sparse noise at reach 0, 8-connected: much of what joins two pieces there is one diagonal step
    # across the seam (the ``r < ny - 1`` line of tr_merge_kernel), and nothing in the plane before joins them another way
    TrackDraw(Stack(48, 3, _sparse(2, 76, (0.41, 0.41))), 2, True, 0, "largest", (0.0, 0.25), 0.0),
    TrackDraw(Stack(48, 9, _sparse(3, 77, (0.1, 0.1)), "float32"), 2, True, 0, "above", (0.0, 0.5), float("nan")),
    TrackDraw(Stack(47, 5, _sparse(2, 78, (0.41, 0.1))), 2, True, 0, "below", (0.0, 0.5), -1.0),
)


@functools.lru_cache(maxsize=None)
def _tracks(stack, connectivity, cyclic, reach):
    from tests import tracks as TR
    lab, n = TR.label(stack.masks(), connectivity, cyclic, reach)
    lab.setflags(write=False)
    return lab, n, TR.spans(lab, n)


def tracks_reference(draw):
    """``(labels, count, spans)`` of the record by ``tracks.label`` / ``tracks.spans``, computed once per draw and read-only."""
    return _tracks(draw.stack, draw.connectivity, draw.cyclic, draw.reach)


def track_spans_reference(draw):
    """``(n_max, slots, spans)``: ``n_max`` the argument (None: the count, read back by the engine), ``slots`` the length of the
    engine's arrays, ``spans`` cut to the tracks the call measures and padded to ``slots`` with what include/lcs_hip.h promises
    for entries past the count: first = last = -1, duration = volume = 0."""
    _, n, s = tracks_reference(draw)
    n_max = capacity_of(draw, [n])
    slots = max(1, n if n_max is None else n_max)
    k = min(n, slots)
    pad = slots - k
    return n_max, slots, dict(first=np.concatenate([s["first"][:k], np.full(pad, -1, np.int32)]),
                              last=np.concatenate([s["last"][:k], np.full(pad, -1, np.int32)]),
                              duration=np.concatenate([s["duration"][:k], np.zeros(pad, np.int32)]),
                              volume=np.concatenate([s["volume"][:k], np.zeros(pad, np.int64)]))


def track_filter_reference(draw):
    """``(min_duration, min_volume, filtered record)``: each threshold is a value of the reference's own integer table at the
    drawn quantile, so ``>=`` at the value itself is decided."""
    lab, n, s = tracks_reference(draw)
    thresholds = []
    for key, q in zip(("duration", "volume"), draw.quantiles):
        vals = np.unique(s[key])
        thresholds.append(int(vals[int(round(q * (len(vals) - 1)))]) if len(vals) else 1)
    # tracks.filtered on the labels and spans the draw already has (tests/test_mask_draws.py holds the two together)
    masks = draw.stack.masks()
    table = np.concatenate([[False], (s["duration"] >= thresholds[0]) & (s["volume"] >= thresholds[1])])
    return thresholds[0], thresholds[1], np.where(table[lab], masks, np.asarray(draw.fill, dtype=masks.dtype))


# ------------------------------------------------------------------ the great-circle distance
SDC = constants("sphere_distance.hip", "SD_THREADS", "SD_CHUNK")
SD_SIDE_MAX = 520
SD_LONG = sorted({k * SDC["SD_THREADS"] + d for k in (1, 2) for d in (-1, 0, 1)})         # rows or columns around one and two workgroups
SD_WAVE = [1, 2, 3, 63, 64, 65]                                                          # the middle family's sides: around the wave
SD_EDGES = sorted(set(SD_LONG) | set(SD_WAVE))
SD_DENSITIES = (0.02, 0.02, 0.1, 0.1, 0.41)       # a list then crosses SD_CHUNK in many draws, and the brute-force oracle stays cheap
SD_GRIDS = ("global", "poles", "regional", "permuted", "closed")
SD_BOUNDS = (None, 0.5, 1, 2.5, 12, 40, "pi")     # row steps of a global grid of the plane's ny; "pi": pi radius, which is no bound


@dataclasses.dataclass(frozen=True)
class SphereDistanceDraw:
    stack: Stack
    grid: str = "global"
    bound: float | str | None = None
    radius: float = 6371000.0

    def coordinates(self):
        """``(lat, lon)`` in degrees.  ``global``: tests/sphere_distance.py's GRID.  ``poles``: rows exactly at both poles.
        ``regional``: the non-uniform regional grid of tests/test_sphere_distance_gpu.py.  ``permuted``: GRID with its latitudes
        in a seeded random order.  ``closed``: longitudes -180 .. 180 inclusive, the first and the last column one meridian."""
        from tests import sphere_distance as SD
        ny, nx = self.stack.ny, self.stack.nx
        lat, lon = SD.GRID(ny, nx)
        if self.grid == "poles":
            lat = np.linspace(-90.0, 90.0, ny)
        elif self.grid == "regional":
            lat, lon = np.degrees(np.arcsin(np.linspace(-0.7, 0.95, ny))), np.linspace(-90.0, -32.0, nx)
        elif self.grid == "permuted":
            lat = lat[np.random.default_rng([SEED, ny]).permutation(ny)]
        elif self.grid == "closed":
            lon = np.linspace(-180.0, 180.0, nx)
        return lat, lon

    @property
    def max_distance(self):
        if self.bound is None:
            return None
        return np.pi * self.radius if self.bound == "pi" else self.bound * np.pi * self.radius / self.stack.ny


def sphere_distance_draws():
    few = one_of(sampled_from([1, 2, 3]), integers(1, 12))
    long = one_of(sampled_from(SD_LONG), integers(1, SD_SIDE_MAX))
    some = planes(DISTANCE_KINDS, SD_DENSITIES)
    dtype = sampled_from(["float32", "float64"])
    tall = builds(Stack, ny=long, nx=few, planes=tuples_of(some, 1, 3), dtype=dtype)
    # narrow and tall twice: more rows than a workgroup has threads is what the band kernel and the scan have never met
    stack = one_of(tall, tall,
                   builds(Stack, ny=few, nx=long, planes=tuples_of(some, 1, 3), dtype=dtype),            # wide and short
                   builds(Stack, ny=one_of(sampled_from(SD_WAVE), integers(1, 70)), nx=one_of(sampled_from(SD_WAVE), integers(1, 132)),
                          planes=tuples_of(some, 1, 3), dtype=dtype))
    # every bound twice as often as no bound and as pi radius: the band kernel runs under a bound only
    bound = sampled_from([b for b in SD_BOUNDS for _ in range(2 if isinstance(b, (int, float)) else 1)])
    return builds(SphereDistanceDraw, stack=stack, grid=sampled_from(SD_GRIDS), bound=bound,
                  radius=sampled_from([6371000.0, 1.0]))


# more rows than two workgroups have threads under a bound, one and two columns wide: a third round of the band kernel's loop, a
# workgroup whose band is the union of 256 row bands; and the same lengths as one short row
SPHERE_DISTANCE_EXPLICIT = (
    SphereDistanceDraw(Stack(513, 2, (Plane("noise", 0.1, 80), Plane("noise", 0.41, 81, True))), "closed", 2.5),
    SphereDistanceDraw(Stack(515, 1, (Plane("noise", 0.02, 82),), "float32"), "permuted", 12, 1.0),
    SphereDistanceDraw(Stack(257, 3, (Plane("noise", 0.1, 83), Plane("background"), Plane("smooth", salt=84)), "float32"), "poles", 0.5),
    SphereDistanceDraw(Stack(2, 513, (Plane("noise", 0.41, 85),)), "regional", 1, 1.0),
)


@functools.lru_cache(maxsize=None)
def sphere_distance_reference(draw):
    """``[(dist, nearest, cost)]`` of every plane by ``sphere_distance.brute``, computed once per draw and read-only."""
    from tests import sphere_distance as SD
    lat, lon = draw.coordinates()
    out = []
    for m in draw.stack.masks():
        ref = SD.brute(m, lat, lon, draw.max_distance, draw.radius)
        for a in ref:
            a.setflags(write=False)
        out.append(ref)
    return out


def is_bounded(draw):
    """The bound is one: below half the circumference."""
    from tests import sphere_distance as SD
    return SD.chord2_of(draw.max_distance, draw.radius) is not None


# ------------------------------------------------------------------ sphere sums, over the "components" sequence
SPHERE_VARIANTS = ("uniform", "gauss", "global")
SPHERE_RADIUS = 6371000.0


def sphere_variant(draw):
    return SPHERE_VARIANTS[draw.salt % len(SPHERE_VARIANTS)]


def sphere_grid(draw):
    from tests import sphere_props as SP
    return SP.coordinates((draw.stack.ny, draw.stack.nx), sphere_variant(draw))


def sphere_refused(draw):
    """A side of 1 has no width: Engine.sphere_cell_tables refuses it."""
    return min(draw.stack.ny, draw.stack.nx) < 2


@functools.lru_cache(maxsize=None)
def _sphere_full(key):
    """Per plane ``(labels, n, sums, props, bounds)`` of ALL labels of the plane (what the filter decides on)."""
    from tests import sphere_props as SP
    lat, lon = sphere_grid(key)
    v = intensity_of(key)
    out = []
    for (lab, n), vi in zip(labels_reference(key.stack, key.connectivity, key.cyclic), v):
        s = SP.sums(lab, n, lat, lon, vi.astype(np.float64), key.cyclic)
        p = SP.props(s, lat, lon, SPHERE_RADIUS)
        out.append((lab, n, s, p, SP.bounds(s, p, SPHERE_RADIUS)))
    return out


def _key(draw):
    """The fields the sphere references depend on (no NaN fill among them: the key compares equal to itself)."""
    return ComponentDraw(draw.stack, draw.connectivity, draw.cyclic, draw.capacity, draw.nan_intensity, salt=draw.salt)


def sphere_sums_reference(draw):
    """``(intensity, n_max, slots, (lat, lon), planes)`` in the shape of ``sums_reference``: per plane ``measured`` and
    ``sphere_props.sums`` / ``props`` / ``bounds`` cut to the labels the plane measures and padded to ``slots`` with what
    include/lcs_hip.h promises for entries without a component: area 0, root -1, NaN elsewhere, sums 0.  None where a side is 1."""
    from tests import sphere_props as SP
    if sphere_refused(draw):
        return None
    key = _key(draw)
    full = _sphere_full(key)
    counts = [n for _, n, *_ in full]
    n_max = capacity_of(draw, counts)
    slots = max(1, max(counts) if n_max is None else n_max)
    lat, lon = sphere_grid(draw)
    out = []
    for lab, n, s, _, _ in full:
        k = min(n, slots)
        pad = slots - k
        cut = dict(root=np.concatenate([s["root"][:k], np.full(pad, -1, np.int32)]),
                   count=np.concatenate([s["count"][:k], np.zeros(pad, np.int64)]),
                   sums=np.concatenate([s["sums"][:, :k], np.zeros((11, pad))], axis=1),
                   abs=np.concatenate([s["abs"][:, :k], np.zeros((11, pad))], axis=1),
                   max=np.concatenate([s["max"][:k], np.full(pad, np.nan)]),
                   min=np.concatenate([s["min"][:k], np.full(pad, np.nan)]))
        p = SP.props(cut, lat, lon, SPHERE_RADIUS)
        out.append(dict(measured=k, sums=cut, props=p, bounds=SP.bounds(cut, p, SPHERE_RADIUS)))
    return intensity_of(draw), n_max, slots, (lat, lon), out


def sphere_admitted(plane):
    """Which labels of a plane of ``sphere_sums_reference`` the direction checks admit, on the reference alone: ``(centroid,
    orientation, multi)`` as boolean arrays over the slots.  The centroid where ``rho >= 1e-5`` and the bound on its turn is in
    its linear range (``<= 1e-3``); the orientation on multi-pixel labels whose major axis is a direction (``e1 - e2 >= 0.1
    e1``), whose Davis-Kahan bound is in its range (``E_over_gap <= 0.25``) and whose centroid, which that bound is
    evaluated at, is admitted."""
    s, p, b = plane["sums"], plane["props"], plane["bounds"]
    with np.errstate(invalid="ignore"):
        some, multi = s["count"] > 0, s["count"] > 1
        centroid = some & (p["rho"] >= 1e-5) & (b["centroid_turn"] <= 1e-3)
        e1, e2 = p["e"][:, 0], p["e"][:, 1]
        oriented = multi & centroid & (e1 - e2 >= 0.1 * e1) & (b["E_over_gap"] <= 0.25)
    return centroid, oriented, multi


def sphere_filter_reference(draw):
    """``(thresholds, filtered stack)`` of ``filter_components(metric='sphere')`` with the draw's criteria, or None where a side
    is 1 or no area threshold is decided.  ``max_intensity`` is exact: its threshold is one of the reference's own values at the
    drawn quantile.  ``area`` is a float64 sum: its threshold is the midpoint between two consecutive distinct reference areas
    (0, the area of a label without a pixel, counts as the one below the smallest), the first pair at or above the drawn
    quantile whose gap exceeds eight times the sum of their two area bounds and whose midpoint is further from every label's
    area than that label's bound -- so the device's ``>=`` is decided."""
    if sphere_refused(draw):
        return None
    full = _sphere_full(_key(draw))
    thresholds = []
    for k, q in zip(draw.criteria, draw.quantiles):
        if k == "max_intensity":
            vals = np.concatenate([s["max"] for _, _, s, _, _ in full])
            vals = np.unique(vals[np.isfinite(vals)])
            thresholds.append(float(vals[int(round(q * (len(vals) - 1)))]) if len(vals) else 1.0)
            continue
        area = np.concatenate([p["area"] for _, _, _, p, _ in full])
        bound = np.concatenate([b["area"] for *_, b in full])
        if not area.size:
            thresholds.append(1.0)                     # nothing to keep or drop: any threshold is decided
            continue
        vals = np.unique(area)
        worst = np.array([bound[area == a].max() for a in vals])
        # below the smallest area lies 0, the area of a label without a pixel, exactly: one label alone is decided too
        first = int(round(q * (len(vals) - 1))) + 1
        vals, worst = np.concatenate([[0.0], vals]), np.concatenate([[0.0], worst])
        found = None
        for i in range(first, len(vals)):
            th = (vals[i - 1] + vals[i]) / 2
            if vals[i] - vals[i - 1] > 8 * (worst[i - 1] + worst[i]) and (np.abs(area - th) > bound).all():
                found = float(th)
                break
        if found is None:
            return None
        thresholds.append(found)
    # sphere_props.filtered on the labels and properties the draw already has (tests/test_mask_draws.py holds the two together)
    masks = draw.stack.masks()
    want = []
    for m, (lab, n, s, p, _) in zip(masks, full):
        keep = np.ones(n, bool)
        for k, th in zip(draw.criteria, thresholds):
            with np.errstate(invalid="ignore"):
                keep &= (s["max"] if k == "max_intensity" else p[k]) >= th
        want.append(np.where(np.concatenate([[False], keep])[lab], m, np.asarray(draw.fill, dtype=masks.dtype)))
    return thresholds, np.stack(want)



# ------------------------------------------------------------------ the six sequences, by name
DRAWS = {"components": (component_draws, COMPONENT_EXPLICIT), "distance": (distance_draws, ()), "thin": (thin_draws, ()),
         "dilate": (dilate_draws, DILATE_EXPLICIT), "tracks": (track_draws, TRACK_EXPLICIT),
         "sphere_distance": (sphere_distance_draws, SPHERE_DISTANCE_EXPLICIT)}
_MASKS = dict(ny=NY_MAX, nx=NX_MAX, planes=3, kinds=KINDS, densities=DENSITIES, edges=EDGES)
# what the draws of a SPACE stay inside, by sequence (the two track records of 2047 and 2049 voxels alone are wider)
LIMITS = {"components": _MASKS, "distance": _MASKS, "thin": _MASKS, "dilate": _MASKS,
          "tracks": dict(ny=TRACK_NY_MAX, nx=TRACK_NX_MAX, planes=TRACK_PLANES, kinds=KINDS, densities=DENSITIES, edges=TRACK_EDGES),
          "sphere_distance": dict(ny=SD_SIDE_MAX, nx=SD_SIDE_MAX, planes=3, kinds=KINDS, densities=DENSITIES, edges=SD_EDGES)}


def run(name, body):
    """``body(draw)`` over the named sequence as the environment asks for it: what a GPU test calls."""
    space, explicit = DRAWS[name]
    each(name, space(), body, explicit)


@functools.lru_cache(maxsize=None)
def drawn(name):
    """The derandomised draws of the named sequence, explicit ones first: what ``run`` passes to its body by default."""
    space, explicit = DRAWS[name]
    return tuple(collect(name, space(), explicit))
