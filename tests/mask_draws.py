"""TEST SUPPORT -- randomised draws for the ridge-mask kernels (csrc/components.hip, csrc/distance.hip, csrc/morphology.hip) and
the numpy / scipy reference of every draw.  No GPU here: tests/test_mask_draws.py pins the references and the conditions the
draws must meet, tests/test_mask_hypothesis_gpu.py runs the same draws through the engine.

- ``EDGES``: the plane sides worth drawing on purpose -- 1 .. 5 and ``k - 1, k, k + 1`` around the tile constants, which are read
  out of the ``.hip`` sources (``constants``), so a kernel whose tile changes moves the draws with it.
- ``Plane`` / ``Stack``: one plane is white noise (``components._random``), thresholded smoothed noise (``skeleton._smooth``), all
  background or all foreground, optionally sprinkled with NaN (background) and negative values (foreground; an all-background
  plane gets the NaN only and stays empty); a stack is 1 .. 3 planes of one shape and dtype.  A draw holds parameters only; the
  arrays are built from them on demand (``Stack.masks``), so a failing draw prints as something one can paste back.
- ``ComponentDraw`` / ``DistanceDraw`` / ``ThinDraw`` / ``DilateDraw`` and their strategies, and ``*_reference`` for each, built
  on tests/components.py, tests/distance.py and tests/skeleton.py.
- ``dilate_reference`` / ``scipy_structure``: dilation by any of the 255 structures of ``lc_morph_args.structure``.
- ``Space``: a hypothesis strategy and a plain seeded sampler over the same values, built together by combinators named after
  hypothesis's.  ``each`` runs a body over the draws of a space: by default the sampler's, handed to hypothesis as explicit
  examples, so that the CPU test that checks the conditions and the GPU test see the same draws; with ``LCS_HYP_RANDOM``
  hypothesis's own.
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


# ------------------------------------------------------------------ the four sequences, by name
DRAWS = {"components": (component_draws, COMPONENT_EXPLICIT), "distance": (distance_draws, ()), "thin": (thin_draws, ()),
         "dilate": (dilate_draws, DILATE_EXPLICIT)}


def run(name, body):
    """``body(draw)`` over the named sequence as the environment asks for it: what a GPU test calls."""
    space, explicit = DRAWS[name]
    each(name, space(), body, explicit)


@functools.lru_cache(maxsize=None)
def drawn(name):
    """The derandomised draws of the named sequence, explicit ones first: what ``run`` passes to its body by default."""
    space, explicit = DRAWS[name]
    return tuple(collect(name, space(), explicit))
