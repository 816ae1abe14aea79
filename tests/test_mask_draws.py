"""The randomised mask draws without a GPU: tests/mask_draws.py's references pinned against scipy by another route on the very
draws tests/test_mask_hypothesis_gpu.py runs, the sides drawn on purpose against the tile constants of the kernels, and the
conditions that make those draws worth running -- every one of them a statement about the draws and their references, none
about the engine."""
import os
import re

import numpy as np
import pytest

from lagrangiancoherence_amd import build
from tests import components as CO
from tests import distance as DT
from tests import mask_draws as MD
from tests import skeleton as SK


# ------------------------------------------------------------------ the draws themselves
def test_the_sides_drawn_on_purpose_follow_the_constants_of_the_kernels():
    assert MD.TILE_SIDES == [8, 16, 48, 56, 64, 112, 120, 128, 256]
    assert MD.EDGES == sorted({1, 2, 3, 4, 5} | {k + d for k in (8, 16, 48, 56, 64, 112, 120, 128, 256) for d in (-1, 0, 1)})
    assert (MD.CC_TILE, MD.CS_TILE) == (1024, 2048)
    assert (MD.DTC["DT_SEG"], MD.DTC["DT_THREADS"]) == (64, 256) and MD.MO == {"MO_HALO": 8, "MO_TW": 112, "MO_TH": 48}
    src = {f: build._strip_comments(open(os.path.join(build.CSRC, f)).read()) for f in ("components.hip", "distance.hip", "morphology.hip")}
    # the derived sides are the kernels' own expressions
    assert "constexpr int MO_LW = MO_TW + 2 * MO_HALO;" in src["morphology.hip"] and "constexpr int MO_LH = MO_TH + 2 * MO_HALO;" in src["morphology.hip"]
    assert "constexpr int CC_TILE = CC_THREADS * CC_ITEMS;" in src["components.hip"] and "constexpr int CS_TILE = CC_THREADS * CS_ITEMS;" in src["components.hip"]
    assert re.search(r"ctiles = \(a->nx \+ DT_THREADS - 1\) / DT_THREADS", src["distance.hip"])
    # what the largest plane reaches: three row segments and two column passes of the distance transform, a 3 x 3 grid of
    # morphology tiles, 37 label tiles
    ny, nx = MD.NY_MAX, MD.NX_MAX
    assert -(-ny // MD.DTC["DT_SEG"]) == 3 and -(-nx // MD.DTC["DT_THREADS"]) == 2
    assert (-(-ny // MD.MO["MO_TH"]), -(-nx // MD.MO["MO_TW"])) == (3, 3) and -(-ny * nx // MD.CC_TILE) == 37
    assert max(MD.EDGES) <= nx and max(e for e in MD.EDGES if e <= ny) == 129


@pytest.mark.parametrize("name", list(MD.DRAWS))
def test_a_sequence_is_the_same_whenever_it_is_asked_for_and_stays_inside_its_limits(name):
    strategy, explicit = MD.DRAWS[name]
    draws = MD.drawn(name)
    assert list(map(repr, MD.collect(name, strategy(), explicit))) == list(map(repr, draws))        # (repr: a NaN fill equals itself)
    assert len(draws) == MD.EXAMPLES + len(explicit) and list(map(repr, draws[:len(explicit)])) == list(map(repr, explicit))
    for d in draws:
        s = d.stack
        assert 1 <= s.ny <= MD.NY_MAX and 1 <= s.nx <= MD.NX_MAX and 1 <= len(s.planes) <= 3 and s.dtype in ("float32", "float64")
        m = s.masks()
        assert m.shape == (len(s.planes), s.ny, s.nx) and m.dtype == np.dtype(s.dtype)
    sides = {v for d in draws for v in (d.stack.ny, d.stack.nx)}
    assert sides & set(MD.EDGES) and sides - set(MD.EDGES)              # sides drawn on purpose and sides in between
    kinds = {p.kind for d in draws for p in d.stack.planes}
    assert kinds == set(MD.KINDS)
    assert {d.stack.dtype for d in draws} == {"float32", "float64"} and {len(d.stack.planes) for d in draws} == {1, 2, 3}


def test_a_sprinkled_plane_holds_nan_and_negative_values_and_an_empty_one_stays_empty():
    m = MD.Plane("noise", 0.41, 3, True).mask(67, 130)
    assert np.isnan(m).any() and (m < 0).any() and (m == 1).any() and (m == 0).any()
    assert not CO.foreground(MD.Plane("background", sprinkle=True).mask(67, 130)).any()
    assert np.isnan(MD.Plane("background", sprinkle=True).mask(67, 130)).any()
    assert CO.foreground(MD.Plane("foreground").mask(3, 5)).all()


@pytest.mark.parametrize("name", list(MD.DRAWS))
def test_what_hypothesis_generates_from_a_space_stays_inside_the_same_limits(name):
    """The strategy half of a space (what LCS_HYP_RANDOM explores with) beside its sampler half."""
    space, _ = MD.DRAWS[name]
    seen = []

    def body(d):
        s = d.stack
        assert type(d) is type(MD.drawn(name)[-1])
        assert 1 <= s.ny <= MD.NY_MAX and 1 <= s.nx <= MD.NX_MAX and 1 <= len(s.planes) <= 3 and s.dtype in ("float32", "float64")
        assert all(p.kind in MD.KINDS and p.density in MD.DENSITIES for p in s.planes)
        seen.append(d)
    MD.each(name, space(), body, examples=25, derandomize=False, scale=1)
    assert len(seen) >= 20


# ------------------------------------------------------------------ dilation
SINGLE = [1 << k for k in range(8)]
TWELVE = SINGLE + [2 + 8, 1 + 16 + 128, 170, 255]


@pytest.mark.parametrize("structure", TWELVE)
def test_the_reflected_structure_makes_scipy_dilate_as_the_header_says(structure):
    from scipy import ndimage
    fg = CO.foreground(SK.mask_of("noise-67x130-0.3")) & (np.random.default_rng([MD.SEED, structure]).random((67, 130)) < 0.1)
    for iterations in (1, 4):
        want = ndimage.binary_dilation(fg, MD.scipy_structure(structure), iterations)
        assert np.array_equal(MD.dilate_reference(fg, structure, iterations, False), want)
    if structure in SINGLE:          # one neighbour: the plane moves one pixel against it, and nothing else happens
        dr, dc = MD.NEIGHBOURS[SINGLE.index(structure)]
        moved = np.zeros_like(fg)
        rows, cols = np.nonzero(fg)
        ok = (rows - dr >= 0) & (rows - dr < 67) & (cols - dc >= 0) & (cols - dc < 130)
        moved[rows[ok] - dr, cols[ok] - dc] = True
        assert np.array_equal(MD.dilate_reference(fg, structure, 1, False), fg | moved)


def _tiles_for(iterations, nx):
    """An odd number of copies, three where nothing travels further than one copy."""
    return 2 * max(1, -(-iterations // nx)) + 1


def test_dilate_reference_equals_scipy_on_every_dilation_draw():
    from scipy import ndimage
    for d in MD.drawn("dilate"):
        got = MD.dilate_draw_reference(d)
        for m, g in zip(d.stack.masks(), got):
            fg, st = CO.foreground(m), MD.scipy_structure(d.structure)
            if d.cyclic:
                k, nx = _tiles_for(d.iterations, d.stack.nx), d.stack.nx
                want = ndimage.binary_dilation(np.tile(fg, (1, k)), st, d.iterations)[:, (k // 2) * nx:(k // 2 + 1) * nx]
            else:
                want = ndimage.binary_dilation(fg, st, d.iterations)
            assert g.dtype == np.uint8 and np.array_equal(g.astype(bool), want), d
    assert _tiles_for(12, 270) == 3 and _tiles_for(12, 5) == 7 and _tiles_for(5, 5) == 3


def test_the_dilation_draws_tell_west_from_east():
    draws = MD.drawn("dilate")
    alone = {d.structure for d in draws if d.structure in SINGLE}
    assert alone == set(SINGLE)                                           # every neighbour bit alone, at least once
    asymmetric = [d for d in draws if MD.mirrored(d.structure) != d.structure]
    assert 4 * len(asymmetric) >= len(draws)
    assert MD.mirrored(8) == 128 and MD.mirrored(1 + 64) == 4 + 16 and MD.mirrored(2 + 32) == 2 + 32
    # and on such a draw the mirrored structure gives another plane: a swap of W and E in the kernel could not hide
    differs = sum(not np.array_equal(MD.dilate_draw_reference(d),
                                     MD.dilate_draw_reference(MD.DilateDraw(d.stack, MD.mirrored(d.structure), d.iterations, d.cyclic)))
                  for d in asymmetric)
    assert 4 * differs >= len(draws)
    assert {d.cyclic for d in draws} == {False, True} and {d.per_launch for d in draws} >= {None, 1, 8}
    assert max(d.iterations for d in draws) > MD.MO["MO_HALO"]           # more than one launch can do


# ------------------------------------------------------------------ thinning
def test_the_thinning_tables_are_what_they_are_called():
    for method in SK.METHODS:
        assert np.array_equal(MD.Table("shipped", method).codes(), SK.table(method))
        t = MD.Table("redrawn", method, entries=16, salt=5).codes()
        assert 0 < np.count_nonzero(t != SK.table(method)) <= 16 and t.max() <= 3
    for density in (0.1, 0.3):
        share = np.mean([np.count_nonzero(MD.Table("sparse", density=density, salt=s).codes()) for s in range(40)]) / 256
        assert abs(share - density) < 0.03
    t = MD.Table("sparse", density=0.3, salt=1).codes()
    assert t.dtype == np.uint8 and set(np.unique(t)) == {0, 1, 2, 3}
    kinds = {d.table.kind for d in MD.drawn("thin")}
    assert kinds == {"shipped", "redrawn", "sparse"}


def test_most_thinning_draws_end_between_nothing_and_everything():
    """On at least 80 % of the thinning draws with a non-empty plane the reference neither deletes the stack nor leaves it."""
    total = good = 0
    for d in MD.drawn("thin"):
        fg = CO.foreground(d.stack.masks())
        if not fg.any():
            continue
        total += 1
        want = MD.thin_reference(d)
        assert want.dtype == np.uint8 and not (want.astype(bool) & ~fg).any()      # thinning only deletes
        good += bool(want.any()) and not np.array_equal(want.astype(bool), fg)
    print(f"thinning draws that test something: {good} of {total}")
    assert total >= 30 and good >= 0.8 * total
    draws = MD.drawn("thin")
    assert {d.max_iterations for d in draws} == {None, 1, 2, 5} and {d.per_launch for d in draws} >= {None, 1, 4}
    assert {d.cyclic for d in draws} == {False, True}


# ------------------------------------------------------------------ distance
def test_brute_equals_scipy_on_every_draw_it_reaches_and_it_reaches_half_of_them():
    draws = MD.drawn("distance")
    reached = [d for d in draws if MD.takes_the_brute_path(d)]
    print(f"distance draws the brute-force oracle reaches: {len(reached)} of {len(draws)}")
    assert 2 * len(reached) >= len(draws)
    non_trivial = 0
    for d in reached:
        dist, nearest = MD.distance_reference(d)
        for m, want, near in zip(d.stack.masks(), dist, nearest):
            got_d, got_n = DT.brute(m, d.cyclic, d.sampling, d.max_distance)
            assert np.array_equal(got_d, want), d                         # scipy, with the bound and the empty-plane rule
            assert near is not None and np.array_equal(got_n, near)
            assert MD.nearest_is_a_nearest_pixel(m, want, near, d.cyclic, d.sampling), d
            fg = CO.foreground(m)
            non_trivial += bool(fg.any() and not fg.all())
    assert non_trivial >= len(reached) // 2
    assert {d.cyclic for d in draws} == {False, True} and {d.sampling for d in draws} == set(MD.SAMPLINGS)
    assert {d.bound for d in draws} == set(MD.BOUNDS)
    assert any(d.cyclic and d.sampling != (1.0, 1.0) and d.bound is not None for d in draws)      # all three together


def test_the_weaker_demand_on_nearest_still_refuses_a_wrong_pixel():
    m = DT.mask_of("random-67x130-0.02")
    for cyclic in (False, True):
        dist, nearest = DT.brute(m, cyclic, (1.0, 0.7), 12 * 0.7)
        assert MD.nearest_is_a_nearest_pixel(m, dist, nearest, cyclic, (1.0, 0.7))
        p = int(np.flatnonzero((nearest.ravel() >= 0) & ~CO.foreground(m).ravel())[0])
        for wrong in (nearest.ravel()[p] + 1, -1, m.size):
            bad = nearest.copy()
            bad.flat[p] = wrong
            assert not MD.nearest_is_a_nearest_pixel(m, dist, bad, cyclic, (1.0, 0.7))
    m = DT.mask_of("cyclic-column-0")                   # the seam is part of the demand: the last column is one step from the first
    plain, cyclic = DT.brute(m), DT.brute(m, True)
    assert MD.nearest_is_a_nearest_pixel(m, *plain, False, (1.0, 1.0)) and MD.nearest_is_a_nearest_pixel(m, *cyclic, True, (1.0, 1.0))
    assert not MD.nearest_is_a_nearest_pixel(m, *plain, True, (1.0, 1.0)) and not MD.nearest_is_a_nearest_pixel(m, *cyclic, False, (1.0, 1.0))


# ------------------------------------------------------------------ components
def test_cyclic_labels_equal_scipy_on_the_tiled_plane_on_every_component_draw():
    for d in MD.drawn("components"):
        for m, (lab, n) in zip(d.stack.masks(), MD.labels_reference(d.stack, d.connectivity, True)):
            want, count = MD.tiled_label(m, d.connectivity)
            assert n == count and np.array_equal(lab, want), d
    # a bar across the seam that does not close the circle: one component, two pieces inside the middle copy
    m = np.zeros((3, 9))
    m[1, 6:] = m[1, :3] = 1
    assert CO.label(m, 1, True)[1] == MD.tiled_label(m, 1)[1] == 1 and CO.label(m, 1, False)[1] == 2


def test_the_component_draws_cross_tiles_and_capacities():
    draws = MD.drawn("components")
    busy = straddling = 0
    for d in draws:
        counts = [n for _, n in MD.labels_reference(d.stack, d.connectivity, d.cyclic)]
        tiles = -(-d.stack.ny * d.stack.nx // MD.CC_TILE)
        busy += tiles >= 2 and max(counts) >= 10
        straddling += MD.straddles(d)
    print(f"component draws with two tiles and ten components: {busy} of {len(draws)}; capacity between two counts: {straddling}")
    assert 3 * busy >= len(draws) and straddling >= 5
    assert {d.connectivity for d in draws} == {1, 2} and {d.cyclic for d in draws} == {False, True}
    assert {d.capacity for d in draws} == set(MD.CAPACITIES) and {d.criteria for d in draws} == set(MD.CRITERIA)


def test_the_sums_reference_fills_the_slots_as_the_header_says():
    header = " ".join(open(os.path.join(os.path.dirname(build.HERE), "include", "lcs_hip.h")).read().replace("\n *", " ").split())
    assert "labels above min(counts[m], n_max) are not measured, entries without a component hold area 0, root -1 and NaN extrema" in header
    seen = set()
    for d in MD.drawn("components"):
        counts = [n for _, n in MD.labels_reference(d.stack, d.connectivity, d.cyclic)]
        v, n_max, slots, sums = MD.sums_reference(d)
        assert slots == max(1, max(counts) if n_max is None else n_max) and v.dtype == np.dtype(d.stack.dtype)
        assert int(np.isnan(v).sum()) == int(d.nan_intensity)
        for n, s in zip(counts, sums):
            k = s["measured"]
            assert k == min(n, slots) and all(s[key].shape[-1] == slots for key in ("root", "area", "moments", "sum", "max", "min"))
            assert (s["area"][:k] > 0).all() and (s["root"][:k] >= 0).all() and (np.diff(s["root"][:k]) > 0).all()
            assert not s["area"][k:].any() and (s["root"][k:] == -1).all() and not s["moments"][:, k:].any()
            assert not s["sum"][k:].any() and np.isnan(s["max"][k:]).all() and np.isnan(s["min"][k:]).all()
            seen |= {"cut" if n > slots else "padded" if n < slots else "full"}
    assert seen == {"cut", "padded", "full"}


def test_the_filter_thresholds_are_values_of_the_reference_and_keep_some_and_drop_some():
    mixed = 0
    for d in MD.drawn("components"):
        v, thresholds, want = MD.filter_reference(d)
        masks = d.stack.masks()
        assert want.shape == masks.shape and want.dtype == masks.dtype and len(thresholds) == len(d.criteria)
        kept = CO.foreground(masks) & (want == masks)           # (no fill is a value of these masks, and a NaN equals nothing)
        mixed += 0 < np.count_nonzero(kept) < np.count_nonzero(CO.foreground(masks))
        gone = ~kept
        assert np.array_equal(want[gone], np.full(int(gone.sum()), d.fill, dtype=want.dtype), equal_nan=True)
    assert 3 * mixed >= len(MD.drawn("components"))
