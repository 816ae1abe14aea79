"""The randomised mask draws without a GPU: tests/mask_draws.py's references pinned against scipy by another route on the very
draws tests/test_mask_hypothesis_gpu.py runs, the sides drawn on purpose against the tile constants of the kernels, and the
conditions that make those draws worth running -- every one of them a statement about the draws and their references, none
about the engine.

Six sequences: components, distance, thin, dilate, tracks and sphere_distance; the sums on the sphere ride on the component
draws.  Figures of the derandomised draws, as the tests print them (-s): of 82 track draws 52 have more than one track, 47
fewer tracks than at reach 0 and 44 a filter that keeps some voxels and drops some, and 180 of their 268 planes are sparse
noise; every condition drawn on purpose (the three window widths at four reaches, the six tile records, the empty plane
between two others, planes smaller than a thread's span) is met by name.  Of 102 great-circle planes 68 are bounded, 19 of
those with more than SD_THREADS rows, 28 narrow and tall, 34 partly within their bound and 12 empty; 30 lists are longer and
72 shorter than SD_CHUNK; the reference takes 2.6 s; 81 planes of at most 2000 pixels agree with the haversine formula to
5.6e-9 m; on the closed grid 13 planes hold a pixel in the first or last column and 7 of them 224 bit-equal minima, all named
at the first column.  On the sphere the centroid check leaves out 5 of 5266 labels and the orientation check 53 of 1638
multi-pixel labels, every draw with an area criterion finds a decided threshold, 32 of 57 filters keep some and drop some,
4 draws on the global grid straddle their capacity and 6 hold a NaN intensity.  The file takes 11 s."""
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
    assert MD.TRC == {"TR_THREADS": 256, "TR_ITEMS": 4, "TS_ITEMS": 8} and (MD.TR_TILE, MD.TS_TILE) == (1024, 2048)
    assert MD.SDC == {"SD_THREADS": 256, "SD_CHUNK": 256} and MD.SD_LONG == [255, 256, 257, 511, 512, 513]
    assert MD.SD_EDGES == [1, 2, 3, 63, 64, 65, 255, 256, 257, 511, 512, 513] and max(MD.SD_EDGES) <= MD.SD_SIDE_MAX
    assert MD.TRACK_EDGES == [1, 2, 3, 4, 5, 31, 32, 33, 34, 35] and 2 * MD.TRACK_MAX_REACH + 1 in MD.TRACK_EDGES
    src = {f: build._strip_comments(open(os.path.join(build.CSRC, f)).read())
           for f in ("components.hip", "distance.hip", "morphology.hip", "tracks.hip", "sphere_distance.hip")}
    assert "constexpr int TR_TILE = TR_THREADS * TR_ITEMS;" in src["tracks.hip"] and "constexpr int TS_TILE = TR_THREADS * TS_ITEMS;" in src["tracks.hip"]
    # the sphere search's workgroup is SD_THREADS consecutive pixels, the band kernel's and the scan's loops go by SD_THREADS rows
    assert "p0 = (long long)b * SD_THREADS" in src["sphere_distance.hip"] and "q0 += SD_THREADS" in src["sphere_distance.hip"]
    assert "j0 += SD_CHUNK" in src["sphere_distance.hip"] and "seg = ((long long)g.ny + SD_THREADS - 1) / SD_THREADS" in src["sphere_distance.hip"]
    # the window in time of the track merge: as wide as the plane from 2 reach + 1 columns on
    assert "wrap && 2 * reach + 1 >= nx" in src["tracks.hip"]
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
    lim = MD.LIMITS[name]
    for k, d in enumerate(draws):
        s = d.stack
        wide = name == "tracks" and k < len(explicit) and s.ny * s.nx * len(s.planes) in (MD.TS_TILE - 1, MD.TS_TILE + 1)
        assert 1 <= s.ny <= lim["ny"] and 1 <= len(s.planes) <= lim["planes"] and s.dtype in ("float32", "float64")
        assert 1 <= s.nx <= lim["nx"] or wide                           # 2047 = 23 x 89 and 2049 = 3 x 683 have no other factors
        m = s.masks()
        assert m.shape == (len(s.planes), s.ny, s.nx) and m.dtype == np.dtype(s.dtype)
    sides = {v for d in draws for v in (d.stack.ny, d.stack.nx)}
    assert sides & set(lim["edges"]) and sides - set(lim["edges"])      # sides drawn on purpose and sides in between
    kinds = {p.kind for d in draws for p in d.stack.planes}
    assert kinds == set(lim["kinds"])
    assert {d.stack.dtype for d in draws} == {"float32", "float64"}
    assert {len(d.stack.planes) for d in draws} == set(range(1, lim["planes"] + 1))


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
    lim = MD.LIMITS[name]
    seen = []

    def body(d):
        s = d.stack
        assert type(d) is type(MD.drawn(name)[-1])
        assert 1 <= s.ny <= lim["ny"] and 1 <= s.nx <= lim["nx"] and 1 <= len(s.planes) <= lim["planes"] and s.dtype in ("float32", "float64")
        assert all(p.kind in lim["kinds"] and p.density in lim["densities"] for p in s.planes)
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


# ------------------------------------------------------------------ tracks
def test_the_track_draws_follow_the_constants_and_scipy_labels_the_same_where_it_can():
    from scipy import ndimage
    from tests import tracks as TR
    draws = MD.drawn("tracks")
    checked = 0
    for d in draws:
        lab, n, s = MD.tracks_reference(d)
        assert lab.shape == d.stack.masks().shape and lab.dtype == np.int32 and n == int(lab.max(initial=0))
        assert all(s[k].shape == (n,) for k in ("first", "last", "duration", "volume"))
        if not d.cyclic and d.reach <= 1:                # the same relation by another route: scipy's 3-D label
            want, count = ndimage.label(TR.foreground(d.stack.masks()), structure=TR.structure(d.connectivity, d.reach))
            assert count == n and np.array_equal(lab, want), d
            checked += 1
    assert checked >= 10
    assert {d.connectivity for d in draws} == {1, 2} and {d.cyclic for d in draws} == {False, True}
    assert {d.capacity for d in draws} == set(MD.CAPACITIES) and {d.reach for d in draws} >= set(MD.REACHES)
    assert max(d.reach for d in draws) == MD.TRACK_MAX_REACH == 16 and {d.reach for d in draws} - set(MD.REACHES)
    header = open(os.path.join(os.path.dirname(build.HERE), "include", "lcs_hip.h")).read()
    assert "#define LC_TRACK_MAX_REACH %d\n" % MD.TRACK_MAX_REACH in header


def test_the_track_draws_have_tracks_to_join_and_the_filter_keeps_some_and_drops_some():
    from tests import tracks as TR
    draws = MD.drawn("tracks")
    several = joined = mixed = sparse = planes = 0
    for d in draws:
        masks = d.stack.masks()
        _, n, _ = MD.tracks_reference(d)
        several += n > 1
        joined += n < TR.label(masks, d.connectivity, d.cyclic, 0)[1]          # the reach joins what reach 0 leaves apart
        min_duration, min_volume, want = MD.track_filter_reference(d)
        assert want.shape == masks.shape and want.dtype == masks.dtype and min_duration >= 1 and min_volume >= 1
        assert np.array_equal(want, TR.filtered(masks, min_duration, min_volume, d.connectivity, d.cyclic, d.reach, d.fill), equal_nan=True), d
        fg = TR.foreground(masks)
        kept = fg & (want == masks)                     # (no fill is a value of these masks, and a NaN equals nothing)
        mixed += 0 < np.count_nonzero(kept) < np.count_nonzero(fg)
        assert np.array_equal(want[~kept], np.full(int((~kept).sum()), d.fill, dtype=want.dtype), equal_nan=True)
        sparse += sum(p.kind == "noise" and p.density <= 0.1 for p in d.stack.planes)
        planes += len(d.stack.planes)
    print(f"track draws: {several} of {len(draws)} with more than one track, {joined} with fewer tracks than at reach 0, "
          f"{mixed} whose filter keeps some and drops some; {sparse} of {planes} planes are sparse noise")
    assert 3 * several >= len(draws) and 3 * joined >= len(draws) and 3 * mixed >= len(draws) and 2 * sparse >= planes


def _voxels(d):
    return d.stack.ny * d.stack.nx * len(d.stack.planes)


TRACK_CONDITIONS = {
    **{f"cyclic, reach {r}, nx = 2 reach + {k}": (lambda d, r=r, k=k: d.cyclic and d.reach == r and d.stack.nx == 2 * r + k and
                                                  len(d.stack.planes) in (2, 3)) for r in (1, 2, 8, 16) for k in (0, 1, 2)},
    **{f"not cyclic, nx = 2 reach + {k}": (lambda d, k=k: not d.cyclic and d.reach >= 1 and d.stack.nx == 2 * d.reach + k and
                                          len(d.stack.planes) >= 2) for k in (0, 1, 2)},
    **{f"{name} {'%+d' % k}": (lambda d, tile=tile, k=k: _voxels(d) == tile + k)
       for name, tile in (("TR_TILE", MD.TR_TILE), ("TS_TILE", MD.TS_TILE)) for k in (-1, 0, 1)},
    **{f"{name}: planes that do not divide it": (lambda d, tile=tile: abs(_voxels(d) - tile) <= 1 and len(d.stack.planes) > 1 and
                                                 tile % (d.stack.ny * d.stack.nx) != 0)
       for name, tile in (("TR_TILE", MD.TR_TILE), ("TS_TILE", MD.TS_TILE))},
    "an empty plane between two others": lambda d: any(not CO.foreground(m).any() for m in d.stack.masks()[1:-1]) and
    CO.foreground(d.stack.masks()[0]).any() and CO.foreground(d.stack.masks()[-1]).any(),
    "one plane": lambda d: len(d.stack.planes) == 1,
    "planes smaller than a thread's span of the spans kernel, and a track that lasts": lambda d: d.stack.ny * d.stack.nx < MD.TRC["TS_ITEMS"] and
    (MD.tracks_reference(d)[2]["duration"] > 1).any(),
    "a narrow cyclic 8-connected record at reach 0": lambda d: d.cyclic and d.connectivity == 2 and d.reach == 0 and d.stack.nx <= 9 and
    d.stack.ny >= 40 and len(d.stack.planes) > 1,
    "a capacity below the count": lambda d: d.capacity == "below" and MD.tracks_reference(d)[1] >= 2,
}


@pytest.mark.parametrize("name", list(TRACK_CONDITIONS))
def test_a_track_draw_meets_each_condition_drawn_on_purpose(name):
    assert any(TRACK_CONDITIONS[name](d) for d in MD.drawn("tracks")), name


def test_the_window_widths_are_met_with_both_connectivities_and_two_non_cyclic_reaches():
    draws = MD.drawn("tracks")[:len(MD.TRACK_EXPLICIT)]
    cyclic = [d for d in draws if d.cyclic and d.reach and d.stack.nx in (2 * d.reach, 2 * d.reach + 1, 2 * d.reach + 2)]
    plain = [d for d in draws if not d.cyclic and d.reach and d.stack.nx in (2 * d.reach, 2 * d.reach + 1, 2 * d.reach + 2)]
    assert {d.connectivity for d in cyclic} == {1, 2} and {d.reach for d in cyclic} >= {1, 2, 8, 16}
    assert len({d.reach for d in plain}) >= 2 and all(CO.foreground(d.stack.masks()).any() for d in cyclic + plain)
    # the tile records exist under the limits wherever the tile's neighbours factor that way
    assert MD.TS_TILE - 1 == 23 * 89 and MD.TS_TILE + 1 == 3 * 683 and (MD.TR_TILE, MD.TS_TILE) == (1024, 2048)


# ------------------------------------------------------------------ the great-circle distance
def _sphere_planes():
    """Every plane of the sequence: (draw, mask, (dist, nearest, cost))."""
    return [(d, m, ref) for d in MD.drawn("sphere_distance") for m, ref in zip(d.stack.masks(), MD.sphere_distance_reference(d))]


def test_the_sphere_distance_reference_is_quick_and_the_haversine_distance_on_small_planes():
    import time
    from tests import sphere_distance as SD
    MD.sphere_distance_reference.cache_clear()
    start = time.perf_counter()
    planes = _sphere_planes()
    took = time.perf_counter() - start
    print(f"sphere distance: the reference of {len(planes)} planes took {took:.1f} s")
    assert took < 10.0
    small = worst = 0
    for d, m, (dist, nearest, cost) in planes:
        assert dist.shape == m.shape == nearest.shape == cost.shape and nearest.dtype == np.int32
        if m.size <= 2000:
            # 1e-7 m on a sphere of 6371 km, in the unit of the draw's radius; under a bound, where the distance is finite
            want = SD.haversine_min(m, *d.coordinates(), d.radius)
            f = np.isfinite(dist)
            assert MD.is_bounded(d) or np.array_equal(f, np.isfinite(want)), d
            err = float(np.max(np.abs(dist[f] - want[f]), initial=0.0)) * SD.RADIUS / d.radius
            worst, small = max(worst, err), small + 1
            assert err <= 1e-7, d
    print(f"sphere distance: {small} planes of at most 2000 pixels against the haversine formula, largest difference {worst:.2e} m")
    assert small >= 20


def test_the_sphere_distance_draws_reach_what_no_case_table_does():
    from tests import sphere_distance as SD
    planes = _sphere_planes()
    draws = MD.drawn("sphere_distance")
    bounded = [(d, m, ref) for d, m, ref in planes if MD.is_bounded(d)]
    tall = sum(d.stack.ny > MD.SDC["SD_THREADS"] for d, _, _ in bounded)
    narrow = sum(d.stack.nx <= 3 and d.stack.ny > 64 for d, _, _ in bounded)
    partly = sum(0 < np.count_nonzero(np.isfinite(ref[0])) < m.size for _, m, ref in bounded)
    empty = sum(not CO.foreground(m).any() for _, m, _ in bounded)
    more = sum(np.count_nonzero(CO.foreground(m)) > MD.SDC["SD_CHUNK"] for _, m, _ in planes)
    fewer = sum(np.count_nonzero(CO.foreground(m)) < MD.SDC["SD_CHUNK"] for _, m, _ in planes)
    print(f"sphere distance: {len(bounded)} of {len(planes)} planes bounded, {tall} of them with more than SD_THREADS rows, {narrow} "
          f"narrow and tall, {partly} partly within their bound, {empty} empty; {more} lists longer and {fewer} shorter than SD_CHUNK")
    assert tall >= 10 and narrow >= 5 and 4 * partly >= len(bounded) and empty >= 1 and more >= 10 and fewer >= 10
    assert {d.grid for d in draws} == set(MD.SD_GRIDS) and {d.bound for d in draws} == set(MD.SD_BOUNDS)
    assert {d.radius for d in draws} == {SD.RADIUS, 1.0}
    assert any(not MD.is_bounded(d) and d.bound == 40 for d in draws) or any(d.bound == "pi" for d in draws)      # a bound that is none
    # two rounds of the band kernel's loop and rows per thread of the scan above 1
    assert any(d.stack.ny > 2 * MD.SDC["SD_THREADS"] and d.stack.nx <= 3 for d, _, _ in bounded)
    # the three families
    assert any(d.stack.ny > 132 and d.stack.nx <= 12 for d in draws) and any(d.stack.nx > 132 and d.stack.ny <= 12 for d in draws)
    assert any(12 < d.stack.ny <= 70 and 12 < d.stack.nx <= 132 for d in draws)
    assert all(p.density <= 0.41 for d in draws for p in d.stack.planes)


def test_on_the_closed_grid_equal_costs_go_to_the_first_column():
    """The first and the last column of the closed grid are one meridian: X is equal, Y differs in sign only and is a few
    1e-17, so the costs of a pixel to the two ends of a row are bit-equal wherever that difference is lost in the pixel's own
    Y -- and distinct, the end on the pixel's own side nearer by a last bit, elsewhere.  So the oracle MAY name the last column
    beside a foreground first column of the same row, but never at an equal cost."""
    from tests import sphere_distance as SD
    with_ends = tied_planes = ties = 0
    for d, m, (dist, nearest, cost) in _sphere_planes():
        fg = CO.foreground(m)
        nx = d.stack.nx
        if d.grid != "closed" or nx < 2 or not (fg[:, 0].any() or fg[:, -1].any()):
            continue
        with_ends += 1
        lat, lon = d.coordinates()
        assert lon[0] == -180.0 and lon[-1] == 180.0
        X, Y, Z = SD.unit_vectors(lat, lon)
        at = np.flatnonzero(nearest.ravel() >= 0)
        q = nearest.ravel()[at].astype(np.int64)
        r, c = np.divmod(q, nx)
        other = r * nx + np.where(c == 0, nx - 1, 0)                      # the other end of the nearest pixel's row
        both = ((c == 0) | (c == nx - 1)) & fg.ravel()[other]
        tied = both & (SD.cost_of((X[at], Y[at], Z[at]), (X[other], Y[other], Z[other])) == cost.ravel()[at])
        assert not (tied & (c != 0)).any(), d                             # at an equal cost the smaller index, column 0, is named
        ties += int(tied.sum())
        tied_planes += bool(tied.any())
    print(f"closed grid: {with_ends} planes with a pixel in the first or last column, {tied_planes} with bit-equal minima, {ties} of those")
    assert with_ends >= 5 and tied_planes >= 3 and ties >= 50


# ------------------------------------------------------------------ sphere sums over the component draws
def test_the_sphere_sums_reference_fills_the_slots_as_the_header_says():
    header = " ".join(open(os.path.join(os.path.dirname(build.HERE), "include", "lcs_hip.h")).read().replace("\n *", " ").split())
    assert "Entries past a plane's count and labels without a pixel in the plane: area 0, everything else NaN." in header
    seen, refused = set(), 0
    for d in MD.drawn("components"):
        ref = MD.sphere_sums_reference(d)
        if ref is None:
            assert min(d.stack.ny, d.stack.nx) == 1
            refused += 1
            continue
        v, n_max, slots, (lat, lon), planes = ref
        counts = [n for _, n in MD.labels_reference(d.stack, d.connectivity, d.cyclic)]
        _, same_n_max, same_slots, index = MD.sums_reference(d)
        assert (n_max, slots) == (same_n_max, same_slots) and lat.shape == (d.stack.ny,) and lon.shape == (d.stack.nx,)
        for n, pl, ix in zip(counts, planes, index):
            k, s, p = pl["measured"], pl["sums"], pl["props"]
            assert k == min(n, slots) == ix["measured"] and np.array_equal(s["root"], ix["root"]) and np.array_equal(s["count"], ix["area"])
            assert np.array_equal(s["max"], ix["max"], equal_nan=True) and np.array_equal(s["min"], ix["min"], equal_nan=True)
            assert s["sums"].shape == (11, slots) and not s["sums"][:, k:].any() and (s["sums"][0, :k] > 0).all()
            assert not p["area"][k:].any() and (p["area"][:k] > 0).all()
            for key in ("major_axis_length", "minor_axis_length", "centroid_latitude", "centroid_longitude", "orientation",
                        "mean_intensity", "total_intensity"):
                assert np.isnan(p[key][k:]).all(), key
            seen |= {"cut" if n > slots else "padded" if n < slots else "full"}
    assert seen == {"cut", "padded", "full"} and 1 <= refused <= len(MD.drawn("components")) // 4
    assert {MD.sphere_variant(d) for d in MD.drawn("components")} == set(MD.SPHERE_VARIANTS)


def test_the_sphere_checks_leave_few_labels_out_and_the_area_thresholds_are_decided():
    from tests import sphere_props as SP
    draws = MD.drawn("components")
    labels = no_centroid = multi = no_orientation = with_area = undecided = mixed = filtered = 0
    straddling = with_nan = 0
    for d in draws:
        ref = MD.sphere_sums_reference(d)
        if ref is None:
            continue
        if MD.sphere_variant(d) == "global":
            straddling += MD.straddles(d)
            with_nan += d.nan_intensity
        for pl in ref[4]:
            s, p, b = pl["sums"], pl["props"], pl["bounds"]
            centroid, oriented, many = MD.sphere_admitted(pl)
            some = s["count"] > 0
            labels, no_centroid = labels + int(some.sum()), no_centroid + int((some & ~centroid).sum())
            multi, no_orientation = multi + int(many.sum()), no_orientation + int((many & ~oriented).sum())
            assert (b["E_over_gap"][oriented] <= 0.25).all()
            # what the orientation's NaN rule rests on: a one-pixel label has none; a multi-pixel label whose centroid is
            # admitted and whose e1 exceeds its own bound has one
            assert np.isnan(p["orientation"][s["count"] == 1]).all()
            with np.errstate(invalid="ignore"):
                assert not np.isnan(p["orientation"][many & centroid & (p["e"][:, 0] > b["e"])]).any()
        if "area" in d.criteria:
            with_area += 1
        f = MD.sphere_filter_reference(d)
        if f is None:
            undecided += "area" in d.criteria
            continue
        thresholds, want = f
        masks = d.stack.masks()
        kept = CO.foreground(masks) & (want == masks)
        filtered += 1
        mixed += 0 < np.count_nonzero(kept) < np.count_nonzero(CO.foreground(masks))
        assert want.shape == masks.shape and want.dtype == masks.dtype and len(thresholds) == len(d.criteria)
        lat, lon = MD.sphere_grid(d)
        for m, vi, w in zip(masks, MD.intensity_of(d), want):
            assert np.array_equal(w, SP.filtered(m, vi.astype(np.float64), d.criteria, thresholds, lat, lon, d.connectivity, d.cyclic, d.fill,
                                                 MD.SPHERE_RADIUS), equal_nan=True), d
    print(f"sphere sums: centroid check leaves out {no_centroid} of {labels} labels, orientation check {no_orientation} of {multi} "
          f"multi-pixel labels; {undecided} of {with_area} draws with an area criterion find no decided threshold; {mixed} of {filtered} "
          f"filters keep some and drop some; on the global grid {straddling} draws straddle their capacity, {with_nan} hold a NaN intensity")
    assert no_centroid <= 0.01 * labels and no_orientation <= 0.05 * multi and undecided <= 0.1 * len(draws)
    assert straddling >= 1 and with_nan >= 1 and 3 * mixed >= filtered
