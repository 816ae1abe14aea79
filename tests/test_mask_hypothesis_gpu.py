"""Randomised exact checks of the ridge-mask kernels: the draws of tests/mask_draws.py through Engine.label_components,
component_sums, filter_components (csrc/components.hip), distance_transform (csrc/distance.hip), thin and the dilation of
lc_mask_morphology (csrc/morphology.hip), label_tracks, track_spans, filter_tracks (csrc/tracks.hip), sphere_distance
(csrc/sphere_distance.hip) and component_sphere_props / filter_components(metric='sphere') (the sp_* kernels of
csrc/components.hip), each against the numpy / scipy reference of its draw.

What is drawn and never varied by the case tables of tests/test_components_gpu.py, test_distance_gpu.py and test_skeleton_gpu.py:
plane sides 1 .. 140 x 1 .. 270 with the sides one below, at and one above every tile constant drawn on purpose; stacks of 1 .. 3
planes of different kinds side by side; any of the 255 dilation structures, every single neighbour among them; thinning tables
with entries no shipped rule sets; cyclic, a non-unit sampling, a bound and the nearest index together; a capacity of the sums
between the counts of two planes of one stack.  Everything is integer-exact (``np.array_equal``) except the float64 sum of an
intensity, which has the bound tests/test_components_gpu.py uses for the mean, times the area.

And by those of tests/test_tracks_gpu.py, test_sphere_distance_gpu.py and test_sphere_props_gpu.py: records of 1 .. 6 planes up to
48 x 80 at every reach 0 .. 16 on random masks, the plane widths 2 reach, 2 reach + 1 and 2 reach + 2 with and without cyclic,
records of one voxel below, at and above the label tile and the spans tile, a capacity of the spans below the count; a bound
of the great-circle distance on planes of more rows than a workgroup has threads (two and three rounds of the band kernel,
several rows per thread of the scan), on planes 1 .. 3 columns wide whose workgroups span up to 256 rows, on five grids (global,
rows at both poles, regional and non-uniform, unsorted latitudes, first and last column one meridian: bit-equal costs), lists
shorter and longer than the staging chunk; the sums on the sphere on random masks of every shape above, with a capacity
below one plane's count in a stack, a NaN intensity on a grid whose outer rows are the poles, and the sphere filter at
thresholds the reference's own bounds decide.  Labels, counts, spans, filtered records, squared chords and nearest indices
are compared with ``np.array_equal``; distances within the 16 ulp tests/test_sphere_distance_gpu.py derives; the sums and
properties on the sphere inside the bounds of tests/sphere_props.py:bounds, none of which comes from a device output.  An
orientation must be NaN on every one-pixel label and a number wherever the reference tells ``e1`` from 0 at an admitted
centroid (a label whose every pixel is the pole itself, or whose centroid is the centre of the sphere, has no direction
on either side).

Derandomised by default -- the same 50 draws per sequence and its explicit ones on every run, the ones whose conditions
tests/test_mask_draws.py checks without a GPU (the five component tests share one sequence and its labels, the two track tests
theirs), run as explicit examples; ``LCS_HYP_RANDOM=1 LCS_HYP_SCALE=10`` lets hypothesis generate 500 of its own and shrink what
fails.  The float buffers the module's engine allocates start as NaN, so an element no kernel wrote fails its comparison.

Measured on an MI355X, wall time of each whole test with its references (the numpy side is most of it): labels 0.4 s, sums 0.3 s,
filter 1.4 s (components.props loops over the components in python), distance 0.3 s, thinning and dilation 0.2 s, track labels
and spans 0.35 s, track filter 0.35 s, great-circle distance 0.95 s, sums on the sphere 0.4 s, sphere filter 0.35 s; the module
in 7 s (5 s before the five new tests).  With LCS_HYP_RANDOM=1 LCS_HYP_SCALE=10: 1.4, 2.0, 8.6, 1.8, 2.7, 2.2, 3.1, 5.2, 3.8 and
5.1 s, the module in 38 s, all ten passing.  Largest figures seen: the sum of an intensity at 0.66 of its bound; every exact
comparison held, 58 of the 100 distance planes against the brute-force oracle (681 of 1068 in the random run); 82 records with
2669 tracks (532 with 14399); 102 great-circle planes at 2.00 ulp at most (1108 planes, 2.00 ulp); on the sphere, as error /
bound, W 0.66, S 0.64, the nine moment sums 0.45 - 0.50, area 0.37, total_intensity 0.47, mean_intensity 0.36,
minor_axis_length 0.16, major_axis_length 0.06, centroid latitude 0.17, longitude 0.12, orientation 0.02, with 5 of 5266
labels left out of the centroid check and 53 of 1638 multi-pixel labels out of the orientation check, 57 filters compared
(random run: W 0.66, S 0.67, moments 0.50, area 0.48, centroid 0.21 and 0.19, orientation 0.02; 29 of 76186 and 377 of 25671
left out; 420 filters).

Sensitivity, tried once on a scratch build: with SE and SW exchanged in mo_step_kernel's
neighbourhood index 43 of the 50 thinning draws and 13 of the 37 dilation draws whose structure names SE or SW fail (none of
the other 21); with ``idx > bidx`` in dt_rows_kernel 22 of the 50 distance draws fail; without the ``r < ny - 1`` seam line of
cc_merge_kernel 6, 5 and 4 of the 17 cyclic 8-connected draws fail the label, sums and filter tests (none of the other 41).
The same for the three later families, every change one that keeps each index inside its array, none of which faulted or
hung: with ``cost <= best`` in sd_search_kernel 19 of the 54 great-circle draws fail (5 of the 12 on the closed grid); with
``s_hi[0] - 1`` written as a row's upper band where it exceeds the row 7 of the 38 bounded draws (3 of the 10 with more than
256 rows); without the ``r < ny - 1`` seam line of tr_merge_kernel 5 of the 26 cyclic 8-connected track draws fail the labels
and 2 the filter (none of the other 56); with ``2 * reach + 1 > nx`` for ``>=`` nothing fails, as expected -- at nx = 2 reach + 1
the wrapped window is every column once as well; without ``tmax = t`` in ts_spans_kernel 3 of the 82 track draws fail the
spans and the filter -- the three whose planes are smaller than one thread's span, drawn on purpose after the first trial, in
which none of 76 failed (on a larger plane another thread starts on the label in the track's last plane); with ``wy * dx``
for ``wx * dy`` in sp_sums_kernel, terms that differ in their last bit only, 2 of the 58 component draws fail the bounds.
"""
import numpy as np
import pytest

from tests import mask_draws as MD

pytestmark = pytest.mark.gpu

SEEN = {}          # the largest figures of this run, printed by the tests that have a bound (pytest -s)


@pytest.fixture(scope="module")
def eng():
    from lagrangiancoherence_amd.engine import Engine
    e = Engine(0)
    e._poison = True
    yield e
    e.close()


def _np(t):
    return t.detach().cpu().numpy()


def _labelled(eng, d):
    return eng.label_components(d.stack.masks(), d.connectivity, d.cyclic)


# ------------------------------------------------------------------ csrc/components.hip
def check_labels(eng, d):
    labels, counts = _labelled(eng, d)
    assert labels.dtype == eng.torch.int32 and tuple(labels.shape) == (len(d.stack.planes), d.stack.ny, d.stack.nx)
    got, n_got = _np(labels), _np(counts)
    for i, (lab, n) in enumerate(MD.labels_reference(d.stack, d.connectivity, d.cyclic)):
        assert int(n_got[i]) == n, (i, int(n_got[i]), n)
        assert np.array_equal(got[i], lab), i


def test_labels_and_counts_equal_scipy_on_every_draw(eng):
    MD.run("components", lambda d: check_labels(eng, d))


def check_sums(eng, d):
    v, n_max, slots, want = MD.sums_reference(d)
    labels, counts = _labelled(eng, d)
    got = {k: _np(t) for k, t in eng.component_sums(labels, counts, v, d.cyclic, n_max=n_max).items()}
    assert got["area"].shape == (len(want), slots) and got["moments"].shape == (5, len(want), slots)
    for i, w in enumerate(want):
        # exact: the first pixels, the areas, the five integer sums, the extrema -- measured labels and empty slots alike
        assert np.array_equal(got["root"][i], w["root"]) and np.array_equal(got["area"][i], w["area"]), i
        assert np.array_equal(got["moments"][:, i], w["moments"]), i
        assert np.array_equal(got["max"][i], w["max"], equal_nan=True) and np.array_equal(got["min"][i], w["min"], equal_nan=True), i
        # the sum: NaN exactly where the component holds the NaN, else inside the bound of a sum of `area` terms in any order
        assert np.array_equal(np.isnan(got["sum"][i]), np.isnan(w["sum"])), i
        ok = ~np.isnan(w["sum"])
        err, bound = np.abs(got["sum"][i] - w["sum"])[ok], (w["area"] * MD.EPS * w["abs_sum"])[ok]
        assert (err <= bound).all(), (i, float(err.max()))
        assert not got["sum"][i, w["measured"]:].any()
        if ok.any() and bound.max() > 0:
            SEEN["sum"] = max(SEEN.get("sum", 0.0), float(np.max(err / np.maximum(bound, 1e-300))))


def test_component_sums_equal_the_oracle_on_every_draw_and_at_every_capacity(eng):
    try:
        MD.run("components", lambda d: check_sums(eng, d))
    finally:
        print(f"sum of the intensity: largest error / bound {SEEN.get('sum', 0.0):.3g}")


def check_filter(eng, d):
    v, thresholds, want = MD.filter_reference(d)
    masks = d.stack.masks()
    got = _np(eng.filter_components(masks, v, list(d.criteria), thresholds, d.connectivity, d.cyclic, d.fill))
    assert got.dtype == masks.dtype and got.shape == masks.shape
    for i in range(len(masks)):
        assert np.array_equal(got[i], want[i], equal_nan=True), i


def test_filter_components_equals_the_oracle_on_every_draw(eng):
    MD.run("components", lambda d: check_filter(eng, d))


# ------------------------------------------------------------------ csrc/distance.hip
def check_distance(eng, d):
    masks = d.stack.masks()
    want_d, want_n = MD.distance_reference(d)
    dist, nearest = eng.distance_transform(masks, cyclic=d.cyclic, sampling=d.sampling, max_distance=d.max_distance, return_nearest=True)
    assert dist.dtype == eng.torch.float64 and nearest.dtype == eng.torch.int32 and tuple(dist.shape) == masks.shape == tuple(nearest.shape)
    dist, nearest = _np(dist), _np(nearest)
    for i, m in enumerate(masks):
        assert np.array_equal(dist[i], want_d[i]), i                      # scipy, bit for bit, +inf beyond the bound
        if want_n[i] is not None:
            assert np.array_equal(nearest[i], want_n[i]), i               # the brute-force minimum, smallest index among equals
            SEEN["brute"] = SEEN.get("brute", 0) + 1
        else:
            assert MD.nearest_is_a_nearest_pixel(m, want_d[i], nearest[i], d.cyclic, d.sampling), i
            SEEN["weaker"] = SEEN.get("weaker", 0) + 1


def test_distance_equals_scipy_and_nearest_the_brute_force_oracle_on_every_draw(eng):
    try:
        MD.run("distance", lambda d: check_distance(eng, d))
    finally:
        print(f"planes compared with the brute-force oracle: {SEEN.get('brute', 0)}, held to the weaker demand: {SEEN.get('weaker', 0)}")


# ------------------------------------------------------------------ csrc/morphology.hip
def _plane_by_plane(got, call, masks):
    """A stack equals its planes through single calls: nothing leaks over a plane's first or last row."""
    if len(masks) > 1:
        for i, m in enumerate(masks):
            one = call(m)
            assert tuple(one.shape) == m.shape and np.array_equal(_np(one), got[i]), i


def check_thin(eng, d):
    masks, codes = d.stack.masks(), d.table.codes()

    def call(m):
        return eng.thin(m, codes, cyclic=d.cyclic, max_iterations=d.max_iterations, iterations_per_launch=d.per_launch)
    got = call(masks)
    assert got.dtype == eng.torch.uint8 and tuple(got.shape) == masks.shape
    got = _np(got)
    want = MD.thin_reference(d)
    for i in range(len(masks)):
        assert np.array_equal(got[i], want[i]), i
    _plane_by_plane(got, call, masks)


def check_dilate(eng, d):
    from lagrangiancoherence_amd import _capi
    masks = d.stack.masks()

    def call(m):
        return eng._morphology(m, _capi.LC_MORPH_DILATE, None, d.structure, d.cyclic, d.iterations, d.per_launch)
    got = call(masks)
    assert got.dtype == eng.torch.uint8 and tuple(got.shape) == masks.shape
    got = _np(got)
    want = MD.dilate_draw_reference(d)
    for i in range(len(masks)):
        assert np.array_equal(got[i], want[i]), i
    _plane_by_plane(got, call, masks)


def test_thinning_and_dilation_equal_their_restatements_on_every_draw(eng):
    MD.run("thin", lambda d: check_thin(eng, d))
    MD.run("dilate", lambda d: check_dilate(eng, d))


# ------------------------------------------------------------------ csrc/tracks.hip
def check_tracks(eng, d):
    masks = d.stack.masks()
    lab, n, _ = MD.tracks_reference(d)
    labels, count = eng.label_tracks(masks, d.connectivity, d.cyclic, d.reach)
    assert labels.dtype == eng.torch.int32 and tuple(labels.shape) == masks.shape and tuple(count.shape) == (1,)
    assert int(count[0]) == n, (int(count[0]), n)
    assert np.array_equal(_np(labels), lab)
    if len(masks) == 1:          # one plane is label_components of it, whatever the reach
        want, counts = eng.label_components(masks[0], d.connectivity, d.cyclic)
        assert int(counts[0]) == n and np.array_equal(_np(want), lab[0])
    # the spans at the drawn capacity: the measured tracks, and the tail as the header promises it
    n_max, slots, want = MD.track_spans_reference(d)
    got = {k: _np(v) for k, v in eng.track_spans(labels, count, n_max=n_max).items()}
    assert got["first"].dtype == got["last"].dtype == got["duration"].dtype == np.int32 and got["volume"].dtype == np.int64
    for k in ("first", "last", "duration", "volume"):
        assert got[k].shape == (slots,) and np.array_equal(got[k], want[k]), k
    SEEN["tracks"] = SEEN.get("tracks", 0) + n
    SEEN["records"] = SEEN.get("records", 0) + 1


def check_track_filter(eng, d):
    masks = d.stack.masks()
    min_duration, min_volume, want = MD.track_filter_reference(d)
    got = _np(eng.filter_tracks(masks, min_duration, min_volume, d.connectivity, d.cyclic, d.reach, d.fill))
    assert got.dtype == masks.dtype and got.shape == masks.shape and np.array_equal(got, want, equal_nan=True)


def test_track_labels_and_spans_equal_the_oracle_on_every_draw(eng):
    try:
        MD.run("tracks", lambda d: check_tracks(eng, d))
    finally:
        print(f"records labelled: {SEEN.get('records', 0)}, tracks among them: {SEEN.get('tracks', 0)}")


def test_filter_tracks_equals_the_oracle_on_every_draw(eng):
    MD.run("tracks", lambda d: check_track_filter(eng, d))


# ------------------------------------------------------------------ csrc/sphere_distance.hip
def check_sphere_distance(eng, d):
    masks = d.stack.masks()
    lat, lon = d.coordinates()

    def call(m):
        return tuple(_np(t) for t in eng.sphere_distance(m, lat, lon, radius=d.radius, max_distance=d.max_distance, return_nearest=True,
                                                         return_cost=True))
    got = call(masks)
    assert all(g.shape == masks.shape for g in got) and got[0].dtype == got[2].dtype == np.float64 and got[1].dtype == np.int32
    for i, (want_d, want_n, want_c) in enumerate(MD.sphere_distance_reference(d)):
        dist, nearest, cost = (g[i] for g in got)
        assert np.array_equal(cost, want_c) and np.array_equal(nearest, want_n), i          # bit for bit, the first of equal costs
        assert not dist[want_c == 0].any(), i
        assert np.array_equal(np.isposinf(dist), np.isposinf(want_d)) and np.array_equal(nearest == -1, np.isposinf(want_d)), i
        f = np.isfinite(want_d) & (want_d != 0)
        ulp = np.abs(dist[f] - want_d[f]) / np.spacing(want_d[f])
        SEEN["ulp"] = max(SEEN.get("ulp", 0.0), float(ulp.max(initial=0.0)))
        assert (ulp <= 16).all(), (i, float(ulp.max()))
        SEEN["sphere planes"] = SEEN.get("sphere planes", 0) + 1
    if len(masks) > 1:          # a stack equals its planes through single calls, distances included
        for i, m in enumerate(masks):
            assert all(np.array_equal(o, g[i]) for o, g in zip(call(m), got)), i


def test_sphere_distance_equals_the_brute_force_oracle_on_every_draw(eng):
    try:
        MD.run("sphere_distance", lambda d: check_sphere_distance(eng, d))
    finally:
        print(f"great-circle distance: {SEEN.get('sphere planes', 0)} planes, largest |dist - oracle| {SEEN.get('ulp', 0.0):.2f} ulp")


# ------------------------------------------------------------------ csrc/components.hip: the sums on the sphere
def _inside(what, got, ref, bound):
    """NaN exactly where the reference has NaN, elsewhere |got - ref| <= bound; keeps the largest error / bound under ``what``."""
    got, ref, bound = (np.asarray(a, dtype=np.float64) for a in (got, ref, bound))
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what
    ok = ~np.isnan(ref)
    err, lim = np.abs(got[ok] - ref[ok]), bound[ok]
    assert not np.isnan(lim).any(), what
    ratio = float(np.max(err[err > 0] / lim[err > 0], initial=0.0)) if (lim[err > 0] > 0).all() else float("inf")
    assert (err <= lim).all(), f"{what}: largest error / bound {ratio:.3g} (error {err.max():.3g})"
    SEEN[what] = max(SEEN.get(what, 0.0), ratio)


SPHERE_FLOATS = ("area", "major_axis_length", "minor_axis_length", "mean_intensity", "total_intensity")


def check_sphere_sums(eng, d):
    from tests import sphere_props as SP
    labels, counts = _labelled(eng, d)
    lat, lon = MD.sphere_grid(d)
    ref = MD.sphere_sums_reference(d)
    if ref is None:             # a side of 1 has no width
        with pytest.raises(ValueError, match="at least two"):
            eng.component_sphere_props(labels, counts, lat, lon, MD.intensity_of(d), d.cyclic, MD.SPHERE_RADIUS)
        return
    v, n_max, slots, _, want = ref
    got = {k: _np(t) for k, t in eng.component_sphere_props(labels, counts, lat, lon, v, d.cyclic, MD.SPHERE_RADIUS, n_max=n_max,
                                                            return_sums=True).items()}
    assert got["area"].shape == (len(want), slots) and got["M1"].shape == (len(want), slots, 3) and got["M2"].shape == (len(want), slots, 6)
    G = np.concatenate([got["W"][None], np.moveaxis(got["M1"], -1, 0), np.moveaxis(got["M2"], -1, 0), got["S"][None]])      # (11, planes, slots)
    for i, w in enumerate(want):
        s, p, b, k = w["sums"], w["props"], w["bounds"], w["measured"]
        # exact: the first pixels and the extrema, measured labels and empty slots alike
        assert np.array_equal(got["root"][i], s["root"]), i
        assert np.array_equal(got["max_intensity"][i], s["max"], equal_nan=True) and np.array_equal(got["min_intensity"][i], s["min"], equal_nan=True), i
        assert not G[:, i, k:].any() and not got["area"][i, k:].any(), i
        for j, name in enumerate(SP.NAMES):
            _inside(name, G[j, i, :k], s["sums"][j, :k], b["sums"][j, :k])
        for key in SPHERE_FLOATS:
            _inside(key, got[key][i, :k], p[key][:k], b[key][:k])
            assert key == "area" or np.isnan(got[key][i, k:]).all(), key
        centroid, oriented, multi = (a[:k] for a in MD.sphere_admitted(w))
        _inside("centroid_latitude", got["centroid_latitude"][i, :k][centroid], p["centroid_latitude"][:k][centroid], b["centroid_latitude"][:k][centroid])
        _inside("centroid_longitude", SP.angle_difference(got["centroid_longitude"][i, :k][centroid], p["centroid_longitude"][:k][centroid], 360.0),
                np.zeros(int(centroid.sum())), b["centroid_longitude"][:k][centroid])
        # orientation: NaN on every one-pixel label and in every empty slot; a number on every multi-pixel label whose centroid is
        # admitted and whose e1 the reference tells from 0; inside its bound where the major axis is a direction
        orientation = got["orientation"][i]
        assert np.isnan(orientation[:k][s["count"][:k] == 1]).all() and np.isnan(orientation[k:]).all(), i
        with np.errstate(invalid="ignore"):
            certain = multi & centroid & (p["e"][:k, 0] > b["e"][:k])
        assert not np.isnan(orientation[:k][certain]).any(), i
        assert ((orientation[:k][certain] > -90.0) & (orientation[:k][certain] <= 90.0)).all(), i
        _inside("orientation", SP.angle_difference(orientation[:k][oriented], p["orientation"][:k][oriented], 180.0), np.zeros(int(oriented.sum())),
                b["orientation"][:k][oriented])
        for name, left in (("labels", k), ("no centroid", k - int(centroid.sum())), ("multi", int(multi.sum())),
                           ("no orientation", int(multi.sum() - oriented.sum()))):
            SEEN[name] = SEEN.get(name, 0) + left


def check_sphere_filter(eng, d):
    f = MD.sphere_filter_reference(d)
    if f is None:               # a side of 1 (refused, above), or no area threshold that the reference decides
        return
    thresholds, want = f
    masks = d.stack.masks()
    lat, lon = MD.sphere_grid(d)
    got = _np(eng.filter_components(masks, MD.intensity_of(d), list(d.criteria), thresholds, d.connectivity, d.cyclic, d.fill, metric="sphere",
                                    lat=lat, lon=lon, radius=MD.SPHERE_RADIUS))
    assert got.dtype == masks.dtype and got.shape == masks.shape
    for i in range(len(masks)):
        assert np.array_equal(got[i], want[i], equal_nan=True), i
    SEEN["sphere filters"] = SEEN.get("sphere filters", 0) + 1


def test_sphere_sums_and_properties_are_inside_their_bounds_on_every_component_draw(eng):
    from tests import sphere_props as SP
    try:
        MD.run("components", lambda d: check_sphere_sums(eng, d))
    finally:
        print("sphere sums, largest error / bound: " + ", ".join(f"{k} {SEEN.get(k, 0.0):.2f}" for k in SP.NAMES))
        print("sphere properties, largest error / bound: " +
              ", ".join(f"{k} {SEEN.get(k, 0.0):.2f}" for k in SPHERE_FLOATS + ("centroid_latitude", "centroid_longitude", "orientation")))
        print(f"labels measured: {SEEN.get('labels', 0)}, left out of the centroid check: {SEEN.get('no centroid', 0)}; multi-pixel labels: "
              f"{SEEN.get('multi', 0)}, left out of the orientation check: {SEEN.get('no orientation', 0)}")


def test_filter_components_on_the_sphere_equals_the_restatement_on_every_component_draw(eng):
    try:
        MD.run("components", lambda d: check_sphere_filter(eng, d))
    finally:
        print(f"sphere filters compared: {SEEN.get('sphere filters', 0)}")
