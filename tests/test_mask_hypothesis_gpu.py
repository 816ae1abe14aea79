"""Randomised exact checks of the ridge-mask kernels: the draws of tests/mask_draws.py through Engine.label_components,
component_sums, filter_components (csrc/components.hip), distance_transform (csrc/distance.hip), thin and the dilation of
lc_mask_morphology (csrc/morphology.hip), each against the numpy / scipy reference of its draw.

What is drawn and never varied by the case tables of tests/test_components_gpu.py, test_distance_gpu.py and test_skeleton_gpu.py:
plane sides 1 .. 140 x 1 .. 270 with the sides one below, at and one above every tile constant drawn on purpose; stacks of 1 .. 3
planes of different kinds side by side; any of the 255 dilation structures, every single neighbour among them; thinning tables
with entries no shipped rule sets; cyclic, a non-unit sampling, a bound and the nearest index together; a capacity of the sums
between the counts of two planes of one stack.  Everything is integer-exact (``np.array_equal``) except the float64 sum of an
intensity, which has the bound tests/test_components_gpu.py uses for the mean, times the area.

Derandomised by default -- the same 50 draws per sequence on every run, the ones whose conditions tests/test_mask_draws.py checks
without a GPU (the three component tests share one sequence and its labels), run as explicit examples;
``LCS_HYP_RANDOM=1 LCS_HYP_SCALE=10`` lets hypothesis generate 500 of its own and shrink what fails.  The float buffers the
module's engine allocates start as NaN, so an element no kernel wrote fails its comparison.

Measured on an MI355X, wall time of each whole test with its references (the numpy side is most of it): labels 0.6 s, sums 0.3 s,
filter 1.4 s (components.props loops over the components in python), distance 0.3 s, thinning and dilation 0.2 s; the module
in 5 s.  With LCS_HYP_RANDOM=1 LCS_HYP_SCALE=10: 1.4, 2.4, 5.6, 3.1 and 2.6 s, all five passing.  Largest figures seen: the sum of
an intensity at 0.66 of its bound; every exact comparison held, 58 of the 100 distance planes against the brute-force oracle
(666 of 1079 in the random run).  Sensitivity, tried once on a scratch build: with SE and SW exchanged in mo_step_kernel's
neighbourhood index 43 of the 50 thinning draws and 13 of the 37 dilation draws whose structure names SE or SW fail (none of
the other 21); with ``idx > bidx`` in dt_rows_kernel 22 of the 50 distance draws fail; without the ``r < ny - 1`` seam line of
cc_merge_kernel 6, 5 and 4 of the 17 cyclic 8-connected draws fail the label, sums and filter tests (none of the other 41).
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
