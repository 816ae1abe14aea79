"""The component filter on the GPU against tests/components.py (scipy.ndimage.label + numpy): labels and counts equal, the
integer sums and the extrema equal, the mean and the inertia eigenvalues inside bounds that follow from the arithmetic, the
filtered mask equal -- on the smallest planes that cross every boundary of csrc/components.hip: one pixel, one row, one
column, sizes that are no multiple of the 1024-pixel tile, several tiles, more tiles than one pass of the tile scan takes
(256), the longest parent chains (a serpentine), equivalences found last (a comb), sprawling components near the percolation
thresholds, the seam, several planes per launch, NaN and negative mask values.

Every reference is computed once per case and shared.  The float buffers the module's engine allocates start as NaN.  Each
bounded comparison prints its measured error beside its bound before asserting (pytest -s).

Bounds.  mean_intensity: area 2^-53 sum|v| / area, the standard bound of a float64 sum of `area` terms taken in any order,
divided by the area.  l1, l2: 64 2^-53 (a + c) -- the engine computes them from exact integers with fewer than ten
roundings, a + c = l1 + l2 bounds every intermediate, and 64 is a loose cover, not a tuned value.

Largest figures seen on an MI355X: mean_intensity 0.54 of its bound (random-0.59, connectivity 1), l1 / l2 7.1e-15 absolute
(seam-random-0.41) and 4.6e-13 on the serpentine against a bound of 1.2e-11; labels, counts, integer sums, extrema and
filtered masks equal everywhere.
"""
import functools

import numpy as np
import pytest

from tests import components as CO
from tests.labelled import DataArray

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
DTYPES = [np.float32, np.float64]


@pytest.fixture(scope="module")
def eng():
    from lagrangiancoherence_amd.engine import Engine
    e = Engine(0)
    e._poison = True
    yield e
    e.close()


def _np(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _ref(name, connectivity, cyclic=False):
    mask = CO.mask_of(name)
    lab, n = CO.label(mask, connectivity, cyclic)
    mask.setflags(write=False)
    lab.setflags(write=False)
    return mask, lab, n


# ------------------------------------------------------------------ labels and counts
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("connectivity", [1, 2])
@pytest.mark.parametrize("name", list(CO.CASES))
def test_labels_and_counts_equal_scipy(eng, name, connectivity, dtype):
    mask, lab, n = _ref(name, connectivity)
    labels, counts = eng.label_components(mask.astype(dtype), connectivity)
    assert labels.dtype == eng.torch.int32 and tuple(labels.shape) == mask.shape and tuple(counts.shape) == (1,)
    assert int(counts[0]) == n
    assert np.array_equal(_np(labels), lab)


def test_the_checkerboards_overflow_the_scan_as_intended(eng):
    assert _ref("checkerboard-96x130", 1)[2] == 6240 and _ref("checkerboard-96x130", 2)[2] == 1
    assert eng.lib.lc_label_work_elems(96, 130, 1) == 13            # several tiles: the tile sums are scanned
    assert eng.lib.lc_label_work_elems(515, 513, 1) > 256           # more than one pass of the tile scan


@pytest.mark.parametrize("connectivity", [1, 2])
@pytest.mark.parametrize("name", list(CO.SEAM_CASES))
def test_the_seam_joins_only_when_cyclic(eng, name, connectivity):
    mask, lab, n = _ref(name, connectivity, True)
    labels, counts = eng.label_components(mask, connectivity, cyclic=True)
    assert int(counts[0]) == n and np.array_equal(_np(labels), lab)
    _, plain, n_plain = _ref(name, connectivity, False)
    labels, counts = eng.label_components(mask, connectivity, cyclic=False)
    assert int(counts[0]) == n_plain and np.array_equal(_np(labels), plain)
    if name.startswith("seam-2"):
        assert n < n_plain


BATCH = ["random-0.41", "serpentine-67x130", "random-0.9", "comb-67x130", "random-0.1"]


@pytest.mark.parametrize("connectivity", [1, 2])
def test_a_batch_equals_its_planes_one_by_one(eng, connectivity):
    stack = np.stack([CO.mask_of(n) for n in BATCH])
    labels, counts = eng.label_components(stack, connectivity)
    assert tuple(labels.shape) == stack.shape and tuple(counts.shape) == (len(BATCH),)
    for i, name in enumerate(BATCH):
        one, c = eng.label_components(stack[i], connectivity)
        assert np.array_equal(_np(labels[i]), _np(one)) and int(counts[i]) == int(c[0])
        _, lab, n = _ref(name, connectivity)
        assert np.array_equal(_np(labels[i]), lab) and int(counts[i]) == n
        assert _np(labels[i]).max() == n and (n == 0 or 1 in _np(labels[i]))     # the numbering restarts in every plane


def test_nan_is_background_and_negative_values_are_foreground(eng):
    mask, lab, n = _ref("nan-negative", 2)
    assert np.isnan(mask).any() and (mask < 0).any()
    got = _np(eng.label_components(mask)[0])
    assert np.array_equal(got, lab)
    assert not got[np.isnan(mask)].any() and got[mask < 0].all()


# ------------------------------------------------------------------ sums and properties
SUM_CASES = [("random-0.41", 2, False), ("random-0.59", 1, False), ("67x130", 2, False), ("seam-random-0.41", 2, True),
             ("seam-20x13", 2, True), ("seam-20x12", 1, True), ("checkerboard-96x130", 1, False), ("serpentine-67x130", 1, False),
             ("1x1", 2, False)]


@functools.lru_cache(maxsize=None)
def _props_ref(name, connectivity, cyclic, with_nan=False):
    mask, lab, n = _ref(name, connectivity, cyclic)
    v = CO.intensity_of(mask.shape) - 0.25          # both signs
    if with_nan:
        v[np.unravel_index(np.flatnonzero(lab == 1)[:1], lab.shape)] = np.nan      # in component 1
        v[np.unravel_index(np.flatnonzero(lab == 0)[:3], lab.shape)] = np.nan      # and on background
    v.setflags(write=False)
    return v, CO.sums(lab, n, v, cyclic), CO.props(lab, n, v, cyclic)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "f64"])
@pytest.mark.parametrize("name, connectivity, cyclic", SUM_CASES)
def test_integer_sums_and_extrema_equal_the_oracle(eng, name, connectivity, cyclic, dtype):
    mask, lab, n = _ref(name, connectivity, cyclic)
    v = _props_ref(name, connectivity, cyclic)[0].astype(dtype)
    ref = CO.sums(lab, n, v, cyclic)                 # of the values as the kernel sees them
    labels, counts = eng.label_components(mask, connectivity, cyclic)
    got = {k: _np(t) for k, t in eng.component_sums(labels, counts, v, cyclic).items()}
    assert got["area"].shape == (1, max(n, 1)) and got["moments"].shape == (5, 1, max(n, 1))
    assert np.array_equal(got["root"][0, :n], ref["root"]) and np.array_equal(got["area"][0, :n], ref["area"])
    assert np.array_equal(got["moments"][:, 0, :n], ref["moments"])
    assert np.array_equal(got["max"][0, :n], ref["max"]) and np.array_equal(got["min"][0, :n], ref["min"])
    assert got["max"].dtype == got["sum"].dtype == np.float64 and got["area"].dtype == np.int64


def test_a_capacity_above_and_below_the_count(eng):
    """Entries past a plane's count are empty (area 0, root -1, NaN extrema); labels past the capacity are not measured."""
    mask, lab, n = _ref("random-0.41", 2)
    v, ref, _ = _props_ref("random-0.41", 2, False)
    labels, counts = eng.label_components(mask)
    big = {k: _np(t) for k, t in eng.component_sums(labels, counts, v, n_max=n + 5).items()}
    assert np.array_equal(big["area"][0], np.concatenate([ref["area"], np.zeros(5, np.int64)]))
    assert (big["root"][0, n:] == -1).all() and np.isnan(big["max"][0, n:]).all() and (big["sum"][0, n:] == 0).all()
    assert not big["moments"][:, 0, n:].any()
    small = {k: _np(t) for k, t in eng.component_sums(labels, counts, v, n_max=3).items()}
    assert np.array_equal(small["area"][0], ref["area"][:3]) and np.array_equal(small["max"][0], ref["max"][:3])
    both = eng.torch.stack([labels, eng.torch.zeros_like(labels)])       # a plane without components beside it
    two = {k: _np(t) for k, t in eng.component_sums(both, eng.torch.tensor([n, 0], dtype=eng.torch.int32, device=eng.device),
                                                   np.stack([v, v])).items()}
    assert np.array_equal(two["area"][0], ref["area"]) and not two["area"][1].any() and (two["root"][1] == -1).all()


@pytest.mark.parametrize("name, connectivity, cyclic", SUM_CASES)
def test_mean_and_axis_moments_are_inside_their_bounds(eng, name, connectivity, cyclic):
    mask, lab, n = _ref(name, connectivity, cyclic)
    v, _, ref = _props_ref(name, connectivity, cyclic)
    labels, counts = eng.label_components(mask, connectivity, cyclic)
    got = {k: _np(t) for k, t in eng.component_props(labels, counts, v, cyclic).items()}
    assert got["area"].shape == (n,) and np.array_equal(got["area"], ref["area"])
    area = ref["area"].astype(np.float64)
    bound = area * EPS * ref["abs_sum"] / area
    err = np.abs(got["mean_intensity"] - ref["mean_intensity"])
    print(f"{name}: mean_intensity max err / bound {np.max(err / np.maximum(bound, 1e-300)):.3g}")
    assert (err <= bound).all()
    ac = ref["l1"] + ref["l2"]
    bound = 64 * EPS * ac
    for i, k in enumerate(("l1", "l2")):
        err = np.abs(got["axis_moments"][:, i] - ref[k])
        print(f"{name}: {k} max err {err.max():.3g}, smallest slack {np.min(bound - err):.3g}")
        assert (err <= bound).all(), k
    assert np.array_equal(got["max_intensity"], ref["max_intensity"]) and np.array_equal(got["min_intensity"], ref["min_intensity"])
    # the lengths are 4 sqrt of those, the centroid the root plus the mean offset
    assert np.allclose(got["major_axis_length"], ref["major_axis_length"], rtol=1e-12, atol=1e-7)
    assert np.allclose(got["centroid"], ref["centroid"], rtol=1e-13, atol=1e-12)


def test_a_nan_intensity_makes_its_component_nan_and_no_other(eng):
    mask, lab, n = _ref("random-0.41", 2)
    v, _, ref = _props_ref("random-0.41", 2, False, True)
    assert np.isnan(ref["mean_intensity"][0]) and not np.isnan(ref["mean_intensity"][1:]).any()
    labels, counts = eng.label_components(mask)
    got = {k: _np(t) for k, t in eng.component_props(labels, counts, v).items()}
    for k in ("mean_intensity", "max_intensity", "min_intensity"):
        assert np.isnan(got[k][0]) and not np.isnan(got[k][1:]).any(), k
    assert np.array_equal(got["max_intensity"][1:], ref["max_intensity"][1:])


def test_bars_have_the_axis_lengths_of_the_formula(eng):
    m = np.zeros((9, 40))
    lengths = [1, 2, 7, 30]
    for i, L in enumerate(lengths):
        m[2 * i, 3:3 + L] = 1
    labels, counts = eng.label_components(m)
    p = {k: _np(t) for k, t in eng.component_props(labels, counts).items()}
    assert "mean_intensity" not in p and list(p["area"]) == lengths
    assert np.allclose(p["major_axis_length"], [4 * np.sqrt((L * L - 1) / 12) for L in lengths], rtol=1e-15, atol=0)
    assert (p["minor_axis_length"] <= 4 * np.sqrt(64 * EPS * (np.array(lengths) ** 2 - 1) / 12)).all()      # l2 = 0 within its bound
    assert np.array_equal(p["centroid"], [[2 * i, 3 + (L - 1) / 2] for i, L in enumerate(lengths)])


# ------------------------------------------------------------------ the filter
FILTERS = [["area"], ["mean_intensity", "major_axis_length"], ["max_intensity"]]
FILTER_MASKS = [("random-0.1", False), ("random-0.41", False), ("random-0.59", False), ("random-0.9", False), ("seam-random-0.41", True)]


@functools.lru_cache(maxsize=None)
def _filter_ref(name, cyclic, criteria):
    """Intensity, thresholds and the properties they are away from.  A threshold is the midpoint between the median value of
    its property and the next larger one; the assertion below, on the oracle alone, is that no component lies within the
    comparison's error of it, so that the kept set cannot depend on the last bits."""
    mask, lab, n = _ref(name, 2, cyclic)
    v = CO.intensity_of(mask.shape, salt=1)
    p = CO.props(lab, n, v, cyclic)
    thresholds = []
    for k in criteria:
        vals = np.unique(p[k].astype(np.float64))
        i = min(len(vals) // 2, len(vals) - 1)
        th = vals[0] / 2 if len(vals) == 1 else (vals[i - 1] + vals[i]) / 2      # one value only: nothing to stand between
        area = p["area"].astype(np.float64)
        d = 64 * EPS * (p["l1"] + p["l2"])              # the bound on l1; the length is 4 sqrt of it, rounded twice more
        err = {"mean_intensity": area * EPS * p["abs_sum"] / area,
               "major_axis_length": 4 * (np.sqrt(p["l1"] + d) - np.sqrt(np.maximum(p["l1"] - d, 0))) + 8 * EPS * p["major_axis_length"]}.get(k, 0.0)
        assert (np.abs(p[k] - th) > err).all(), (name, k)
        thresholds.append(float(th))
    v.setflags(write=False)
    return v, tuple(thresholds)


@pytest.mark.parametrize("fill", [0.0, np.nan], ids=["fill0", "fillnan"])
@pytest.mark.parametrize("criteria", FILTERS, ids=["+".join(c) for c in FILTERS])
@pytest.mark.parametrize("name, cyclic", FILTER_MASKS)
def test_filter_components_equals_the_oracle(eng, name, cyclic, criteria, fill):
    mask = _ref(name, 2, cyclic)[0]
    v, thresholds = _filter_ref(name, cyclic, tuple(criteria))
    want = CO.filtered(mask, v, criteria, thresholds, 2, cyclic, fill)
    kept, all_ = np.count_nonzero(CO.foreground(want)), np.count_nonzero(CO.foreground(mask))
    assert 0 < kept and (kept < all_ or _ref(name, 2, cyclic)[2] == 1)      # some kept, some dropped wherever there are two
    got = _np(eng.filter_components(mask, v, criteria, thresholds, 2, cyclic, fill))
    assert got.dtype == mask.dtype and np.array_equal(got, want, equal_nan=True)


def test_filter_components_keeps_float32_and_a_stack(eng):
    names = ["random-0.41", "random-0.59", "random-0.1"]
    stack = np.stack([CO.mask_of(n) * 3 for n in names]).astype(np.float32)
    v = CO.intensity_of(stack.shape, np.float32, salt=2)
    want = np.stack([CO.filtered(stack[i], v[i], ["area"], [2.5], fill=-1.0) for i in range(3)])
    got = _np(eng.filter_components(stack, v, ["area"], [2.5], fill=-1.0))
    assert got.dtype == np.float32 and np.array_equal(got, want)
    with pytest.raises(ValueError, match="criterion"):
        eng.filter_components(stack, v, ["perimeter"], [1.0])
    with pytest.raises(ValueError, match="needs an intensity"):
        eng.filter_components(stack, None, ["mean_intensity"], [1.0])


# ------------------------------------------------------------------ the labelled surface
def test_filter_ridges_sorts_and_returns_the_callers_order():
    from LagrangianCoherence.LCS.tools import filter_ridges
    mask = _ref("random-0.41", 2)[0]
    v, thresholds = _filter_ref("random-0.41", False, ("mean_intensity", "major_axis_length"))
    ny, nx = mask.shape
    lat, lon = np.linspace(-33.0, 33.0, ny), np.linspace(-60.0, 69.0, nx)
    want = CO.filtered(mask, v, ["mean_intensity", "major_axis_length"], thresholds, fill=np.nan)
    # descending latitude, (longitude, latitude) order: the same field as the caller holds it
    ridges = DataArray(mask[::-1].T.copy(), ("longitude", "latitude"), {"latitude": lat[::-1], "longitude": lon}, name="ridges")
    ftle = DataArray(v[::-1].T.copy(), ("longitude", "latitude"), {"latitude": lat[::-1], "longitude": lon})
    out = filter_ridges(ridges, ftle, criteria=["mean_intensity", "major_axis_length"], thresholds=list(thresholds), fill=np.nan)
    assert type(out) is DataArray and out.dims == ("longitude", "latitude") and out.name == "ridges"
    assert np.array_equal(out.coords["latitude"], lat) and np.array_equal(out.coords["longitude"], lon)
    assert np.array_equal(out.values, want.T, equal_nan=True)


def test_filter_ridges_of_a_stack_equals_its_planes():
    from lagrangiancoherence_amd.tools import filter_ridges
    names = ["random-0.41", "random-0.59", "seam-random-0.41"]
    stack = np.stack([CO.mask_of(n) for n in names])
    v = CO.intensity_of(stack.shape, salt=3)
    ny, nx = stack.shape[1:]
    coords = {"time": np.arange(3), "latitude": np.linspace(-33.0, 33.0, ny), "longitude": np.linspace(-180.0, 177.0, nx)}
    kw = dict(criteria=["area", "max_intensity"], thresholds=[3, 0.9], cyclic=True, connectivity=1)
    dims = ("latitude", "time", "longitude")
    out = filter_ridges(DataArray(stack.transpose(1, 0, 2), dims, coords), DataArray(v.transpose(1, 0, 2), dims, coords), **kw)
    assert out.dims == dims and np.array_equal(out.coords["time"], coords["time"])
    for i in range(3):
        c2 = {k: coords[k] for k in ("latitude", "longitude")}
        one = filter_ridges(DataArray(stack[i], ("latitude", "longitude"), c2), DataArray(v[i], ("latitude", "longitude"), c2), **kw)
        assert np.array_equal(out.values[:, i, :], one.values)
        assert np.array_equal(one.values, CO.filtered(stack[i], v[i], kw["criteria"], kw["thresholds"], 1, True))
