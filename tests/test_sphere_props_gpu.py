"""The spherical ridge properties on the GPU (lc_component_sphere_sums, Engine.component_sphere_props, filter_components and
filter_ridges with metric='sphere', tools.ridge_properties) against the numpy restatement of tests/sphere_props.py, on the masks
of tests/components.py: one tile, several tiles, more tiles than one pass of the tile scan takes, runs of one label longer
than a thread's span (serpentine, foreground), thousands of one-pixel labels (checkerboards at connectivity 1), labels across
the seam, several planes per launch, NaN and negative mask values, both connectivities, both intensity dtypes, three grids
(uniform, Gaussian-like, global with the outer bands clipped at the poles).  The float buffers the module's engine allocates
start as NaN.

The device's terms are the restatement's terms bit for bit (the tables are equal: tests/test_sphere_props.py; the kernel
contracts nothing), so only the order of each sum differs.  Every bound is derived from the arithmetic in
tests/sphere_props.py:bounds and none from an output; each bounded comparison prints its largest error / bound ratio before
it asserts (pytest -s).  Roots, extrema, NaN patterns, labels and filtered masks are compared for equality.

Largest figures seen on an MI355X, as error / bound: raw sums W 0.63 (random-0.41, connectivity 1), S 0.65 (33x65,
connectivity 1), the nine moment sums 0.48-0.50; area 0.46, total_intensity 0.46, mean_intensity 0.35, minor_axis_length 0.18
(seam-random-0.59), major_axis_length 0.05, centroid latitude 0.16, longitude 0.12, orientation 0.02 -- 4.6e-13 degrees at
most, on every multi-pixel label the check admits (all but 1-3 of them per case, 8 of 9 on 33x65 at connectivity 2); a batch
against its planes one by one 0.17 of twice the bound; the owner map's totals add up to the field's within 0.03 of a bound
of 41 (in square metres times the field's unit, of a total near 2e14).  Roots, extrema, NaN patterns and filtered masks equal
everywhere.  Zonal lines of 40 pixels: 1282.59 km at 0.125 degrees, 638.87 km at 60.125 degrees, ratio 0.498111.
"""
import functools
import math

import numpy as np
import pytest

from tests import components as CO
from tests import sphere_props as SP
from tests.labelled import DataArray

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
R = 6371000.0
DTYPES = {"f32": np.float32, "f64": np.float64}
NAMES = ["2x2", "33x65", "67x130", "random-0.1", "random-0.41", "random-0.59", "random-0.9", "serpentine-67x130", "comb-67x130",
         "checkerboard-96x130", "checkerboard-515x513", "nan-negative", "foreground", "background"]
SEAM = ["seam-20x13", "seam-20x12", "seam-random-0.41", "seam-random-0.59", "seam-two-columns"]      # seam-one-column: see below
# (name, cyclic, grid): every case on the uniform grid, a few on the other two as well
GRIDS = ([(n, False, "uniform") for n in NAMES] + [(n, True, "uniform") for n in SEAM] +
         [("33x65", False, "gauss"), ("random-0.41", False, "global"), ("seam-random-0.41", True, "gauss"), ("nan-negative", False, "global")])
IDS = [f"{n}-{g}" for n, _, g in GRIDS]
# one label that spans the planet: its major axis is not a direction anyone can compare (exempt from the orientation check only)
SPANNING = {"foreground", "serpentine-67x130", "comb-67x130", "random-0.9", "checkerboard-96x130", "checkerboard-515x513"}
# where the issue states that the reference leaves at most 20 % of the multi-pixel labels out of the orientation check
ORIENTED = {"33x65", "67x130", "random-0.1", "random-0.41", "random-0.59"}
FLOATS = ("area", "major_axis_length", "minor_axis_length", "mean_intensity", "total_intensity")


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
def _ref(name, connectivity, cyclic, grid="uniform", dtype="f64"):
    """mask, labels, count, (lat, lon), the intensity as the kernel sees it, and the restatement's sums, properties, bounds."""
    mask = CO.mask_of(name)
    lab, n = CO.label(mask, connectivity, cyclic)
    lat, lon = SP.coordinates(mask.shape, grid)
    v = (CO.intensity_of(mask.shape) - 0.25).astype(DTYPES[dtype])          # both signs
    if name == "nan-negative":
        v[np.unravel_index(np.flatnonzero(lab == 1)[:1], lab.shape)] = np.nan      # in label 1
        v[np.unravel_index(np.flatnonzero(lab == 0)[:3], lab.shape)] = np.nan      # and on background
    s = SP.sums(lab, n, lat, lon, v.astype(np.float64), cyclic)
    p = SP.props(s, lat, lon, R)
    b = SP.bounds(s, p, R)
    for a in (mask, lab, v):
        a.setflags(write=False)
    return mask, lab, n, (lat, lon), v, s, p, b


def _device(eng, name, connectivity, cyclic, grid, dtype, **kw):
    mask, lab, n, (lat, lon), v, *_ = _ref(name, connectivity, cyclic, grid, dtype)
    labels, counts = eng.label_components(mask, connectivity, cyclic)
    assert int(counts[0]) == n and np.array_equal(_np(labels), lab)
    return {k: _np(t) for k, t in eng.component_sphere_props(labels, counts, lat, lon, v, cyclic, R, **kw).items()}


def _inside(what, got, ref, bound, factor=1.0):
    """NaN where the restatement has NaN, elsewhere |got - ref| <= factor * bound; returns the largest error / bound."""
    got, ref, bound = (np.asarray(a, dtype=np.float64) for a in (got, ref, bound))
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what
    ok = ~np.isnan(ref)
    err, lim = np.abs(got[ok] - ref[ok]), factor * bound[ok]
    assert not np.isnan(lim).any(), what
    ratio = float(np.max(err / np.maximum(lim, 1e-300), initial=0.0))
    assert (err <= lim).all(), f"{what}: largest error / bound {ratio:.3g} (error {err.max():.3g})"
    return ratio


def _stacked_sums(got):
    return np.concatenate([got["W"][None], np.moveaxis(got["M1"], -1, 0), np.moveaxis(got["M2"], -1, 0), got["S"][None]])


# ------------------------------------------------------------------ the raw sums
@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("connectivity", [1, 2])
@pytest.mark.parametrize("name, cyclic, grid", GRIDS, ids=IDS)
def test_raw_sums_are_inside_the_bound_of_a_float64_sum(eng, name, cyclic, grid, connectivity, dtype):
    """|error| <= area * 2^-53 * sum|term| for each of the eleven sums; roots and extrema equal, NaN rules included."""
    _, _, n, _, _, s, _, b = _ref(name, connectivity, cyclic, grid, dtype)
    got = _device(eng, name, connectivity, cyclic, grid, dtype, return_sums=True)
    assert got["W"].shape == (max(n, 1),) and got["M1"].shape == (max(n, 1), 3) and got["M2"].shape == (max(n, 1), 6)
    assert all(got[k].dtype == np.float64 for k in ("W", "M1", "M2", "S", "max_intensity")) and got["root"].dtype == np.int32
    if n == 0:          # capacity 1, nothing in it
        assert got["root"][0] == -1 and got["area"][0] == 0 and not _stacked_sums(got).any()
        assert all(np.isnan(got[k][0]) for k in got if k not in ("root", "area", "W", "M1", "M2", "S"))
        return
    assert np.array_equal(got["root"], s["root"])
    assert np.array_equal(got["max_intensity"], s["max"], equal_nan=True) and np.array_equal(got["min_intensity"], s["min"], equal_nan=True)
    G = _stacked_sums(got)
    ratios = [_inside(f"{name} {SP.NAMES[j]}", G[j], s["sums"][j], b["sums"][j]) for j in range(11)]
    print(f"{name}-{grid} c{connectivity} {dtype}: sums, largest error / bound " + " ".join(f"{SP.NAMES[j]} {r:.2f}" for j, r in enumerate(ratios)))


def test_one_longitude_has_no_width_and_is_refused(eng):
    mask = CO.mask_of("seam-one-column")
    labels, counts = eng.label_components(mask, 2, True)
    with pytest.raises(ValueError, match="at least two"):
        eng.component_sphere_props(labels, counts, np.linspace(-78.0, 81.0, mask.shape[0]), np.array([0.0]), cyclic=True)
    with pytest.raises(ValueError, match="len"):
        eng.component_sphere_props(labels, counts, np.linspace(-78.0, 81.0, 5), np.array([0.0, 1.0]))


# ------------------------------------------------------------------ the derived properties
@pytest.mark.parametrize("connectivity", [1, 2])
@pytest.mark.parametrize("name, cyclic, grid", GRIDS, ids=IDS)
def test_derived_properties_are_inside_their_bounds(eng, name, cyclic, grid, connectivity):
    _, _, n, _, _, s, p, b = _ref(name, connectivity, cyclic, grid)
    if n == 0:
        return
    # on the reference alone: no centroid near the 1e-6 rule, every direction bound in its linear range
    assert (p["rho"] >= 1e-5).all() and (b["centroid_turn"] <= 1e-3).all()
    got = _device(eng, name, connectivity, cyclic, grid, "f64")
    assert set(got) == {*FLOATS, "centroid_latitude", "centroid_longitude", "orientation", "max_intensity", "min_intensity"}
    line = [f"{k} {_inside(f'{name} {k}', got[k], p[k], b[k]):.2f}" for k in FLOATS]
    line.append(f"lat {_inside(f'{name} latitude', got['centroid_latitude'], p['centroid_latitude'], b['centroid_latitude']):.2f}")
    d = SP.angle_difference(got["centroid_longitude"], p["centroid_longitude"], 360.0)
    line.append(f"lon {_inside(f'{name} longitude', d, np.zeros(n), b['centroid_longitude']):.2f}")
    # orientation: NaN exactly where the restatement's is (one pixel); compared where the major axis is a direction
    assert np.array_equal(np.isnan(got["orientation"]), np.isnan(p["orientation"])) and np.array_equal(np.isnan(p["orientation"]), s["count"] == 1)
    assert ((got["orientation"] > -90.0) & (got["orientation"] <= 90.0))[s["count"] > 1].all()
    multi = s["count"] > 1
    inc = multi & (p["e"][:, 0] - p["e"][:, 1] >= 0.1 * p["e"][:, 0])
    if name in ORIENTED:
        assert multi.sum() - inc.sum() <= 0.2 * multi.sum(), (name, int(inc.sum()), int(multi.sum()))
    if name not in SPANNING and inc.any():
        assert (b["E_over_gap"][inc] <= 0.25).all()          # on the reference: the Davis-Kahan bound is in its range
        d = SP.angle_difference(got["orientation"][inc], p["orientation"][inc], 180.0)
        line.append(f"orientation {_inside(f'{name} orientation', d, np.zeros(int(inc.sum())), b['orientation'][inc]):.2f} "
                    f"({int(inc.sum())} of {int(multi.sum())} multi-pixel labels, largest {d.max():.3g} degrees)")
    print(f"{name}-{grid} c{connectivity}: error / bound " + ", ".join(line))


def test_without_an_intensity_there_are_no_intensity_columns(eng):
    mask, lab, n, (lat, lon), _, s, p, b = _ref("random-0.41", 2, False)
    labels, counts = eng.label_components(mask)
    got = {k: _np(t) for k, t in eng.component_sphere_props(labels, counts, lat, lon, return_sums=True).items()}
    assert set(got) == {"area", "major_axis_length", "minor_axis_length", "centroid_latitude", "centroid_longitude", "orientation",
                        "root", "W", "M1", "M2"}
    _inside("area", got["area"], p["area"], b["area"])
    _inside("major", got["major_axis_length"], p["major_axis_length"], b["major_axis_length"])


def test_a_capacity_above_and_below_the_count_and_a_plane_without_labels(eng):
    mask, lab, n, (lat, lon), v, s, p, b = _ref("random-0.41", 2, False)
    labels, counts = eng.label_components(mask)
    big = {k: _np(t) for k, t in eng.component_sphere_props(labels, counts, lat, lon, v, n_max=n + 5, return_sums=True).items()}
    assert (big["area"][n:] == 0).all() and (big["root"][n:] == -1).all() and not big["W"][n:].any()
    for k in ("major_axis_length", "minor_axis_length", "centroid_latitude", "centroid_longitude", "orientation", "mean_intensity",
              "total_intensity", "max_intensity", "min_intensity"):
        assert np.isnan(big[k][n:]).all(), k
    _inside("area", big["area"][:n], p["area"], b["area"])
    small = {k: _np(t) for k, t in eng.component_sphere_props(labels, counts, lat, lon, v, n_max=3).items()}
    assert small["area"].shape == (3,)
    _inside("area", small["area"], p["area"][:3], b["area"][:3])
    both = eng.torch.stack([labels, eng.torch.zeros_like(labels)])
    two = {k: _np(t) for k, t in eng.component_sphere_props(both, eng.torch.tensor([n, 0], dtype=eng.torch.int32, device=eng.device),
                                                            lat, lon, np.stack([v, v])).items()}
    _inside("area", two["area"][0], p["area"], b["area"])
    assert (two["area"][1] == 0).all() and np.isnan(two["mean_intensity"][1]).all()
    # a label map that skips a label: no pixel of label 2 in the plane
    gap = np.where(lab == 2, 0, lab).astype(np.int32)
    got = {k: _np(t) for k, t in eng.component_sphere_props(eng.torch.from_numpy(gap).to(eng.device), counts, lat, lon, v).items()}
    assert got["area"][1] == 0 and np.isnan(got["major_axis_length"][1]) and np.isnan(got["max_intensity"][1])
    _inside("area", np.delete(got["area"], 1), np.delete(p["area"], 1), np.delete(b["area"], 1))


BATCH = ["random-0.41", "serpentine-67x130", "random-0.9", "comb-67x130", "random-0.1"]


@pytest.mark.parametrize("connectivity", [1, 2])
def test_a_batch_equals_its_planes_one_by_one(eng, connectivity):
    """Integer parts and extrema equal; every float inside TWICE its bound (two device results, each inside once)."""
    refs = [_ref(n, connectivity, False) for n in BATCH]
    lat, lon = refs[0][3]
    stack, v = np.stack([r[0] for r in refs]), np.stack([r[4] for r in refs])
    labels, counts = eng.label_components(stack, connectivity)
    many = {k: _np(t) for k, t in eng.component_sphere_props(labels, counts, lat, lon, v, return_sums=True).items()}
    n_max = max(r[2] for r in refs)
    assert many["area"].shape == (len(BATCH), n_max) and many["M2"].shape == (len(BATCH), n_max, 6)
    worst = 0.0
    for i, (name, r) in enumerate(zip(BATCH, refs)):
        n, s, p, b = r[2], r[5], r[6], r[7]
        one = {k: _np(t) for k, t in eng.component_sphere_props(labels[i], counts[i:i + 1], lat, lon, v[i], return_sums=True).items()}
        assert np.array_equal(many["root"][i, :n], one["root"]) and (many["root"][i, n:] == -1).all() and (many["area"][i, n:] == 0).all()
        for k in ("max_intensity", "min_intensity"):
            assert np.array_equal(many[k][i, :n], one[k], equal_nan=True) and np.isnan(many[k][i, n:]).all()
        A, B = _stacked_sums({k: many[k][i, :n] for k in ("W", "M1", "M2", "S")}), _stacked_sums(one)
        for j in range(11):
            worst = max(worst, _inside(f"{name} {SP.NAMES[j]}", A[j], B[j], b["sums"][j], 2.0))
            _inside(f"{name} {SP.NAMES[j]} against the restatement", A[j], s["sums"][j], b["sums"][j])
        for k in FLOATS + ("centroid_latitude",):
            worst = max(worst, _inside(f"{name} {k}", many[k][i, :n], one[k], b[k], 2.0))
    print(f"batch c{connectivity}: largest |batch - single| / (2 bound) {worst:.2f}")


# ------------------------------------------------------------------ closed cases through ridge_properties
def _quarter_degree():
    lat, lon = -89.875 + 0.25 * np.arange(720), -180.0 + 0.25 * np.arange(1440)
    assert lat[360] == 0.125 and lat[600] == 60.125
    return lat, lon


def test_lines_on_the_quarter_degree_grid():
    from LagrangianCoherence.LCS.tools import ridge_properties
    lat, lon = _quarter_degree()
    m = np.zeros((720, 1440))
    m[200, :5] = m[200, 1435:] = 1          # 5 + 5 pixels across the seam
    m[300:340, 700] = 1                     # meridional
    m[360, 100:140] = 1                     # zonal, 0.125 degrees
    m[600, 100:140] = 1                     # zonal, 60.125 degrees
    coords = {"latitude": lat, "longitude": lon}
    ridges = DataArray(m, ("latitude", "longitude"), coords, name="ridges")
    labels, t = ridge_properties(ridges, cyclic=True)
    assert type(labels) is DataArray and labels.values.dtype == np.int32 and labels.dims == ridges.dims and labels.name == "ridges"
    assert list(t["label"]) == [1, 2, 3, 4] and not t["plane"].any() and "mean_intensity" not in t and "centroid_row" not in t
    assert labels.values[200, 0] == labels.values[200, 1439] == 1 and labels.values[600, 120] == 4          # one ridge across the seam
    major = t["major_axis_length"]
    ratio = math.cos(math.radians(60.125)) / math.cos(math.radians(0.125))
    print(f"zonal lines of 40 pixels: {major[2] / 1e3:.2f} km at 0.125, {major[3] / 1e3:.2f} km at 60.125, ratio {major[3] / major[2]:.6f} (cos ratio {ratio:.6f})")
    assert abs(major[3] / major[2] / ratio - 1) <= 1e-3
    assert abs(major[2] - 1282.59e3) <= 10.0 and abs(major[3] - 638.87e3) <= 10.0          # the numpy prototype's figures, to their last digit
    assert (SP.angle_difference(t["orientation"], [0.0, 90.0, 0.0, 0.0], 180.0) <= 1e-6).all()
    # latitudes: the mean of an arc's nodes lies polewards of it (0.002 degrees), cell areas pull a meridional line's centroid
    # towards the equator (0.026 degrees)
    assert abs(t["centroid_longitude"][0] - 179.875) <= 1e-9 and abs(t["centroid_latitude"][0] - lat[200]) <= 0.01
    assert abs(t["centroid_longitude"][1] - lon[700]) <= 1e-9 and abs(t["centroid_latitude"][1] - (lat[300] + lat[339]) / 2) <= 0.05
    # without cyclic the seam cuts the ridge in two; the index metric cannot tell the two zonal lines apart
    labels, ti = ridge_properties(ridges, metric="index")
    assert list(ti["label"]) == [1, 2, 3, 4, 5] and "orientation" not in ti
    assert np.allclose(ti["major_axis_length"][3:], 4 * math.sqrt((40 * 40 - 1) / 12), rtol=1e-14) and abs(ti["major_axis_length"][3] - 46.17) < 5e-3
    assert np.array_equal(ti["centroid_row"][3:], [360.0, 600.0]) and np.array_equal(ti["centroid_column"][3:], [119.5, 119.5])
    assert np.array_equal(ti["area"], [5, 5, 40, 40, 40]) and ti["area"].dtype == np.int64


# ------------------------------------------------------------------ labelled=True
def test_owner_map_totals_equal_the_restatement_and_add_up_to_the_field(eng):
    from LagrangianCoherence.LCS.tools import distance_to_ridges, ridge_properties
    mask, lab, n, (lat, lon), v, *_ = _ref("33x65", 2, False)
    coords = {"latitude": lat, "longitude": lon}
    ridges = DataArray(mask, ("latitude", "longitude"), coords)
    rain = DataArray(np.abs(v) + 0.1, ("latitude", "longitude"), coords)
    _, owner = distance_to_ridges(ridges, return_labels=True, connectivity=2)
    assert owner.values.min() >= 1 and owner.values.max() == n          # every pixel belongs to some ridge's area of influence
    labels, t = ridge_properties(owner, rain, labelled=True)
    assert np.array_equal(labels.values, owner.values) and labels.values.dtype == np.int32
    s = SP.sums(owner.values, n, lat, lon, rain.values)
    p = SP.props(s, lat, lon, R)
    b = SP.bounds(s, p, R)
    some = s["count"] > 0
    assert np.array_equal(t["label"], np.flatnonzero(some) + 1) and not t["plane"].any()
    for k in FLOATS:
        print(f"owner map {k}: error / bound {_inside(k, t[k], p[k][some], b[k][some]):.2f}")
    assert np.array_equal(t["max_intensity"], s["max"][some]) and np.array_equal(t["min_intensity"], s["min"][some])
    # over all owners: the field's area-weighted total; each row inside its bound, the exact total rounded once
    _, _, rw, _, _, cw = SP.tables(lat, lon)
    exact = R * R * math.fsum((np.outer(rw, cw) * rain.values).ravel())
    err, bound = abs(math.fsum(t["total_intensity"]) - exact), float(b["total_intensity"][some].sum()) + 4 * EPS * exact
    print(f"owner map: sum of totals off by {err:.3g}, bound {bound:.3g}")
    assert err <= bound


def test_track_ids_give_one_row_per_plane_and_track(eng):
    from LagrangianCoherence.LCS.tools import ridge_properties, track_ridges
    base = CO.mask_of("random-0.1")
    record = np.stack([base, np.roll(base, 1, axis=1), np.roll(base, 2, axis=1) * (np.arange(base.shape[0]) % 3 != 0)[:, None]])
    lat, lon = SP.coordinates(base.shape)
    dims, coords = ("time", "latitude", "longitude"), {"time": np.arange(3), "latitude": lat, "longitude": lon}
    v = CO.intensity_of(record.shape, salt=5)
    ids = track_ridges(DataArray(record, dims, coords), reach=1, cyclic=True)
    field = DataArray(v, dims, coords)
    labels, t = ridge_properties(ids, field, labelled=True, cyclic=True)
    assert np.array_equal(labels.values, ids.values) and labels.dims == dims
    rows = 0
    for i in range(3):
        here = t["plane"] == i
        present = np.unique(ids.values[i])
        present = present[present > 0]
        assert np.array_equal(t["label"][here], present)          # one row per (plane, track), by plane and then by label
        _, one = ridge_properties(ids.isel(time=i), field.isel(time=i), labelled=True, cyclic=True)
        assert np.array_equal(one["label"], present) and not one["plane"].any()
        s = SP.sums(ids.values[i], int(ids.values.max()), lat, lon, v[i], True)
        p = SP.props(s, lat, lon, R)
        b = SP.bounds(s, p, R)
        some = s["count"] > 0
        for k in FLOATS + ("centroid_latitude",):
            _inside(f"plane {i} {k}", t[k][here], one[k], b[k][some], 2.0)
            _inside(f"plane {i} {k} against the restatement", t[k][here], p[k][some], b[k][some])
        assert np.array_equal(t["max_intensity"][here], one["max_intensity"]) and np.array_equal(t["min_intensity"][here], s["min"][some])
        rows += int(here.sum())
    assert rows == t["label"].size and len({a.size for a in t.values()}) == 1
    bad = ids.copy(ids.values.astype(np.float64))
    bad.values[0, 3, 3] = 2.5
    with pytest.raises(ValueError, match="whole number"):
        ridge_properties(bad, labelled=True)


# ------------------------------------------------------------------ the filter
FILTERS = [["area"], ["mean_intensity", "major_axis_length"], ["max_intensity"], ["minor_axis_length"]]
FILTER_MASKS = [("random-0.1", False), ("random-0.41", False), ("random-0.59", False), ("seam-random-0.41", True)]


@functools.lru_cache(maxsize=None)
def _filter_ref(name, cyclic, criteria):
    """Thresholds at the midpoint between two neighbouring sorted reference values of each property, chosen -- on the restatement
    alone -- to lie further from every label's value than that label's bound: no last bit flips a decision."""
    mask, lab, n, (lat, lon), v, s, p, b = _ref(name, 2, cyclic)
    p = dict(p, max_intensity=s["max"], min_intensity=s["min"])
    thresholds = []
    for k in criteria:
        vals = np.unique(p[k])
        assert len(vals) >= 2
        # from the median pair upwards, the first pair whose midpoint no label's bound reaches (minor axes of thin ridges are
        # zero within a bound of decimetres: a threshold among them would be decided by rounding)
        mids = [(vals[i - 1] + vals[i]) / 2 for i in range(len(vals) // 2, len(vals))]
        safe = [th for th in mids if (np.abs(p[k] - th) > b.get(k, np.zeros(n))).all()]
        assert safe, (name, k)
        thresholds.append(float(safe[0]))
    return tuple(thresholds)


@pytest.mark.parametrize("fill", [0.0, np.nan], ids=["fill0", "fillnan"])
@pytest.mark.parametrize("criteria", FILTERS, ids=["+".join(c) for c in FILTERS])
@pytest.mark.parametrize("name, cyclic", FILTER_MASKS)
def test_filter_components_on_the_sphere_equals_the_restatement(eng, name, cyclic, criteria, fill):
    mask, _, n, (lat, lon), v, *_ = _ref(name, 2, cyclic)
    thresholds = _filter_ref(name, cyclic, tuple(criteria))
    want = SP.filtered(mask, v, criteria, thresholds, lat, lon, 2, cyclic, fill, R)
    kept, all_ = np.count_nonzero(CO.foreground(want)), np.count_nonzero(CO.foreground(mask))
    assert 0 < kept < all_
    got = _np(eng.filter_components(mask, v, criteria, thresholds, 2, cyclic, fill, metric="sphere", lat=lat, lon=lon, radius=R))
    assert got.dtype == mask.dtype and np.array_equal(got, want, equal_nan=True)
    with pytest.raises(ValueError, match="needs lat and lon"):
        eng.filter_components(mask, v, criteria, thresholds, metric="sphere")
    with pytest.raises(ValueError, match="metric"):
        eng.filter_components(mask, v, criteria, thresholds, metric="km")


def test_filter_ridges_index_is_unchanged_and_the_sphere_keeps_another_set():
    from LagrangianCoherence.LCS.tools import filter_ridges
    mask, _, _, (lat, lon), v, *_ = _ref("random-0.41", 2, False)
    criteria = ["mean_intensity", "major_axis_length"]
    thresholds = list(_filter_ref("random-0.41", False, tuple(criteria)))
    # descending latitude, (longitude, latitude) order, a stack of two planes: the same field as the caller holds it
    dims = ("longitude", "time", "latitude")
    coords = {"latitude": lat[::-1], "longitude": lon, "time": np.arange(2)}
    stack = np.stack([mask, np.roll(mask, 7, axis=1)])
    vv = np.stack([v, v])
    ridges = DataArray(stack[:, ::-1].transpose(2, 0, 1).copy(), dims, coords, name="ridges")
    ftle = DataArray(vv[:, ::-1].transpose(2, 0, 1).copy(), dims, coords)
    out = filter_ridges(ridges, ftle, criteria, thresholds, fill=np.nan, metric="sphere")
    assert type(out) is DataArray and out.dims == dims and out.name == "ridges"
    want0 = SP.filtered(mask, v, criteria, thresholds, lat, lon, fill=np.nan)
    assert np.array_equal(out.values[:, 0, :], want0.T, equal_nan=True)
    one = filter_ridges(DataArray(mask, ("latitude", "longitude"), {"latitude": lat, "longitude": lon}),
                        DataArray(v, ("latitude", "longitude"), {"latitude": lat, "longitude": lon}), criteria, thresholds, fill=np.nan,
                        metric="sphere")
    assert np.array_equal(one.values, want0, equal_nan=True)
    # metric='index' is the call without the keyword, byte for byte
    index_thresholds = [thresholds[0], 3.0]
    a = filter_ridges(ridges, ftle, criteria, index_thresholds, fill=np.nan)
    b = filter_ridges(ridges, ftle, criteria, index_thresholds, fill=np.nan, metric="index", radius=1.0)
    assert a.values.tobytes() == b.values.tobytes() and a.dims == b.dims
    assert np.array_equal(a.values[:, 0, :], CO.filtered(mask, v, criteria, index_thresholds, fill=np.nan).T, equal_nan=True)


def test_two_equal_pixel_lengths_are_kept_differently_by_the_two_metrics():
    from LagrangianCoherence.LCS.tools import filter_ridges
    lat, lon = _quarter_degree()
    rows = slice(340, 620)          # both lines and the latitudes between them: a quarter of the planet is enough
    m = np.zeros((720, 1440), np.float32)
    m[360, 100:140] = 1             # 1282.59 km
    m[600, 100:140] = 1             # 638.87 km
    coords = {"latitude": lat[rows], "longitude": lon}
    ridges = DataArray(m[rows], ("latitude", "longitude"), coords)
    ftle = DataArray(np.ones_like(m[rows]), ("latitude", "longitude"), coords)
    by_index = filter_ridges(ridges, ftle, ["major_axis_length"], [30])          # the driver's 30 pixels: both are 46.17
    assert by_index.values.dtype == np.float32 and np.array_equal(by_index.values, m[rows])
    on_sphere = filter_ridges(ridges, ftle, ["major_axis_length"], [830e3], metric="sphere")      # what 30 pixels stands for
    want = m[rows].copy()
    want[600 - 340] = 0
    assert np.array_equal(on_sphere.values, want) and not np.array_equal(on_sphere.values, by_index.values)
    assert np.array_equal(filter_ridges(ridges, ftle, ["major_axis_length", "area"], [600e3, 1e9], metric="sphere").values, m[rows])
