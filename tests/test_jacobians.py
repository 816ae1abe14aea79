"""The designed cells of tests/jacobians.py on the CPU: the longdouble judge against the 50-digit fixture
(tests/golden/jacobians_mp.npz, written by tests/golden/make_jacobians_mp.py), the rule results of the numpy restatement of
csrc/flowmap_gradient.h's Gram and strain steps (tests/aux_gradient.py) on the cells built to reach each rule, and the table's
own claims: the designed ratios survive the planes' rounding, and the generic cells reach both sides of ``p >= q`` and the
``vx < 0`` flip.  What the kernels make of the same cells is tests/test_jacobians_gpu.py's."""
import numpy as np
import pytest

from tests import aux_gradient as AG
from tests import jacobians as JC

EPS = np.finfo(np.longdouble).eps
DTYPES = [np.float32, np.float64]


def _cells(t, cls):
    return t.cls == cls


@pytest.mark.parametrize("dtype", DTYPES)
def test_table_shape_and_classes(dtype):
    t = JC.table(dtype)
    ny, nx = t.cls.shape
    assert all(t.planes[k].shape == (ny, nx) and t.planes[k].dtype == dtype for k in AG.PLANES)
    assert t.seed_lat.shape == t.sep_lat.shape == (ny,) and t.sep_lon.shape == (nx,)
    assert set(np.unique(t.cls)) == set(JC.FINITE_CLASSES)
    assert all(np.isfinite(t.planes[k]).all() for k in AG.PLANES)
    assert len(t.index) == len(t.cells) and len(set(t.index.values())) == len(t.cells)
    assert 300 <= ny * nx <= 1200
    # both ends of the seed range, and the cells the float32 rows never reached
    assert {0.0, 60.0, 85.0, -85.0, 89.75, -89.75} <= {c.lat for c in t.cells if c.cls == "generic"}
    for c in t.cells:                                   # the metric is the nominal one: the row's and the column's separations
        r, k = t.index[c.name]
        assert t.seed_lat[r] == dtype(c.lat) and t.sep_lat[r] == dtype(2 * c.d_ns) and t.sep_lon[k] == dtype(2 * c.d_ew), c.name
    # the seam cells are what their names say
    r, k = t.index["seam_wrapped"]
    assert t.planes["x_e"][r, k] < -179.7 and t.planes["x_w"][r, k] > 179.6
    r, k = t.index["seam_unwrapped"]
    assert 180.1 < t.planes["x_e"][r, k] < 180.3
    kf = np.float32(np.pi) / np.float32(180)
    for name, lo, hi in (("seam_plus3960", 64.0, 80.0), ("seam_plus3420", 62.0, 64.0)):
        r, k = t.index[name]
        mean = np.float32(0.5) * (t.planes["x_e"][r, k].astype(np.float32) + t.planes["x_w"][r, k].astype(np.float32)) * kf
        assert lo <= abs(mean) < hi, (name, mean)
    half = sorted({float(abs(t.planes["x_e"] - t.planes["x_w"])[_cells(t, "wide")].max() / 2)} |
                  {round(float(v) / 2) for v in np.abs(t.planes["y_n"] - t.planes["y_s"])[_cells(t, "wide")]})
    assert {30, 50, 89} <= set(half)
    tiny = np.abs(t.planes["y_n"] - t.planes["y_s"])[_cells(t, "tiny")].max() / 2
    assert tiny <= 1.01 * JC.D_TINY[np.dtype(dtype)] + (4e-6 if dtype == np.float32 else 0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_judge_agrees_with_the_50_digit_fixture(dtype):
    """s1 and the reference layout's sigma to 8 eps relative, s2 to 8 eps s1, the direction to 8 eps / gap where gap > 1e-3
    (eps of longdouble), on every cell of the plane.  Measured: 2.0, 1.8, 1.5 and 1.6 eps at the most."""
    t = JC.table(dtype)
    mp = JC.load_mp(dtype)
    j = JC.judge(t.planes, t.seed_lat, t.sep_lat, t.sep_lon)
    jr = JC.judge(t.planes, t.seed_lat, t.sep_lat, t.sep_lon, "reference")
    s1 = mp["s1"]
    some = s1 > 0
    assert np.array_equal(some, t.cls != "collapsed") and np.all(j["s1"][~some] == 0) and np.all(j["s2"][~some] == 0)
    assert np.all(jr["sigma"][~some] == 0) and np.all(mp["sigma_reference"][~some] == 0)
    e1 = np.abs(j["s1"] - s1)[some] / s1[some]
    er = np.abs(jr["sigma"] - mp["sigma_reference"])[some] / mp["sigma_reference"][some]
    e2 = np.abs(j["s2"] - mp["s2"])[some] / s1[some]
    gap = 1 - (mp["s2"][some] / s1[some]) ** 2
    sn = (JC.sine(j["e_lon"], j["e_lat"], mp["e_lon"], mp["e_lat"])[some] * gap)[gap > 1e-3]
    print(f"{np.dtype(dtype).name}: judge against 50 digits, in eps: s1 {float(e1.max() / EPS):.2f} sigma(reference) "
          f"{float(er.max() / EPS):.2f} s2 / s1 {float(e2.max() / EPS):.2f} sine x gap {float(sn.max() / EPS):.2f}")
    assert e1.max() <= 8 * EPS and er.max() <= 8 * EPS and e2.max() <= 8 * EPS and sn.max() <= 8 * EPS
    assert (gap > 1e-3).sum() >= 100
    assert np.array_equal(j["sigma"], j["s1"]) and JC.sign_convention_holds(j["e_lon"], j["e_lat"])
    # the rule cells at 50 digits (the judge rotates by the longdouble pi / 2, whose cosine is -2.5e-20: it is held to the bounds
    # above there, not to zeros)
    for cls, e in (("rank_one_ew", (0, 1)), ("rank_one_ns", (1, 0)), ("collapsed", (1, 0))):
        m = _cells(t, cls)
        assert np.all(mp["s2"][m] == 0) and np.all(mp["e_lon"][m] == e[0]) and np.all(mp["e_lat"][m] == e[1]), cls
    m = _cells(t, "collapsed")
    assert np.all(j["e_lon"][m] == 1) and np.all(j["e_lat"][m] == 0)


@pytest.mark.parametrize("dtype", DTYPES)
def test_degree_reduced_derivatives_against_the_restatements(dtype):
    """The judge's derivative step against tests/aux_gradient.py's in longdouble.  That one rounds k and the product
    ``degrees x k`` (eps / 2 each, relative) before the sine or cosine, which carries angle x tan(angle) of it near a zero of the
    cosine -- 359 at the metric's cos(89.75 k) -- and the angle itself where the sine is of order one -- 72.3 rad in the
    shifted seam cell; a chord is a sum of two products of four such factors: 4 x 359 eps of |F| at the most.  Measured: 249
    eps (float32 plane), 204 eps (float64)."""
    t = JC.table(dtype)
    own = np.stack(JC.derivatives(t.planes, t.seed_lat, t.sep_lat, t.sep_lon))
    old = np.stack(AG.derivatives(t.planes, t.seed_lat, t.sep_lat, t.sep_lon, np.longdouble))
    scale = np.sqrt((own ** 2).sum(axis=0))
    assert np.array_equal(scale == 0, t.cls == "collapsed") and np.all(old[:, scale == 0] == 0)
    err = (np.abs(own - old).max(axis=0)[scale > 0] / scale[scale > 0]).max() / EPS
    amp = 4 * max(np.tan(np.deg2rad(89.75)) * np.deg2rad(89.75), np.deg2rad(3960.0 + 180.0))
    print(f"{np.dtype(dtype).name}: derivative steps differ by {float(err):.1f} eps of |F| (bound {amp:.0f})")
    assert err <= amp


def test_restatement_meets_the_rules_exactly_in_float64():
    t = JC.table(np.float64)
    r = AG.restatement(t.planes, t.seed_lat, t.sep_lat, t.sep_lon, np.float64)
    m = _cells(t, "collapsed")
    assert m.sum() >= 7
    for k, v in (("sigma", 0), ("s1", 0), ("s2", 0), ("e_lon", 1), ("e_lat", 0)):
        assert np.all(r[k][m] == v), k
    for cls, e in (("rank_one_ew", (0, 1)), ("rank_one_ns", (1, 0))):
        m = _cells(t, cls)
        assert m.sum() == 8 and np.all(r["s1"][m] > 0.5) and np.all(r["s2"][m] == 0), cls
        assert np.all(r["e_lon"][m] == e[0]) and np.all(r["e_lat"][m] == e[1]), cls
    m = _cells(t, "isotropic_exact")
    assert m.sum() == 1
    p, q, rr = r["p"][m][0], r["q"][m][0], r["r"][m][0]
    assert p == q and rr == 0 and p > 0                     # the n == 0 branch: vx = lam - q = 0, vy = r = 0
    assert r["lam"][m][0] == q
    assert (r["s1"][m][0], r["s2"][m][0], r["e_lon"][m][0], r["e_lat"][m][0]) == (np.sqrt(p), np.sqrt(p), 1.0, 0.0)
    # the same cells in float32 planes reach the same rules (the Gram and strain steps are float64 there too)
    t32 = JC.table(np.float32)
    r32 = AG.restatement(t32.planes, t32.seed_lat, t32.sep_lat, t32.sep_lon, np.float32)
    for cls, e in (("rank_one_ew", (0, 1)), ("rank_one_ns", (1, 0)), ("collapsed", (1, 0))):
        m = _cells(t32, cls)
        assert np.all(r32["s2"][m] == 0) and np.all(r32["e_lon"][m] == e[0]) and np.all(r32["e_lat"][m] == e[1]), cls


@pytest.mark.parametrize("dtype", DTYPES)
def test_designed_ratios_survive_the_rounding_of_the_planes(dtype):
    """s1 / s2 of the judge on the rounded planes within a factor 2 of every generic cell's designed ratio -- the table drops
    what does not survive (its docstring's generic row), no cell is left out here."""
    t = JC.table(dtype)
    j = JC.judge(t.planes, t.seed_lat, t.sep_lat, t.sep_lon)
    gen = [c for c in t.cells if c.cls == "generic"]
    ratios = sorted({c.ratio for c in gen})
    assert ratios[:2] == [1.5, 30.0 if dtype == np.float32 else 1e3] and {1.5, 1e3} <= set(ratios)
    assert (1e6 in ratios) == (dtype == np.float64)
    for lat in (0.0, 60.0, 85.0, -85.0, 89.75, -89.75):
        assert len({c.ratio for c in gen if c.lat == lat}) >= 2, lat
    worst = 0.0
    for c in gen:
        r, k = t.index[c.name]
        got = float(j["s1"][r, k] / j["s2"][r, k])
        assert c.ratio / 2 <= got <= c.ratio * 2, (c.name, got)
        worst = max(worst, abs(np.log2(got / c.ratio)))
        # and the designed direction is the cell's: the stretching direction is (cos beta, sin beta) up to its sign
        sn = float(JC.sine(j["e_lon"][r, k], j["e_lat"][r, k], np.cos(c.beta), np.sin(c.beta)))
        assert sn <= (0.2 if c.ratio >= 1e3 else 0.02), (c.name, sn)
    print(f"{np.dtype(dtype).name}: designed ratios kept within a factor {2 ** worst:.3f}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_generic_cells_reach_both_rows_and_the_flip(dtype):
    t = JC.table(dtype)
    r = AG.restatement(t.planes, t.seed_lat, t.sep_lat, t.sep_lon, dtype)
    g = _cells(t, "generic")
    p, q, rr = r["p"][g], r["q"][g], r["r"][g]
    flip = (rr < 0) & (p < q)                                  # vx = r < 0: the first sign flip
    print(f"{np.dtype(dtype).name}: {g.sum()} generic cells, p >= q in {(p >= q).sum()}, p < q in {(p < q).sum()}, flipped {flip.sum()}")
    assert (p >= q).sum() >= 20 and (p < q).sum() >= 20 and flip.sum() >= 7
    assert ((rr > 0) & (p < q)).sum() >= 7 and ((rr < 0) & (p >= q)).sum() >= 7
    # reflections: the sign of det of (E - W, N - S) in degrees is the sign of det J; both are there
    dets = [np.sign(np.linalg.det(np.array(c.values).reshape(4, 2)[[0, 2]] - np.array(c.values).reshape(4, 2)[[1, 3]]))
            for c in t.cells if c.cls == "generic"]
    assert len(dets) == g.sum() and dets.count(-1.0) >= 20 and dets.count(1.0) >= 20


def test_poisons_name_generic_cells_and_mixed_lines():
    for dtype in DTYPES:
        t = JC.table(dtype)
        ps = JC.poisons(t)
        assert [p[1] for p in ps[:8]] == list(AG.PLANES) and all(np.isnan(p[3]) for p in ps[:8])
        assert {p[3] for p in ps[8:10]} == {np.inf, -np.inf}
        assert len({p[2] for p in ps[:10]}) == 10 and all(t.cls[p[2]] == "generic" for p in ps[:10])
        (_, k1, (row, _), v1), (_, k2, (_, col), v2) = ps[10:]
        assert (k1, k2) == ("sep_lat", "sep_lon") and np.isnan(v1) and np.isnan(v2)
        assert len(set(t.cls[row, :])) >= 3 and len(set(t.cls[:, col])) >= 2
