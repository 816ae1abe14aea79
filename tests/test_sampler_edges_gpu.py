"""The point sampler (``sample_kernel``, ``tracer_kernel``: ``locate`` + ``fetch`` in csrc/advect.hip) on the edges of its
index map, on the MI355X.  The battery and the generic grid are tests/sampler_edges.py's; test_sampler_edges.py proves
without a GPU what is relied on here.  Every expected value comes from ``O.xr_map_coordinates`` (scipy), never the engine."""
import numpy as np
import pytest

from oracle import lcs_oracle as O
from tests import sampler_edges as SE
from tests.test_tracer_gpu import _mean_within_one_ulp

pytestmark = pytest.mark.gpu

LAT, LON = SE.dyadic_grid()
U, V = SE.dyadic_field()
FMAX = float(max(np.abs(U).max(), np.abs(V).max()))
BOTH = (np.float64, np.float32)


@pytest.fixture(scope="module")
def eng():
    from lagrangiancoherence_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _np(t):
    return t.cpu().numpy()


_FIELDS = {}


def _field(eng, dtype, order, **kw):
    """The dyadic field, packed once per (dtype, order, options) and shared (nothing writes to it)."""
    key = (np.dtype(dtype).name, order, tuple(sorted(kw.items())))
    if key not in _FIELDS:
        _FIELDS[key] = eng.prepare_field(U.astype(dtype), V.astype(dtype), LAT.astype(dtype), LON.astype(dtype), order, **kw)
    return _FIELDS[key]


@pytest.fixture(scope="module", autouse=True)
def _drop_fields():
    yield
    _FIELDS.clear()


_ORACLE = {}


def _oracle(dtype, order, level=SE.LEVEL, shift=0.0):
    """``(u, v)`` of the oracle on the battery, on the field as ``dtype`` holds it: for float32 both the float64 answer on the
    float32-valued field and the float32 oracle's own."""
    key = (np.dtype(dtype).name, order, level, shift)
    if key not in _ORACLE:
        px, py = SE.battery(order, shift)
        res = []
        for f in (U[level], V[level]):
            f = f.astype(dtype)
            want = O.xr_map_coordinates(f.astype(np.float64), LAT, LON, px, py, order=order)
            own = O.xr_map_coordinates(f, LAT.astype(dtype), LON.astype(dtype), px.astype(dtype), py.astype(dtype), order=order)
            res.append((want, own))
        _ORACLE[key] = res
    return _ORACLE[key]


def _sample(eng, field, px, py, order, dtype, level=SE.LEVEL, **kw):
    su, sv = eng.sample(field, px.astype(dtype), py.astype(dtype), level=level, interp_order=order, **kw)
    return _np(su), _np(sv)


def _check_zeros(got, want, order, what):
    pole = SE.pole_mask(order, len(got))
    assert np.array_equal(got[pole] == 0, want[pole] == 0), f"{what}: a constant row's zeros are not the oracle's"
    assert np.all(got[~pole] != 0), what


# ------------------------------------------------------------------ float64, the dyadic battery
@pytest.mark.parametrize("order", SE.ORDERS)
def test_float64_on_the_dyadic_battery_vs_oracle(eng, order):
    px, py = SE.battery(order)
    got = _sample(eng, _field(eng, np.float64, order), px, py, order, np.float64)
    for g, (want, _), name in zip(got, _oracle(np.float64, order), "uv"):
        err = np.abs(g - want)
        print(f"float64 order {order} {name}: max err {err.max():.3e} (tolerance {SE.TOL64[order]:.0e})")
        assert err.max() <= SE.TOL64[order], (name, int(err.argmax()) % 1600, err.max())
        _check_zeros(g, want, order, f"float64 order {order} {name}")


# ------------------------------------------------------------------ float64, the generic grid with ulp neighbours
@pytest.mark.parametrize("order", SE.GENERIC_ORDERS)
def test_float64_on_the_generic_grid_lands_on_the_oracles_side_of_every_jump(eng, order):
    lat, lon = SE.generic_grid()
    u, v = SE.generic_field()
    px, py, _ = SE.generic_points(order)
    f = eng.prepare_field(u, v, lat, lon, order)
    got = _sample(eng, f, px, py, order, np.float64)
    for g, fld, name in zip(got, (u, v), "uv"):
        want = O.xr_map_coordinates(fld[SE.LEVEL], lat, lon, px, py, order=order)
        err = np.abs(g - want)
        print(f"float64 order {order} {name}, generic grid: max err {err.max():.3e} (tolerance {SE.TOL64[order]:.0e})")
        assert err.max() <= SE.TOL64[order], (name, np.unravel_index(err.argmax(), err.shape), err.max())
        pole = SE.pole_mask(order)
        assert np.array_equal(g[pole] == 0, want[pole] == 0)


# ------------------------------------------------------------------ float32, the dyadic battery, no point left out
@pytest.mark.parametrize("order", SE.ORDERS)
def test_float32_on_the_dyadic_battery_vs_oracle(eng, order):
    """Judged against the float64 oracle on the same float32-valued inputs, inside test_sampler_on_own_trajectories_vs_oracle's
    bound: 4 x the float32 oracle's own maximum error + 1e-6 max|field|.  Measured on an MI355X (the larger of u and v; the
    float32 oracle's own error is 6.0e-8 .. 1.1e-7, the bound 4.2e-6 .. 4.4e-6; ``pytest -s`` prints every figure):
    order 1: 2.1e-7, order 2: 2.4e-7, order 3: 1.3e-6, order 4: 7.3e-7, order 5: 1.6e-6."""
    px, py = SE.battery(order)
    got = _sample(eng, _field(eng, np.float32, order), px, py, order, np.float32)
    for g, (want, own), name in zip(got, _oracle(np.float32, order), "uv"):
        assert g.dtype == np.float32
        e_gpu = np.abs(g.astype(np.float64) - want)
        e_or = np.abs(own.astype(np.float64) - want).max()
        bound = SE.f32_bound(e_or, FMAX)
        print(f"float32 order {order} {name}: max err {e_gpu.max():.3e} (float32 oracle's own {e_or:.3e}, bound {bound:.3e})")
        assert e_gpu.max() <= bound, (name, int(e_gpu.argmax()) % 1600, e_gpu.max(), bound)
        _check_zeros(g, want, order, f"float32 order {order} {name}")


# ------------------------------------------------------------------ sources: raw planes against the lin image
@pytest.mark.parametrize("dtype,order", [(np.float64, 1), (np.float64, 3), (np.float32, 3)])
def test_raw_planes_and_lin_image_give_the_same_bits(eng, dtype, order):
    """The order-1 source (every row at order 1, the pole rows at order 3) is the raw planes by default and the lin image with
    ``lin_image=True``; float32 at order 1 has the image only."""
    px, py = SE.battery(order)
    raw, lin = _field(eng, dtype, order), _field(eng, dtype, order, lin_image=True)
    assert raw.lin is None and raw.u is not None and lin.lin is not None and lin.u is None
    a, b = _sample(eng, raw, px, py, order, dtype), _sample(eng, lin, px, py, order, dtype)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.isfinite(a[0]).all()


# ------------------------------------------------------------------ row blocks
@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("order", SE.ORDERS)
def test_row_blocks_equal_the_rows_of_the_whole_call(eng, dtype, order):
    px, py = SE.battery(order)
    rows = len(px)
    f = _field(eng, dtype, order)
    whole = _sample(eng, f, px, py, order, dtype)
    for a, b in ((0, order), (order - 1, order + 2), (rows - order - 1, rows)):
        part = _sample(eng, f, px[a:b], py[a:b], order, dtype, row0=a, ny_global=rows)
        assert np.array_equal(part[0], whole[0][a:b]) and np.array_equal(part[1], whole[1][a:b]), (a, b)


# ------------------------------------------------------------------ sample_kernel's grid-stride loop
def test_the_grid_stride_loop_equals_two_calls_under_the_cap_and_the_oracle(eng):
    """float32, order 1, one interior row of 8192 * 256 + 257 positions (the battery tiled): beyond the grid's 8192 x 256
    threads the kernel's loop takes a second trip."""
    n = SE.STRIDE_POSITIONS
    bx, by = SE.battery(1)
    reps = -(-n // 1600)
    px = np.tile(bx[0], reps)[:n].astype(np.float32)[None]
    py = np.tile(by[0], reps)[:n].astype(np.float32)[None]
    f = _field(eng, np.float32, 1)
    kw = dict(level=SE.LEVEL, interp_order=1, row0=1, ny_global=3)
    px_d, py_d = eng.to_device(px, np.float32), eng.to_device(py, np.float32)
    one = eng.sample(f, px_d, py_d, **kw)
    h = n // 2
    assert h <= SE.SAMPLE_GRID_CAP * SE.SAMPLE_BLOCK and n - h <= SE.SAMPLE_GRID_CAP * SE.SAMPLE_BLOCK
    lo = eng.sample(f, px_d[:, :h].contiguous(), py_d[:, :h].contiguous(), **kw)
    hi = eng.sample(f, px_d[:, h:].contiguous(), py_d[:, h:].contiguous(), **kw)
    for k in range(2):
        assert eng.torch.equal(one[k][:, :h], lo[k]) and eng.torch.equal(one[k][:, h:], hi[k])
    for sl in (slice(0, 1600), slice(n - 1600, n)):
        x, y = px[0, sl].astype(np.float64), py[0, sl].astype(np.float64)
        for k, fld in enumerate((U, V)):
            f32 = fld[SE.LEVEL].astype(np.float32)
            want = O.xr_map_coordinates(f32.astype(np.float64), LAT, LON, np.tile(x, (3, 1)), np.tile(y, (3, 1)), order=1)[1]
            own = O.xr_map_coordinates(f32, LAT.astype(np.float32), LON.astype(np.float32), np.tile(px[0, sl], (3, 1)),
                                       np.tile(py[0, sl], (3, 1)), order=1)[1]
            e_or = np.abs(own.astype(np.float64) - want).max()
            e_gpu = np.abs(_np(one[k][0, sl]).astype(np.float64) - want).max()
            assert e_gpu <= SE.f32_bound(e_or, FMAX), (sl, k, e_gpu, e_or)


# ------------------------------------------------------------------ tracer_walk's register ring
@pytest.mark.parametrize("dtype,order", [(np.float64, 3), (np.float32, 1)])
def test_tracer_ring_entries_equal_the_sampler_level_by_level(eng, dtype, order):
    """Every entry of the trajectory is the battery, entry j moved by j / 8 index units, for trajectories shorter than, as long
    as and longer than the ring of TRACER_DEPTH = 4: entry j's values are ``eng.sample`` at level j on entry j's positions."""
    torch = eng.torch
    tr = eng.prepare_tracer(U.astype(dtype), V.astype(dtype), LAT.astype(dtype), LON.astype(dtype), order)
    f = _field(eng, dtype, order)
    pos = [SE.battery(order, 0.125 * j) for j in range(SE.NT)]
    tx = eng.to_device(np.stack([p[0] for p in pos]).astype(dtype), dtype)
    ty = eng.to_device(np.stack([p[1] for p in pos]).astype(dtype), dtype)
    per_level = [eng.sample(f, tx[j], ty[j], level=j, interp_order=order) for j in range(SE.NT)]
    name = f"tracer_kernel<{'double' if dtype == np.float64 else 'float'}, {order}>"
    for nl in SE.RING_LEVELS:
        (c1, c2), (m1, m2) = eng.sample_tracer(tr, tx[:nl].contiguous(), ty[:nl].contiguous(), 0, order, mean_count=nl)
        assert eng.last_tracer_kernel() == name
        assert tuple(c1.shape) == (nl, SE.seed_rows(order), 1600)
        for j in range(nl):
            assert torch.equal(c1[j], per_level[j][0]) and torch.equal(c2[j], per_level[j][1]), (nl, j)
        _mean_within_one_ulp(_np(m1), _np(c1))
        _mean_within_one_ulp(_np(m2), _np(c2))
    # and the sampler itself is the oracle's on a moved entry (entry 0 is the battery of the tests above)
    j = SE.NT - 1
    for g, (want, own) in zip(per_level[j], _oracle(dtype, order, level=j, shift=0.125 * j)):
        e = np.abs(_np(g).astype(np.float64) - want).max()
        assert e <= (SE.TOL64[order] if dtype == np.float64 else SE.f32_bound(np.abs(own.astype(np.float64) - want).max(), FMAX)), e


# ------------------------------------------------------------------ non-finite positions
NAN, INF = float("nan"), float("inf")
# (x, y) in index coordinates; "in" is a finite coordinate inside the field, off the nodes
BAD = [(b, "in") for b in (NAN, INF, -INF)] + [("in", b) for b in (NAN, INF, -INF)] + [(b, b) for b in (NAN, INF, -INF)] + \
      [(NAN, INF), (-INF, NAN), (INF, -INF)]


@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("order", SE.ORDERS)
def test_non_finite_positions(eng, dtype, order):
    """The rule of ``lc_sample`` (include/lcs_hip.h) for positions that are not finite, at every order:

    - a NaN coordinate gives NaN (on a constant row too, while the other coordinate is inside the field);
    - an infinite coordinate gives NaN on a wrap row (scipy's wrap of it is ``inf - inf``);
    - an infinite coordinate gives exactly 0 on a constant row: it is outside, and there outside wins whatever the other
      coordinate is;
    - every finite position of the same call gets the bits of a call without the non-finite ones.

    This departs from scipy on purpose: scipy 1.15 returns 0 for a NaN or ``-inf`` coordinate on a wrap row, because it casts the
    coordinate to an integer, which is undefined for such a value; so there is no oracle value to compare with here."""
    px, py = SE.battery(order)
    rows = len(px)
    x_in, y_in = LON[0] + 8.0 * 2.5, LAT[0] + 8.0 * 1.5
    bx = np.array([x_in if x == "in" else x for x, _ in BAD])
    by = np.array([y_in if y == "in" else y for _, y in BAD])
    # the non-finite columns in the middle of the finite ones
    qx = np.concatenate([px[:, :800], np.tile(bx, (rows, 1)), px[:, 800:]], axis=1)
    qy = np.concatenate([py[:, :800], np.tile(by, (rows, 1)), py[:, 800:]], axis=1)
    f = _field(eng, dtype, order)
    clean = _sample(eng, f, px, py, order, dtype)
    mixed = _sample(eng, f, qx, qy, order, dtype)
    pole = SE.pole_mask(order)
    nb = len(BAD)
    has_nan = np.array([(x != "in" and np.isnan(x)) or (y != "in" and np.isnan(y)) for x, y in BAD])
    has_inf = np.array([(x != "in" and np.isinf(x)) or (y != "in" and np.isinf(y)) for x, y in BAD])
    for got, ref in zip(mixed, clean):
        assert np.array_equal(got[:, :800], ref[:, :800]) and np.array_equal(got[:, 800 + nb:], ref[:, 800:])
        bad = got[:, 800:800 + nb]
        assert np.isnan(bad[~pole]).all(), (order, np.argwhere(~np.isnan(bad[~pole])).tolist())
        assert np.all(bad[pole][:, has_inf] == 0), order
        assert np.isnan(bad[pole][:, has_nan & ~has_inf]).all(), order
    # the tracer kernel follows the same rule (one entry; its c1 / c2 are the sampler's bits, NaN for NaN)
    tr = eng.prepare_tracer(U.astype(dtype), V.astype(dtype), LAT.astype(dtype), LON.astype(dtype), order)
    (c1, c2), _ = eng.sample_tracer(tr, eng.to_device(qx[None].astype(dtype), dtype), eng.to_device(qy[None].astype(dtype), dtype),
                                    SE.LEVEL, order)
    assert np.array_equal(_np(c1)[0], mixed[0], equal_nan=True) and np.array_equal(_np(c2)[0], mixed[1], equal_nan=True)
