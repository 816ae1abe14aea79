"""Footprints without a device: the C boundary of lc_footprint_update (symbols, the structure's size, every refusal before the
first HIP call), the host-side refusals of Engine.checked_footprint_grid / footprint_weights / footprint_update / footprint,
LCS.footprint and tools.trajectory_density, the weight quantisation, and the numpy restatement (tests/footprint.py) against
its own properties: the conservation identity, block splits, the edge rule, hand-worked records."""
import ctypes as C
import inspect
import os
import re
import types

import numpy as np
import pandas as pd
import pytest

from lagrangiancoherence_amd import _capi, build, dropin
from lagrangiancoherence_amd.engine import Engine
from tests import footprint as P
from tests import labelled
from tests import lavd as L
from tests.test_capi_symbols import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("lc_footprint_update", "lc_ctx_last_footprint_kernel", "lc_ctx_set_footprint_form")


@pytest.fixture(scope="module")
def lib():
    build.build_library(verbose=False)
    return _capi.load()


# ------------------------------------------------------------------ C ABI
def test_symbols_in_header_prototypes_library_and_sources(lib):
    for name in SYMBOLS:
        assert name in declared_symbols() and name in _capi.PROTOTYPES and hasattr(lib, name), name
    assert lib.lc_version() == 104 == _capi.LC_VERSION          # additive: no argument list changed
    assert "footprint.hip" in build.SOURCES and build.ARCH == "gfx950"
    assert lib.lc_ctx_last_footprint_kernel(None) == b""
    assert _capi.FootprintArgs._fields_[0][0] == "struct_size"
    assert (_capi.LC_FOOTPRINT_AUTO, _capi.LC_FOOTPRINT_DIRECT, _capi.LC_FOOTPRINT_TILED) == (-1, 0, 1)
    header = open(os.path.join(ROOT, "include", "lcs_hip.h")).read()
    body = header[header.index("typedef struct lc_footprint_args {"):header.index("} lc_footprint_args;")]
    declared = re.findall(r"(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert declared == [f[0] for f in _capi.FootprintArgs._fields_]                     # the mirror, field for field


def test_the_kernel_source_keeps_to_its_means():
    """Plain HIP: no inline assembly, no floating-point atomics (every sum is an integer add), both forms in one file."""
    code = build._strip_comments(open(os.path.join(build.CSRC, "footprint.hip")).read())
    for word in ("asm(", "asm volatile", "cooperative", "__threadfence", "atomicAdd((float", "atomicAdd((double", "float *", "double *"):
        assert word not in code, word
    for word in ("footprint_direct_kernel", "footprint_tile_kernel", "__shared__", "atomicAdd(", "#pragma clang fp contract(off)", "rint("):
        assert word in code, word


def test_lc_footprint_update_checks_arguments_before_any_device_call(lib):
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p).value
    ctx = C.c_void_p(1)             # never dereferenced: every case below is refused by the checks that precede the first HIP call

    def args(**kw):
        a = _capi.FootprintArgs(struct_size=C.sizeof(_capi.FootprintArgs), traj_x=p, traj_y=p, c=p, q=p, dtype=_capi.LC_F32, ny=2, nx=4, n=8,
                                n_levels=3, level0=0, final=1, ny_t=19, nx_t=36, lat0=-90.0, lat1=90.0, lon0=-180.0, lon1=170.0, cyclic_x=1,
                                c_scale=1024.0, zero_first=1, hits=p, mass=p, csum=p, chits=p, stats=p)
        for k, v in kw.items():
            setattr(a, k, v)
        return C.byref(a)

    def refused(ctx_, a, text):
        return lib.lc_footprint_update(ctx_, a) == _capi.LC_EINVAL and text in lib.lc_last_error()
    assert refused(None, args(), b"lc_footprint_update: null context")
    assert refused(ctx, None, b"lc_footprint_update: null argument structure")
    wrong = C.sizeof(_capi.FootprintArgs) - 8
    assert refused(ctx, args(struct_size=wrong), b"struct_size %d, this library has %d" % (wrong, wrong + 8))
    assert refused(ctx, args(struct_size=wrong, dtype=7), b"struct_size")              # ... before anything else
    assert refused(ctx, args(dtype=7), b"bad dtype 7") and refused(ctx, args(dtype=_capi.LC_F64_WIND_F32), b"bad dtype")
    assert refused(ctx, args(n=0, ny=0), b"n 0") and refused(ctx, args(n=-3), b"n -3")
    assert refused(ctx, args(ny=3), b"seed grid 3x4 for n 8") and refused(ctx, args(ny=0, nx=8), b"seed grid 0x8")
    assert refused(ctx, args(ny=1 << 16, nx=1 << 16, n=1), b"seed grid")
    assert refused(ctx, args(n_levels=1), b"n_levels 1") and refused(ctx, args(n_levels=0), b"n_levels 0")
    assert refused(ctx, args(level0=-1), b"level0 -1")
    assert refused(ctx, args(ny_t=1), b"target grid 1x36") and refused(ctx, args(nx_t=1), b"target grid 19x1")
    assert refused(ctx, args(ny_t=1 << 16, nx_t=1 << 15), b"2^31")
    for kw in (dict(lat0=float("nan")), dict(lat1=float("inf")), dict(lat0=0.0, lat1=0.0), dict(lat0=10.0, lat1=-10.0)):
        assert refused(ctx, args(**kw), b"bad latitudes"), kw
    for kw in (dict(lon0=float("nan")), dict(lon1=-float("inf")), dict(lon0=5.0, lon1=5.0), dict(lon0=170.0, lon1=-180.0)):
        assert refused(ctx, args(**kw), b"bad longitudes"), kw
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert refused(ctx, args(c_scale=bad), b"c_scale"), bad
    assert lib.lc_footprint_update(ctx, args(c=None, csum=None, chits=None, c_scale=0.0, traj_x=None)) == _capi.LC_EINVAL
    assert b"null pointer" in lib.lc_last_error()                                       # (c_scale is not looked at without c)
    assert refused(ctx, args(c=None), b"csum and chits need c") and refused(ctx, args(c=None, csum=None), b"need c")
    assert refused(ctx, args(csum=None), b"both or neither") and refused(ctx, args(chits=None), b"both or neither")
    assert refused(ctx, args(hits=None, mass=None, csum=None, chits=None), b"no output")
    assert refused(ctx, args(c=None, hits=None, mass=None, csum=None, chits=None), b"no output")
    for k in ("traj_x", "traj_y", "stats"):
        assert refused(ctx, args(**{k: None}), b"null pointer"), k
    assert lib.lc_ctx_set_footprint_form(None, 0) == _capi.LC_EINVAL and b"null context" in lib.lc_last_error()
    with pytest.raises(ValueError, match="lc_footprint_update"):
        _capi.check(lib.lc_footprint_update(None, args()), lib)


# ------------------------------------------------------------------ the Python surfaces refuse before any device work
def test_the_target_grid_check():
    lat, lon = np.linspace(-90.0, 90.0, 19), np.linspace(-180.0, 170.0, 36)
    assert Engine.checked_footprint_grid(lat, lon, True) == (19, 36, -90.0, 90.0, -180.0, 170.0)
    assert Engine.checked_footprint_grid(lat.astype(np.float32), lon[:20], False) == (19, 20, -90.0, 90.0, -180.0, 10.0)
    assert Engine.checked_footprint_grid([0.0, 1.0], [5.0, 6.0]) == (2, 2, 0.0, 1.0, 5.0, 6.0)
    uneven = lat.copy()
    uneven[4] += 2.0
    for kw in (dict(lat=lat[:1]), dict(lon=lon[:1]), dict(lat=lat[None]), dict(lat=lat[::-1]), dict(lon=lon[::-1]), dict(lat=uneven),
               dict(lat=lat * 1.5), dict(lat=np.where(np.arange(19) == 3, np.nan, lat)), dict(lon=np.where(np.arange(36) == 3, np.inf, lon)),
               dict(lat="north"), dict(lon=lon[:20], cyclic=True), dict(lon=np.linspace(-180.0, 180.0, 37), cyclic=True)):
        with pytest.raises(ValueError, match="footprint grid"):
            Engine.checked_footprint_grid(**{**dict(lat=lat, lon=lon, cyclic=False), **kw})


def test_the_weight_quantisation():
    w = np.array([[0.0, 1.0, 0.5, np.nan], [2.0, 2.0 ** -20, 3.0 * 2.0 ** -20, 5.0 * 2.0 ** -20]])
    q, wscale = Engine.footprint_weights(w, (2, 4))
    assert q.dtype == np.int32 and wscale == 2.0 / (1 << 20)
    # the largest is 2^20; 1, 3 and 5 x 2^-21 of the largest are ties (to even: 0, 2 and 2); NaN and 0 exclude
    assert q.tolist() == [[0, 1 << 19, 1 << 18, 0], [1 << 20, 0, 2, 2]]
    assert np.isnan(w[0, 3])                                                 # the caller's array is left alone
    rng = np.random.default_rng(5)
    w = rng.random((33, 130)) * 7.3
    q, wscale = Engine.footprint_weights(w, w.shape)
    assert q.max() == 1 << 20 and q.min() >= 0 and np.abs(q * wscale - w).max() <= w.max() * 2.0 ** -21
    assert Engine.footprint_weights(None, (3, 3)) == (None, 1.0)
    q, wscale = Engine.footprint_weights(np.zeros((2, 2)), (2, 2))
    assert not q.any() and wscale == 0.0
    for bad in (-np.ones((2, 2)), np.full((2, 2), np.inf), np.ones((2, 3)), "heavy"):
        with pytest.raises(ValueError, match="weights"):
            Engine.footprint_weights(bad, (2, 2))
    area = Engine.seed_cell_areas(np.array([-60.0, 0.0, 60.0]), np.array([0.0, 2.0, 4.0, 6.0]), 2.0)
    k = np.pi / 180
    assert area.shape == (3, 4) and np.array_equal(area[:, 0], area[:, 3])
    np.testing.assert_allclose(area[:, 0], 4.0 * np.cos(k * np.array([-60.0, 0.0, 60.0])) * (60 * k) * (2 * k), rtol=1e-15)


def test_the_engine_refuses_bad_arguments_without_a_device():
    eng = Engine.__new__(Engine)             # no device: the checks come before anything is touched
    lat, lon = np.linspace(-40.0, 0.0, 5), np.linspace(-80.0, -30.0, 6)
    traj = np.zeros((4, 3, 5))
    good = dict(traj_x=traj, traj_y=traj, grid_lat=lat, grid_lon=lon, level0=0, final=True)
    big = types.SimpleNamespace(shape=(2, 1 << 15, 1 << 15))                 # 2^30 parcels over 2^12 levels: 2^63
    for kw in (dict(grid_lat=lat[::-1]), dict(grid_lon=lon[:1]), dict(cyclic=True), dict(level0=-1), dict(traj_x=traj[0, 0, :1][0]),
               dict(traj_y=traj[:3]), dict(c=traj[:, :2], c_scale=1.0), dict(traj_x=traj[:1], traj_y=traj[:1]), dict(level0=2),
               dict(traj_x=big, traj_y=big, level0=(1 << 12) - 2, acc={}), dict(want=("hits", "csum")), dict(want=()), dict(want="residence"),
               dict(c=traj), dict(c=traj, c_scale=0.0), dict(c=traj, c_scale=np.inf), dict(c=traj, c_scale="fine")):
        with pytest.raises(ValueError, match="footprint"):
            eng.footprint_update(**{**good, **kw})
    sig = inspect.signature(Engine.footprint_update).parameters
    assert list(sig)[1:] == ["traj_x", "traj_y", "grid_lat", "grid_lon", "level0", "final", "q", "c", "c_scale", "acc", "cyclic", "want"]
    assert sig["want"].default == ("hits", "mass") and sig["cyclic"].default is False

    field = types.SimpleNamespace(order=1, nt=6, ny_f=5, nx_f=6, lat_min=-40.0, lat_max=0.0, lon_min=-80.0, lon_max=-30.0, dtype=np.dtype(np.float64))
    good = dict(field=field, seed_lat=lat, seed_lon=lon, timestep=900.0, grid_lat=lat, grid_lon=lon)
    other = types.SimpleNamespace(**{**vars(field), "dtype": np.dtype(np.float32)})
    shifted = types.SimpleNamespace(**{**vars(field), "lon_max": -20.0})
    for kw in (dict(timestep=0), dict(timestep=np.inf), dict(timestep="fast"), dict(interp_order=3), dict(t0=-1), dict(nsteps=0), dict(nsteps=6),
               dict(t0=3, nsteps=3), dict(t0=5), dict(level_chunk=0), dict(seed_lat=lat[None]), dict(tracer=other), dict(tracer=shifted),
               dict(grid_lat=lat[::-1]), dict(grid_lon=lon[:1]), dict(weights=-np.ones((5, 6))), dict(weights=np.ones((5, 5))),
               dict(weights=np.full((5, 6), np.inf)), dict(into={}), dict(into="earlier"),
               dict(cyclic_xboundary=False, noncyclic_clamp="nearest")):
        with pytest.raises(ValueError):
            eng.footprint(**{**good, **kw})
    sig = inspect.signature(Engine.footprint).parameters
    assert list(sig)[:7] == ["self", "field", "seed_lat", "seed_lon", "timestep", "grid_lat", "grid_lon"]
    assert list(sig)[7:] == ["weights", "tracer", "c_scale", "t0", "nsteps", "level_chunk", "SETTLS_order", "interp_order", "cyclic_xboundary",
                             "noncyclic_clamp", "into"]
    assert sig["level_chunk"].default == 16 and sig["cyclic_xboundary"].default is True and sig["weights"].default is None
    assert list(inspect.signature(Engine.checked_footprint_grid).parameters) == ["lat", "lon", "cyclic"]
    assert callable(Engine.last_footprint_kernel) and callable(Engine.set_footprint_form)


def _dataset(u, v, lat, lon):
    times = pd.date_range("2010-01-01", periods=u.shape[0], freq="15min").values
    coords = {"latitude": lat, "longitude": lon, "time": times}
    U = labelled.DataArray(u.transpose(1, 2, 0), ["latitude", "longitude", "time"], coords, name="u")
    V = labelled.DataArray(v.transpose(1, 2, 0), ["latitude", "longitude", "time"], coords, name="v")
    return labelled.Dataset({"u": U, "v": V}), times


def test_lcs_footprint_refuses_bad_arguments_before_an_engine_is_asked_for(monkeypatch):
    from LagrangianCoherence.LCS.LCS import LCS
    assert LCS is dropin.LCS

    def no_engine():
        raise AssertionError("an engine was asked for")
    monkeypatch.setattr(dropin, "get_engine", no_engine)
    u, v, lat, lon = L.vortex_record(d=5.0, nt=4)
    ds, _ = _dataset(u, v, lat, lon)
    lcs = LCS(**L.PHYSICAL)
    with pytest.raises(ValueError, match="aux"):
        LCS(aux_grid=0.05, **L.PHYSICAL).footprint(ds)
    with pytest.raises(ValueError, match="timestep"):
        LCS(timestep=0).footprint(ds)
    for kw in (dict(window=1), dict(window=2.5), dict(window=True), dict(window=5), dict(window=2, stride=0)):
        with pytest.raises(ValueError, match="window|stride"):
            lcs.footprint(ds, verbose=False, **kw)
    with pytest.raises(ValueError, match="level_chunk"):
        lcs.footprint(ds, level_chunk=0, verbose=False)
    with pytest.raises(ValueError, match="weights"):
        lcs.footprint(ds, weights="mass", verbose=False)
    for bad in ((lat,), lat, (lat[::-1], lon), (lat, lon[:1]), (lat, np.array([0.0, 1.0, 3.0]))):
        with pytest.raises(ValueError, match="grid"):
            lcs.footprint(ds, grid=bad, verbose=False)
    with pytest.raises(AssertionError, match="an engine was asked for"):       # ... and a good call does ask for one
        lcs.footprint(ds, grid=(lat, lon), weights=None, verbose=False)
    params = inspect.signature(LCS.footprint).parameters
    assert list(params)[:10] == ["self", "ds", "u", "v", "receptors", "weights", "C", "grid", "window", "stride"]
    assert params["level_chunk"].default == 16 and params["weights"].default == "area" and params["receptors"].default is None
    assert set(inspect.signature(LCS.strain).parameters) <= set(params)
    # the receptor mask: strictly inside the subdomain, != 0 and not NaN, labelled on part of the grid or plain
    rec = types.SimpleNamespace(lat=lat, lon=lon)
    ridge = np.ones((lat.size, lon.size))
    ridge[0, 0], ridge[1, 1], ridge[2, 2] = 0.0, np.nan, -3.0
    m = lcs._seed_mask(ridge, rec)
    assert m.dtype == bool and m.sum() == ridge.size - 2 and m[2, 2] and not m[0, 0] and not m[1, 1]
    assert lcs._seed_mask(None, rec).all()
    sub = LCS(subdomain={"latitude": slice(-30.0, -10.0), "longitude": slice(-65.0, -45.0)}, **L.PHYSICAL)
    inside = (lat[:, None] > -30) & (lat[:, None] < -10) & (lon[None, :] > -65) & (lon[None, :] < -45)
    assert np.array_equal(sub._seed_mask(None, rec), inside) and np.array_equal(sub._seed_mask(ridge, rec), inside & m)
    cropped = ridge[(lat > -30) & (lat < -10)][:, (lon > -65) & (lon < -45)]
    assert np.array_equal(sub._seed_mask(cropped, rec), inside & m)
    part = labelled.DataArray(ridge[1:4, 2:5].T, ["longitude", "latitude"], {"latitude": lat[1:4], "longitude": lon[2:5]})
    want = np.zeros_like(m)
    want[1:4, 2:5] = m[1:4, 2:5]
    assert np.array_equal(lcs._seed_mask(part, rec), want)
    off = labelled.DataArray(ridge[1:4, 2:5], ["latitude", "longitude"], {"latitude": lat[1:4] + 0.1, "longitude": lon[2:5]})
    for bad in (ridge[:2], off, labelled.DataArray(ridge[None], ["time", "latitude", "longitude"], {"latitude": lat, "longitude": lon, "time": [0]})):
        with pytest.raises(ValueError, match="receptors"):
            lcs._seed_mask(bad, rec)
    from LagrangianCoherence.LCS import tools
    assert list(inspect.signature(tools.trajectory_density).parameters) == ["x", "y", "lat", "lon", "weights", "values", "cyclic"]
    x = np.zeros((3, 2, 2))
    for kw in (dict(y=x[:2]), dict(x=x[:1], y=x[:1]), dict(lat=lat[::-1]), dict(lon=lon, cyclic=True), dict(weights=-np.ones((2, 2))),
               dict(weights=np.ones(3)), dict(values=x[:2])):
        with pytest.raises(ValueError):
            tools.trajectory_density(**{**dict(x=x, y=x, lat=lat, lon=lon), **kw})


# ------------------------------------------------------------------ the restatement's own properties
def test_hand_worked_records():
    g = P.GRID_2X2                                   # cells centred on (-10, 10) x (0, 20): edges at -20, 0, 20 and -10, 10, 30
    tx = np.array([0.0, 19.0, 10.0, 31.0, np.nan]).reshape(5, 1, 1)
    ty = np.array([-10.0, 9.0, 0.0, 0.0, 0.0]).reshape(5, 1, 1)
    c = np.array([1.0, 2.5, 3.5, 7.0, 9.0]).reshape(5, 1, 1)
    acc = P.fold(tx, ty, g, q=np.array([[3]]), c=c, c_scale=1.0)
    # entry 0 (h 1) in (0, 0); entry 1 (h 2) in (1, 1); entry 2 on both edges: the upper cells (1, 1); entries 3 and 4 outside
    assert acc["hits"].tolist() == [[1, 0], [0, 4]] and acc["mass"].tolist() == [[3, 0], [0, 12]]
    assert acc["csum"].tolist() == [[1, 0], [0, 2 * 2 + 2 * 4]] and acc["chits"].tolist() == [[1, 0], [0, 4]]       # rint: 2.5 -> 2, 3.5 -> 4
    assert acc["stats"].tolist() == [3, 0, 0, 0] and P.conserved(acc, 5, None, (1, 1))
    assert P.half_weights(5, 0, True).tolist() == [1, 2, 2, 2, 1] and P.half_weights(3, 4, False).tolist() == [0, 2, 2]
    assert P.half_weights(2, 0, True).tolist() == [1, 1]
    # q == 0: nothing anywhere, stats included; values that do not count are dropped, the hit stays
    none = P.fold(tx, ty, g, q=np.array([[0]]), c=c, c_scale=1.0)
    assert not any(none[k].any() for k in P.PLANES + ("stats",))
    bad = P.fold(tx[:3], ty[:3], g, c=np.array([np.nan, 2.0 ** 31 + 1.0, -(2.0 ** 31)]).reshape(3, 1, 1), c_scale=1.0)
    assert bad["hits"].sum() == 4 and bad["chits"].tolist() == [[0, 0], [0, 1]] and bad["csum"][1, 1] == -(1 << 31) and bad["stats"].tolist() == [0, 3, 0, 0]
    # cyclic: any turn of the circle is the same column; 1e30 and inf are in none
    gc = P.GRID_CYCLIC
    x = np.array([-180.0, 180.0, 540.0, -540.0, 175.0, 174.9, 1e30, np.inf]).reshape(8, 1, 1)
    ok, row, col = P.cells(x, np.zeros_like(x), gc)
    assert ok.ravel().tolist() == [True] * 6 + [False] * 2 and col.ravel()[:6].tolist() == [0, 0, 0, 0, 0, 35] and set(row.ravel()[:6]) == {9}


def test_the_edge_rule_on_the_half_degree_grid():
    """On the 0.5 degree grid from -180 every k 0.5 - 0.25 is exact in float32 and inv_dx is exactly 2: the products and sums of
    the index map are exact there, so an edge is an edge in both dtypes and belongs to the upper cell."""
    g = P.GRID_HALF
    assert g.inv_dx == 2.0 and g.inv_dy == 2.0
    for dtype in (np.float32, np.float64):
        tx, ty = P.edge_case(dtype)
        assert np.array_equal(tx.astype(np.float64), P.edge_case(np.float64)[0])            # exact in float32
        ok, row, col = P.cells(tx, ty, g)
        k = np.arange(-2, g.nx_t + 3)
        assert np.array_equal(col[0, 0], np.mod(k, g.nx_t)) and np.array_equal(col[1, 0], col[0, 0]) and np.array_equal(col[2, 0][ok[2, 0]], col[0, 0][::-1][ok[2, 0]])
        rows = np.arange(k.size) % g.ny_t
        assert ok[:2].all() and np.array_equal(row[0, 0], rows) and np.array_equal(row[2, 0][ok[2, 0]], rows[ok[2, 0]] + 1)
        assert (~ok[2, 0]).sum() == (rows == g.ny_t - 1).sum() > 0                          # the upper edge of the last row is outside
        assert col[0, 0][2] == 0 and col[0, 0][g.nx_t + 2] == 0                             # lon1 + 0.25 wraps to column 0
        acc = P.fold(tx, ty, g)
        assert P.conserved(acc, 3, None, tx.shape[1:])
    # without wrapping the same columns are outside
    open_ = P.Grid(g.lat, g.lon, cyclic=False)
    ok, _, _ = P.cells(*P.edge_case(np.float32), open_)
    assert (~ok[0, 0]).sum() == 5


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_conservation_and_block_splits_of_the_restatement(dtype):
    for g in P.GRIDS.values():
        for kind, make in P.KINDS.items():
            for shape in ((1, 1), (5, 7)):
                tx, ty, c, c_scale = make(6, shape, dtype, g)
                q = P.weights_case(shape)
                whole = P.fold(tx, ty, g, 0, True, q, c, c_scale)
                assert P.conserved(whole, 6, q, shape), (kind, shape)
                assert np.array_equal(whole["chits"] <= whole["hits"], np.ones(g.shape, bool)) and (whole["mass"] >= whole["hits"]).all()
                assert whole["hits"].sum() - whole["chits"].sum() == whole["stats"][1]
                for block in (1, 2, 5):
                    assert P.same(P.fold_in_blocks(tx, ty, g, block, q, c, c_scale), whole), (kind, shape, block)
                assert P.conserved(P.fold(tx, ty, g), 6, None, shape)
    # the mixed record does what it is for
    tx, ty, c, c_scale = P.mixed_case(17, (33, 130), dtype, P.GRID_CYCLIC)
    acc = P.fold(tx, ty, P.GRID_CYCLIC, c=c, c_scale=c_scale)
    assert acc["stats"][0] > 0 and acc["stats"][1] > 0 and np.isnan(tx).any() and np.isinf(ty).any() and (np.abs(tx) == 1e30).any()
    assert np.count_nonzero(acc["hits"]) == acc["hits"].size and (acc["csum"] < 0).any() and (acc["csum"] > 0).any()
    tx, ty, c, c_scale = P.one_cell_case(17, (33, 130), dtype, P.GRID_REGIONAL)
    acc = P.fold(tx, ty, P.GRID_REGIONAL, q=np.full((33, 130), P.Q_MAX), c=c, c_scale=c_scale)
    assert acc["mass"].max() == 32 * 33 * 130 * P.Q_MAX and acc["csum"].min() == -32 * 33 * 130 * (1 << 31)
