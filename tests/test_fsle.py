"""Finite-size Lyapunov exponents without a device: the C boundary of lc_fsle_update (symbols, structure size, every refusal
before the first HIP call), the host-side refusals of Engine.fsle_update / Engine.fsle / LCS.fsle, and the numpy restatement of the
definition (tests/fsle.py) against hand-worked cases, against itself cut into blocks, and on the records the GPU tests use."""
import ctypes as C
import inspect
import os
import types

import numpy as np
import pytest

from lagrangiancoherence_amd import _capi, build, dropin
from lagrangiancoherence_amd.engine import Engine
from tests import fsle as F
from tests.test_capi_symbols import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = np.pi / 180
DT = 3600.0


@pytest.fixture(scope="module")
def lib():
    build.build_library(verbose=False)
    return _capi.load()


# ------------------------------------------------------------------ C ABI
def test_symbols_in_header_prototypes_library_and_sources(lib):
    for name in ("lc_fsle_update", "lc_ctx_last_fsle_kernel"):
        assert name in declared_symbols() and name in _capi.PROTOTYPES and hasattr(lib, name)
    assert lib.lc_version() == 104 == _capi.LC_VERSION          # additive: no argument list changed
    assert "fsle.hip" in build.SOURCES and build.ARCH == "gfx950"
    assert lib.lc_ctx_last_fsle_kernel(None) == b""
    assert (_capi.LC_FSLE_RATIO, _capi.LC_FSLE_DISTANCE) == (0, 1)
    header = open(os.path.join(ROOT, "include", "lcs_hip.h")).read()
    assert "enum lc_fsle_mode { LC_FSLE_RATIO = 0, LC_FSLE_DISTANCE = 1 };" in header
    assert _capi.FsleArgs._fields_[0][0] == "struct_size"


def test_the_kernel_source_keeps_to_its_means():
    code = build._strip_comments(open(os.path.join(build.CSRC, "fsle.hip")).read())
    for word in ("atomic", "asm(", "asm volatile", "cooperative", "__threadfence"):
        assert word not in code, word
    assert "__shared__" in code and "__shfl_up" in code and "fsle_update_kernel" in code


def test_lc_fsle_update_checks_arguments_before_any_device_call(lib):
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p).value
    ctx = C.c_void_p(1)             # never dereferenced: every case below is refused by the checks that precede the first HIP call

    def args(thresholds=(2.0, 3.0), **kw):
        a = _capi.FsleArgs(struct_size=C.sizeof(_capi.FsleArgs), traj_x=p, traj_y=p, dtype=_capi.LC_F64, ny=4, nx=4, n_levels=3, level0=0,
                           seed_lat_dev=p, seed_lon_dev=p, mode=_capi.LC_FSLE_RATIO, n_thr=len(thresholds),
                           thresholds=(C.c_double * 8)(*thresholds), radius=6371000.0, timestep=-3600.0, cyclic_x=1, tau=p, fsle=p)
        for k, v in kw.items():
            setattr(a, k, v)
        return C.byref(a)

    def refused(ctx_, a, text):
        return lib.lc_fsle_update(ctx_, a) == _capi.LC_EINVAL and text in lib.lc_last_error()
    assert refused(None, args(), b"lc_fsle_update: null context")
    assert refused(ctx, None, b"lc_fsle_update: null argument structure")
    wrong = C.sizeof(_capi.FsleArgs) - 8
    assert refused(ctx, args(struct_size=wrong), b"struct_size %d, this library has %d" % (wrong, wrong + 8))
    assert refused(ctx, args(dtype=7), b"bad dtype 7") and refused(ctx, args(dtype=_capi.LC_F64_WIND_F32), b"bad dtype")
    assert refused(ctx, args(mode=2), b"bad mode 2") and refused(ctx, args(mode=-1), b"bad mode -1")
    assert refused(ctx, args(ny=0), b"bad grid 0x4") and refused(ctx, args(nx=0), b"bad grid 4x0")
    assert refused(ctx, args(ny=1, nx=1), b"bad grid 1x1")
    assert refused(ctx, args(n_levels=1), b"n_levels 1") and refused(ctx, args(n_levels=0), b"n_levels 0")
    assert refused(ctx, args(level0=-1), b"level0 -1")
    assert refused(ctx, args(n_thr=0), b"n_thr 0") and refused(ctx, args(n_thr=9), b"n_thr 9")
    for bad in (float("nan"), float("inf"), 1.0, 0.5, -2.0):
        assert refused(ctx, args(thresholds=(2.0, bad)), b"threshold 1 is"), bad
    for bad in (float("nan"), float("inf"), 0.0, -5.0):
        assert refused(ctx, args(thresholds=(bad,), mode=_capi.LC_FSLE_DISTANCE), b"threshold 0 is"), bad
    assert not refused(ctx, args(thresholds=(0.5,), mode=_capi.LC_FSLE_DISTANCE, tau=None), b"threshold")   # 0.5 m is a distance
    # the checks see a threshold as the kernel will: rounded to the dtype
    assert refused(ctx, args(thresholds=(1.0 + 1e-9,), dtype=_capi.LC_F32), b"threshold 0 is 1 once rounded to the dtype")
    assert refused(ctx, args(thresholds=(1e-50,), dtype=_capi.LC_F32, mode=_capi.LC_FSLE_DISTANCE), b"threshold 0 is 0 once rounded")
    assert refused(ctx, args(thresholds=(1e39,), dtype=_capi.LC_F32), b"threshold 0 is inf once rounded")
    assert not refused(ctx, args(thresholds=(1.0 + 1e-9,), tau=None), b"threshold")                          # float64 keeps it
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert refused(ctx, args(radius=bad), b"radius"), bad
    for bad in (0.0, float("nan"), float("inf"), -float("inf")):
        assert refused(ctx, args(timestep=bad), b"timestep"), bad
    assert refused(ctx, args(ny=1 << 16, nx=1 << 15), b"2^31")
    assert refused(ctx, args(ny=1, nx=(1 << 31) - 1), b"too many for one launch")
    for k in ("traj_x", "traj_y", "seed_lat_dev", "seed_lon_dev", "tau", "fsle"):
        assert refused(ctx, args(**{k: None}), b"null pointer"), k
    with pytest.raises(ValueError, match="lc_fsle_update"):
        _capi.check(lib.lc_fsle_update(None, args()), lib)


# ------------------------------------------------------------------ the Python surfaces refuse before any device work
def test_the_engine_refuses_bad_arguments_without_a_device():
    eng = Engine.__new__(Engine)             # no device: the checks come before anything is touched
    lat, lon = np.arange(3.0), np.arange(4.0)
    traj = np.zeros((5, 3, 4))
    good = dict(traj_x=traj, traj_y=traj, seed_lat=lat, seed_lon=lon, thresholds=[2.0], mode="ratio", timestep=-DT, level0=0)
    for kw in (dict(mode="both"), dict(thresholds=[]), dict(thresholds=[2.0] * 9), dict(thresholds=[[2.0]]), dict(thresholds="x"),
               dict(thresholds=[1.0]), dict(thresholds=[2.0, np.nan]), dict(thresholds=[np.inf]), dict(thresholds=0.0, mode="distance"),
               dict(thresholds=[-1.0], mode="distance"), dict(timestep=0.0), dict(timestep=np.nan), dict(timestep="fast"),
               dict(radius=0.0), dict(radius=-1.0), dict(radius=np.inf), dict(level0=-1), dict(traj_x=traj[0]), dict(traj_y=traj[:4]),
               dict(traj_x=traj[:1], traj_y=traj[:1]), dict(traj_x=traj[:, :1, :1], traj_y=traj[:, :1, :1], seed_lat=lat[:1], seed_lon=lon[:1]),
               dict(seed_lat=lon), dict(seed_lon=lat), dict(level0=3), dict(tau=np.zeros((1, 3, 4))), dict(fsle=np.zeros((1, 3, 4)))):
        with pytest.raises(ValueError):
            eng.fsle_update(**{**good, **kw})
    for kw in (dict(thresholds=[1.0 + 1e-9]), dict(thresholds=[1e-50], mode="distance"), dict(thresholds=[1e39])):
        Engine.checked_fsle_options(kw["thresholds"], kw.get("mode", "ratio"), -DT, dtype=np.float64)
        with pytest.raises(ValueError, match="once rounded to float32"):
            eng.fsle_update(**{**good, **kw, "traj_x": traj.astype(np.float32), "traj_y": traj.astype(np.float32)})
    thr, mode, dt, radius = Engine.checked_fsle_options(2, "ratio", -DT)
    assert thr.tolist() == [2.0] and (mode, dt, radius) == ("ratio", -DT, 6371000.0)
    assert Engine.checked_fsle_options((5e4, 1e5), "distance", DT, 1.0)[0].tolist() == [5e4, 1e5]

    field = types.SimpleNamespace(order=1, nt=6, dtype=np.dtype(np.float64))
    good = dict(field=field, seed_lat=lat, seed_lon=lon, timestep=-DT, thresholds=[2.0])
    with pytest.raises(ValueError, match="once rounded to float32"):
        eng.fsle(**{**good, "field": types.SimpleNamespace(order=1, nt=6, dtype=np.dtype(np.float32)), "thresholds": [1.0 + 1e-9]})
    for kw in (dict(thresholds=[0.9]), dict(mode="size"), dict(timestep=0), dict(radius=np.nan), dict(interp_order=3), dict(t0=-1),
               dict(nsteps=0), dict(nsteps=6), dict(t0=3, nsteps=3), dict(t0=5), dict(level_chunk=0), dict(seed_lat=lat[None]),
               dict(seed_lat=lat[:1], seed_lon=lon[:1]), dict(cyclic_xboundary=False, noncyclic_clamp="nearest")):
        with pytest.raises(ValueError):
            eng.fsle(**{**good, **kw})
    sig = inspect.signature(Engine.fsle).parameters
    assert list(sig)[:6] == ["self", "field", "seed_lat", "seed_lon", "timestep", "thresholds"]
    assert sig["mode"].default == "ratio" and sig["level_chunk"].default == 16 and sig["cyclic_xboundary"].default is True
    assert list(inspect.signature(Engine.fsle_update).parameters)[1:9] == ["traj_x", "traj_y", "seed_lat", "seed_lon", "thresholds",
                                                                           "mode", "timestep", "level0"]


def test_lcs_fsle_refuses_bad_arguments_without_a_device():
    from LagrangianCoherence.LCS.LCS import LCS
    assert LCS is dropin.LCS
    lcs = LCS(timestep=-DT)
    with pytest.raises(ValueError, match="exactly one"):
        lcs.fsle(u=None, v=None)
    with pytest.raises(ValueError, match="exactly one"):
        lcs.fsle(ratio=2.0, final_separation=1e5)
    for kw in (dict(ratio=1.0), dict(ratio=[2.0, 0.5]), dict(ratio=[1.5] * 9), dict(ratio=np.nan), dict(ratio=[]),
               dict(final_separation=0.0), dict(final_separation=[1e5, -1.0]), dict(final_separation=np.inf), dict(ratio="two")):
        with pytest.raises(ValueError, match="fsle"):
            lcs.fsle(**kw)
    with pytest.raises(ValueError, match="aux"):
        LCS(timestep=-DT, aux_grid=0.05).fsle(ratio=2.0)
    with pytest.raises(ValueError, match="timestep"):
        LCS(timestep=0).fsle(ratio=2.0)
    params = inspect.signature(LCS.fsle).parameters
    assert list(params)[:8] == ["self", "ds", "u", "v", "ratio", "final_separation", "window", "stride"]
    assert set(inspect.signature(LCS.strain).parameters) <= set(params)


# ------------------------------------------------------------------ the restatement against hand-worked cases
def both(tx, ty, lat, lon, thr, mode, cyclic=False, T=np.float64):
    """The literal definition and the streaming form (one block): the same arrays."""
    J = F.definition(tx, ty, lat, lon, thr, mode, -DT, T, cyclic)
    tau, fs = F.update(tx, ty, lat, lon, thr, mode, -DT, 0, T, cyclic=cyclic)
    assert np.array_equal(tau, J["tau"], equal_nan=True) and np.array_equal(fs, J["fsle"], equal_nan=True)
    return J


def test_a_meridional_stretch_has_the_closed_form():
    """phi(t) = phi0 e^{st} on one meridian (an n x 1 grid): every N / S pair grows exactly as e^{st}, so a ratio r is crossed in
    the interval j with e^{s(j-1)} < r <= e^{sj} and tau is the linear interpolation of that interval."""
    s, L = 0.11, 13
    tx, ty, lat, lon = F.meridional_stretch(s, L)
    g = np.exp(s * np.arange(L))
    ratios = [1.3, 2.0, 3.5, 4.0]                             # e^{12 s} = 3.74: the last is never reached
    J = both(tx, ty, lat, lon, ratios, "ratio")
    for q, r in enumerate(ratios):
        if r > g[-1]:
            assert np.all(np.isnan(J["tau"][q])) and np.all(np.isnan(J["fsle"][q])) and np.all(J["pair"][q] == -1)
            continue
        j = int(np.searchsorted(g, r))                        # g[j-1] < r <= g[j]
        tau = (j - 1 + (r - g[j - 1]) / (g[j] - g[j - 1])) * DT
        assert np.all(J["level"][q] == j)
        np.testing.assert_allclose(J["tau"][q].astype(float), tau, rtol=1e-11)
        np.testing.assert_allclose(J["fsle"][q].astype(float), np.log(r) / tau, rtol=1e-11)
    assert J["pair"][0, 0, 0] == 2 and J["pair"][0, -1, 0] == 3 and np.all(J["pair"][0] >= 2)   # N or S: there is no other pair
    # the same as final separations: T = r d0 with d0 = R k dphi on a meridian
    d0 = F.R_EARTH * K * (lat[1] - lat[0])
    Jd = both(tx, ty, lat, lon, [r * d0 for r in ratios[:3]], "distance")
    np.testing.assert_allclose(Jd["tau"].astype(float), J["tau"][:3].astype(float), rtol=1e-9)
    np.testing.assert_allclose(Jd["fsle"].astype(float), J["fsle"][:3].astype(float), rtol=1e-9)


def test_a_zonal_stretch_on_the_equator_a_one_row_grid():
    s, L = 0.2, 9
    lat, lon = np.array([0.0]), np.array([1.0, 2.0, 3.0, 4.0])
    g = np.exp(s * np.arange(L))
    tx = (lon[None, None, :] * g[:, None, None]).copy()
    ty = np.zeros_like(tx)
    J = both(tx, ty, lat, lon, [2.0], "ratio")
    j = int(np.searchsorted(g, 2.0))
    tau = (j - 1 + (2.0 - g[j - 1]) / (g[j] - g[j - 1])) * DT
    np.testing.assert_allclose(J["tau"][0].astype(float), tau, rtol=1e-11)
    assert J["pair"][0, 0, 0] == 0 and J["pair"][0, 0, -1] == 1 and np.all(J["pair"][0] <= 1)    # E or W: there is no other pair


def test_a_nan_level_contributes_nothing():
    """A NaN at the crossing level of one parcel: its two pairs see d(j) = NaN, then d(j) = NaN as the level before, then a
    separation already past T -- they never upcross.  Its own cell loses both pairs; the neighbours keep their other pair."""
    s, L = 0.11, 13
    tx, ty, lat, lon = F.meridional_stretch(s, L)
    clean = both(tx, ty, lat, lon, [2.0], "ratio")
    j = int(clean["level"][0, 2, 0])
    ty[j, 2, 0] = np.nan
    J = both(tx, ty, lat, lon, [2.0], "ratio")
    assert np.isnan(J["tau"][0, 2, 0]) and np.isnan(J["fsle"][0, 2, 0])
    keep = np.arange(lat.size) != 2
    np.testing.assert_allclose(J["tau"][0, keep].astype(float), clean["tau"][0, keep].astype(float), rtol=1e-13)   # (the other pair: an ulp)
    assert np.array_equal(J["tau"][0, [0, 4]], clean["tau"][0, [0, 4]])                          # their one pair is untouched
    assert J["pair"][0, :, 0].tolist() == [2, 3, -1, 2, 3]
    # a NaN one level earlier hides d(j-1) only: the pairs still never see d(j-1) < T <= d(j) with both finite
    ty[j, 2, 0], ty[j - 1, 2, 0] = lat[2] * np.exp(s * j), np.nan
    assert np.isnan(both(tx, ty, lat, lon, [2.0], "ratio")["tau"][0, 2, 0])
    # and a NaN well before the crossing changes nothing
    tx, ty, lat, lon = F.meridional_stretch(s, L)
    ty[1, 2, 0] = np.nan
    assert np.array_equal(both(tx, ty, lat, lon, [2.0], "ratio")["tau"], clean["tau"])


def test_an_ineligible_pair_is_skipped():
    """Rows 0, 1, 3 degrees apart and T = 150 km: the upper pair starts at 222 km >= T and is not eligible, however it moves."""
    lat, lon = np.array([0.0, 1.0, 3.0]), np.array([10.0])
    L = 6
    ty = lat[None, :, None] * (1 + 0.2 * np.arange(L))[:, None, None]
    tx = np.full_like(ty, 10.0)
    J = both(tx, ty, lat, lon, [150e3], "distance")
    assert J["pair"][0, :, 0].tolist() == [2, 3, -1] and np.isnan(J["tau"][0, 2, 0])
    d = F.R_EARTH * K * (1 + 0.2 * np.arange(L))               # the lower pair: 111 km growing by 22 km a level
    j = int(np.searchsorted(d, 150e3))
    np.testing.assert_allclose(J["tau"][0, :2, 0].astype(float), (j - 1 + (150e3 - d[j - 1]) / (d[j] - d[j - 1])) * DT, rtol=1e-9)
    # a pair of coincident seeds (d0 = 0) is not eligible either, in ratio mode
    J0 = both(np.zeros((3, 1, 2)), np.zeros((3, 1, 2)), np.array([0.0]), np.array([5.0, 5.0]), [2.0], "ratio")
    assert np.all(J0["pair"] == -1)


def test_ties_go_to_the_first_pair_in_e_w_n_s_order():
    tx, ty, lat, lon, thr = F.tie_case()
    J = both(tx, ty, lat, lon, [thr], "distance")
    D = J["D"]
    assert np.array_equal(D[1:, 0, 0, 0], D[1:, 2, 0, 0]) and D[0, 0, 0, 0] != D[0, 2, 0, 0]       # E and N of cell (0, 0): the same
    assert J["pairs"]["t"][0, 0, 0, 0] == J["pairs"]["t"][0, 2, 0, 0]                               # separations, the same time
    assert J["pair"][0, 0, 0] == 0                                                                 # ... and E wins
    d0_e = F.R_EARTH * K * 1.0
    np.testing.assert_allclose(float(J["fsle"][0, 0, 0]), np.log(thr / d0_e) / float(J["tau"][0, 0, 0]), rtol=1e-12)
    assert abs(float(J["fsle"][0, 0, 0]) / float(J["pairs"]["fsle"][0, 2, 0, 0]) - 1) > 0.1       # N's value is another one


def test_the_seam_pair_exists_only_on_a_cyclic_grid():
    tx, ty, lat, lon = F.seam_case()
    J = both(tx, ty, lat, lon, [1.1], "ratio", cyclic=True)
    assert J["pair"][0, 0].tolist() == [1, -1, -1, 0]                                             # W of column 0, E of column 3
    np.testing.assert_allclose(J["tau"][0, 0, [0, 3]].astype(float), 1.8 * DT, rtol=1e-11)         # 90 -> 95 -> 100 degrees, T = 99
    np.testing.assert_allclose(J["fsle"][0, 0, [0, 3]].astype(float), np.log(1.1) / (1.8 * DT), rtol=1e-11)
    Jn = both(tx, ty, lat, lon, [1.1], "ratio", cyclic=False)
    assert np.all(Jn["pair"] == -1)
    assert not np.any(np.isnan(J["D"][:, 1, 0, 0])) and np.all(np.isnan(Jn["D"][:, 1, 0, 0]))


# ------------------------------------------------------------------ the records of the GPU tests
CASES = [(shape, dtype, mode, cyclic) for shape in F.GRIDS for dtype in (np.float64, np.float32) for mode in ("ratio", "distance")
         for cyclic in (True, False)]
# numpy's own distance error on these records.  The worst pairs are those whose raw longitude difference is near 360 degrees (the
# seam pairs, and pairs one of whose parcels has been wrapped): the argument k dlambda / 2 is near pi and rounds by eps / 2 * pi,
# while the sine it feeds is k s / 2 for a true separation of s degrees, 1.5 at the least here; at most four roundings of that size
# meet (the difference, the product with k, the sine, the square root; the halving is exact)
ERROR_CAP = {dt: 4 * (np.finfo(dt).eps / 2 * np.pi) / (K * 1.5 / 2) for dt in (np.float32, np.float64)}       # 5.7e-5, 1.1e-13


@pytest.mark.parametrize("shape,dtype,mode,cyclic", CASES)
def test_the_test_records_keep_their_caps_and_the_restatement_is_split_invariant(shape, dtype, mode, cyclic):
    tx, ty, lat, lon, thr = F.case(shape, dtype, mode)
    assert tx.dtype == dtype and np.array_equal(tx[0], np.broadcast_to(lon, tx[0].shape)) and np.array_equal(ty[0], np.broadcast_to(lat[:, None], ty[0].shape))
    assert tx.min() >= -180 and tx.max() < 180
    err = F.distance_error(tx, ty, lat, lon, dtype, cyclic)
    assert err <= ERROR_CAP[dtype], err
    J = F.definition(tx, ty, lat, lon, thr, mode, F.TIMESTEP, np.longdouble, cyclic)
    B = F.bounds(J, 8 * err, np.finfo(dtype).eps, F.TIMESTEP)
    crossed = (J["pair"] >= 0).reshape(3, -1).mean(axis=1)
    assert np.all(crossed >= 0.10) and np.all(crossed <= 0.90), crossed
    assert B["left_out"].mean() <= (0.01 if dtype is np.float32 else 0.0), B["left_out"].mean()
    # the restatement in the kernel's dtype: blocks of 1, 3, 5 and all levels give the same bits, and the literal definition's
    whole = F.update_in_blocks(tx, ty, lat, lon, thr, mode, F.TIMESTEP, dtype, F.N_LEVELS - 1, cyclic=cyclic)
    D = F.definition(tx, ty, lat, lon, thr, mode, F.TIMESTEP, dtype, cyclic)
    assert np.array_equal(whole[0], D["tau"], equal_nan=True) and np.array_equal(whole[1], D["fsle"], equal_nan=True)
    for block in (1, 3, 5):
        cut = F.update_in_blocks(tx, ty, lat, lon, thr, mode, F.TIMESTEP, dtype, block, cyclic=cyclic)
        assert np.array_equal(cut[0], whole[0], equal_nan=True) and np.array_equal(cut[1], whole[1], equal_nan=True), block
    # ... and it passes the judge's check it holds the kernel to
    F.check_against_judge(whole[0], whole[1], J, B, F.TIMESTEP)


def test_the_hand_cases_pass_the_judges_check_too():
    for tx, ty, lat, lon, thr, mode, cyclic in F.hand_cases():
        J = F.definition(tx, ty, lat, lon, thr, mode, F.TIMESTEP, np.longdouble, cyclic)
        B = F.bounds(J, 8 * max(F.distance_error(tx, ty, lat, lon, np.float64, cyclic), np.finfo(np.float64).eps), np.finfo(np.float64).eps, F.TIMESTEP)
        tau, fs = F.update(tx, ty, lat, lon, thr, mode, F.TIMESTEP, 0, np.float64, cyclic=cyclic)
        F.check_against_judge(tau, fs, J, B, F.TIMESTEP)
