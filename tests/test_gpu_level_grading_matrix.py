"""Graded level counts on the device, over everything the dispatcher and the kernel vary (lc_ctx_set_level_grading; the
``MODE == PATCH_TALL && A.grade.n > 0`` branch of advect_lds2_kernel): every tall-patch instance (SETTLS_order 0 ... 5, cyclic
and pointwise), row shards of a 328-row global grid with the low pole row, no pole row and the high pole row, zones of one
and three eights, 3 / 4 / 5 launches, capped and zeroed wishes, a continuation in a shard, every form of the block -> tile
map (contiguous bands, two tile rows per chunk, whole rows, tile orders 0-3), LCS_POLE_BLOCKS=0, and the calls that must keep
their launches.  tests/test_gpu_level_grading.py is the one-instance, one-grid version of this.

A 48 x 96-node float32 field with 41 levels; 328 x 136 seeds and row windows of them.  Tall patches are 8 x 64 seeds: 17
tile columns, 34 / 68 / 102 tiles in grids of 48 / 72 / 120 blocks (tests/c/level_grading_test.cpp states each plan used here
by name, from the header's own functions).  At these sizes the by-size level chunk is one launch, so the launch count is
the witness: n_chunks(41, chunk) launches exactly when the plan is graded, 1 when grading() zeroes it or the dispatcher
declines.  Every graded result is compared bit for bit (torch.equal) with the one-launch run of the same call; the one-launch
runs are tied to each other (a window = those rows of the whole grid; K = 0 and 4 = the direct-gather kernel) and, once per
boundary at K = 4 and K = 0, to oracle.lcs_oracle.parcel_propagation inside the float32 oracle's band."""
import numpy as np
import pytest
import torch

from lagrangiancoherence_amd import flows
from tests import kernel_routes as KR
from tests._fullsize import positions_check, subset

pytestmark = pytest.mark.gpu

NT, DT = 42, -3600.0
NY, NX = 328, 136
CYCLIC = dict(cyclic_xboundary=True)
POINTWISE = dict(cyclic_xboundary=False, noncyclic_clamp="pointwise")
BOUNDARIES = {"cyclic": CYCLIC, "pointwise": POINTWISE}
# (first row, end row, rows of the global grid the window belongs to)
WHOLE, OWN200 = (0, NY, NY), (0, 200, 200)          # the 328-row grid; its first 200 rows as a global grid of their own
LOW, MID_A, MID_B, HIGH = (0, 128, NY), (64, 264, NY), (100, 300, NY), (128, 328, NY)
DIRECT = "advect_kernel_f32<1>"
OFF = (0, -1, 0)


def tall_instance(K, cyclic):
    """The tall-patch two-seed instance SETTLS_order K runs on, from the route table."""
    c = "true" if cyclic else "false"
    names = [n for n, r in KR.ROUTES.items()
             if n.startswith("advect_lds2_kernel<") and n.endswith(f", {c}, 0>") and K in r["Ks"] and r["xmode"] == ("cyclic" if cyclic else "pointwise")]
    if not names:
        # pointwise, SETTLS orders above 4: the table lists the run-time-K instance at 1, 2, 3; the dispatcher sends these there too
        assert not cyclic and K > 4, (K, cyclic)
        names = ["advect_lds2_kernel<-1, false, 0>"]
    assert len(names) == 1, names
    return names[0]


class Runs:
    """One context with the field packed, and the one-launch results of it, each computed once and never written to."""

    def __init__(self, eng, u, v, lat, lon, glat, glon):
        self.eng, self.glat, self.glon = eng, glat, glon
        self.f = eng.prepare_field(u, v, lat, lon, 1)
        self.refs = {}

    def advect(self, win, K, boundary, **kw):
        lo, hi, nyg = win
        return self.eng.advect(self.f, self.glat[lo:hi], self.glon, DT, SETTLS_order=K, interp_order=1, row0=lo, ny_global=nyg,
                               **BOUNDARIES[boundary], **kw)

    def one_launch(self, win, K, boundary):
        """The call in one launch (set_level_chunk(0): grading moot), checked against the other kernels that must give
        the same bits: for K = 0 and 4 the direct-gather kernel, for a window the rows of the whole grid's result."""
        key = (win, K, boundary)
        if key in self.refs:
            return self.refs[key]
        eng = self.eng
        eng.set_lds_tiles(1)
        eng.set_level_chunk(0)
        try:
            x, y = self.advect(win, K, boundary)
            assert eng.last_advect_launches() == 1
            assert eng.last_advect_kernel() == tall_instance(K, boundary == "cyclic"), (key, eng.last_advect_kernel())
            if K in (0, 4):
                eng.set_lds_tiles(0)
                xd, yd = self.advect(win, K, boundary)
                assert eng.last_advect_kernel() == DIRECT and eng.last_advect_launches() == 1, (key, eng.last_advect_kernel())
                assert torch.equal(x, xd) and torch.equal(y, yd), key
        finally:
            eng.set_lds_tiles(1)
            eng.set_level_chunk(-1)
        lo, hi, nyg = win
        if nyg == NY and win != WHOLE:
            xw, yw = self.one_launch(WHOLE, K, boundary)
            assert torch.equal(x, xw[lo:hi]) and torch.equal(y, yw[lo:hi]), key
        elif win == OWN200:     # advection is per seed: all but its own last row (a pole row there only) are the 328-row grid's
            xw, yw = self.one_launch(WHOLE, K, boundary)
            assert torch.equal(x[:199], xw[:199]) and torch.equal(y[:199], yw[:199]), key
        self.refs[key] = (x, y)
        return x, y

    def graded(self, win, K, boundary, grading, launches, want, **kw):
        """The call under the by-size chunk with `grading` set: the launches made, the instance, the bits of `want`."""
        eng = self.eng
        eng.set_level_chunk(-1)
        eng.set_level_grading(*grading)
        x, y = self.advect(win, K, boundary, **kw)
        what = (win, K, boundary, grading)
        assert eng.last_advect_launches() == launches, (what, eng.last_advect_launches())
        assert eng.last_advect_kernel() == tall_instance(K, boundary == "cyclic"), (what, eng.last_advect_kernel())
        assert torch.equal(x, want[0]) and torch.equal(y, want[1]), what
        return x, y


def _enter(eng):
    eng.set_lds_tiles(1)        # the two-seed kernel whatever the size
    eng.set_level_chunk(-1)
    eng.set_level_grading(0, -1, -1)


def _reset(eng):
    eng.set_level_chunk(-1)
    eng.set_level_grading(0, -1, -1)
    eng.set_lds_tiles(-1)


@pytest.fixture(scope="module")
def inputs():
    u, v, lat, lon = flows.era5_like(nt=NT, ny=48, nx=96)
    glat, glon = flows.seed_grid(NY, NX, lat, lon)
    return u, v, lat, lon, glat, glon


@pytest.fixture(scope="module")
def runs(inputs):
    from lagrangiancoherence_amd.engine import Engine
    eng = Engine(0)
    yield Runs(eng, *inputs)
    eng.close()


def _context(monkeypatch, inputs, **env):
    """A fresh context created with `env` set (the variables are read once, at creation)."""
    from lagrangiancoherence_amd.engine import Engine
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    eng = Engine(0)
    try:
        return Runs(eng, *inputs)
    except BaseException:
        eng.close()
        raise


# ---- a. every instance ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("boundary, K", [("cyclic", k) for k in (0, 1, 2, 3, 4, 5)] + [("pointwise", k) for k in (0, 2, 4, 5)])
def test_every_tall_instance_graded_equals_one_launch(runs, boundary, K):
    eng = runs.eng
    want = {("cyclic", 5): "advect_lds2_kernel<-1, true, 0>", ("pointwise", 2): "advect_lds2_kernel<-1, false, 0>",
            ("pointwise", 5): "advect_lds2_kernel<-1, false, 0>"}.get((boundary, K),
                                                                      "advect_lds2_kernel<%d, %s, 0>" % (K, "true" if boundary == "cyclic" else "false"))
    assert tall_instance(K, boundary == "cyclic") == want
    try:
        _enter(eng)
        ref = runs.one_launch(OWN200, K, boundary)
        runs.graded(OWN200, K, boundary, (14, 8, 14), 3, ref)
        assert eng.last_advect_kernel() == want
    finally:
        _reset(eng)


# ---- b. row shards ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("boundary", ["cyclic", "pointwise"])
@pytest.mark.parametrize("K", [4, 1])
@pytest.mark.parametrize("win, grading", [(LOW, (14, 8, 14)), (MID_A, (14, 8, 14)), (MID_B, (14, 8, 14)), (HIGH, (14, 8, 14)),
                                          (WHOLE, (14, 24, 14))],
                         ids=["rows0-128", "rows64-264", "rows100-300", "rows128-328", "whole-zone24"])
def test_row_shards_graded_equal_one_launch_and_the_whole_grid(runs, win, grading, K, boundary):
    """row0 > 0, with the low pole row only (8 pole blocks before 48), no pole row (no pole blocks: d = blockIdx.x), the high
    pole row only, and the whole grid with a zone of three eights (120 blocks)."""
    eng = runs.eng
    try:
        _enter(eng)
        ref = runs.one_launch(win, K, boundary)      # (itself equal to rows [lo, hi) of the whole grid's)
        runs.graded(win, K, boundary, grading, 3, ref)
    finally:
        _reset(eng)


# ---- c. plan families -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("boundary", ["cyclic", "pointwise"])
@pytest.mark.parametrize("win", [MID_A, OWN200], ids=["rows64-264", "own200"])
def test_plan_families(runs, win, boundary):
    eng = runs.eng
    try:
        _enter(eng)
        ref = runs.one_launch(win, 4, boundary)
        for grading, launches in (((12, 8, 12), 4), ((9, 8, 9), 5), ((14, 8, 1), 3), ((14, 8, 20), 3), ((14, 1000, 14), 3)):
            runs.graded(win, 4, boundary, grading, launches, ref)
    finally:
        _reset(eng)


@pytest.mark.parametrize("boundary", ["cyclic", "pointwise"])
def test_a_wish_grading_zeroes_makes_one_launch(runs, boundary):
    """48 blocks / (5 launches + 2) < 8: no zone, so the dispatcher keeps the by-size chunk."""
    eng = runs.eng
    try:
        _enter(eng)
        ref = runs.one_launch(LOW, 4, boundary)
        runs.graded(LOW, 4, boundary, (9, 8, 9), 1, ref)
        runs.graded(LOW, 4, boundary, (14, 8, 14), 3, ref)      # (the same seeds are graded where the plan fits)
    finally:
        _reset(eng)


# ---- d. continuation in a shard -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [4, 0])
def test_graded_continuation_in_a_shard(runs, K):
    """lc_advect_from with row0 > 0: a range that begins at the call's first level starts from the given positions, in a
    later launch too, also when they are the output."""
    eng = runs.eng
    try:
        _enter(eng)
        ref = runs.one_launch(MID_B, K, "cyclic")
        eng.set_level_chunk(0)
        xa, ya = runs.advect(MID_B, K, "cyclic", nsteps=7)
        assert eng.last_advect_launches() == 1
        xk, yk = xa.clone(), ya.clone()
        runs.graded(MID_B, K, "cyclic", (12, 8, 12), 3, ref, t0=7, nsteps=NT - 1 - 7, start=(xa, ya))
        assert torch.equal(xa, xk) and torch.equal(ya, yk)       # (the start positions are read only)
        xi, yi = runs.graded(MID_B, K, "cyclic", (12, 8, 12), 3, ref, t0=7, nsteps=NT - 1 - 7, start=(xa, ya), out=(xa, ya))
        assert xi.data_ptr() == xa.data_ptr() and yi.data_ptr() == ya.data_ptr()
    finally:
        _reset(eng)


# ---- e. tile maps -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env", [{"LCS_XCD_CHUNK_ROWS": "0"}, {"LCS_XCD_CHUNK_ROWS": "2"}, {"LCS_XCD_SPLIT": "0"},
                                 {"LCS_TILE_ORDER": "0"}, {"LCS_TILE_ORDER": "1"}, {"LCS_TILE_ORDER": "2"}, {"LCS_TILE_ORDER": "3"}],
                         ids=lambda e: "-".join(f"{k}={v}" for k, v in e.items()))
def test_tile_maps_graded_equal_the_default_contexts_one_launch(runs, inputs, monkeypatch, env):
    """graded_slot feeds tile_of_block: contiguous bands (72 blocks), two tile rows per chunk (80), whole rows (136), the four
    tile orders.  The bits are those of the DEFAULT context's one-launch run."""
    try:
        _enter(runs.eng)
        refs = {win: runs.one_launch(win, 4, "cyclic") for win in (OWN200, MID_B)}
    finally:
        _reset(runs.eng)
    other = _context(monkeypatch, inputs, **env)
    try:
        _enter(other.eng)
        for win in (OWN200, MID_B):
            for grading, launches in (((14, 8, 14), 3), ((12, 8, 12), 4)):
                other.graded(win, 4, "cyclic", grading, launches, refs[win])
    finally:
        other.eng.close()


# ---- f. LCS_POLE_BLOCKS=0 -----------------------------------------------------------------------------------------------------
def test_pole_rows_inside_the_tiles_are_not_graded(runs, inputs, monkeypatch):
    try:
        _enter(runs.eng)
        refs = {win: runs.one_launch(win, 4, "cyclic") for win in (OWN200, MID_B)}
    finally:
        _reset(runs.eng)
    other = _context(monkeypatch, inputs, LCS_POLE_BLOCKS="0")
    try:
        _enter(other.eng)
        other.graded(OWN200, 4, "cyclic", (14, 8, 14), 1, refs[OWN200])   # pole rows in the tiles: their seeds go by the launch's range
        other.graded(MID_B, 4, "cyclic", (14, 8, 14), 3, refs[MID_B])     # no pole rows: graded as in any context
    finally:
        other.eng.close()


# ---- g. calls that must not be graded -----------------------------------------------------------------------------------------
def _both_settings(eng, call):
    """`call()` with grading forced and off: (launches, kernel, tensors) of each; the two must be the same."""
    made = []
    for grading in ((14, 8, 14), OFF):
        eng.set_level_chunk(-1)
        eng.set_level_grading(*grading)
        out = call()
        made.append((eng.last_advect_launches(), eng.last_advect_kernel(), [t.clone() for t in out]))
    (n_on, k_on, t_on), (n_off, k_off, t_off) = made
    assert n_on == n_off == 1, (n_on, n_off)          # 27 200 seeds (x 3 members): one launch by size
    assert k_on == k_off, (k_on, k_off)
    for a, b in zip(t_on, t_off):
        assert torch.equal(a, b)
    return k_on, t_on


def test_ensembles_are_not_graded(runs):
    eng, lo, hi = runs.eng, *OWN200[:2]
    try:
        _enter(eng)
        name, (x, y) = _both_settings(eng, lambda: eng.advect_batch(runs.f, runs.glat[lo:hi], runs.glon, DT, 3, NT - 1 - 2, SETTLS_order=4))
        assert name == "advect_lds2_kernel<4, true, 3>"
        eng.set_level_chunk(0)
        for m in range(3):      # each member is advect(t0 = m) bit for bit
            xm, ym = runs.advect(OWN200, 4, "cyclic", t0=m, nsteps=NT - 1 - 2)
            assert torch.equal(x[m], xm) and torch.equal(y[m], ym), m
    finally:
        _reset(eng)


def test_wide_patches_are_not_graded(runs, inputs, monkeypatch):
    try:
        _enter(runs.eng)
        ref = runs.one_launch(OWN200, 4, "cyclic")
    finally:
        _reset(runs.eng)
    other = _context(monkeypatch, inputs, LCS_PATCH_MODE="1")
    try:
        _enter(other.eng)
        name, (x, y) = _both_settings(other.eng, lambda: other.advect(OWN200, 4, "cyclic"))
        assert name == "advect_lds2_kernel<4, true, 1>"
        assert torch.equal(x, ref[0]) and torch.equal(y, ref[1])
    finally:
        other.eng.close()


def test_order_3_the_one_seed_kernel_and_float64_are_not_graded(runs, inputs):
    eng, lo, hi = runs.eng, *OWN200[:2]
    u, v, lat, lon, glat, glon = inputs
    try:
        _enter(eng)
        ref = runs.one_launch(OWN200, 4, "cyclic")
        f3 = eng.prepare_field(u, v, lat, lon, 3)
        name, _ = _both_settings(eng, lambda: eng.advect(f3, glat[lo:hi], glon, DT, SETTLS_order=4, interp_order=3))
        assert name == "advect_lds2_o3_kernel<4, true, 0>"
        eng.set_lds_tiles(2)
        name, (x, y) = _both_settings(eng, lambda: runs.advect(OWN200, 4, "cyclic"))
        assert name == "advect_lds_kernel<1, 4, true>"
        assert torch.equal(x, ref[0]) and torch.equal(y, ref[1])
        eng.set_lds_tiles(1)
        d = np.float64
        f64 = eng.prepare_field(u.astype(d), v.astype(d), lat.astype(d), lon.astype(d), 1)
        name, (x64, y64) = _both_settings(eng, lambda: eng.advect(f64, glat[lo:hi].astype(d), glon.astype(d), DT, SETTLS_order=4, interp_order=1))
        assert name.startswith("advect_lds64_kernel<4, true"), name
        assert x64.dtype == torch.float64
    finally:
        _reset(eng)


# ---- the oracle anchor: where the chain of bit identities ends ------------------------------------------------------------------
@pytest.mark.parametrize("boundary", ["cyclic", "pointwise"])
@pytest.mark.parametrize("K", [4, 0])
def test_the_one_launch_run_sits_in_the_float32_oracles_band(runs, inputs, K, boundary):
    """The whole 328 x 136 grid in one launch against oracle.lcs_oracle.parcel_propagation in float32 and float64 on 46 rows
    (the rows on either side of the shards' and the tiles' edges among them) x 34 columns.  Floors: the full-size C3 test's
    (1e-4, 5e-4, 2e-3) degrees for 96 steps of 5 position updates, scaled by the updates made here, 41 (1 + K) / (96 x 5).
    Measured on an MI355X (degrees; median, p99, max; the float32 oracle's own error after the bar; no seed off by 0.5):
      cyclic    K = 4   3.113e-05 7.559e-04 2.392e-03 | 3.000e-05 6.702e-04 3.162e-03
      pointwise K = 4   2.308e-05 5.232e-04 2.392e-03 | 2.179e-05 4.030e-04 3.162e-03
      cyclic    K = 0   1.385e-05 1.179e-04 3.849e-04 | 1.103e-05 1.269e-04 3.697e-04
      pointwise K = 0   1.261e-05 1.149e-04 2.060e-04 | 1.014e-05 1.136e-04 2.217e-04
    The scaled floors are (4.3e-5, 2.1e-4, 8.5e-4) at K = 4 and (8.5e-6, 4.3e-5, 1.7e-4) at K = 0: each is below the oracle's own
    figure times its factor (2, 3, 4), so the oracle's error sets the band in all four cases."""
    from oracle import lcs_oracle as O
    u, v, lat, lon, glat, glon = inputs
    eng = runs.eng
    try:
        _enter(eng)
        x, y = runs.one_launch(WHOLE, K, boundary)
        rows, cols = subset(NY, 40, 1, must=(63, 64, 127, 128, 263, 264)), subset(NX, 34, 0)
        xg = x[rows][:, cols].cpu().numpy().astype(np.float64)
        yg = y[rows][:, cols].cpu().numpy().astype(np.float64)
        kw = dict(timestep=DT, SETTLS_order=K, interp_order=1, **BOUNDARIES[boundary])
        o = {}
        for d in (np.float32, np.float64):
            c = lambda a: np.asarray(a).astype(d)
            o[d] = O.parcel_propagation(c(u), c(v), c(lat), c(lon), seed_lat=c(glat)[rows], seed_lon=c(glon)[cols], **kw)
        scale = (NT - 1) * (1 + K) / (96 * 5)
        floors = tuple(fl * scale for fl in (1e-4, 5e-4, 2e-3))
        positions_check(eng, runs.f, glat, glon, rows, cols, xg, yg, o[np.float32], o[np.float64],
                        f"graded anchor {boundary} K={K} (41 steps)", floors, interp_order=1, K=K, timestep=DT)
    finally:
        _reset(eng)
