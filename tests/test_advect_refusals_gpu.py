"""Every refusal of lc_advect_ex / lc_advect_series / lc_advect_series_dirs and of lc_sample_raw, through the C ABI: the
status code and a distinctive fragment of lc_last_error() for each, one row per check of the argument intake
(advect.hip: advect_ex_checked, lc_sample_raw), in the order of the checks.

Every row is the valid call below (an 8 x 8 field of 2 levels, 4 x 4 seeds) with the named fields changed so that ONLY
the refusal it names can fire: the checks before it pass and so would the ones after it.  The rows of ``ORDER`` break
two rules at once and expect the earlier check's answer.  No row reaches a kernel launch: the call returns from the
checks (the one launch of this file is the valid call itself, which shows that the rows start from an accepted one)."""
import ctypes as C

import pytest

from lagrangiancoherence_amd import _capi, build
from lagrangiancoherence_amd._capi import (LC_EINVAL, LC_EUNSUPPORTED, LC_F32, LC_F64, LC_F64_WIND_F32, LC_F64_WIND_F32_LIN32,
                                           LC_OK, LC_X_CLAMP_REFERENCE_OUTER, LC_X_CYCLIC)

pytestmark = pytest.mark.gpu

NT, NF, NS = 2, 8, 4          # levels, field rows = columns, seed rows = columns
NONE = None                   # a pointer field set to NULL


@pytest.fixture(scope="module")
def lib():
    build.build_library(verbose=False)
    return _capi.load()


@pytest.fixture(scope="module")
def ctx(lib):
    c = C.c_void_p()
    _capi.check(lib.lc_ctx_create(0, C.byref(c)), lib)
    yield c
    lib.lc_ctx_destroy(c)


@pytest.fixture(scope="module")
def buffers():
    """Zeroed device buffers, each large enough for whatever a row names it as (float64 images of the field, 4 members of
    positions, a trajectory): a row that was wrongly accepted would run on valid memory."""
    import torch
    names = ("lin", "cub", "ext", "u", "v", "slat", "slon", "xs", "ys", "xo", "yo", "tx", "ty", "px", "py", "ou", "ov")
    buf = {n: torch.zeros(1024, dtype=torch.float64, device="cuda") for n in names}
    torch.cuda.synchronize()
    return buf


def base_args(buf):
    """The valid call: float32, order 1, one SETTLS iteration, cyclic, one step from level 0, no trajectory."""
    p = {k: t.data_ptr() for k, t in buf.items()}
    return dict(struct_size=C.sizeof(_capi.AdvectArgs), packed_lin=p["lin"], packed_cub=NONE, packed_ext=NONE, u_raw=NONE,
                v_raw=NONE, dtype=LC_F32, nt=NT, ny_f=NF, nx_f=NF, lat_min=-40.0, lat_max=40.0, lon_min=-180.0, lon_max=135.0,
                seed_lat_dev=p["slat"], ny=NS, seed_lon_dev=p["slon"], nx=NS, row0=0, ny_global=NS, x_start=NONE, y_start=NONE,
                timestep=3600.0, settls_order=1, interp_order=1, cyclic_x=LC_X_CYCLIC, t0=0, nsteps=1, n_members=1, t0_stride=0,
                x_out=p["xo"], y_out=p["yo"], traj_x=NONE, traj_y=NONE, fuse_levels_raw=0)


def call(lib, ctx, entry, fields):
    a = _capi.AdvectArgs(**fields)
    if entry == "ex":
        return lib.lc_advect_ex(ctx, C.byref(a))
    if entry == "series":
        return lib.lc_advect_series(ctx, C.byref(a))
    return lib.lc_advect_series_dirs(ctx, C.byref(a), int(entry))   # "0" .. "3": lc_advect_series_dirs with that n_dirs


# (id, entry point, fields changed -- a str value names a buffer --, status, fragment of the message)
LIN32_O3 = dict(dtype=LC_F64_WIND_F32_LIN32, interp_order=3, packed_lin=NONE, packed_cub="cub", u_raw="u", v_raw="v")
ROWS = [
    ("n_members_0", "ex", dict(n_members=0), LC_EINVAL, "bad n_members 0 / t0_stride 0"),
    ("n_members_times_dirs_too_many", "2", dict(n_members=32768), LC_EINVAL, "bad n_members 32768"),
    ("t0_stride_negative", "ex", dict(t0_stride=-1), LC_EINVAL, "bad n_members 1 / t0_stride -1"),
    ("series_with_traj", "series", dict(traj_x="tx", traj_y="ty"), LC_EINVAL, "lc_advect_series: traj_x / traj_y must be NULL"),
    ("series_row_block", "series", dict(row0=1, ny=3), LC_EUNSUPPORTED, "whole seed grids only (rows [1,4) of 4 given)"),
    ("batch_with_traj", "ex", dict(n_members=2, traj_x="tx", traj_y="ty"), LC_EINVAL, "lc_advect_batch: trajectories are per member"),
    ("batch_outer_clamp", "ex", dict(n_members=2, cyclic_x=LC_X_CLAMP_REFERENCE_OUTER), LC_EUNSUPPORTED,
     "lc_advect_batch: LC_X_CLAMP_REFERENCE_OUTER is decided per member"),
    ("x_start_without_y_start", "ex", dict(x_start="xs"), LC_EINVAL, "x_start and y_start must both be set or both NULL"),
    ("y_start_without_x_start", "ex", dict(y_start="ys"), LC_EINVAL, "x_start and y_start must both be set or both NULL"),
    ("x_start_outer_clamp", "ex", dict(x_start="xs", y_start="ys", cyclic_x=LC_X_CLAMP_REFERENCE_OUTER), LC_EUNSUPPORTED,
     "cannot continue from given positions"),
    ("bad_dtype", "ex", dict(dtype=7), LC_EINVAL, "lc_advect: bad dtype 7"),
    ("wind_f32_with_ext", "ex", dict(dtype=LC_F64_WIND_F32, packed_ext="ext"), LC_EINVAL, "LC_F64_WIND_F32 keeps the two-sample form (no ext)"),
    ("lin32_with_ext", "ex", dict(dtype=LC_F64_WIND_F32_LIN32, packed_ext="ext"), LC_EINVAL, "LC_F64_WIND_F32 keeps the two-sample form (no ext)"),
    ("lin32_order_2", "ex", dict(dtype=LC_F64_WIND_F32_LIN32, interp_order=2, packed_cub="cub"), LC_EUNSUPPORTED,
     "LC_F64_WIND_F32_LIN32 serves interp_order 1 and 3 with cyclic / per-point boundaries; interp_order 2"),
    ("lin32_outer_clamp", "ex", dict(dtype=LC_F64_WIND_F32_LIN32, cyclic_x=LC_X_CLAMP_REFERENCE_OUTER), LC_EUNSUPPORTED,
     "LC_F64_WIND_F32_LIN32 serves interp_order 1 and 3 with cyclic / per-point boundaries; interp_order 1"),
    ("lin32_order_1_with_cub", "ex", dict(dtype=LC_F64_WIND_F32_LIN32, packed_cub="cub"), LC_EINVAL,
     "LC_F64_WIND_F32_LIN32 at order 1 takes packed_lin"),
    ("lin32_order_1_with_planes", "ex", dict(dtype=LC_F64_WIND_F32_LIN32, u_raw="u", v_raw="v"), LC_EINVAL,
     "LC_F64_WIND_F32_LIN32 at order 1 takes packed_lin"),
    ("lin32_order_3_without_planes", "ex", dict(LIN32_O3, u_raw=NONE, v_raw=NONE), LC_EINVAL, "LC_F64_WIND_F32_LIN32 at order 3 takes packed_cub"),
    ("lin32_order_3_with_lin", "ex", dict(LIN32_O3, packed_lin="lin"), LC_EINVAL, "LC_F64_WIND_F32_LIN32 at order 3 takes packed_cub"),
    ("interp_order_0", "ex", dict(interp_order=0), LC_EUNSUPPORTED, "lc_advect: interp_order 0 unsupported"),
    ("interp_order_6", "ex", dict(interp_order=6, packed_cub="cub"), LC_EUNSUPPORTED, "lc_advect: interp_order 6 unsupported"),
    ("u_raw_without_v_raw", "ex", dict(dtype=LC_F64, u_raw="u"), LC_EINVAL, "lc_advect_ex: u_raw and v_raw must both be set or both NULL"),
    ("no_packed_lin", "ex", dict(packed_lin=NONE), LC_EINVAL, "lc_advect: packed_lin is required"),
    ("no_packed_lin_f32_order_1_planes", "ex", dict(packed_lin=NONE, u_raw="u", v_raw="v"), LC_EINVAL, "lc_advect: packed_lin is required"),
    ("no_packed_cub_order_3", "ex", dict(interp_order=3), LC_EINVAL, "interp_order > 1 needs packed_cub"),
    ("packed_ext_order_2", "ex", dict(interp_order=2, packed_cub="cub", packed_ext="ext"), LC_EINVAL, "orders 2, 4, 5 take no packed_ext"),
    ("field_too_small", "ex", dict(ny_f=3), LC_EINVAL, "field too small (nt=2 ny_f=3 nx_f=8)"),
    ("null_seed_lat", "ex", dict(seed_lat_dev=NONE), LC_EINVAL, "lc_advect: bad seed grid"),
    ("no_seed_columns", "ex", dict(nx=0), LC_EINVAL, "lc_advect: bad seed grid"),
    ("rows_outside_global_grid", "ex", dict(row0=2), LC_EINVAL, "rows [2,6) outside global grid of 4 rows"),
    ("settls_order_negative", "ex", dict(settls_order=-1), LC_EINVAL, "SETTLS_order must be >= 0"),
    ("cyclic_x_3", "ex", dict(cyclic_x=3), LC_EINVAL, "lc_advect: bad cyclic_x 3"),
    ("cyclic_x_negative", "ex", dict(cyclic_x=-1), LC_EINVAL, "lc_advect: bad cyclic_x -1"),
    ("outer_clamp_row_block_without_reducer", "ex", dict(cyclic_x=LC_X_CLAMP_REFERENCE_OUTER, ny_global=8), LC_EUNSUPPORTED,
     "a row block (rows [0,4) of 8) needs lc_ctx_set_flag_allreduce"),
    ("steps_past_the_last_level", "ex", dict(nsteps=2), LC_EINVAL, "steps [0,2) need levels up to 2, have 2"),
    ("members_past_the_last_level", "series", dict(n_members=2, t0_stride=1), LC_EINVAL, "steps [0,2) need levels up to 2, have 2"),
    ("null_x_out", "ex", dict(x_out=NONE), LC_EINVAL, "lc_advect: null output"),
    ("traj_x_without_traj_y", "ex", dict(traj_x="tx"), LC_EINVAL, "traj_x and traj_y must both be set or both NULL"),
    ("descending_latitudes", "ex", dict(lat_min=40.0, lat_max=-40.0), LC_EINVAL, "lc_advect: field coordinates must be ascending"),
    ("equal_longitudes", "ex", dict(lon_max=-180.0), LC_EINVAL, "lc_advect: field coordinates must be ascending"),
    # (nsteps = 0: were these ever accepted, the call would sample nothing of a field this size)
    ("level_too_large_f32", "ex", dict(ny_f=1 << 15, nx_f=1 << 15, nsteps=0), LC_EUNSUPPORTED,
     "a 32768x32768 time level is too large for 32-bit tap offsets"),
    ("row_too_long", "ex", dict(nx_f=(1 << 24) - 3, nsteps=0), LC_EUNSUPPORTED, "a 8x16777213 time level is too large for 32-bit tap offsets"),
]

# two rules broken at once: the check that comes first in the intake answers
ORDER = [
    ("members_before_dtype", "ex", dict(n_members=0, dtype=7), LC_EINVAL, "bad n_members 0"),
    ("series_traj_before_row_block", "series", dict(traj_x="tx", traj_y="ty", row0=1, ny=3), LC_EINVAL, "traj_x / traj_y must be NULL"),
    ("start_pair_before_dtype", "ex", dict(x_start="xs", dtype=7), LC_EINVAL, "x_start and y_start"),
    ("dtype_before_interp_order", "ex", dict(dtype=7, interp_order=0), LC_EINVAL, "bad dtype 7"),
    ("lin32_shape_before_interp_order", "ex", dict(dtype=LC_F64_WIND_F32_LIN32, interp_order=0), LC_EUNSUPPORTED, "LC_F64_WIND_F32_LIN32 serves"),
    ("interp_order_before_planes", "ex", dict(interp_order=6, dtype=LC_F64, u_raw="u"), LC_EUNSUPPORTED, "interp_order 6 unsupported"),
    ("planes_before_packed_lin", "ex", dict(dtype=LC_F64, u_raw="u", packed_lin=NONE), LC_EINVAL, "u_raw and v_raw must both"),
    ("packed_lin_before_packed_cub", "ex", dict(packed_lin=NONE, interp_order=3), LC_EINVAL, "packed_lin is required"),
    ("packed_cub_before_field_size", "ex", dict(interp_order=3, ny_f=3), LC_EINVAL, "needs packed_cub"),
    ("field_size_before_seeds", "ex", dict(ny_f=3, seed_lon_dev=NONE), LC_EINVAL, "field too small"),
    ("seeds_before_rows", "ex", dict(seed_lon_dev=NONE, row0=2), LC_EINVAL, "bad seed grid"),
    ("rows_before_settls_order", "ex", dict(row0=2, settls_order=-1), LC_EINVAL, "outside global grid"),
    ("settls_order_before_cyclic_x", "ex", dict(settls_order=-1, cyclic_x=3), LC_EINVAL, "SETTLS_order"),
    ("row_block_before_steps", "ex", dict(cyclic_x=LC_X_CLAMP_REFERENCE_OUTER, ny_global=8, nsteps=2), LC_EUNSUPPORTED, "needs lc_ctx_set_flag_allreduce"),
    ("steps_before_output", "ex", dict(nsteps=2, y_out=NONE), LC_EINVAL, "need levels up to 2"),
    ("output_before_traj_pair", "ex", dict(y_out=NONE, traj_y="ty"), LC_EINVAL, "null output"),
    ("traj_pair_before_coordinates", "ex", dict(traj_y="ty", lon_max=-180.0), LC_EINVAL, "traj_x and traj_y must both"),
    ("coordinates_before_level_size", "ex", dict(lat_max=-40.0, nx_f=(1 << 24) - 3, nsteps=0), LC_EINVAL, "must be ascending"),
]


def resolved(fields, buf):
    return {k: (buf[v].data_ptr() if isinstance(v, str) else v) for k, v in fields.items()}


def test_the_rows_start_from_an_accepted_call(lib, ctx, buffers):
    import torch
    for entry in ("ex", "series", "1", "2"):
        _capi.check(call(lib, ctx, entry, base_args(buffers)), lib)
    torch.cuda.synchronize()


@pytest.mark.parametrize("name,entry,changed,status,fragment", ROWS + ORDER, ids=[r[0] for r in ROWS + ORDER])
def test_advect_refusal(lib, ctx, buffers, name, entry, changed, status, fragment):
    fields = dict(base_args(buffers), **resolved(changed, buffers))
    assert call(lib, ctx, entry, fields) == status
    assert fragment in lib.lc_last_error().decode()


def test_advect_refusals_that_need_no_context(lib, buffers):
    """What is checked before the context: the argument structure itself and lc_advect_series_dirs's n_dirs; then the
    context."""
    good = _capi.AdvectArgs(**base_args(buffers))
    assert lib.lc_advect_ex(None, None) == LC_EINVAL and "lc_advect_ex: null arguments" in lib.lc_last_error().decode()
    short = _capi.AdvectArgs(**dict(base_args(buffers), struct_size=C.sizeof(_capi.AdvectArgs) - 8))
    for fn in (lib.lc_advect_ex, lib.lc_advect_series):
        assert fn(None, C.byref(short)) == LC_EINVAL
        assert f"struct_size {C.sizeof(_capi.AdvectArgs) - 8}, this library's lc_advect_args has {C.sizeof(_capi.AdvectArgs)} bytes" \
            in lib.lc_last_error().decode()
    for n_dirs in (0, 3, -1):
        assert lib.lc_advect_series_dirs(None, C.byref(good), n_dirs) == LC_EINVAL
        assert f"lc_advect_series_dirs: n_dirs {n_dirs} (1 or 2)" in lib.lc_last_error().decode()
    # struct_size before n_dirs, n_dirs before the context
    assert lib.lc_advect_series_dirs(None, C.byref(short), 3) == LC_EINVAL and "struct_size" in lib.lc_last_error().decode()
    for fn in (lib.lc_advect_ex, lib.lc_advect_series):
        assert fn(None, C.byref(good)) == LC_EINVAL and "lc_advect: null context" in lib.lc_last_error().decode()
    assert lib.lc_advect_series_dirs(None, C.byref(good), 2) == LC_EINVAL and "lc_advect: null context" in lib.lc_last_error().decode()
    # the context before everything else in the structure
    bad = _capi.AdvectArgs(**dict(base_args(buffers), n_members=0, dtype=7))
    assert lib.lc_advect_ex(None, C.byref(bad)) == LC_EINVAL and "null context" in lib.lc_last_error().decode()


# ------------------------------------------------------------------ lc_sample_raw
def sample_args(buf):
    p = {k: t.data_ptr() for k, t in buf.items()}
    return dict(packed_lin=p["lin"], packed_cub=NONE, u_raw=NONE, v_raw=NONE, dtype=LC_F32, nt=NT, ny_f=NF, nx_f=NF, lat_min=-40.0,
                lat_max=40.0, lon_min=-180.0, lon_max=135.0, level=0, pos_x=p["px"], pos_y=p["py"], ny=NS, nx=NS, row0=0,
                ny_global=NS, interp_order=1, out_u=p["ou"], out_v=p["ov"])


def sample_call(lib, ctx, fields):
    order = ("packed_lin", "packed_cub", "u_raw", "v_raw", "dtype", "nt", "ny_f", "nx_f", "lat_min", "lat_max", "lon_min", "lon_max",
             "level", "pos_x", "pos_y", "ny", "nx", "row0", "ny_global", "interp_order", "out_u", "out_v")
    return lib.lc_sample_raw(ctx, *(fields[k] for k in order))


SAMPLE_ROWS = [
    ("bad_dtype", dict(dtype=5), LC_EINVAL, "lc_sample: bad dtype 5"),
    ("wind_f32_dtype", dict(dtype=LC_F64_WIND_F32), LC_EINVAL, "lc_sample: bad dtype 2"),
    ("interp_order_0", dict(interp_order=0), LC_EUNSUPPORTED, "lc_sample: interp_order 0 unsupported"),
    ("interp_order_6", dict(interp_order=6, packed_cub="cub"), LC_EUNSUPPORTED, "lc_sample: interp_order 6 unsupported"),
    ("u_raw_without_v_raw", dict(dtype=LC_F64, u_raw="u"), LC_EINVAL, "lc_sample_raw: u_raw and v_raw must both be set or both NULL"),
    ("no_image", dict(packed_lin=NONE), LC_EINVAL, "lc_sample: missing field image"),
    ("no_image_f32_order_1_planes", dict(packed_lin=NONE, u_raw="u", v_raw="v"), LC_EINVAL, "lc_sample: missing field image"),
    ("no_cub_order_3", dict(interp_order=3), LC_EINVAL, "lc_sample: missing field image"),
    ("null_positions", dict(pos_y=NONE), LC_EINVAL, "lc_sample: null pointer"),
    ("null_output", dict(out_u=NONE), LC_EINVAL, "lc_sample: null pointer"),
    ("level_is_nt", dict(level=NT), LC_EINVAL, "lc_sample: bad sizes"),
    ("level_negative", dict(level=-1), LC_EINVAL, "lc_sample: bad sizes"),
    ("field_too_small", dict(nx_f=3), LC_EINVAL, "lc_sample: bad sizes"),
    ("rows_outside_global_grid", dict(row0=1), LC_EINVAL, "lc_sample: rows outside the global grid"),
    ("descending_longitudes", dict(lon_min=135.0, lon_max=-180.0), LC_EINVAL, "lc_sample: field coordinates must be ascending"),
    # two at once: the earlier check answers
    ("dtype_before_interp_order", dict(dtype=5, interp_order=0), LC_EINVAL, "bad dtype 5"),
    ("interp_order_before_planes", dict(interp_order=0, dtype=LC_F64, v_raw="v"), LC_EUNSUPPORTED, "interp_order 0 unsupported"),
    ("planes_before_image", dict(dtype=LC_F64, v_raw="v", packed_lin=NONE), LC_EINVAL, "u_raw and v_raw must both"),
    ("image_before_pointers", dict(packed_lin=NONE, pos_x=NONE), LC_EINVAL, "missing field image"),
    ("pointers_before_sizes", dict(out_v=NONE, level=NT), LC_EINVAL, "null pointer"),
    ("sizes_before_rows", dict(level=NT, row0=1), LC_EINVAL, "bad sizes"),
    ("rows_before_coordinates", dict(row0=1, lat_max=-40.0), LC_EINVAL, "rows outside the global grid"),
]


def test_sample_rows_start_from_an_accepted_call(lib, ctx, buffers):
    import torch
    _capi.check(sample_call(lib, ctx, sample_args(buffers)), lib)
    torch.cuda.synchronize()


@pytest.mark.parametrize("name,changed,status,fragment", SAMPLE_ROWS, ids=[r[0] for r in SAMPLE_ROWS])
def test_sample_refusal(lib, ctx, buffers, name, changed, status, fragment):
    fields = dict(sample_args(buffers), **resolved(changed, buffers))
    assert sample_call(lib, ctx, fields) == status
    assert fragment in lib.lc_last_error().decode()


def test_sample_refuses_a_null_context_first(lib, buffers):
    assert sample_call(lib, None, dict(sample_args(buffers), dtype=5)) == LC_EINVAL
    assert "lc_sample: null context" in lib.lc_last_error().decode()
