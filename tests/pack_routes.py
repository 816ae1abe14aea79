"""Route table: every distinct path through the pack dispatcher (``pack_impl`` in ``csrc/pack.hip``) and how it is reached.

Plain data, imported by ``test_pack_routes.py`` (completeness, no GPU) and ``test_pack_routes_gpu.py`` (forces every route on
the GPU, asserts the name ``lc_ctx_last_pack_kernel`` reports and compares the whole image with scipy).  Routes may share a
reported name (the float32 and float64 instances of one kernel, the forms of ``pack_fused_kernel``), so the key is a route id.

An entry is a dict:

- ``name``: what ``lc_ctx_last_pack_kernel`` must report;
- ``dtype``: ``float32``, ``float64`` or ``f64_wind_f32`` (float32 planes in, float64 coefficients out: ``LC_F64_WIND_F32``,
  orders 2..5 without the fused-level image);
- ``order`` (1..5);
- ``env``: ``LCS_FIR_PREFILTER`` / ``LCS_FUSED_PREFILTER``, read once at context creation (absent: the default, 1);
- ``ext``: the fused-level image ``ext[t] = 2 img[t] - img[t+1]`` is built in the same call (a series of one level has none:
  there the call is made without it, as ``Engine.prepare_field`` does);
- ``lin``: order 1 only; False is the ``packed_dev == NULL`` form (the fused-level image alone; the C ABI wants ``nt >= 2``);
- ``shapes``: ``(nt, ny, nx)`` tuples, the smallest at which the kernel's own structure is exercised;
- ``tol``: a class of ``TOL`` (``exact``: order 1, the raw values).

``dispatch`` restates the dispatcher's conditions; ``test_pack_routes.py`` proves with it that every shape reaches the route
it is listed under, before any GPU time is spent, and the GPU test takes from it the name of the call without ``ext``.
"""

FIR_MIN = 16        # FHALO + 2: each reflection of the FIR kernel's 14-node halo stays inside the grid
STREAM_MIN = 64     # PR_CHUNK, RS_RING, the 64-term horizon of the column-stream and fused forms
FIR_TILE = 32       # FT: nodes per FIR tile edge; also PR_ROWS / RS_ROWS, the rows of a row-sweep block

ENV_KNOBS = ("LCS_FIR_PREFILTER", "LCS_FUSED_PREFILTER")

# Tolerance classes: max |image - scipy.ndimage.spline_filter(float64(F), order, mode="mirror")| over the interior.
#   ("rel", c): c * max|F|;  ("abs", c): c (fields of scale 20);  "f32_store": see f32_store_bound().
# The first five are the bounds the parity tests already state for the same kernels, not new numbers.
TOL = {
    "exact": ("abs", 0.0),
    "f64_o3": ("rel", 2e-14),      # streaming-prefilter tests
    "f64_o2": ("abs", 1e-12),      # generic-order test
    "f64_o45": ("abs", 5e-11),     # generic-order test (scipy's pole constants of orders 4, 5 differ in the last bit)
    "f32_fir": ("rel", 3e-6),      # one-pass FIR test: the 14-tap cut (1.2e-8) plus a few float32 ulps of the field's scale
    # float32 image from double arithmetic (the recursive sweeps, the generic orders).  The existing caps (2e-5 .. 4e-5 at unit
    # scale) are loose; the floor is computable: rounding scipy's float64 result to float32.  Bound: 4 x that rounding error
    # + one float32 ulp of max|coefficients| per sweep (a sweep stores its line in float32 before the next one reads it:
    # order 2, 3: one pole x two axes = 2; orders 4, 5: two poles x two axes = 4).
    # Measured on an MI355X, fields of scale 20 (max error, its bound, the ratio; the worst shape of each group; the GPU test
    # prints every case, pytest -s):
    #   f32_o3_small 1.9e-5 / 6.1e-5 (0.31)   f32_o3_small_wide 2.3e-5 / 9.8e-5 (0.24)
    #   f32_o3_sweeps 2.4e-5 / 6.1e-5 (0.39)  f32_o3_sweeps_lds 3.3e-5 / 9.1e-5 (0.36)
    #   float32_o2 1.5e-5 / 6.1e-5 (0.25)     float32_o4 8.2e-5 / 1.8e-4 (0.45)     float32_o5 1.2e-4 / 3.7e-4 (0.33)
    #   3 x 65540 x 4 at order 3: 4.0e-5 / 1.2e-4 (0.33)   65600 x 4 x 4 at order 2: 2.6e-5 / 6.1e-5 (0.43)
    # (f32_fir on the same run: img 0.19 .. 0.36 of its bound, the mode-2 ext 0.21 .. 0.41; the float64 classes 0.07 .. 0.43.)
    # Every route fitted its class on its first run.
    "f32_store": "f32_store",
}


def sweeps(order):
    """Recursive passes whose result is stored in the image's dtype: poles x axes."""
    return 2 * (1 if order in (2, 3) else 2)


def f32_store_bound(ref64, order):
    """The ``f32_store`` bound for a float64 scipy result ``ref64`` (numpy array)."""
    import numpy as np
    floor = float(np.abs(ref64.astype(np.float32).astype(np.float64) - ref64).max())
    return 4.0 * floor + sweeps(order) * float(np.spacing(np.float32(np.abs(ref64).max())))


def dispatch(dtype, order, nt, ny, nx, fir=1, fused=1, ext=False):
    """(reported name, tail kernel or None) of lc_field_pack: pack_impl's conditions, restated."""
    f64 = dtype != "float32"
    tin = "float" if dtype != "float64" else "double"
    ext = bool(ext) and nt >= 2
    tail = "pads_ext_kernel" if ext else "pads_only_kernel"
    if order == 1:
        assert dtype != "f64_wind_f32"          # refused by lc_field_pack
        return "pack_fused_kernel", None
    assert not (dtype == "f64_wind_f32" and ext)
    if dtype == "float32" and order == 3 and ny >= FIR_MIN and nx >= FIR_MIN and fir:
        if ext and fir == 2:
            return "prefilter_fir_kernel (img + ext)", None
        return "prefilter_fir_kernel", ("pads_ext_kernel" if ext else None)
    if order != 3:
        return "pack_interior_kernel + prefilter_general_kernel", tail
    stream = f64 and bool(fir)
    cols_stream = stream and ny >= STREAM_MIN
    if cols_stream and nx >= STREAM_MIN and fused:
        return f"prefilter_fused_stream_kernel<{tin}>", tail
    cols = "prefilter_cols_stream_kernel" if cols_stream else "prefilter_cols_kernel"
    if stream and nx >= STREAM_MIN:
        rows = "prefilter_rows_stream_kernel"
    elif nx >= STREAM_MIN:
        rows = "prefilter_rows_lds_kernel"
    else:
        rows = "prefilter_rows_kernel"
    return f"{cols} + {rows}", tail


ROUTES = {}


def _add(rid, name, **kw):
    assert rid not in ROUTES, rid
    r = dict(dtype="float32", order=3, env={}, ext=True, lin=True, tol="f32_store")
    r.update(kw)
    r["name"] = name
    r["shapes"] = tuple(r["shapes"])
    ROUTES[rid] = r


def _nt(nts, grids):
    return tuple((t,) + g for g in grids for t in nts)


FIR0 = {"LCS_FIR_PREFILTER": "0"}
FIR2 = {"LCS_FIR_PREFILTER": "2"}
UNFUSED = {"LCS_FUSED_PREFILTER": "0"}

# ------------------------------------------------------------------ order 1: pack_fused_kernel (level chunk PACK_LV = 2)
for _dt in ("float32", "float64"):
    _add(f"{_dt}_o1_lin_ext", "pack_fused_kernel", dtype=_dt, order=1, shapes=_nt((1, 2, 3, 5), [(9, 11)]), tol="exact")
    _add(f"{_dt}_o1_lin", "pack_fused_kernel", dtype=_dt, order=1, ext=False, shapes=_nt((1, 2, 3, 5), [(9, 11)]), tol="exact")
    _add(f"{_dt}_o1_ext", "pack_fused_kernel", dtype=_dt, order=1, lin=False, shapes=_nt((2, 3, 5), [(9, 11)]), tol="exact")

# ------------------------------------------------------------------ float32, order 3
# the FIR: the smallest legal grid (the 14-node halo reflected at both ends of one tile), less than one 32-node tile, ragged last
# tiles, and ny = 33, 34, 35: the pads' source rows 1, ny-2, ny-3 in different tiles
FIR_GRIDS = [(16, 16), (16, 47), (33, 31), (34, 65), (35, 33)]
_add("f32_o3_fir", "prefilter_fir_kernel", shapes=_nt((1, 3), FIR_GRIDS), tol="f32_fir")
_add("f32_o3_fir_no_ext", "prefilter_fir_kernel", ext=False, shapes=[(3, 16, 16), (3, 34, 65)], tol="f32_fir")
# mode 2: ext[t] = P(2 F[t] - F[t+1]) as a second filtered image (nt 2: its last level returns at once; a single level has no
# ext and reports the plain name: f32_o3_fir's nt = 1 shapes)
_add("f32_o3_fir2", "prefilter_fir_kernel (img + ext)", env=FIR2, shapes=_nt((2, 3), FIR_GRIDS), tol="f32_fir")
_add("f32_o3_fir2_no_ext", "prefilter_fir_kernel", env=FIR2, ext=False, shapes=[(3, 33, 31)], tol="f32_fir")
# too small for the FIR: the recursive sweeps in the default configuration
_add("f32_o3_small", "prefilter_cols_kernel + prefilter_rows_kernel", shapes=_nt((1, 3), [(15, 40), (40, 15)]))
_add("f32_o3_small_wide", "prefilter_cols_kernel + prefilter_rows_lds_kernel", shapes=_nt((1, 3), [(12, 150)]))
# the FIR off: both row sweeps (PR_CHUNK 64: one chunk, one node over; PR_ROWS 32: one row over a block)
_add("f32_o3_sweeps", "prefilter_cols_kernel + prefilter_rows_kernel", env=FIR0, shapes=_nt((1, 3), [(16, 47), (35, 33), (65, 63)]))
_add("f32_o3_sweeps_lds", "prefilter_cols_kernel + prefilter_rows_lds_kernel", env=FIR0,
     shapes=_nt((1, 3), [(33, 64), (33, 65), (12, 150)]))

# ------------------------------------------------------------------ float64 coefficients, order 3: float64 and float32 planes
STREAM_GRIDS = [(64, 64), (65, 97), (257, 70)]
for _dt, _tin, _ext in (("float64", "double", True), ("f64_wind_f32", "float", False)):
    _kw = dict(dtype=_dt, ext=_ext, tol="f64_o3")
    _add(f"{_dt}_o3_fused", f"prefilter_fused_stream_kernel<{_tin}>", shapes=_nt((3,), STREAM_GRIDS) + ((1, 64, 64),), **_kw)
    _add(f"{_dt}_o3_cs_rs", "prefilter_cols_stream_kernel + prefilter_rows_stream_kernel", env=UNFUSED,
         shapes=_nt((3,), STREAM_GRIDS) + ((1, 65, 97),), **_kw)
    _add(f"{_dt}_o3_cs_r", "prefilter_cols_stream_kernel + prefilter_rows_kernel", shapes=_nt((3,), [(129, 40), (64, 63)]) + ((1, 129, 40),), **_kw)
    _add(f"{_dt}_o3_c_rs", "prefilter_cols_kernel + prefilter_rows_stream_kernel", shapes=_nt((3,), [(37, 129), (63, 64)]) + ((1, 37, 129),), **_kw)
    _add(f"{_dt}_o3_c_r", "prefilter_cols_kernel + prefilter_rows_kernel", shapes=_nt((3,), [(21, 37), (63, 63)]) + ((1, 21, 37),), **_kw)
    _add(f"{_dt}_o3_fir0_c_r", "prefilter_cols_kernel + prefilter_rows_kernel", env=FIR0, shapes=_nt((3,), [(129, 40), (21, 37)]), **_kw)
    _add(f"{_dt}_o3_fir0_c_lds", "prefilter_cols_kernel + prefilter_rows_lds_kernel", env=FIR0,
         shapes=_nt((3,), [(33, 64), (33, 65), (12, 150), (65, 97)]) + ((1, 33, 65),), **_kw)

# ------------------------------------------------------------------ orders 2, 4, 5: the generic pole lists
for _o in (2, 4, 5):
    _gen = "pack_interior_kernel + prefilter_general_kernel"
    _add(f"float32_o{_o}", _gen, order=_o, shapes=_nt((1, 3), [(21, 37)]))
    _add(f"float64_o{_o}", _gen, dtype="float64", order=_o, shapes=_nt((1, 3), [(21, 37)]), tol="f64_o2" if _o == 2 else "f64_o45")
    _add(f"f64_wind_f32_o{_o}", _gen, dtype="f64_wind_f32", order=_o, ext=False, shapes=_nt((1, 3), [(21, 37)]),
         tol="f64_o2" if _o == 2 else "f64_o45")

# Grids beyond the 65535-block cap of grid.y / grid.z, where the kernels loop over what is beyond (float32, checked like a route):
#   3 x 65540 x 4: 65543 padded rows -- order 1 with lin + ext: the row loop of pack_fused_kernel; order 3 (nx < 16: the sweeps):
#   the row loop of pads_ext_kernel.  65600 x 4 x 4 at order 2 without ext: the level loop of pads_only_kernel (a 26 MB image).
CAPPED = {
    "capped_rows_o1": dict(name="pack_fused_kernel", dtype="float32", order=1, env={}, ext=True, lin=True, shapes=((3, 65540, 4),), tol="exact"),
    "capped_rows_o3": dict(name="prefilter_cols_kernel + prefilter_rows_kernel", dtype="float32", order=3, env={}, ext=True, lin=True,
                           shapes=((3, 65540, 4),), tol="f32_store"),
    "capped_levels_o2": dict(name="pack_interior_kernel + prefilter_general_kernel", dtype="float32", order=2, env={}, ext=False, lin=True,
                             shapes=((65600, 4, 4),), tol="f32_store"),
}
GRID_CAP = 65535

# lc_field_extrapolate (extrapolate_kernel: 8192 blocks of 256 threads, grid-stride): small, and large enough that the loop iterates
EXTRAPOLATE_SHAPES = ((3, 9, 11), (11, 300, 400))
EXTRAPOLATE_GRID = 8192 * 256
