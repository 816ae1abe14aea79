"""Route table: how each kernel name the advect and sigma dispatchers report is reached through public settings.

Plain data, imported by ``test_kernel_routes.py`` (completeness, no GPU) and ``test_kernel_routes_gpu.py`` (forces every
route on the GPU and compares it with the float64 CPU oracle).  One entry per name literal in ``csrc/advect.hip`` and
``csrc/sigma.hip``; a name no public setting reaches goes in ``UNREACHABLE`` with the reason read off the dispatcher.

An advect-side entry is a dict:

- ``call``: ``advect`` (Engine.advect), ``batch`` (Engine.advect_batch), ``abi_batch`` (lc_advect_ex with
  ``n_members > 1`` and ``LC_X_CLAMP_POINT``: the C ABI's ensemble form, which Engine.advect_batch does not offer),
  ``series`` (Engine.lcs_series), ``tracer`` (Engine.advect_tracer);
- ``dtype``: ``float32``, ``float64`` or ``f64_wind_f32`` (float32 wind on float64 coordinates);
- ``order`` (interp_order), ``Ks`` (the SETTLS orders run: the generic-K instances take 1, 2 and 3, more where the
  dispatcher sends other K there too), ``xmode`` (``cyclic``, ``pointwise`` or ``reference_outer``);
- ``prepare``: keyword arguments of Engine.prepare_field (``fuse_levels``, ``lin_image``, ``ext_image``);
- ``traj`` (return_traj), ``members`` (ensemble members / series windows);
- ``setters``: Engine setters applied before the call (``set_lds_tiles``, ``set_verify``, ``set_level_chunk``,
  ``set_sigma_march``, ``set_f64_fidelity``); ``env``: variables read once at context creation;
- ``sibling``: the direct-gather route of the same dtype, order, K and boundary whose bits this one must equal
  (every kernel family of one dtype is bit-identical to the others), or None;
- ``name_on``: ``{grid: kernel name}`` for the longitude grids of ``GRIDS`` on which the dispatcher sends the route's
  settings to another kernel than on ``m180`` (itself a route of this table); empty for most;
- ``tol``: ``exact64`` (numpy / scipy operation order: <= 1e-12 degrees), ``fast64`` (fused-level form: <= 1e-10 degrees),
  ``band32`` (inside the float32 oracle's own band: median, p99 and max).

Shared inputs (``FLOW``, ``SEEDS``, ``T0``, ``NSTEPS``, ``TIMESTEPS``, ``LEVEL_CHUNK``): ``flows.era5_like`` at 5 degrees,
a 45 x 76 seed grid spanning the field (ragged against every tile shape, the global first and last rows included, so
the pole-row rule runs), 10 steps from level 1 in level chunks of 4, both signs of the time step.  Parcels cross +-180
in cyclic routes and leave the box in the others.

Longitude grids (``GRIDS``): offsets added to the flow's longitudes, the wind arrays unchanged (the flow is periodic), the
seeds spanning the shifted coordinates.  The reference wraps at a hard-coded +-180 whatever the field's longitudes are (Q7),
so on ``e0`` and ``seam_inside`` the wrap happens in the field's interior and the next sample reaches scipy's ``wrap`` map
with an index a period below zero; the non-cyclic routes see ``lon_min != -180`` in the index transform and the clamp
bounds.  Every advect-side route runs on all three; on the two added grids at the smallest and largest of its ``Ks``.
"""

FLOW = dict(nt=14, ny=36, nx=72, dt_seconds=3600.0, scale=1.0)   # flows.era5_like; u, v times `scale`
SEEDS = (45, 76)            # not a multiple of any tile edge (8, 16, 32, 64); 76 % 4 == 0 keeps whole-line stores possible
T0, NSTEPS = 1, 10
TIMESTEPS = (-1800.0, 1800.0)
LEVEL_CHUNK = 4             # 10 steps = three launches wherever a route takes chunks
MEMBERS = 3                 # ensembles / series windows, t0 stride 1
GRIDS = {"m180": 0.0,            # -180 ... 175: the flow's own longitudes
         "e0": 180.0,            # 0 ... 355: ERA5's convention, the +-180 meridian on a node in the middle of the field
         "seam_inside": 97.5}    # -82.5 ... 272.5: the meridian off any node, lon_min no multiple of the cell

TOL = {"exact64": 1e-12, "fast64": 1e-10, "sigma64": 1e-7, "sigma64_nocast": 1e-9}

ROUTES = {}
UNREACHABLE = {}


def _xmode(cyc):
    return "cyclic" if cyc else "pointwise"


def _add(name, **kw):
    assert name not in ROUTES, name
    r = dict(call="advect", dtype="float32", order=1, Ks=(4,), xmode="cyclic", prepare={}, traj=False, members=1,
             setters={}, env={}, sibling=None, tol="band32", name_on={})
    r.update(kw)
    r["name"] = name
    ROUTES[name] = r


def _kf_ks(kf, generic=(1, 2, 3)):
    return (4,) if kf == 4 else ((0,) if kf == 0 else (generic if kf == -1 else (kf,)))


# ------------------------------------------------------------------ float32: direct gathers
_add("advect_kernel_f32<1>", Ks=(0, 4), setters={"set_lds_tiles": 0})
_add("advect_kernel_f32_wide<3>", order=3, Ks=(0, 4), setters={"set_lds_tiles": 0})
for _o in (2, 4, 5):
    _add(f"advect_kernel_f32_wide<{_o}>", order=_o, Ks=(0, 2), xmode="cyclic")
    # (orders 2, 4, 5: the generic kernel whatever the LDS setting)

# bit-identity with the direct-gather kernel holds for float32 order 1 only: the order-3 LDS-tile kernels (one and two
# seeds per lane) differ from advect_kernel_f32_wide<3> in the last bits (measured on every order-3 route here, each
# inside the float32 oracle's band); no document or test states it for them, so they have no sibling
_DIRECT32 = {1: "advect_kernel_f32<1>", 3: None}

# ------------------------------------------------------------------ float32, one seed per lane (lc_ctx_set_lds_tiles 2)
for _o in (1, 3):
    for _kf in (4, -1):
        for _cyc in (True, False):
            # order 3 also sends SETTLS_order 0 to the run-time-K instance (order 1 at K = 0 takes the direct kernel)
            _ks = _kf_ks(_kf, (0, 1, 2, 3) if _o == 3 else (1, 2, 3))
            _c = "true" if _cyc else "false"
            base = dict(order=_o, Ks=_ks, xmode=_xmode(_cyc), sibling=_DIRECT32[_o])
            _add(f"advect_lds_kernel<{_o}, {_kf}, {_c}>", setters={"set_lds_tiles": 2}, **base)
            _add(f"advect_lds_kernel<{_o}, {_kf}, {_c}, lines>", setters={"set_lds_tiles": 2}, traj=True, **base)
            _add(f"advect_lds_kernel<{_o}, {_kf}, {_c}, verify>", setters={"set_lds_tiles": 2, "set_verify": 1}, **base)

# ------------------------------------------------------------------ float32, two seeds per lane (lc_ctx_set_lds_tiles 1)
# patch modes (LCS_PATCH_MODE): 0 tall, 1 wide, 2 lines, 3 member pairs (ensembles)
for _cyc in (True, False):
    _c = "true" if _cyc else "false"
    for _md in (1, 2):
        for _kf in (4, -1):
            _add(f"advect_lds2_kernel<{_kf}, {_c}, {_md}>", Ks=_kf_ks(_kf, (0, 1, 2, 3)), xmode=_xmode(_cyc),
                 setters={"set_lds_tiles": 1}, env={"LCS_PATCH_MODE": str(_md)}, traj=_md == 2, sibling=_DIRECT32[1])
            _add(f"advect_lds2_o3_kernel<{_kf}, {_c}, {_md}>", order=3, Ks=_kf_ks(_kf, (0, 1, 2, 3)), xmode=_xmode(_cyc),
                 setters={"set_lds_tiles": 1}, env={"LCS_PATCH_MODE": str(_md)}, traj=_md == 2, sibling=_DIRECT32[3])
    for _kf in (0, 4):
        _add(f"advect_lds2_kernel<{_kf}, {_c}, 0>", Ks=_kf_ks(_kf), xmode=_xmode(_cyc), setters={"set_lds_tiles": 1},
             sibling=_DIRECT32[1])
        _add(f"advect_lds2_o3_kernel<{_kf}, {_c}, 0>", order=3, Ks=_kf_ks(_kf), xmode=_xmode(_cyc),
             setters={"set_lds_tiles": 1}, sibling=_DIRECT32[3])
    _add(f"advect_lds2_o3_kernel<-1, {_c}, 0>", order=3, Ks=(1, 2, 3), xmode=_xmode(_cyc), setters={"set_lds_tiles": 1},
         sibling=_DIRECT32[3])
    # member pairs: an ensemble of order 1 with K > 0 and no trajectories
    _add(f"advect_lds2_kernel<4, {_c}, 3>", call="batch" if _cyc else "abi_batch", Ks=(4,), xmode=_xmode(_cyc),
         members=MEMBERS, setters={"set_lds_tiles": 1}, sibling=_DIRECT32[1])
    _add(f"advect_lds2_kernel<-1, {_c}, 3>", call="batch" if _cyc else "abi_batch", Ks=(1, 2, 3), xmode=_xmode(_cyc),
         members=MEMBERS, setters={"set_lds_tiles": 1}, sibling=_DIRECT32[1])
for _k in (1, 2, 3):   # compiled for SETTLS_order 1, 2, 3 (cyclic only)
    _add(f"advect_lds2_kernel<{_k}, true, 0>", Ks=(_k,), setters={"set_lds_tiles": 1}, sibling=_DIRECT32[1])
# the run-time-K tall instances: cyclic takes only SETTLS orders above 4 (0..4 have their own instances)
_add("advect_lds2_kernel<-1, true, 0>", Ks=(5, 6), setters={"set_lds_tiles": 1}, sibling=_DIRECT32[1])
_add("advect_lds2_kernel<-1, false, 0>", Ks=(1, 2, 3), xmode="pointwise", setters={"set_lds_tiles": 1}, sibling=_DIRECT32[1])

# The float32 LDS-tile kernels wrap the longitude once per time level and rely on the next sample's window test in between,
# which holds only on longitudes that start at -180: a cyclic float32 call on a grid with the +-180
# meridian inside takes the direct-gather kernel of its order, whatever lc_ctx_set_lds_tiles says.
_DIRECT32_NAME = {1: "advect_kernel_f32<1>", 3: "advect_kernel_f32_wide<3>"}
for _r in ROUTES.values():
    if _r["xmode"] == "cyclic" and _r["name"].startswith(("advect_lds_kernel<", "advect_lds2_kernel<", "advect_lds2_o3_kernel<")):
        _r["name_on"] = {_g: _DIRECT32_NAME[_r["order"]] for _g in ("e0", "seam_inside")}

# ------------------------------------------------------------------ float64, direct gathers
_add("advect_kernel<double, 1, false, 0>", dtype="float64", Ks=(0, 4), prepare={"fuse_levels": False, "lin_image": True},
     tol="exact64")
_add("advect_kernel<double, 1, false, 1>", dtype="float64", Ks=(0, 4), prepare={"fuse_levels": False}, tol="exact64")
_add("advect_kernel<double, 1, true, 0>", dtype="float64", Ks=(0, 4), prepare={"lin_image": True},
     setters={"set_lds_tiles": 0}, tol="fast64")
_add("advect_kernel<double, 1, true, 1>", dtype="float64", Ks=(0, 4), setters={"set_lds_tiles": 0}, tol="fast64")
_add("advect_kernel<double, 1, true, 2>", dtype="float64", Ks=(0, 4), prepare={"ext_image": False},
     setters={"set_lds_tiles": 0}, tol="fast64")
for _o in (2, 4, 5):
    _add(f"advect_kernel<double, {_o}, false, 0>", dtype="float64", order=_o, Ks=(0, 2), tol="exact64")
_add("advect_kernel<double, 3, false, 0>", dtype="float64", order=3, Ks=(0, 4), prepare={"fuse_levels": False},
     tol="exact64")
_add("advect_kernel<double, 3, true, 0>", dtype="float64", order=3, Ks=(0, 4), setters={"set_lds_tiles": 0},
     tol="fast64")

# ------------------------------------------------------------------ float64, order 1, fused levels: per-wave / per-workgroup tiles
# source (last template argument): 0 lin + ext images, 1 raw planes for the Euler sample + ext image, 2 raw planes only
_SR_PREP = {0: {"lin_image": True}, 1: {}, 2: {"ext_image": False}}
for _sr in (0, 1, 2):
    _sib = f"advect_kernel<double, 1, true, {_sr}>"
    for _cyc in (True, False):
        _c = "true" if _cyc else "false"
        for _kf in (4, -1):
            _add(f"advect_lds64_kernel<{_kf}, {_c}, {_sr}>", dtype="float64", Ks=_kf_ks(_kf), xmode=_xmode(_cyc),
                 prepare=_SR_PREP[_sr], sibling=_sib, tol="fast64")
        # LCS_F64_WG_TILE=1: no K = 4 non-cyclic instance; SETTLS_order 4 goes to the run-time-K one
        for _kf in ((4, -1) if _cyc else (-1,)):
            _add(f"advect_wg64_kernel<{_kf}, {_c}, {_sr}>", dtype="float64", Ks=_kf_ks(_kf, (1, 2, 3) if _cyc else (1, 2, 3, 4)),
                 xmode=_xmode(_cyc), prepare=_SR_PREP[_sr], env={"LCS_F64_WG_TILE": "1"}, sibling=_sib, tol="fast64")

# ------------------------------------------------------------------ float64, order 3, fused levels
for _cyc in (True, False):
    _c = "true" if _cyc else "false"
    for _kf in (4, -1):
        for _cub in (False, True):
            _add(f"advect_lds64_o3_kernel<{_kf}, {_c}{', cub' if _cub else ''}>", dtype="float64", order=3,
                 Ks=_kf_ks(_kf, (0, 1, 2, 3)), xmode=_xmode(_cyc), prepare={"ext_image": False} if _cub else {},
                 sibling="advect_kernel<double, 3, true, 0>", tol="fast64")

# ------------------------------------------------------------------ float32 wind on float64 coordinates (numpy's promotion)
_add("advect_w32_kernel", dtype="f64_wind_f32", Ks=(0, 4), setters={"set_lds_tiles": 0}, tol="exact64")
for _cyc in (True, False):
    _c = "true" if _cyc else "false"
    for _kf in (4, -1):
        _add(f"advect_lds64w_kernel<{_kf}, {_c}>", dtype="f64_wind_f32", Ks=_kf_ks(_kf), xmode=_xmode(_cyc),
             sibling="advect_w32_kernel", tol="exact64")
        _add(f"advect_lds64w_o3_kernel<{_kf}, {_c}>", dtype="f64_wind_f32", order=3, Ks=_kf_ks(_kf, (0, 1, 2, 3)),
             xmode=_xmode(_cyc), sibling="advect_kernel<double, 3, false, 0>", tol="exact64")

# ------------------------------------------------------------------ the reference's outer-product clamp (parcels leave the box)
_add("outer_substep_kernel", dtype="float64", Ks=(0, 2), xmode="reference_outer", prepare={"fuse_levels": False},
     tol="exact64")
_add("outer_substep_batch_kernel", call="series", dtype="float64", Ks=(0, 2), xmode="reference_outer",
     prepare={"fuse_levels": False}, members=MEMBERS, tol="exact64")

# ------------------------------------------------------------------ tracers
for _dt, _t in (("float32", "float"), ("float64", "double")):
    for _o in (1, 2, 3, 4, 5):
        _add(f"tracer_kernel<{_t}, {_o}>", call="tracer", dtype=_dt, order=_o, Ks=(0, 4) if _o in (1, 3) else (2,),
             prepare={"fuse_levels": False} if _dt == "float64" else {}, tol="tracer")

# ------------------------------------------------------------------ sigma (lc_sigma, lc_sigma_batch, lc_flowmap_gradient)
# call: sigma (Engine.sigma), batch (Engine.sigma_batch), tensor (Engine.flowmap_gradient)
SIGMA_WIDTHS = (5, 63, 64, 65, 1440)
SIGMA_ROWS = (5, 6)


def _sig(name, **kw):
    r = dict(call="sigma", dtype="float32", fd_fp32_cast=True, setters={}, env={}, widths=SIGMA_WIDTHS)
    r.update(kw)
    r["name"] = name
    r["tol"] = ("sigma64" if r["fd_fp32_cast"] else "sigma64_nocast") if r["dtype"] == "float64" else "band32"
    assert name not in ROUTES, name
    ROUTES[name] = r


_sig("sigma_kernel_f32", setters={"set_sigma_march": 0})
_sig("sigma_march_kernel_f32", setters={"set_sigma_march": 1}, widths=(64, 1440))     # even widths only (two columns per lane)
_sig("sigma_kernel<float, float>", call="tensor")
_sig("sigma_kernel<double, float>", dtype="float64")
_sig("sigma_kernel<double, double>", dtype="float64", fd_fp32_cast=False)
_sig("sigma_batch_kernel_f32", call="batch", setters={"set_sigma_march": 0})
_sig("sigma_march_batch_kernel_f32", call="batch", setters={"set_sigma_march": 1}, widths=(64, 1440))
_sig("sigma_batch_kernel<double, float>", call="batch", dtype="float64")
_sig("sigma_batch_kernel<double, double>", call="batch", dtype="float64", fd_fp32_cast=False)


def grid_ks(route, grid):
    """The SETTLS orders a route runs on a grid: all of them on ``m180``, the smallest and the largest on the others."""
    ks = route["Ks"]
    return tuple(ks) if grid == "m180" else tuple(sorted({min(ks), max(ks)}))


def name_on(route, grid):
    """The kernel name the dispatcher must report for a route's settings on a grid."""
    return route["name_on"].get(grid, route["name"])


# the knobs a route may name, and where each lives
SETTERS = ("set_lds_tiles", "set_verify", "set_level_chunk", "set_sigma_march", "set_f64_fidelity")
ENV_KNOBS = ("LCS_PATCH_MODE", "LCS_F64_WG_TILE", "LCS_LDS_TILES", "LCS_TILE_ORDER", "LCS_POLE_BLOCKS", "LCS_XCD_SPLIT")
PREPARE_KW = ("fuse_levels", "lin_image", "ext_image")
CALLS = {"advect": "advect", "batch": "advect_batch", "series": "lcs_series", "tracer": "advect_tracer",
         "sigma": "sigma", "tensor": "flowmap_gradient", "abi_batch": "lc_advect_ex"}
