"""The route table (tests/kernel_routes.py) against the dispatchers' kernel-name literals.  No GPU, no build.

Every advect / sigma launch site reports the kernel it launched as a string literal (``return "name";``,
``ctx->last_sigma_kernel = "name"``), which advect.hip's launch macros put together from the tokens that instantiate the
kernel (``#FAMILY "<" ... ">"``): a literal exists once the preprocessor has run.  So the sources are read after
``hipcc --cuda-host-only -E -P`` with adjacent literals joined, as the compiler joins them.  The set of those literals must
equal ``ROUTES`` plus ``UNREACHABLE``: a new instance without a route fails here, and so does a route whose kernel is gone."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import kernel_routes as KR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lagrangiancoherence_amd", "csrc")
SOURCES = ("advect.hip", "sigma.hip")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not found")

# a quoted kernel name as the dispatch macros and returns spell it: family, optional template arguments
NAME_RE = re.compile(r'"((?:advect|outer_substep|tracer|sigma)\w*(?:<[^"<>]*>)?)"')


def kernel_names(text):
    """The kernel-name literals of one source text, code only (comments dropped), adjacent literals joined."""
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    code = re.sub(r"//[^\n]*", "", code)
    code = re.sub(r'"\s+"', "", code)        # "a" "b" is "ab" (no name literal holds an escaped quote)
    return set(NAME_RE.findall(code))


def preprocessed(path, *flags):
    """A source file as the host compiler sees it after macro expansion (no line markers)."""
    r = subprocess.run([HIPCC, "--cuda-host-only", "-E", "-P", "-std=c++17", *flags, path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


_DISPATCHED = []


def dispatched_names():
    if not _DISPATCHED:
        _DISPATCHED.append(set().union(*(kernel_names(preprocessed(os.path.join(CSRC, f))) for f in SOURCES)))
    return set(_DISPATCHED[0])


def check_complete(names, routes, unreachable):
    """Raises AssertionError naming every literal without an entry and every entry without a literal."""
    both = set(routes) & set(unreachable)
    assert not both, f"in both ROUTES and UNREACHABLE: {sorted(both)}"
    listed = set(routes) | set(unreachable)
    missing, extra = sorted(names - listed), sorted(listed - names)
    assert not missing and not extra, f"kernel names without a route: {missing}; routes without a kernel name: {extra}"


def test_extractor_sees_the_dispatch_forms():
    snippet = '''
        if (A.K == 4) return launch_kernel(advect_lds2_kernel<4, false, PATCH_LINES>, g2, st, A, "advect_lds2_kernel<4, false, 2>");
        return launch_kernel(advect_lds_kernel<ORDER, -1, false, true>, g1, st, A, ORDER == 3 ? "advect_lds_kernel<3, -1, false, lines>" : "advect_lds_kernel<1, -1, false, lines>");
            return "advect_lds64_o3_kernel<4, true, cub>";
        ctx->last_advect_kernel = "outer_substep_kernel";
        ctx->last_sigma_kernel = fd_fp32_cast ? "sigma_kernel<double, float>" : "sigma_kernel<double, double>";
        return launch_kernel(advect_lds2_kernel<7, true, PATCH_TALL>, g2, st, A, "advect_lds2_kernel<7, true, 0>");   // "advect_in_a_comment<1>"
        lc_set_error("lc_advect: bad dtype %d", dtype);
        {4, true, advect_lds64_kernel<4, true, 2>, "advect_lds64_kernel" "<" "4, true, 2" ">"},
        {-1, false, advect_lds_kernel<ORDER, -1, false, false, true>, ORDER == 3 ? "advect_lds_kernel<3, " "-1" ", " "false" ", verify" ">" : "advect_lds_kernel<1, " "-1" ", "
             "false" ", verify" ">"}
        name = sizeof(T) == 8 ? "tracer_kernel<double, " "5" ">" : "tracer_kernel<float, " "5" ">";
    '''
    assert kernel_names(snippet) == {
        "advect_lds2_kernel<4, false, 2>", "advect_lds_kernel<3, -1, false, lines>", "advect_lds_kernel<1, -1, false, lines>",
        "advect_lds64_o3_kernel<4, true, cub>", "outer_substep_kernel", "sigma_kernel<double, float>",
        "sigma_kernel<double, double>", "advect_lds2_kernel<7, true, 0>", "advect_lds64_kernel<4, true, 2>",
        "advect_lds_kernel<3, -1, false, verify>", "advect_lds_kernel<1, -1, false, verify>", "tracer_kernel<double, 5>",
        "tracer_kernel<float, 5>"}


def test_the_preprocessor_makes_the_names_the_extractor_reads(tmp_path):
    """The macros' own spelling through the real preprocessor: stringified tokens, with and without trailing arguments."""
    src = tmp_path / "names.hip"
    src.write_text('''
        #define LC_STR(...) #__VA_ARGS__
        #define LC_INSTANCE(KF, CYC, FAMILY, ...) {KF, CYC, FAMILY<KF, CYC, ##__VA_ARGS__>, #FAMILY "<" LC_STR(KF, CYC, ##__VA_ARGS__) ">"}
        #define LC_K4(INSTANCE, ...) INSTANCE(4, true, __VA_ARGS__), INSTANCE(-1, false, __VA_ARGS__)
        x = {LC_K4(LC_INSTANCE, advect_fake_kernel, 2 /* PATCH_LINES */), LC_K4(LC_INSTANCE, advect_bare_kernel)};
    ''')
    assert kernel_names(preprocessed(str(src), "-nogpuinc", "-nogpulib")) == {
        "advect_fake_kernel<4, true, 2>", "advect_fake_kernel<-1, false, 2>", "advect_bare_kernel<4, true>", "advect_bare_kernel<-1, false>"}


def test_a_new_launch_site_or_a_stale_route_is_caught():
    names = dispatched_names()
    added = names | kernel_names('LC_LDS2(7, true, PATCH_TALL, "advect_lds2_kernel<7, true, 0>")  "advect_fake<1>"')
    with pytest.raises(AssertionError, match=r"advect_fake<1>.*advect_lds2_kernel<7, true, 0>|advect_lds2_kernel<7, true, 0>.*advect_fake<1>"):
        check_complete(added, KR.ROUTES, KR.UNREACHABLE)
    dropped = dict(KR.ROUTES)
    dropped.pop("advect_lds64_kernel<-1, false, 2>")
    with pytest.raises(AssertionError, match=re.escape("advect_lds64_kernel<-1, false, 2>")):
        check_complete(names, dropped, KR.UNREACHABLE)


def test_every_dispatched_name_has_exactly_one_route():
    names = dispatched_names()
    assert len([n for n in names if not n.startswith("sigma")]) >= 124 and len([n for n in names if n.startswith("sigma")]) >= 9
    check_complete(names, KR.ROUTES, KR.UNREACHABLE)
    for name, why in KR.UNREACHABLE.items():
        assert isinstance(why, str) and why.strip(), name


def test_every_knob_a_route_names_exists():
    from lagrangiancoherence_amd.engine import Engine
    with open(os.path.join(CSRC, "api.hip")) as fh:
        api = fh.read()
    with open(os.path.join(ROOT, "include", "lcs_hip.h")) as fh:
        header = fh.read()
    for knob in KR.ENV_KNOBS:
        assert f'getenv("{knob}")' in api, knob
    for s in KR.SETTERS:
        assert callable(getattr(Engine, s, None)), s
        assert f"lc_ctx_{s}(" in api, s
    for c, sym in KR.CALLS.items():
        assert callable(getattr(Engine, sym, None)) or f"{sym}(" in header, (c, sym)
    import inspect
    prep = inspect.signature(Engine.prepare_field).parameters
    for name, r in KR.ROUTES.items():
        assert r["call"] in KR.CALLS, name
        assert set(r["setters"]) <= set(KR.SETTERS), name
        assert set(r["env"]) <= set(KR.ENV_KNOBS), name
        assert r["dtype"] in ("float32", "float64", "f64_wind_f32"), name
        if name.startswith("sigma"):
            assert set(r["widths"]) and all(w >= 5 for w in r["widths"]), name
            continue
        assert set(r["prepare"]) <= set(KR.PREPARE_KW) and set(KR.PREPARE_KW) <= set(prep), name
        assert r["xmode"] in ("cyclic", "pointwise", "reference_outer"), name
        assert r["order"] in (1, 2, 3, 4, 5) and r["Ks"] and all(k >= 0 for k in r["Ks"]), name
        assert r["tol"] in ("exact64", "fast64", "band32", "tracer"), name
        assert set(r["name_on"]) <= set(KR.GRIDS) - {"m180"}, name
        for g, other in r["name_on"].items():       # a grid's own kernel is itself a route, of the same dtype and order
            o = KR.ROUTES[other]
            assert other != name and (o["dtype"], o["order"], o["xmode"]) == (r["dtype"], r["order"], r["xmode"]), (name, g)
            assert not o["name_on"] and "lds" not in other, (name, g)
        if r["sibling"] is not None:
            s = KR.ROUTES[r["sibling"]]
            assert s["sibling"] is None and s["order"] == r["order"] and "lds" not in r["sibling"], name
        # the generic-K instances are run at K = 1, 2 and 3 at least
        if re.search(r"<(\d, )?-1,", name) and name.startswith("advect_") and "lds2_kernel<-1, true, 0>" not in name:
            assert {1, 2, 3} <= set(r["Ks"]), name


def test_route_inputs_meet_the_edges():
    ny, nx = KR.SEEDS
    for tile in (8, 16, 32, 64):
        assert ny % tile and nx % tile
    assert nx % 4 == 0 and nx >= 32            # whole-line stores stay possible (PATCH_LINES, lines instances)
    assert KR.NSTEPS > 2 * KR.LEVEL_CHUNK      # at least three level chunks
    assert min(KR.TIMESTEPS) < 0 < max(KR.TIMESTEPS)


def test_grids_and_their_settls_orders():
    assert list(KR.GRIDS) == ["m180", "e0", "seam_inside"] and KR.GRIDS["m180"] == 0.0
    assert KR.GRIDS["e0"] == 180.0 and KR.GRIDS["seam_inside"] == 97.5
    cell = 360.0 / KR.FLOW["nx"]
    assert (KR.GRIDS["seam_inside"] / cell) % 1 == 0.5         # +-180 half way between two nodes, lon_min off the cell grid
    for name, r in KR.ROUTES.items():
        if name.startswith("sigma"):
            continue
        assert KR.grid_ks(r, "m180") == tuple(r["Ks"]), name
        for g in ("e0", "seam_inside"):
            assert KR.grid_ks(r, g) == tuple(sorted({min(r["Ks"]), max(r["Ks"])})), name
        assert KR.name_on(r, "m180") == name
    # the float32 LDS-tile kernels defer the longitude wrap inside a level: every cyclic route of theirs is re-routed
    lds32 = [n for n, r in KR.ROUTES.items() if n.startswith(("advect_lds_kernel<", "advect_lds2_")) and r["xmode"] == "cyclic"]
    assert lds32 and all(set(KR.ROUTES[n]["name_on"]) == {"e0", "seam_inside"} for n in lds32)
    assert all(not r.get("name_on") for n, r in KR.ROUTES.items() if n not in lds32)


SEAM_CASES = [(g, o, dt) for g in ("e0", "seam_inside") for o in (1, 3) for dt in KR.TIMESTEPS]


@pytest.mark.parametrize("grid,order,dt", SEAM_CASES)
def test_added_grids_put_the_wrap_inside_the_field(grid, order, dt):
    """Oracle-only conditions of the added longitude grids (K = 4): parcels cross +-180 in numbers, the float64 oracle is
    well conditioned there, few seeds come near the seam, the float32 oracle stays close to the float64 one."""
    from oracle import lcs_oracle as O
    from tests import _seam as S
    K = 4
    u, v, lat, lon, slat, slon = S.inputs("float64", grid)
    assert lon[0] == -180.0 + KR.GRIDS[grid] and lon[0] < 180.0 < lon[-1]
    kw = dict(timestep=dt, SETTLS_order=K, interp_order=order, cyclic_xboundary=True, return_traj=True, t0=KR.T0, nsteps=KR.NSTEPS)
    x64, y64 = O.parcel_propagation(u, v, lat, lon, seed_lat=slat, seed_lon=slon, **kw)
    # the restatement the near-seam distances come from IS the oracle
    tx, ty, seam = S.restated("float64", order, K, dt, KR.T0, grid)
    assert np.array_equal(tx, x64) and np.array_equal(ty, y64)
    n = x64[0].size
    share = S.crossed(x64).sum() / n
    assert share >= 0.20, f"{share:.1%} of the seeds cross +-180"
    # conditioning: the seeds shifted by 1e-12 degrees
    xs, ys = O.parcel_propagation(u, v, lat, lon, seed_lat=slat + 1e-12, seed_lon=slon + 1e-12, **kw)
    moved = max(np.minimum(np.abs(xs[-1] - x64[-1]), np.abs(np.abs(xs[-1] - x64[-1]) - 360.0)).max(), np.abs(ys[-1] - y64[-1]).max())
    assert moved <= 1e-11, f"the float64 oracle moves by {moved:.2e} degrees"
    # the near-seam seeds a float32 comparison leaves out (float32 inputs, float64 arithmetic): at most 1 %
    for k in (0, K):
        left_out = int(S.near_seam("float32", order, k, dt, KR.T0, grid).sum())
        assert left_out <= n // 100, f"K={k}: {left_out} seeds within {S.NEAR_SEAM} degrees of +-180"
    # the float32 oracle against the float64 answer on the float32 inputs
    a32 = S.inputs("float32", grid)
    a64 = tuple(q.astype(np.float64) for q in a32)
    r32 = O.parcel_propagation(*a32[:4], seed_lat=a32[4], seed_lon=a32[5], **kw)
    r64 = O.parcel_propagation(*a64[:4], seed_lat=a64[4], seed_lon=a64[5], **kw)
    dx = np.abs(r32[0][-1].astype(np.float64) - r64[0][-1])
    err = np.maximum(np.minimum(dx, np.abs(dx - 360.0)), np.abs(r32[1][-1].astype(np.float64) - r64[1][-1]))
    assert (err > 0.1).sum() <= 1 and (err > 0.5).sum() == 0, (int((err > 0.1).sum()), float(err.max()))


@pytest.mark.parametrize("order", (1, 3))
@pytest.mark.parametrize("K", (1, 4))
def test_the_added_grids_can_tell_a_deferred_wrap(order, K):
    """The mutant (tests/_seam.py: the in-level wrap left to the next sample's window test) equals the oracle bit for bit
    on the flow's own longitudes and differs by more than 1e-3 degrees on at least 20 % of the seeds of either added grid:
    the existing assertions separate the two once the inputs do."""
    from tests import _seam as S
    from tests._fullsize import lon_err
    for dt in KR.TIMESTEPS:
        tx, ty, _ = S.restated("float64", order, K, dt, KR.T0, "m180")
        mx, my, _ = S.restated("float64", order, K, dt, KR.T0, "m180", defer=True)
        assert np.array_equal(tx, mx) and np.array_equal(ty, my), (order, K, dt)
        for grid in ("e0", "seam_inside"):
            tx, ty, _ = S.restated("float64", order, K, dt, KR.T0, grid)
            mx, my, _ = S.restated("float64", order, K, dt, KR.T0, grid, defer=True)
            off = np.maximum(lon_err(mx[-1], tx[-1]), np.abs(my[-1] - ty[-1])) > 1e-3
            assert off.mean() >= 0.20, f"{grid} order {order} K={K} dt={dt:+.0f}: the mutant differs on {off.mean():.1%} of the seeds"
