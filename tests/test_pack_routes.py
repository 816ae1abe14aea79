"""The pack route table (tests/pack_routes.py) against the dispatcher in csrc/pack.hip.  No GPU, no build.

Every launch site of ``pack_impl`` reports what it launched as a string literal assigned to ``ctx->last_pack_kernel``.  The
set of those literals must equal the set of ``name`` values in the table: a new launch site without a route fails here, and
so does a route whose name is gone.  A restatement of the dispatcher's conditions (``pack_routes.dispatch``) then maps every
(route, shape) pair of the table to that route's name, so the shapes are known to reach what they claim before any GPU time
is spent on them."""
import os
import re

import numpy as np
import pytest

from tests import pack_routes as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lagrangiancoherence_amd", "csrc")


def strip_comments(text):
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", code)


def pack_names(text):
    """The string literals assigned to ctx->last_pack_kernel in one source text, code only (every literal up to the ';')."""
    names = set()
    for stmt in re.findall(r"ctx->last_pack_kernel\s*=([^;]*);", strip_comments(text)):
        names |= set(re.findall(r'"([^"]*)"', stmt))
    return names


def dispatched_names():
    with open(os.path.join(CSRC, "pack.hip")) as fh:
        return pack_names(fh.read())


def check_complete(names, routes):
    listed = {r["name"] for r in routes.values()}
    missing, extra = sorted(names - listed), sorted(listed - names)
    assert not missing and not extra, f"pack kernel names without a route: {missing}; routes without a kernel name: {extra}"


def _env(r):
    return int(r["env"].get("LCS_FIR_PREFILTER", "1")), int(r["env"].get("LCS_FUSED_PREFILTER", "1"))


def test_extractor_sees_the_assignment_forms():
    snippet = '''
        ctx->last_pack_kernel = "pack_fused_kernel";   // "a_name_in_a_comment"
        ctx->last_pack_kernel = both ? "prefilter_fir_kernel (img + ext)" : "prefilter_fir_kernel";
        /* ctx->last_pack_kernel = "commented_out_kernel"; */
        if (!fused)
            ctx->last_pack_kernel = (a && b) ? "x_kernel + y_kernel"
                                    : c      ? "x_kernel + z_kernel<double>"
                                             : "w_kernel";
        lc_set_error("lc_field_pack: bad dtype %d", dtype);
    '''
    assert pack_names(snippet) == {"pack_fused_kernel", "prefilter_fir_kernel (img + ext)", "prefilter_fir_kernel", "x_kernel + y_kernel",
                                   "x_kernel + z_kernel<double>", "w_kernel"}


def test_a_new_launch_site_or_a_stale_route_is_caught():
    names = dispatched_names()
    with pytest.raises(AssertionError, match="prefilter_new_kernel"):
        check_complete(names | pack_names('ctx->last_pack_kernel = "prefilter_new_kernel";'), PR.ROUTES)
    for rid in ("f32_o3_fir2", "float64_o3_fused"):           # the only route of its name
        dropped = dict(PR.ROUTES)
        name = dropped.pop(rid)["name"]
        assert name not in {r["name"] for r in dropped.values()}
        with pytest.raises(AssertionError, match=re.escape(name)):
            check_complete(names, dropped)


def test_every_reported_name_has_a_route_and_every_route_a_name():
    names = dispatched_names()
    assert len(names) >= 11, names
    check_complete(names, PR.ROUTES)
    # two paths that launch different kernels do not share a string: every kernel of the prefilter stage appears in a name
    with open(os.path.join(CSRC, "pack.hip")) as fh:
        code = strip_comments(fh.read())
    launched = set(re.findall(r"hipLaunchKernelGGL\(\(?(\w+)", code))
    tails = {"pads_ext_kernel", "pads_only_kernel", "extrapolate_kernel"}
    assert tails <= launched
    for k in launched - tails:
        assert any(k in n for n in names), f"{k} is launched but no reported name holds it"


def test_every_knob_a_route_names_exists():
    with open(os.path.join(CSRC, "api.hip")) as fh:
        api = fh.read()
    for knob in PR.ENV_KNOBS:
        assert f'getenv("{knob}")' in api, knob
    for rid, r in {**PR.ROUTES, **PR.CAPPED}.items():
        assert set(r["env"]) <= set(PR.ENV_KNOBS), rid
        assert r["env"].get("LCS_FIR_PREFILTER", "1") in ("0", "1", "2") and r["env"].get("LCS_FUSED_PREFILTER", "1") in ("0", "1"), rid
        assert r["dtype"] in ("float32", "float64", "f64_wind_f32") and r["order"] in (1, 2, 3, 4, 5), rid
        assert r["tol"] in PR.TOL and (r["tol"] == "exact") == (r["order"] == 1), rid
        assert r["lin"] or (r["order"] == 1 and r["ext"] and all(s[0] >= 2 for s in r["shapes"])), rid
        assert not (r["dtype"] == "f64_wind_f32" and (r["ext"] or r["order"] == 1)), rid     # lc_field_pack refuses these
        assert r["shapes"] and all(nt >= 1 and ny >= 4 and nx >= 4 for nt, ny, nx in r["shapes"]), rid
        # the tolerance class belongs to the image's dtype and order
        if r["order"] > 1:
            want = {"float32": ("f32_fir",) if "fir_kernel" in r["name"] else ("f32_store",)}.get(
                r["dtype"], ({3: "f64_o3", 2: "f64_o2"}.get(r["order"], "f64_o45"),))
            assert r["tol"] in want, rid


def test_the_dispatcher_restated_sends_every_shape_to_its_route():
    tails = set()
    for rid, r in {**PR.ROUTES, **PR.CAPPED}.items():
        fir, fused = _env(r)
        for nt, ny, nx in r["shapes"]:
            name, tail = PR.dispatch(r["dtype"], r["order"], nt, ny, nx, fir, fused, r["ext"])
            assert name == r["name"], (rid, (nt, ny, nx), name)
            tails.add(tail)
            if r["ext"] and nt >= 2 and r["order"] > 1:      # the second call of the GPU test, without ext: pads_only_kernel
                tails.add(PR.dispatch(r["dtype"], r["order"], nt, ny, nx, fir, fused, False)[1])
    assert {"pads_ext_kernel", "pads_only_kernel"} <= tails
    # every branch of the dispatcher is some route: no two routes are the same path
    paths = {}
    for rid, r in PR.ROUTES.items():
        key = (r["name"], r["dtype"], r["order"] if r["order"] != 3 else 3, tuple(sorted(r["env"].items())), r["ext"], r["lin"])
        assert key not in paths, (rid, paths[key])
        paths[key] = rid
    # the constants of the restatement are the dispatcher's
    with open(os.path.join(CSRC, "pack.hip")) as fh:
        code = strip_comments(fh.read())
    consts = dict(re.findall(r"\b(FHALO|FT|PR_CHUNK|PR_ROWS|RS_C|RS_ROWS)\s*=\s*(\d+)", code))
    assert int(consts["FHALO"]) + 2 == PR.FIR_MIN and int(consts["FT"]) == PR.FIR_TILE
    assert int(consts["PR_CHUNK"]) == PR.STREAM_MIN == 2 * int(consts["RS_C"]) and int(consts["PR_ROWS"]) == int(consts["RS_ROWS"]) == PR.FIR_TILE
    assert "ny >= FHALO + 2 && nx >= FHALO + 2" in code and "cols_stream = stream && ny >= 64" in code and "nx >= PR_CHUNK" in code
    assert re.search(r"\bconstexpr int PACK_LV = 2;", code)


def test_route_inputs_meet_the_edges():
    R = PR.ROUTES
    fir = [s for rid in ("f32_o3_fir", "f32_o3_fir2") for s in R[rid]["shapes"]]
    for rid in ("f32_o3_fir", "f32_o3_fir2"):
        s = R[rid]["shapes"]
        assert PR.FIR_MIN in {ny for _, ny, _ in s} and PR.FIR_MIN in {nx for _, _, nx in s}, rid      # the smallest legal grid
        assert {33, 34, 35} <= {ny for _, ny, _ in s}, rid         # the pads' three source rows in different tiles
        assert any(ny < PR.FIR_TILE and nx < PR.FIR_TILE for _, ny, nx in s), rid                       # less than one tile
        assert any(nx > 2 * PR.FIR_TILE for _, _, nx in s), rid    # three tiles in x, the last ragged
    assert {1, 3} <= {nt for nt, _, _ in R["f32_o3_fir"]["shapes"]} and fir
    for rid, r in R.items():
        s = r["shapes"]
        if "rows_lds" in r["name"]:                                # one chunk, one node over, a ragged third chunk
            nxs = {nx for _, _, nx in s}
            assert ({64, 65} <= nxs or rid == "f32_o3_small_wide") and any(nx > 128 and nx % 64 for nx in nxs), rid
        if "stream" in r["name"]:
            assert any(PR.STREAM_MIN in (ny, nx) for _, ny, nx in s), rid
            assert all((ny >= 64) == ("cols_stream" in r["name"] or "fused" in r["name"]) for _, ny, _ in s), rid
        if r["name"].endswith("prefilter_rows_kernel") and r["dtype"] != "float32" and "FIR" not in str(r["env"]):
            assert any(nx == PR.STREAM_MIN - 1 for _, _, nx in s), rid                                   # one node under the threshold
        assert any(nt >= 3 for nt, _, _ in s), rid
        assert any(ny % PR.FIR_TILE or nx % PR.FIR_TILE for _, ny, nx in s), rid
        if r["order"] == 1:                                        # PACK_LV = 2: below, at, one over, and an odd count of chunks
            assert {2, 3, 5} <= {nt for nt, _, _ in s} and (not r["lin"] or 1 in {nt for nt, _, _ in s}), rid
    assert {"f32_o3_sweeps_lds", "float64_o3_fir0_c_lds", "f64_wind_f32_o3_fir0_c_lds"} <= set(R)
    # too small for the FIR on either axis, and by one node
    small = R["f32_o3_small"]["shapes"]
    assert any(ny == PR.FIR_MIN - 1 for _, ny, _ in small) and any(nx == PR.FIR_MIN - 1 for _, _, nx in small)
    # the capped grids exceed the cap, the extrapolate shape the grid
    (nt, ny, nx), = PR.CAPPED["capped_rows_o1"]["shapes"]
    assert ny + 3 > PR.GRID_CAP and PR.CAPPED["capped_rows_o3"]["shapes"] == ((nt, ny, nx),) and nx < PR.FIR_MIN
    assert PR.CAPPED["capped_levels_o2"]["shapes"][0][0] > PR.GRID_CAP
    nt, ny, nx = PR.EXTRAPOLATE_SHAPES[-1]
    assert (nt - 1) * (ny + 3) * (nx + 3) * 2 > PR.EXTRAPOLATE_GRID


def test_the_batched_scipy_reference_is_spline_filter_level_by_level():
    """The GPU test filters a whole (nt, ny, nx) series with spline_filter1d along axes 1 and 2: the calls
    scipy.ndimage.spline_filter makes for one level, so the same bits."""
    from scipy.ndimage import spline_filter, spline_filter1d
    F = 20.0 * np.random.default_rng(5).standard_normal((3, 21, 37))
    for order in (2, 3, 4, 5):
        got = spline_filter1d(spline_filter1d(F, order, axis=1, mode="mirror"), order, axis=2, mode="mirror")
        for t in range(3):
            assert np.array_equal(got[t], spline_filter(F[t], order=order, mode="mirror"))


def test_the_f32_store_bound_is_a_few_ulps_of_the_coefficients():
    ref = np.linspace(-30.0, 30.0, 1001)
    ulp = float(np.spacing(np.float32(30.0)))
    b = PR.f32_store_bound(ref, 3)
    assert 2 * ulp < b <= 4 * ulp and PR.f32_store_bound(ref, 5) - b == pytest.approx(2 * ulp)
