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
