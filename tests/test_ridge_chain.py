"""The ridge-chain case tables (tests/ridge_chain.py) against the sources and against their own promises.  No GPU, no build.

Completeness: the ``__global__`` kernels of ``csrc/api.hip`` and ``csrc/ridges.hip``, plus ``index_derivative_kernel`` of
``csrc/sigma.hip``, are exactly ``KERNELS``, and each is launched by the entry point the table names.  The cases: the edges
the tables promise (folds beyond ``2 n``, an axis of one node, radius 0, the rounding at a half, ``GAUSS_MAX_RADIUS`` and one
above, element counts past each launcher's grid cap) are asserted from the tables with the constants read out of the
sources.  The references: the closed form of dgeev equals ``numpy.linalg.eig`` on the special rows, every ``dgeev`` branch is
taken often at the sizes the GPU sees, and no case leaves more than 0.1 % of its points in the borderline window where the
GPU test does not compare masks.  A host restatement of ``gauss_kernel`` meets scipy inside the GPU test's bound on every
case, and stops doing so on the many-fold and one-node cases once ``reflect_index`` folds only once."""
import functools
import os
import re

import numpy as np
import pytest

from oracle import ridges_oracle as RO
from tests import ridge_chain as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lagrangiancoherence_amd", "csrc")


def strip_comments(text):
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", code)


@functools.lru_cache(maxsize=None)
def source(name):
    with open(os.path.join(CSRC, name)) as fh:
        return strip_comments(fh.read())


def global_kernels(code):
    """Names of the __global__ functions of one source text (comments already stripped)."""
    return set(re.findall(r"__global__\s+void\s+(?:__launch_bounds__\([^)]*\)\s*)?(?:__attribute__\(\(.*?\)\)\s*)?(\w+)\s*\(", code))


def body_of(code, name):
    """The braces-balanced body of the function `name` defined in `code` (the first definition, not a call)."""
    for m in re.finditer(r"\b%s\s*\(" % re.escape(name), code):
        depth, i = 0, m.end() - 1
        while True:                                   # the parameter list
            depth += {"(": 1, ")": -1}.get(code[i], 0)
            i += 1
            if depth == 0:
                break
        rest = code[i:].lstrip()
        if not rest.startswith("{"):
            continue                                  # a call or a declaration
        i = code.index("{", i)
        start, depth = i, 0
        while True:
            depth += {"{": 1, "}": -1}.get(code[i], 0)
            i += 1
            if depth == 0:
                return code[start:i]
    raise AssertionError(f"no definition of {name}")


def launched_by(code, entry):
    """Kernels launched with hipLaunchKernelGGL inside the extern "C" function `entry` or the *_impl it calls."""
    assert re.search(r'extern\s+"C"\s+int\s+%s\s*\(' % re.escape(entry), code), entry
    body = body_of(code, entry)
    for impl in set(re.findall(r"\b(\w+_impl)\s*<", body)) | set(re.findall(r"\b(\w+_impl)\s*\(", body)):
        body += body_of(code, impl)
    return set(re.findall(r"hipLaunchKernelGGL\(\s*\(?\s*(\w+)", body))


def chain_kernels(sources):
    names = set()
    for f in RC.WHOLE_FILES:
        names |= global_kernels(sources(f))
    for f, wanted in RC.SHARED_FILES.items():
        names |= global_kernels(sources(f)) & set(wanted)
    return names


def check_complete(names, table, sources):
    missing, extra = sorted(names - set(table)), sorted(set(table) - names)
    assert not missing and not extra, f"kernels without a table entry: {missing}; entries without a kernel: {extra}"
    for k, e in table.items():
        got = launched_by(sources(e["file"]), e["entry"])
        assert got == {k}, f"{e['entry']} launches {sorted(got)}, the table says {k}"


# ------------------------------------------------------------------ completeness
def test_the_chain_kernels_are_the_table_and_each_is_launched_by_its_entry_point():
    names = chain_kernels(source)
    assert len(names) == 3, names
    check_complete(names, RC.KERNELS, source)
    assert "index_derivative_kernel" in global_kernels(source("sigma.hip")) and len(global_kernels(source("sigma.hip"))) >= 7
    with open(os.path.join(ROOT, "lagrangiancoherence_amd", "engine.py")) as fh:
        eng = fh.read()
    for k, e in RC.KERNELS.items():
        m = re.search(r"def %s\(self.*?(?=\n    def |\Z)" % e["engine"], eng, flags=re.S)
        assert m and f"self.lib.{e['entry']}(" in m.group(0), (k, e["engine"])       # the Engine method calls that entry point
        assert getattr(RC, e["cases"]), k


def test_an_added_kernel_or_a_stale_entry_is_caught():
    def with_extra(f):
        return source(f) + ("\n__global__ void __launch_bounds__(256) hessian_fused_kernel(const double *f) {}\n" if f == "ridges.hip" else "")
    assert "hessian_fused_kernel" in global_kernels(with_extra("ridges.hip"))
    with pytest.raises(AssertionError, match="hessian_fused_kernel"):
        check_complete(chain_kernels(with_extra), RC.KERNELS, with_extra)
    stale = dict(RC.KERNELS, find_area_kernel=dict(file="ridges.hip", entry="lc_ridge_classify", engine="ridge_classify", cases="RIDGE_N"))
    with pytest.raises(AssertionError, match="find_area_kernel"):
        check_complete(chain_kernels(source), stale, source)
    wrong = dict(RC.KERNELS, ridge_kernel=dict(RC.KERNELS["ridge_kernel"], file="api.hip", entry="lc_gaussian_filter"))
    with pytest.raises(AssertionError, match="lc_gaussian_filter launches"):
        check_complete(chain_kernels(source), wrong, source)
    # the extractor: templates, launch bounds, attributes, comments
    snippet = strip_comments('''
        template <typename T, int AXIS>
        __global__ void a_kernel(const T *in) {}
        __global__ void __launch_bounds__(BLOCK, 2) __attribute__((amdgpu_num_sgpr(96))) b_kernel(int n) {}
        // __global__ void c_kernel(int n) {}
        /* __global__ void d_kernel(int n) {} */
        extern "C" int lc_x(lc_ctx *ctx, int n) { if (n) return x_impl<float>(ctx, n); return x_impl<double>(ctx, n); }
        template <typename T> int x_impl(lc_ctx *ctx, int n) { hipLaunchKernelGGL((a_kernel<T, 0>), dim3(1), dim3(1), 0, 0, nullptr); return 0; }
    ''')
    assert global_kernels(snippet) == {"a_kernel", "b_kernel"}
    assert launched_by(snippet, "lc_x") == {"a_kernel"}


# ------------------------------------------------------------------ the cases meet the edges
def _const(code, pattern):
    m = re.search(pattern, code)
    assert m, pattern
    return int(m.group(1))


def _cap(code, entry, impl=None):
    """blocks * 256 of a launcher: `< CAP ? ... : CAP` blocks of dim3(256) threads."""
    body = body_of(code, impl or entry)
    m = re.search(r"const int blocks = .*?< (\d+) \? .*? : (\d+)\)?;", body)
    assert m and m.group(1) == m.group(2) and "dim3(blocks), dim3(256)" in body, entry
    return int(m.group(1)) * RC.BLOCK


def test_gauss_cases_meet_the_edges():
    api = source("api.hip")
    max_radius = _const(api, r"constexpr int GAUSS_MAX_RADIUS = (\d+);")
    assert "G.radius = (int)(4.0 * sigma + 0.5)" in api and "G.radius > GAUSS_MAX_RADIUS" in api and "sigma > 0" in api
    cap = _cap(api, "lc_gaussian_filter", "gauss_impl")
    assert cap == 4096 * 256
    f64 = [c for c in RC.GAUSS_CASES if c[3] == "float64"]
    f32 = [c for c in RC.GAUSS_CASES if c[3] == "float32"]
    R = RC.gauss_radius
    assert sum(R(s) > 2 * ny and R(s) > 2 * nx for ny, nx, s, _ in f64) >= 2                   # several folds on both axes
    assert any(ny == 1 and nx > 1 for ny, nx, _, _ in f64) and any(nx == 1 and ny > 1 for ny, nx, _, _ in f64)
    assert any(R(s) == 0 for _, _, s, _ in f64)
    halves = sorted(s for _, _, s, _ in f64 if 4 * s + 0.5 in (2.996, 3.0))
    assert [R(s) for s in halves] == [2, 3] and 4 * halves[1] + 0.5 == 3.0                     # either side of the half
    assert sum(R(s) == max_radius for _, _, s, _ in f64) >= 2
    assert R(RC.GAUSS_REFUSALS[0]) == max_radius + 1 and RC.GAUSS_REFUSALS[1:] == (0.0, -1.0)
    big = [c for c in f64 if c[0] * c[1] > cap]
    assert big and all(ny % RC.BLOCK and nx % RC.BLOCK for ny, nx, _, _ in big)
    # every shape in float64; the first, third, sixth and last in float32 as well
    assert [c[:3] for c in f32] == [f64[i][:3] for i in (0, 2, 5, len(f64) - 1)] and len(set(f64)) == len(f64) == 10
    assert {c[3] for c in RC.GAUSS_NONFINITE} == {"float32", "float64"}
    for ny, nx, s, dt in RC.GAUSS_NONFINITE:
        a = RC.gauss_input(ny, nx, dt, nonfinite=True)
        assert a.dtype == np.dtype(dt) and np.isnan(a[1:-1, 1:-1]).sum() == 1 and np.isinf(a).sum() == 1
        assert np.isinf(a[0, nx - 1]) and np.isfinite(RC.gauss_input(ny, nx, dt)).all()


def test_deriv_cases_meet_the_edges():
    sig = source("sigma.hip")
    cap = _cap(sig, "lc_fourth_order_derivative")
    assert cap == 8192 * 256 and "ny >= 5 && nx >= 5" in body_of(sig, "lc_fourth_order_derivative")
    assert RC.DERIV_CASES[0] == (5, 5) and {(5, 6), (6, 5), (29, 40), (257, 255)} <= set(RC.DERIV_CASES)
    assert any(ny * nx > cap for ny, nx in RC.DERIV_CASES) and RC.DERIV_NONFINITE in RC.DERIV_CASES
    assert set(RC.DERIV_REFUSALS) == {(4, 9, 0), (9, 4, 0), (9, 9, 2)}
    for dt in RC.DERIV_DTYPES:
        a = RC.deriv_input(29, 40, dt, nonfinite=True)
        assert a.dtype == np.dtype(dt) and np.isnan(a[2, 2]) and np.isinf(a[0, 39]) and (~np.isfinite(a)).sum() == 2
        b = RC.deriv_input(29, 40, dt)
        assert np.array_equal(b.astype(np.float32).astype(dt), b) and np.abs(b).max() > 1e6    # float32 values that round when differenced


def test_ridge_sizes_meet_the_edges():
    cap = _cap(source("ridges.hip"), "lc_ridge_classify")
    assert cap == 4096 * 256
    assert RC.RIDGE_N == (257, 60000, cap + 257) and set(RC.RIDGE_SEEDS) == set(RC.RIDGE_N)
    k = len(RC.SPECIAL_ROWS) + len(RC.GRAD_SPECIALS)
    c = RC.ridge_case(RC.RIDGE_N[0])
    assert len(c["special"]) == k and min(c["special"].values()) == RC.RIDGE_N[0] - k        # names are distinct; the tail
    assert RC.RIDGE_N[-1] - k > cap                                                           # ... past the grid cap at the largest n


# ------------------------------------------------------------------ the gaussian, restated on the host
@functools.lru_cache(maxsize=None)
def _scipy_gauss(ny, nx, sigma, dtype, nonfinite=False):
    from scipy.ndimage import gaussian_filter
    return gaussian_filter(RC.gauss_input(ny, nx, dtype, nonfinite), sigma=sigma)


def _gauss_miss(case, reflect, nonfinite=False):
    """max |restatement - scipy| / bound over the finite reference values; inf where the non-finite footprints differ."""
    ny, nx, sigma, dtype = case
    a = RC.gauss_input(ny, nx, dtype, nonfinite)
    ref = _scipy_gauss(ny, nx, sigma, dtype, nonfinite)
    with np.errstate(invalid="ignore"):
        got = RC.gauss_restated(a, sigma, reflect)
    assert got.dtype == ref.dtype == a.dtype
    if not (np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isinf(got), np.isinf(ref))):
        return np.inf
    ok = np.isfinite(ref)
    return float(np.abs(got[ok].astype(np.float64) - ref[ok]).max()) / RC.gauss_bound(a, sigma)


@pytest.mark.parametrize("case", RC.GAUSS_CASES, ids=lambda c: "x".join(map(str, c)))
def test_the_restated_gaussian_meets_scipy_inside_the_bound(case):
    ny, nx, sigma, dtype = case
    miss = _gauss_miss(case, RC.reflect_index)
    assert miss <= 1.0, (case, miss)
    if RC.gauss_radius(sigma) == 0:
        assert np.array_equal(RC.gauss_restated(RC.gauss_input(ny, nx, dtype), sigma), RC.gauss_input(ny, nx, dtype))
        assert np.array_equal(_scipy_gauss(ny, nx, sigma, dtype), RC.gauss_input(ny, nx, dtype))


@pytest.mark.parametrize("case", RC.GAUSS_NONFINITE, ids=lambda c: "x".join(map(str, c)))
def test_the_restated_gaussian_has_scipys_nonfinite_footprint(case):
    assert _gauss_miss(case, RC.reflect_index, nonfinite=True) <= 1.0
    ref = _scipy_gauss(*case, nonfinite=True)
    assert np.isnan(ref).any() and np.isinf(ref).any() and np.isfinite(ref).any()


def test_a_single_fold_reflect_fails_the_many_fold_and_one_node_cases():
    """reflect_index folds as often as it takes and knows the axis of one node: with one fold alone the cases that reach
    beyond ``2 n`` or have such an axis leave the bound, the others do not notice."""
    for case in RC.GAUSS_CASES:
        ny, nx, sigma, _ = case
        if ny * nx > 100000:
            continue
        r = RC.gauss_radius(sigma)
        must_fail = r > min(ny, nx)                  # a second fold, or n == 1 with any radius
        miss = _gauss_miss(case, RC.reflect_single_fold)
        assert (miss > 1.0) == must_fail, (case, miss)
    failing = [c for c in RC.GAUSS_CASES if RC.gauss_radius(c[2]) > min(c[0], c[1])]
    assert {(3, 7), (2, 5), (1, 9), (9, 1), (5, 5), (300, 7)} == {c[:2] for c in failing}
    i = np.arange(-40, 60)
    assert np.array_equal(RC.reflect_index(i, 7), np.pad(np.arange(7), (42, 63), mode="symmetric")[i + 42])    # numpy's name for scipy's 'reflect'
    assert np.array_equal(RC.reflect_index(i, 1), np.zeros_like(i))


# ------------------------------------------------------------------ the classify references
@functools.lru_cache(maxsize=None)
def _ridge(n):
    c = RC.ridge_case(n)
    return c, RC.ridge_reference(c["a"], c["b"], c["d"], c["gx"], c["gy"], c["tol"])


@pytest.mark.parametrize("n", [n for n in RC.RIDGE_N if n >= 60000])
def test_ridge_inputs_take_every_dgeev_branch(n):
    assert min(RC.branch_counts(*RC.ridge_inputs(n, RC.RIDGE_SEEDS[n]))) > 100
    c = RC.ridge_case(n)                                   # ... and still do as the GPU sees them
    ac, bc, dc = (np.where(np.isfinite(v), v, 0.0) for v in (c["a"], c["b"], c["d"]))
    assert min(RC.branch_counts(ac, bc, dc)) > 100


def test_closed_form_equals_numpy_linalg_eig_on_the_special_rows():
    rows = list(RC.SPECIAL_ROWS) + [(name,) + m for name, m, _, _ in RC.GRAD_SPECIALS]
    a, b, d = (np.array([r[i] for r in rows]) for i in (1, 2, 3))
    w, V = np.linalg.eig(np.stack([np.stack([a, b], -1), np.stack([b, d], -1)], -2))
    w0, w1, Vc = RO.dlanv2_sym(a, b, d)
    for i, r in enumerate(rows):
        assert w[i, 0] == w0[i] and w[i, 1] == w1[i], (r, w[i], w0[i], w1[i])                  # bit for bit
        assert np.abs(V[i] - Vc[i]).max() < 1e-15, (r, V[i], Vc[i])
    # what the rows are there for
    named = {r[0]: i for i, r in enumerate(rows)}
    assert len(named) == len(rows)
    ties = [i for n_, i in named.items() if n_.startswith("a,0,a ")]
    assert len(ties) == 6 and all(w[i, 0] == w[i, 1] for i in ties)
    opposite = [i for n_, i in named.items() if n_.startswith("a,0,-a ")]
    assert len(opposite) == 6 and all(w[i, 0] == -w[i, 1] != 0 for i in opposite)
    anti = [i for n_, i in named.items() if n_.startswith("0,b,0 ")]                          # through dlanv2: equal to an ulp or two
    assert len(anti) == 6 and all(np.sign(w[i, 0]) == -np.sign(w[i, 1]) != 0 and abs(w[i, 0] + w[i, 1]) <= 4 * np.finfo(float).eps * abs(w[i, 0]) for i in anti)
    assert not w[named["zero"]].any()
    above = [i for n_, i in named.items() if "above" in n_]
    below = [i for n_, i in named.items() if "below" in n_]
    ulp = np.finfo(float).eps
    assert len(above) == len(below) == 12
    assert all(abs(b[i]) > ulp * (abs(a[i]) + abs(d[i])) for i in above) and all(abs(b[i]) < ulp * (abs(a[i]) + abs(d[i])) for i in below)
    assert all(abs(b[i]) == np.nextafter(abs(b[j]), np.inf, dtype=np.float64) or abs(b[i]) == np.nextafter(np.nextafter(abs(b[j]), np.inf), np.inf)
               for i, j in zip(above, below))
    # magnitudes on both sides of dgeev's own scaling threshold, 2^-459
    assert min(RC.MAGNITUDES) < 2.0 ** -459 < sorted(RC.MAGNITUDES)[1]


@pytest.mark.parametrize("n", RC.RIDGE_N)
def test_the_gradient_specials_do_what_they_are_named_for(n):
    c, (m, em, dt, row) = _ridge(n)
    s, tol = c["special"], c["tol"]
    i = s["gx=inf on a zero of the row, eigmin<0"]
    assert row[i, 0] == 0 and np.isinf(c["gx"][i]) and np.isnan(dt[i]) and em[i] < 0 and m[i] == 1
    i = s["gy=inf on a zero of the row, eigmin>0"]
    assert row[i, 1] == 0 and np.isinf(c["gy"][i]) and np.isnan(dt[i]) and em[i] > 0 and m[i] == 0
    i = s["gx=-inf, no zero in the row"]
    assert row[i].all() and np.isinf(dt[i]) and em[i] < 0 and m[i] == 0
    i = s["gy=NaN"]
    assert np.isnan(dt[i]) and em[i] < 0 and m[i] == 1
    i, j = s["dt==tol"], s["dt==nextafter(tol)"]
    assert c["exact"] == (i, j) and dt[i] == tol and dt[j] == np.nextafter(tol, np.inf) and m[i] == 1 and m[j] == 0 and em[i] < 0 and em[j] < 0
    assert m[13] == (1.0 if em[13] < 0 else 0.0) and np.isnan(dt[13])


# ------------------------------------------------------------------ the borderline caps, for the references alone
@pytest.mark.parametrize("n,tol", [(n, RC.RIDGE_TOL) for n in RC.RIDGE_N] + [(RC.RIDGE_N_TOL0, 0.0)])
def test_few_classify_points_are_borderline(n, tol):
    if tol == RC.RIDGE_TOL:
        c, (m, em, dt, row) = _ridge(n)
    else:
        c = RC.ridge_case(n, tol=tol)
        m, em, dt, row = RC.ridge_reference(c["a"], c["b"], c["d"], c["gx"], c["gy"], tol)
    share = RC.borderline(dt, tol, RC.RIDGE_BORDER, c["exact"]).mean()
    assert share <= RC.BORDER_SHARE, (n, tol, share)
    assert 0 < m.sum() < m.size                               # both answers occur


@functools.lru_cache(maxsize=None)
def chain_reference(name):
    case = RC.CHAIN_CASES[name]
    _, _, _, f, lat, lon = RC.chain_input(case)
    return RO.find_ridges_spherical_hessian(f, lat, lon, sigma=case["sigma"], tolerance_threshold=RC.CHAIN_TOL, isglobal=case["isglobal"])


@pytest.mark.parametrize("name", list(RC.CHAIN_CASES))
def test_few_chain_points_are_borderline(name):
    m, em, dt = chain_reference(name)
    share = RC.borderline(dt, RC.CHAIN_TOL, RC.CHAIN_BORDER_REL * RC.CHAIN_TOL).mean()
    assert share <= RC.BORDER_SHARE, (name, share)
    assert set(np.unique(m)) <= {0.0, 1.0}
    if RC.CHAIN_CASES[name]["ny"] > 7:
        assert 0 < m.sum() < m.size, name


def test_chain_cases_are_what_the_table_promises():
    C = RC.CHAIN_CASES
    assert all(f"{n.rsplit('-', 1)[0]}-{g}" in C for n in C for g in ("global", "regional"))
    assert any(c["lat_desc"] and not c["roll"] for c in C.values()) and any(c["roll"] == 17 and not c["lat_desc"] for c in C.values())
    assert {c["dims"] for c in C.values()} == {RC.LL, RC.LON_LAT}
    narrow = [c for c in C.values() if (c["ny"], c["nx"]) == (7, 12)]
    assert narrow and all(c["sigma"] == 3.0 and RC.gauss_radius(3.0) > c["ny"] and RC.gauss_radius(3.0) >= c["nx"] for c in narrow)
    sig = [c["sigma"] for c in C.values() if c["isglobal"] and c["dims"] == RC.LL and not c["lat_desc"] and not c["roll"] and c["ny"] == 41]
    assert [type(s) for s in sig[-5:]] == [type(None), int, float, np.float64, np.float32]
    assert [RC.smooths(s) for s in RC.SIGMA_VARIANTS] == [False, False, True, True, False]
    # the oracle's isinstance rule decides the same: the variants that skip the filter give sigma=None's bits, the others do not
    names = [n for n in C if n.startswith("sigma") and n.endswith("-global")]
    none = chain_reference(names[0])
    for n, s in zip(names, RC.SIGMA_VARIANTS):
        assert C[n]["sigma"] is s
        same = all(np.array_equal(x, y, equal_nan=True) for x, y in zip(chain_reference(n), none))
        assert same == (not RC.smooths(s)), n
    # the stored layout is what the name says, and sorting it gives the reference's input back
    for n, c in C.items():
        v, lat, lon, f, slat, slon = RC.chain_input(c)
        assert (np.diff(lat) < 0).all() == c["lat_desc"] and (np.diff(lon) > 0).all() == (c["roll"] == 0)
        vv = v.T if c["dims"] == RC.LON_LAT else v
        assert np.array_equal(vv[np.argsort(lat)][:, np.argsort(lon)], f) and np.array_equal(np.sort(lat), slat) and np.array_equal(np.sort(lon), slon)
