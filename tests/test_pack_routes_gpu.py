"""Every route of tests/pack_routes.py forced on the GPU: the name lc_ctx_last_pack_kernel reports is asserted, then the WHOLE
image is checked -- the interior of every level and both components against scipy.ndimage.spline_filter(float64(F), order,
mode="mirror") (order 1: the raw values, exactly), every pad node against the interior node it mirrors (bit for bit, corners
included), the fused-level image against 2 img[t] - img[t+1] bit for bit (FIR mode 2: against scipy on 2 F[t] - F[t+1]),
and the image of the same call without ext against the one with it, bit for bit (pads_only_kernel against pads_ext_kernel).

Inputs: seeded standard normal fields scaled by 20, drawn once per shape and never modified; the scipy result is computed
once per (shape, order).  Every buffer the engines allocate starts as NaN, so a node no kernel wrote fails the comparisons.
Each case prints its measured error beside its bound before asserting (pytest -s)."""
import functools

import numpy as np
import pytest

from tests import pack_routes as PR

pytestmark = pytest.mark.gpu

_ENGINES = {}
F32, F64 = np.dtype(np.float32), np.dtype(np.float64)


@pytest.fixture(scope="module", autouse=True)
def _engines():
    yield
    for e in _ENGINES.values():
        e.close()
    _ENGINES.clear()


def _engine(monkeypatch, env):
    """One Engine per distinct tuple of context-creation knobs (read once, in lc_ctx_create)."""
    key = tuple(sorted(env.items()))
    if key not in _ENGINES:
        for k in PR.ENV_KNOBS:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        from lagrangiancoherence_amd.engine import Engine
        e = Engine(0)
        e._poison = True          # Engine._empty: NaN instead of whatever the caching allocator hands back
        _ENGINES[key] = e
    return _ENGINES[key]


def _np(t):
    return t.detach().cpu().numpy()


def _kind(r):
    return "float64" if r["dtype"] == "float64" else "float32"       # the element type of the raw planes


def _out(r):
    return F32 if r["dtype"] == "float32" else F64                   # ... and of the image


@functools.lru_cache(maxsize=None)
def _planes(nt, ny, nx, kind):
    rng = np.random.default_rng([nt, ny, nx])
    u, v = (20.0 * rng.standard_normal((nt, ny, nx)) for _ in range(2))
    if kind == "float32":
        u, v = u.astype(np.float32), v.astype(np.float32)
    u.setflags(write=False)
    v.setflags(write=False)
    return u, v


def _filtered(F, order):
    """scipy.ndimage.spline_filter(F[t, :, :, c], order, mode="mirror") for every level and component at once: the two
    spline_filter1d calls it makes (test_pack_routes.py checks the bits)."""
    from scipy.ndimage import spline_filter1d
    F = F.astype(np.float64)
    for axis in (1, 2):
        F = spline_filter1d(F, order, axis=axis, mode="mirror")
    return F


@functools.lru_cache(maxsize=None)
def _ref(nt, ny, nx, kind, order):
    """(nt, ny, nx, 2) float64: the interior the image must hold."""
    F = np.stack(_planes(nt, ny, nx, kind), axis=-1).astype(np.float64)
    out = F if order == 1 else _filtered(F, order)
    out.setflags(write=False)
    return out


def _mirror(n):
    """Padded index of the interior node each padded node 0 .. n + 2 mirrors (itself for an interior node)."""
    i = np.abs(np.arange(-1, n + 2))
    return np.where(i > n - 1, 2 * (n - 1) - i, i) + 1


def _check_pads(a, ny, nx, what):
    assert np.array_equal(a, a[:, _mirror(ny)][:, :, _mirror(nx)]), f"{what}: a pad differs from the interior node it mirrors (or was not written)"


def _direct(eng, lc, u, v, order, want_img, want_ext, out):
    """lc_field_pack itself.  -> (img tensor or None, ext tensor or None, reported name)"""
    from lagrangiancoherence_amd import _capi
    nt, ny, nx = u.shape
    ud, vd = eng.to_device(u.copy(), u.dtype), eng.to_device(v.copy(), v.dtype)
    img = eng._empty((eng.lib.lc_packed_elems(nt, ny, nx),), out) if want_img else None
    ext = eng._empty((eng.lib.lc_packed_elems(nt - 1, ny, nx),), out) if want_ext else None
    eng._use_current_stream()
    _capi.check(eng.lib.lc_field_pack(eng.ctx, eng._ptr(ud), eng._ptr(vd), lc, nt, ny, nx, order, eng._ptr(img), eng._ptr(ext)), eng.lib)
    return img, ext, eng.last_pack_kernel()


def _lc(r):
    from lagrangiancoherence_amd import _capi
    return {"float32": _capi.LC_F32, "float64": _capi.LC_F64, "f64_wind_f32": _capi.LC_F64_WIND_F32}[r["dtype"]]


def _pack(eng, r, shape, ext):
    """The route's pack, through Engine.prepare_field where it can express the form, through lc_field_pack where it cannot
    (float32 ext alone, ext at orders 2, 4, 5, float32 planes at orders 2, 4, 5).
    -> (img, ext, name): (levels, ny + 3, nx + 3, 2) numpy arrays or None."""
    nt, ny, nx = shape
    u, v = _planes(nt, ny, nx, _kind(r))
    order, out = r["order"], _out(r)
    ext = bool(ext) and nt >= 2
    if order == 1:
        kw = dict(lin_image=True, fuse_levels=ext) if r["lin"] else (dict(lin_image=False, ext_image=True) if out == F64 else None)
    elif r["dtype"] == "f64_wind_f32":
        kw = {} if order == 3 else None
    elif order == 3:
        kw = dict(fuse_levels=ext, ext_image=True)
    else:
        kw = None if ext else {}
    if kw is not None:
        cdt = F32 if r["dtype"] == "float32" else F64
        lat, lon = np.linspace(-80, 80, ny).astype(cdt), (-180 + 360.0 / nx * np.arange(nx)).astype(cdt)
        f = eng.prepare_field(u.copy(), v.copy(), lat, lon, order, **kw)
        name = eng.last_pack_kernel()
        img, e = (f.lin if order == 1 else f.cub), f.ext
    else:
        img, e, name = _direct(eng, _lc(r), u, v, order, r["lin"], ext, out)
    assert (img is not None) == r["lin"] and (e is not None) == ext
    for t in (img, e):
        assert t is None or t.dtype == getattr(eng.torch, out.name)
    img = None if img is None else _np(img).reshape(nt, ny + 3, nx + 3, 2)
    e = None if e is None else _np(e).reshape(nt - 1, ny + 3, nx + 3, 2)
    return img, e, name


def _bound(r, ref, scale):
    t = PR.TOL[r["tol"]]
    if t == "f32_store":
        return PR.f32_store_bound(ref, r["order"])
    return t[1] * scale if t[0] == "rel" else t[1]


def _check_route(eng, rid, r, shape):
    nt, ny, nx = shape
    order, out = r["order"], _out(r)
    fir, fused = int(r["env"].get("LCS_FIR_PREFILTER", "1")), int(r["env"].get("LCS_FUSED_PREFILTER", "1"))
    img, ext, name = _pack(eng, r, shape, r["ext"])
    assert name == r["name"], (rid, shape, name)
    ref = _ref(nt, ny, nx, _kind(r), order)
    scale = float(np.abs(ref if order == 1 else np.stack(_planes(nt, ny, nx, _kind(r)))).max())
    inner = (slice(None), slice(1, ny + 1), slice(1, nx + 1))
    if img is not None:
        if order == 1:
            assert np.array_equal(img[inner], ref.astype(out)), (rid, shape)
        else:
            err, bound = float(np.abs(img[inner].astype(np.float64) - ref).max()), _bound(r, ref, scale)
            print(f"PACKROUTE {rid} {shape} {r['tol']}: max|img - scipy| = {err:.3e}  bound {bound:.3e}  ({err / bound:.2f})")
            assert err <= bound, (rid, shape, err, bound)      # (NaN: a node no kernel wrote)
        _check_pads(img, ny, nx, f"{rid} {shape} img")
    if ext is not None:
        assert ext.shape[0] == nt - 1
        _check_pads(ext, ny, nx, f"{rid} {shape} ext")
        if name == "prefilter_fir_kernel (img + ext)":
            # a second filtered image of G = 2 F[t] - F[t+1], formed in float32 as the kernel forms it; the FIR bound at G's scale
            F = np.stack(_planes(nt, ny, nx, "float32"), axis=-1)
            G = np.float32(2.0) * F[:-1] - F[1:]
            assert G.dtype == F32
            err, bound = float(np.abs(ext[inner].astype(np.float64) - _filtered(G, 3)).max()), PR.TOL["f32_fir"][1] * float(np.abs(G).max())
            print(f"PACKROUTE {rid} {shape} f32_fir: max|ext - scipy(2F[t] - F[t+1])| = {err:.3e}  bound {bound:.3e}  ({err / bound:.2f})")
            assert err <= bound, (rid, shape, err, bound)
        else:
            # from finished coefficients / raw values: one rounding of 2 a - b (2 a is exact), in the image's dtype
            base = img if img is not None else ref.astype(out)[:, _mirror(ny) - 1][:, :, _mirror(nx) - 1]
            want = out.type(2) * base[:-1] - base[1:]
            assert want.dtype == out and np.array_equal(ext, want), (rid, shape)
    if ext is not None and img is not None:
        # the same call without ext: the same coefficient image, bit for bit (behind the sweeps: pads_only_kernel)
        img2, ext2, name2 = _pack(eng, r, shape, False)
        assert ext2 is None and name2 == PR.dispatch(r["dtype"], order, nt, ny, nx, fir, fused, False)[0], (rid, shape, name2)
        assert np.array_equal(img2, img), (rid, shape)


CASES = [(rid, s) for rid, r in PR.ROUTES.items() for s in r["shapes"]]


@pytest.mark.parametrize("rid,shape", CASES, ids=[f"{rid}-{'x'.join(map(str, s))}" for rid, s in CASES])
def test_pack_route(monkeypatch, rid, shape):
    r = PR.ROUTES[rid]
    _check_route(_engine(monkeypatch, r["env"]), rid, r, shape)


def test_every_name_literal_is_asserted_by_a_case():
    assert {r["name"] for r in PR.ROUTES.values()} == {PR.ROUTES[rid]["name"] for rid, _ in CASES}


@pytest.mark.parametrize("rid", list(PR.CAPPED))
def test_grids_beyond_the_block_cap_are_looped_over(monkeypatch, rid):
    """grid.y / grid.z are capped at 65535 blocks and the kernels loop over what is beyond: 65543 padded rows through
    pack_fused_kernel (order 1) and pads_ext_kernel (order 3 behind the sweeps), 65600 levels through pads_only_kernel.
    The whole image is checked as for a route: rows and levels past the cap hold their values, not the NaN they started as."""
    r = PR.CAPPED[rid]
    shape, = r["shapes"]
    assert max(shape[0], shape[1] + 3) > PR.GRID_CAP
    _check_route(_engine(monkeypatch, r["env"]), rid, r, shape)


W32 = [(rid, s) for rid, r in PR.ROUTES.items() if r["dtype"] == "f64_wind_f32" for s in r["shapes"]]


@pytest.mark.parametrize("rid,shape", W32, ids=[f"{rid}-{'x'.join(map(str, s))}" for rid, s in W32])
def test_float32_planes_give_the_bits_of_the_same_values_widened_first(monkeypatch, rid, shape):
    """LC_F64_WIND_F32 (float32 planes in, float64 coefficients out) against LC_F64 on the same values widened to float64:
    every order-3 route and orders 2, 4, 5, bit for bit."""
    from lagrangiancoherence_amd import _capi
    r = PR.ROUTES[rid]
    eng = _engine(monkeypatch, r["env"])
    nt, ny, nx = shape
    u, v = _planes(nt, ny, nx, "float32")
    a, _, name = _direct(eng, _capi.LC_F64_WIND_F32, u, v, r["order"], True, False, F64)
    assert name == r["name"], (rid, shape, name)
    b, _, name = _direct(eng, _capi.LC_F64, u.astype(np.float64), v.astype(np.float64), r["order"], True, False, F64)
    assert name == r["name"].replace("<float>", "<double>"), (rid, shape, name)
    assert np.array_equal(_np(a), _np(b)), (rid, shape)


@pytest.mark.parametrize("shape", PR.EXTRAPOLATE_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("order", [1, 3])
@pytest.mark.parametrize("kind", ["float32", "float64"])
def test_extrapolate_equals_the_ext_image_of_the_pack(monkeypatch, kind, order, shape):
    """lc_field_extrapolate (extrapolate_kernel, a grid-stride loop over 8192 x 256 threads) on a packed image against the ext
    image lc_field_pack built in the same call as that image: bit for bit, at a size below the grid and at one above it."""
    from lagrangiancoherence_amd import _capi
    eng = _engine(monkeypatch, {})
    nt, ny, nx = shape
    out = np.dtype(kind)
    lc = _capi.LC_F32 if out == F32 else _capi.LC_F64
    u, v = _planes(nt, ny, nx, kind)
    img, ext, _ = _direct(eng, lc, u, v, order, True, True, out)
    got = eng._empty(tuple(ext.shape), out)
    _capi.check(eng.lib.lc_field_extrapolate(eng.ctx, eng._ptr(img), lc, nt, ny, nx, eng._ptr(got)), eng.lib)
    got, ext = _np(got), _np(ext)
    assert np.isfinite(ext).all() and np.array_equal(got, ext)
