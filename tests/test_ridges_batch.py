"""The stacked ridge extraction on the CPU: the new translation unit and its three symbols, ``lc_ridges_batch``'s refusals before
any device call (with their numbers in ``lc_last_error``), the ctypes mirror of its argument structure, the cases of
tests/ridges_batch.py under the oracle alone (few borderline points, both mask values in every stack), and the intake of the N-D
``tools.find_ridges_spherical_hessian`` through a stand-in engine answering with the oracle: what it hands the engine (the sorted,
stacked planes, the sorted coordinates whose metric is tools.py:255-256, the reference's sigma rule) and what it makes of the
answer (dimension order, coordinates, the six-tuple).  Before the feature a 3-D input failed at the transpose.  The arithmetic on
the GPU is tests/test_ridges_batch_gpu.py's."""
import ctypes as C
import functools
import inspect
import os
import re

import numpy as np
import pytest
import torch

from lagrangiancoherence_amd import _capi, build, dropin
from lagrangiancoherence_amd import tools as T
from lagrangiancoherence_amd.engine import Engine
from oracle import ridges_oracle as RO
from tests import labelled
from tests import ridge_chain as RC
from tests import ridges_batch as RB
from tests.test_capi_symbols import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lagrangiancoherence_amd", "csrc")


@pytest.fixture(scope="module")
def lib():
    build.build_library(verbose=False)
    return _capi.load()


# ------------------------------------------------------------------ the translation unit and the C ABI
def test_symbols_in_header_prototypes_and_library(lib):
    for name in ("lc_ridges_work_elems", "lc_ridges_batch", "lc_ctx_last_ridges_kernel"):
        assert name in declared_symbols() and name in _capi.PROTOTYPES and hasattr(lib, name)
    assert lib.lc_version() == 104 == _capi.LC_VERSION          # additive: no argument list changed
    assert "ridges_batch.hip" in build.SOURCES
    assert lib.lc_ctx_last_ridges_kernel(None) == b""


def test_the_new_kernels_live_in_their_own_file_and_share_the_arithmetic():
    from tests.test_ridge_chain import global_kernels, strip_comments
    src = strip_comments(open(os.path.join(CSRC, "ridges_batch.hip")).read())
    assert global_kernels(src) == {"gauss_planes_kernel", "hessian_ridge_kernel"}
    assert not re.search(r"\basm\b", src)
    # one arithmetic: the taps, the stencils and the per-point step come from the shared headers
    for header, names in (("gauss_taps.h", ("gauss_taps<", "gauss_fill_weights(")), ("ridge_point.h", ("ridge_point(",)),
                          ("flowmap_gradient.h", ("centred(", "one_sided("))):
        assert f'#include "{header}"' in src and all(n in src for n in names), header
    api = strip_comments(open(os.path.join(CSRC, "api.hip")).read())
    rid = strip_comments(open(os.path.join(CSRC, "ridges.hip")).read())
    assert '#include "gauss_taps.h"' in api and "gauss_taps<T, AXIS>(" in api and "struct GaussW" not in api
    assert '#include "ridge_point.h"' in rid and "ridge_point(" in rid and "dgeev_sym2" not in rid
    tile = tuple(int(re.search(r"\b%s = (\d+)" % n, src).group(1)) for n in ("RB_TH", "RB_TW"))
    assert tile == RB.TILE
    ny, nx = RB.SHAPES[-1]
    assert RB.SHAPES[0] == (5, 5) and RB.SHAPES[2] == RB.TILE and RB.SHAPES[3] == (RB.TILE[0] + 1, RB.TILE[1] + 1)
    assert ny > 2 * RB.TILE[0] and ny % RB.TILE[0] and nx > 2 * RB.TILE[1] and nx % RB.TILE[1]      # several tiles, ragged
    assert set(RB.SIGMAS) >= {1.2} and RB.SIGMAS[:5] == RC.SIGMA_VARIANTS and RB.TOL == RC.CHAIN_TOL


def test_work_elems_is_pure_arithmetic(lib):
    assert lib.lc_ridges_work_elems(541, 781, 29) == 2 * 541 * 781 * 29
    assert lib.lc_ridges_work_elems(0, 5, 1) == 0 and lib.lc_ridges_work_elems(5, 5, 0) == 0


def _args(**kw):
    """A well-formed argument structure over one host buffer cut into disjoint pieces (never dereferenced: every case is
    refused by the checks that precede the first HIP call)."""
    ny, nx, n = kw.get("ny", 8), kw.get("nx", 9), kw.get("n_members", 2)
    plane = max(ny, 1) * max(nx, 1) * max(n, 1) * 8
    base = 1 << 20
    a = _capi.RidgesArgs(struct_size=C.sizeof(_capi.RidgesArgs))
    a.f, a.dx_dev, a.work_dev = base, base + plane, base + 2 * plane
    a.mask_out, a.eigmin_out, a.dt_out = base + 4 * plane, base + 5 * plane, base + 6 * plane
    a.eigvec_out, a.grad_out = base + 7 * plane, base + 9 * plane
    a.ny, a.nx, a.n_members, a.isglobal = ny, nx, n, 1
    a.dy, a.sigma, a.tolerance = 111e3, 0.5, RC.CHAIN_TOL
    for k, v in kw.items():
        setattr(a, k, v)
    return a, plane, base


def test_lc_ridges_batch_refuses_before_any_device_call(lib):
    ctx = C.c_void_p(1)             # never dereferenced
    size = C.sizeof(_capi.RidgesArgs)

    def refused(a, ctx=ctx, status=_capi.LC_EINVAL):
        assert lib.lc_ridges_batch(ctx, C.byref(a) if a is not None else None) == status
        return lib.lc_last_error().decode()
    a, plane, base = _args()
    assert "lc_ridges_batch: null context" in refused(a, ctx=None)
    assert "null argument structure" in refused(None)
    a.struct_size = size - 8
    assert f"struct_size {size - 8}, this library has {size}" in refused(a)
    assert "grid 4x9 too small" in refused(_args(ny=4)[0]) and "grid 8x4 too small" in refused(_args(nx=4)[0])
    assert "bad n_members 0" in refused(_args(n_members=0)[0])
    assert "46341 x 46341 = 2147488281 points" in refused(_args(ny=46341, nx=46341, n_members=1)[0])
    assert "sigma 64.2 needs radius 257 > 256" in refused(_args(sigma=64.2)[0], status=_capi.LC_EUNSUPPORTED)
    assert "needs radius inf > 256" in refused(_args(sigma=float("inf"))[0], status=_capi.LC_EUNSUPPORTED)
    assert "bad dy" in refused(_args(dy=0.0)[0]) and "bad dy" in refused(_args(dy=float("nan"))[0])
    assert "null pointer" in refused(_args(f=None)[0]) and "null pointer" in refused(_args(dx_dev=None)[0])
    assert "work_dev must hold" in refused(_args(work_dev=None)[0])
    # aliasing: the input with an output, the work buffer's second half with an output, two outputs, partial overlaps
    assert "f and mask_out overlap" in refused(_args(mask_out=base)[0])
    assert "f and work_dev overlap" in refused(_args(work_dev=base + 8)[0])
    assert "work_dev and eigmin_out overlap" in refused(_args(eigmin_out=base + 3 * plane + 8)[0])
    assert "mask_out and dt_out overlap" in refused(_args(dt_out=base + 5 * plane - 8)[0])
    assert "eigvec_out and grad_out overlap" in refused(_args(grad_out=base + 8 * plane)[0])
    assert "dx_dev and grad_out overlap" in refused(_args(grad_out=base + plane)[0])
    with pytest.raises(ValueError, match="lc_ridges_batch"):
        _capi.check(lib.lc_ridges_batch(None, C.byref(a)), lib)


def test_the_ctypes_structure_has_the_size_the_library_checks(lib):
    """A structure of the mirror's size passes the size check (and is refused by the one after it); every other size is not."""
    size = C.sizeof(_capi.RidgesArgs)
    a, _, _ = _args(ny=4)
    assert lib.lc_ridges_batch(C.c_void_p(1), C.byref(a)) == _capi.LC_EINVAL and b"too small" in lib.lc_last_error()
    for wrong in (size - 4, size + 8, 0):
        a.struct_size = wrong
        assert lib.lc_ridges_batch(C.c_void_p(1), C.byref(a)) == _capi.LC_EINVAL
        assert f"struct_size {wrong}, this library has {size}".encode() in lib.lc_last_error()
    names = [f[0] for f in _capi.RidgesArgs._fields_]
    hdr = open(os.path.join(ROOT, "include", "lcs_hip.h")).read()
    body = re.sub(r"/\*.*?\*/", "", hdr[hdr.index("typedef struct lc_ridges_args {"):hdr.index("} lc_ridges_args;")], flags=re.S)
    assert re.findall(r"\b(\w+)\s*[,;]", body) == names              # field for field, in the header's order


def test_signatures():
    sig = inspect.signature(Engine.ridges_batch)
    assert list(sig.parameters) == ["self", "f", "lat", "lon", "sigma", "tolerance", "isglobal", "want"]
    d = {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty}
    assert d == dict(sigma=.5, tolerance=0.0005e-3, isglobal=True, want=("mask", "eigmin"))
    assert callable(Engine.last_ridges_kernel)
    assert inspect.signature(T.find_ridges_spherical_hessian) == inspect.signature(
        lambda da, sigma=.5, scheme='first_order', tolerance_threshold=0.0005e-3, return_eigvectors=False, isglobal=True: None)


# ------------------------------------------------------------------ the cases under the oracle alone
@functools.lru_cache(maxsize=None)
def oracle_plane(ny, nx, m, isglobal, si):
    out = RO.find_ridges_spherical_hessian(RB.plane(ny, nx, m), *RB.grid(ny, nx), sigma=RB.SIGMAS[si], tolerance_threshold=RB.TOL,
                                           return_eigvectors=True, isglobal=isglobal)
    for o in out:
        o.setflags(write=False)
    return out


@pytest.mark.parametrize("ny,nx", RB.SHAPES, ids=lambda v: str(v))
def test_few_points_are_borderline_and_every_stack_has_both_mask_values(ny, nx):
    for g in RB.GLOBAL:
        for si in range(len(RB.SIGMAS)):
            masks = []
            for m in range(max(RB.MEMBERS)):
                mask, _, dt = oracle_plane(ny, nx, m, g, si)[:3]
                share = RC.borderline(dt, RB.TOL, RC.CHAIN_BORDER_REL * RB.TOL).mean()
                assert share <= RC.BORDER_SHARE, (ny, nx, m, g, si, share)
                masks.append(mask)
                if m + 1 in RB.MEMBERS:
                    assert set(np.unique(np.stack(masks))) == {0.0, 1.0}, (ny, nx, m + 1, g, si)
    assert not any(np.array_equal(RB.plane(ny, nx, 0), RB.plane(ny, nx, m)) for m in (1, 2))


# ------------------------------------------------------------------ the intake, through a stand-in engine
class OracleRidgesEngine:
    """Answers ``ridges_batch`` with the oracle plane by plane and records what it was handed."""
    torch = torch

    def __init__(self):
        self.calls = []

    def to_host(self, t):
        return t.numpy()

    def ridges_batch(self, f, lat, lon, sigma=.5, tolerance=0.0005e-3, isglobal=True, want=("mask", "eigmin")):
        self.calls.append(dict(f=f, lat=lat, lon=lon, sigma=sigma, tolerance=tolerance, isglobal=isglobal, want=tuple(want)))
        per = [RO.find_ridges_spherical_hessian(p, lat, lon, sigma=sigma, tolerance_threshold=tolerance, return_eigvectors=True,
                                                isglobal=isglobal) for p in np.asarray(f)]
        planes = dict(mask=[o[0] for o in per], eigmin=[o[1] for o in per], dt=[o[2] for o in per],
                      eigvec=[_unmasked(o) for o in per], grad=[o[4] for o in per])
        return {k: torch.as_tensor(np.stack(planes[k])) for k in want}


def _unmasked(o):
    """A vector field whose masked form and angle are the oracle's: the oracle's masked vector where ``eigmin < 0``, elsewhere any
    vector with the oracle's angle (tan(angle), 1)."""
    mask, eigmin, dt, ev_masked, grad, angle = o
    with np.errstate(invalid="ignore"):
        free = np.stack([np.tan(np.deg2rad(angle)), np.ones_like(angle)])
    return np.where(eigmin[None] < 0, ev_masked, free)


@pytest.fixture
def oracle_engine(monkeypatch):
    eng = OracleRidgesEngine()
    monkeypatch.setattr(dropin, "_ENGINE", eng)
    monkeypatch.setattr(dropin, "get_engine", lambda: eng)
    monkeypatch.setattr(T, "get_engine", lambda: eng)
    return eng


def _record(dims, lat_desc=True, roll=5, ny=9, nx=12, lead=(("time", 3),)):
    """A labelled record with descending latitudes and rolled longitudes in the given dimension order, and its sorted planes."""
    n = int(np.prod([k for _, k in lead]))
    v, lat, lon = RB.stack(ny, nx, n)
    v = v.reshape(*(k for _, k in lead), ny, nx)
    slat, slon, sv = lat, lon, v
    if lat_desc:
        sv, slat = sv[..., ::-1, :], slat[::-1]
    if roll:
        sv, slon = np.roll(sv, roll, axis=-1), np.roll(slon, roll)
    coords = {"latitude": slat.copy(), "longitude": slon.copy()}
    for name, k in lead:
        coords[name] = 100.0 + 6 * np.arange(k)
    order = (*(name for name, _ in lead), "latitude", "longitude")
    da = labelled.DataArray(np.ascontiguousarray(sv), order, coords, name="ftle").transpose(*dims)
    return da, v.reshape(n, ny, nx), lat, lon, coords


@pytest.mark.parametrize("dims", [("time", "latitude", "longitude"), ("latitude", "time", "longitude"), ("longitude", "latitude", "time")])
@pytest.mark.parametrize("sigma", RB.SIGMAS, ids=lambda s: f"{type(s).__name__}_{s}")
def test_intake_hands_the_engine_sorted_stacked_planes_and_the_metric(oracle_engine, dims, sigma):
    da, planes, lat, lon, coords = _record(dims)
    ridges, eigmin = T.find_ridges_spherical_hessian(da, sigma=sigma, tolerance_threshold=RB.TOL, isglobal=False)
    call, = oracle_engine.calls
    assert isinstance(call["f"], np.ndarray) and call["f"].dtype == np.float64 and call["f"].flags.c_contiguous
    assert np.array_equal(call["f"], planes) and np.array_equal(call["lat"], lat) and np.array_equal(call["lon"], lon)
    assert call["want"] == ("mask", "eigmin") and call["isglobal"] is False and call["tolerance"] == RB.TOL
    assert (call["sigma"] is None) == (not RC.smooths(sigma)) and (call["sigma"] is None or call["sigma"] == sigma)
    # dx, dy of tools.py:255-256, from the sorted coordinates
    dx, dy = Engine.ridge_metric(call["lat"], call["lon"])
    assert np.array_equal(dx, (np.pi / 180) * (lon[1] - lon[0]) * 6371000 * np.cos(lat * np.pi / 180))
    assert dy == (np.pi / 180) * (lat[1] - lat[0]) * 6371000 and isinstance(dy, float) and dy > 0 and (dx > 0).all()
    for o in (ridges, eigmin):
        assert o.dims == dims and o.shape == tuple({"time": 3, "latitude": 9, "longitude": 12}[d] for d in dims) and o.name == "ftle"
        assert np.array_equal(o.coords["latitude"], lat) and np.array_equal(o.coords["longitude"], lon)
        assert np.array_equal(o.coords["time"], coords["time"])
    got = ridges.transpose("time", "latitude", "longitude").values
    for m in range(3):
        ref = RO.find_ridges_spherical_hessian(planes[m], lat, lon, sigma=sigma, tolerance_threshold=RB.TOL, isglobal=False)
        assert np.array_equal(got[m], ref[0]) and np.array_equal(eigmin.transpose("time", "latitude", "longitude").values[m], ref[1])


def test_six_tuple_of_a_stack_has_the_label_dimension_leading(oracle_engine):
    dims = ("latitude", "time", "longitude")
    da, planes, lat, lon, coords = _record(dims)
    out = T.find_ridges_spherical_hessian(da, sigma=1.2, tolerance_threshold=RB.TOL, return_eigvectors=True)
    assert len(out) == 6 and oracle_engine.calls[0]["want"] == ("mask", "eigmin", "dt", "eigvec", "grad")
    ridges, eigmin, dt, vec, grad, angle = out
    assert ridges.dims == eigmin.dims == dt.dims == angle.dims == dims
    assert vec.dims == ("eigvectors",) + dims and list(vec.coords["eigvectors"]) == ["d2dadxdy", "d2dadydx"]
    assert grad.dims == ("elements",) + dims and list(grad.coords["elements"]) == ["ddadx", "ddady"]
    tll = ("time", "latitude", "longitude")
    for m in range(3):
        ref = RO.find_ridges_spherical_hessian(planes[m], lat, lon, sigma=1.2, tolerance_threshold=RB.TOL, return_eigvectors=True)
        for o, r in zip((ridges, eigmin, dt), ref[:3]):
            assert np.array_equal(o.transpose(*tll).values[m], r)
        assert np.array_equal(vec.transpose("eigvectors", *tll).values[:, m], ref[3])                  # zeroed where eigmin >= 0
        assert np.array_equal(grad.transpose("elements", *tll).values[:, m], ref[4])
        np.testing.assert_allclose(angle.transpose(*tll).values[m], ref[5], rtol=1e-12, atol=1e-12)    # (tan and atan in between)
    for o in out:
        assert np.array_equal(o.coords["time"], coords["time"]) and np.array_equal(o.coords["latitude"], lat)


def test_every_further_dimension_is_a_stack_of_planes(oracle_engine):
    """(member, time, latitude, longitude): the planes are handed over in the record's own order of (member, time)."""
    dims = ("member", "latitude", "longitude", "time")
    da, planes, lat, lon, coords = _record(dims, lead=(("member", 2), ("time", 3)))
    ridges, eigmin = T.find_ridges_spherical_hessian(da, sigma=None, tolerance_threshold=RB.TOL)
    call, = oracle_engine.calls
    assert call["f"].shape == (6, 9, 12) and np.array_equal(call["f"], planes)
    assert ridges.dims == dims and ridges.shape == (2, 9, 12, 3)
    assert np.array_equal(ridges.coords["member"], coords["member"]) and np.array_equal(ridges.coords["time"], coords["time"])
    got = ridges.transpose("member", "time", "latitude", "longitude").values.reshape(6, 9, 12)
    for m in range(6):
        assert np.array_equal(got[m], RO.find_ridges_spherical_hessian(planes[m], lat, lon, sigma=None, tolerance_threshold=RB.TOL)[0])
