"""Array-level host API over the C ABI (include/lcs_hip.h).

`Engine` keeps wind fields, seeds and results resident in HBM as torch tensors
(torch is plumbing here: device memory, streams, torch.distributed) and calls
the HIP kernels through ctypes on torch's current stream.  `lcs_host` is the
torch-free route: host numpy arrays through the one-call entry point
`lc_lcs_host`.

Everything is arrays `(time, latitude, longitude)`, coordinates ascending; the
xarray-facing drop-in surface (`LagrangianCoherence.LCS.*`) sits on top of this
module in `dropin.py`.
"""
from __future__ import annotations

import ctypes as C
import os
from collections import namedtuple
from dataclasses import dataclass, field as _dc_field

import numpy as np

from . import _capi

__all__ = ["Engine", "PackedField", "PackedTracer", "AuxSeeds", "lcs_host", "lcs_global_host", "common_dtype", "x_boundary_mode"]

_NP2LC = {np.dtype(np.float32): _capi.LC_F32, np.dtype(np.float64): _capi.LC_F64}
_LAYOUTS = {"reference": _capi.LC_LAYOUT_REFERENCE, "physical": _capi.LC_LAYOUT_PHYSICAL}

# Engine.aux_seeds: the shifted seed coordinates of an auxiliary grid (north / south latitudes, east / west longitudes, clipped
# into the field's box), their separations lat_n - lat_s and lon_e - lon_w (NaN on invalid rows / columns) and the validity masks
AuxSeeds = namedtuple("AuxSeeds", "lat_n lat_s lon_e lon_w sep_lat sep_lon row_valid col_valid")


def x_boundary_mode(cyclic_xboundary, noncyclic_clamp=None, whole_grid=True) -> int:
    """lc_advect's ``cyclic_x`` (enum lc_xboundary).  ``cyclic_xboundary=False`` means the reference's own
    outer-product clamp (``noncyclic_clamp='reference_outer'``, LCS/trajectory.py:96-97, Q9).  The rule couples all
    seed rows through the offending columns, so a call on a row block (``whole_grid=False``) is only possible with a
    flag all-reduce over the ranks (:meth:`Engine.set_flag_allreduce`, which ``sharded_lcs`` installs) -- without one
    lc_advect refuses it; nothing is silently replaced by the per-point clamp (``noncyclic_clamp='pointwise'`` asks
    for that one explicitly; it differs from the reference only if a parcel leaves the longitude range)."""
    if cyclic_xboundary:
        return _capi.LC_X_CYCLIC
    if noncyclic_clamp is None:
        noncyclic_clamp = "reference_outer"
    if noncyclic_clamp not in ("pointwise", "reference_outer"):
        raise ValueError(f"noncyclic_clamp {noncyclic_clamp!r}: 'pointwise' or 'reference_outer'")
    return _capi.LC_X_CLAMP_REFERENCE_OUTER if noncyclic_clamp == "reference_outer" else _capi.LC_X_CLAMP_POINT


def common_dtype(*arrays) -> np.dtype:
    """float32 only if every input is float32, else float64.

    The reference lets numpy promote (fp32 wind on fp64 coordinates gives fp64
    positions and fp32 velocities); the kernels have one arithmetic
    type per call, so a mixed call is computed in float64.
    """
    dts = {np.dtype(str(getattr(a, "dtype", "float64")).replace("torch.", "")) for a in arrays if a is not None}
    return np.dtype(np.float32) if dts == {np.dtype(np.float32)} else np.dtype(np.float64)


def _smoothing_width(gauss_sigma) -> float:
    """``gauss_sigma`` as a width: anything that is not a real number (None, a bool) is no smoothing, 0."""
    return float(gauss_sigma) if isinstance(gauss_sigma, (float, int)) and not isinstance(gauss_sigma, bool) else 0.0


def _check_grid(a, b, lat_f, lon_f, what: str):
    """``(nt, ny_f, nx_f)`` of the planes ``a``, ``b`` of a ``what`` ('field', 'tracer'; ``b`` may be None), coordinates checked."""
    if len(a.shape) != 3 or (b is not None and tuple(b.shape) != tuple(a.shape)):
        raise ValueError("u and v must both be (time, latitude, longitude)" if what == "field" else
                         "tracers must be (time, latitude, longitude), both of one shape")
    nt, ny_f, nx_f = (int(s) for s in a.shape)
    if lat_f.shape != (ny_f,) or lon_f.shape != (nx_f,):
        raise ValueError(f"coordinate lengths do not match the {what}")
    if not (np.all(np.diff(lat_f) > 0) and np.all(np.diff(lon_f) > 0)):
        raise ValueError("latitude and longitude must be ascending (sort first)")
    return nt, ny_f, nx_f


def _check_order(thing, interp_order):
    """A field or tracer serves the order it was prepared for, and order 1."""
    if interp_order != 1 and thing.order != interp_order:
        raise ValueError(f"{'tracer' if isinstance(thing, PackedTracer) else 'field'} was prepared for interp_order={thing.order}")


def _on_grid(cls, lat_f, lon_f, dtype, nt, ny_f, nx_f, **buffers):
    """``cls`` -- :class:`PackedField` or :class:`PackedTracer`: the one place either is built -- of these buffers on this
    grid: the coordinate extremes in the arithmetic dtype (what .min() / .max() give numpy), and the version stamps of
    whatever planes a field is given to borrow, so no field exists that :meth:`Engine._check_planes` does not cover."""
    dtype = np.dtype(dtype)
    la, lo = np.asarray(lat_f).astype(dtype), np.asarray(lon_f).astype(dtype)
    for stamp, a, b in (("planes_version", "u", "v"), ("planes32_version", "u32", "v32")):
        if buffers.get(a) is not None:
            buffers[stamp] = (buffers[a]._version, buffers[b]._version)
    return cls(nt=int(nt), ny_f=int(ny_f), nx_f=int(nx_f), lat_min=float(la[0]), lat_max=float(la[-1]), lon_min=float(lo[0]),
               lon_max=float(lo[-1]), dtype=dtype, **buffers)


class PendingPack:
    """The rest of a deferred pack in ``engine``'s context: the four tensors the context still reads and writes (the planes
    ``u``, ``v`` -- borrowed, as given to ``prepare_field`` -- and the images), alive while it is pending whatever becomes of
    the field, and the planes' version stamps: the levels not packed yet are read from the planes LATER, so writing them in
    place before the pack is complete is refused like any other change of borrowed planes (``Engine._check_planes``)."""

    def __init__(self, engine, u, v, lin, ext):
        self.engine, self.tensors, self.versions = engine, (u, v, lin, ext), (u._version, v._version)
        self.spoiled = False   # the pack was completed from planes written meanwhile (Engine.close could not refuse): the images are no field's

    def live(self) -> bool:
        """Still the engine's pending pack and not complete yet (the C side completes it on its own in many calls)."""
        e = self.engine
        if e._pending is self and not (e.ctx and e.lib.lc_ctx_pack_pending(e.ctx)):
            e._pending = None
        if e._pending is not self:
            self.tensors = None
        return e._pending is self

    def moved(self) -> bool:
        return (self.tensors[0]._version, self.tensors[1]._version) != self.versions

    def check(self):
        if self.spoiled or (self.live() and self.moved()):
            raise RuntimeError("the wind tensors given to prepare_field were modified in place while the field's pack was still "
                               "pending: its later levels would be packed from the new values (prepare the field again, or pass copies)")

    def complete(self):
        """Completes the pack (``lc_ctx_flush_pack``) on the stream it began on, unless it is complete already."""
        self.check()
        if self.live():
            e = self.engine
            _capi.check(e.lib.lc_ctx_flush_pack(e.ctx), e.lib)
            e._pending = self.tensors = None


@dataclass
class PackedField:
    """Gather-ready image(s) of a wind time series, resident on the device.  Built by :meth:`on_grid`."""
    on_grid = classmethod(_on_grid)
    nt: int
    ny_f: int
    nx_f: int
    lat_min: float
    lat_max: float
    lon_min: float
    lon_max: float
    dtype: np.dtype
    lin: "torch.Tensor | None" = None     # order-1 image; None when the raw planes ``u``, ``v`` below serve as the order-1 source
    cub: "torch.Tensor | None" = None     # B-spline coefficient image of order ``order`` (2..5), None for order 1
    ext: "torch.Tensor | None" = None     # 2*img[t]-img[t+1] of the image matching interp_order (fused SETTLS sample)
    wind_f32: bool = False          # float32 wind on float64 coordinates: numpy's promotion rules in lc_advect
    order: int = 1                  # interpolation order the field was prepared for (order 1 is always available)
    fuse_raw: bool = False          # float64 at order 1: fused levels with NO packed image (2 F[t] - F[t+1] formed from u, v in the kernels)
    u: "torch.Tensor | None" = None  # the raw planes (nt, ny_f, nx_f) the images were packed from, kept as the ORDER-1 source
    v: "torch.Tensor | None" = None  # (lc_advect_ex: pole rows at any order, the Euler sample in float64) -- not copies: do not
    #                                  modify them in place while the field is in use (Engine._ensure_lin refuses if you did)
    planes_version: "tuple | None" = None  # (u._version, v._version) when the field was prepared
    lin32: "torch.Tensor | None" = None    # wind_f32 at order 1: the order-1 image of the float32 wind AS float32 (LC_F64_WIND_F32_LIN32)
    u32: "torch.Tensor | None" = None      # wind_f32: the float32 planes as given (the float64 copies u, v are made when a call needs them)
    v32: "torch.Tensor | None" = None
    planes32_version: "tuple | None" = None  # (u32._version, v32._version) when the field was prepared: borrowed like u, v
    # A deferred pack (Engine.prepare_field: float32 at order 1 with both images, a series longer than the first launch of a
    # fused advect call reaches): only the first levels of ``lin`` / ``ext`` are packed, the rest is pending in the engine's
    # context (``pending``: a PendingPack) and is packed inside the launches of the advect call that follows -- or, before
    # anything else reads the images, by ``pending.complete()``.  READING ``field.lin`` or ``field.ext`` completes the pack
    # first: whoever takes the images through the attributes sees whole images.  ``image(name)`` is the attribute as it is, for
    # the advect path of the engine that holds the pack, whose C entry point decides itself (lc_field_pack_deferred in
    # include/lcs_hip.h).
    pending: "PendingPack | None" = _dc_field(default=None, repr=False, compare=False)

    def __getattribute__(self, name):
        if name == "lin" or name == "ext":
            d = object.__getattribute__(self, "__dict__")
            pack = d.get("pending")
            if pack is not None:
                pack.complete()        # (refuses if the planes it still reads were written meanwhile: the pack stays pending)
                d["pending"] = None
        return object.__getattribute__(self, name)

    def image(self, name):
        """Attribute ``name`` without completing a pending pack."""
        return object.__getattribute__(self, name)


@dataclass
class PackedTracer:
    """One or two scalar tracers on a wind grid, ready for ``lc_tracer_sample``: the (C1, C2) pair in the (u, v) slots of
    ``lc_field_pack``'s layout (one tracer is the pair (C, C)).  Built by :meth:`on_grid`."""
    on_grid = classmethod(_on_grid)
    lin: "torch.Tensor | None"     # order-1 image: float32 at order 1 only (float64 samples the planes)
    cub: "torch.Tensor | None"     # B-spline coefficient image of order ``order`` (2..5), None for order 1
    c1: "torch.Tensor"             # the planes (nt, ny_f, nx_f): the order-1 source of the pole rows, and of every row in float64
    c2: "torch.Tensor"             # ... of the second tracer (``c1`` itself for one tracer)
    two: bool                      # two tracers
    nt: int
    ny_f: int
    nx_f: int
    lat_min: float
    lat_max: float
    lon_min: float
    lon_max: float
    dtype: np.dtype
    order: int = 1


# What Engine.prepare_field does for one field (field_plan).  upload: the dtype in which the planes go to the device; images:
# which of lin, lin32, cub, ext exist -> their length in time levels; packs: the lc_field_pack calls in order, each (LC dtype
# code, order, image or None, ext passed); planes: the PackedField attributes that keep the uploaded planes -- (u, v), (u32, v32)
# or (); wind_f32, fuse_raw, order: the field's; refusal: the ValueError of a combination that cannot be served, or None.
FieldPlan = namedtuple("FieldPlan", "upload images packs planes wind_f32 fuse_raw order refusal")


def field_plan(dtype, wind_f32, interp_order, nt, fuse_levels, lin_image, ext_image, ext_image_f64, ext_image_f64_o3) -> FieldPlan:
    """:meth:`Engine.prepare_field`'s decisions as a pure function of its options (its docstring says what they mean);
    ``wind_f32``: float32 wind on float64 coordinates; the last two are ``Engine.EXT_IMAGE_F64`` and ``EXT_IMAGE_F64_O3``."""
    f32 = np.dtype(np.float32)
    dtype, order = np.dtype(dtype), int(interp_order)
    if wind_f32 and lin_image is None and order in (1, 3):
        # The wind stays float32.  Order 1: its order-1 image as lc_field_pack builds it for float32 fields, widened node by
        # node inside the kernels (LC_F64_WIND_F32_LIN32: the bits of the float64 images, half the bytes, no conversion pass;
        # LCS/trajectory.py:86-87,110-112).  Order 3: scipy's spline coefficients of a float32 field are float64,
        # so the coefficient image is packed in float64 STRAIGHT from the float32 planes (LC_F64_WIND_F32), which also serve
        # the pole rows.  The float64 planes are made when a call needs them (Engine._planes64).
        image, code = ("lin32", _capi.LC_F32) if order == 1 else ("cub", _capi.LC_F64_WIND_F32)
        return FieldPlan(f32, {image: nt}, ((code, order, image, False),), ("u32", "v32"), True, False, order, None)
    # general orders and a float32 wind's float64 copy: generic direct kernel, two-sample form
    fuse = (fuse_levels is None or bool(fuse_levels)) and nt >= 2 and not wind_f32 and order in (1, 3)
    if lin_image is None:
        lin_image = dtype == f32 and order == 1
    # float64 with fused levels and no image to read them from: the kernels form 2 F[t] - F[t+1] themselves
    fuse_raw = fuse and dtype != f32 and (order == 3 or not lin_image) and \
        not ((ext_image_f64 if order == 1 else ext_image_f64_o3) if ext_image is None else ext_image)
    ext = fuse and not fuse_raw
    refusal = "float32 at interp_order=1 samples the order-1 image: lin_image cannot be False" \
        if dtype == f32 and order == 1 and not lin_image else None
    images = {k: n for k, n, on in (("lin", nt, lin_image), ("cub", nt, order != 1), ("ext", nt - 1, ext)) if on}
    packs = [(_NP2LC[dtype], 1, "lin" if lin_image else None, order == 1 and ext)] if lin_image or (order == 1 and ext) else []
    packs += [(_NP2LC[dtype], order, "cub", ext)] if order != 1 else []
    return FieldPlan(dtype, images, tuple(packs), () if lin_image else ("u", "v"), bool(wind_f32), fuse_raw, order, refusal)


# Where one advect call reads the wind from (call_source).  dtype: the call's LC dtype code; buffers: lc_advect_args pointer
# field -> the PackedField attribute it points at; planes64: the call reads the float64 planes of a field that may keep only
# float32 ones (Engine._planes64 first); lin: it reads the float32 order-1 image (Engine._ensure_lin builds a missing one).
CallSource = namedtuple("CallSource", "dtype buffers fuse_levels_raw planes64 lin")


def call_source(field: PackedField, interp_order, xmode) -> CallSource:
    """The source of a call on ``field`` at ``interp_order`` under the x boundary ``xmode``.  A float32 wind kept float32
    on float64 coordinates is read as it is (no float64 copy of the wind comes into being), except under the reference's
    outer-product clamp, which only the general form serves."""
    order = int(interp_order)
    if field.u32 is not None and xmode != _capi.LC_X_CLAMP_REFERENCE_OUTER:
        if field.lin32 is None and order == 3 == field.order:     # float64 coefficients, the float32 planes for the pole rows
            return CallSource(_capi.LC_F64_WIND_F32_LIN32, {"packed_cub": "cub", "u_raw": "u32", "v_raw": "v32"}, 0, False, False)
        if field.lin32 is not None and order == 1:
            return CallSource(_capi.LC_F64_WIND_F32_LIN32, {"packed_lin": "lin32"}, 0, False, False)
    same = field.order == order
    buffers = {"packed_lin": "lin", "u_raw": "u", "v_raw": "v", **({"packed_cub": "cub"} if order != 1 else {}),
               **({"packed_ext": "ext"} if same else {})}
    return CallSource(_capi.LC_F64_WIND_F32 if field.wind_f32 else _NP2LC[field.dtype], buffers, int(bool(field.fuse_raw and same)),
                      field.u32 is not None, field.dtype == np.dtype(np.float32) and order == 1)


class Engine:
    """One context on one MI355X.  Not a CPU fallback: needs the HIP library and a GPU."""

    def __init__(self, device: int | None = None):
        import torch
        self.torch = torch
        self.lib = _capi.load()
        if not torch.cuda.is_available():
            raise RuntimeError("lagrangiancoherence_amd.Engine needs a GPU (torch.cuda.is_available() is False); "
                               "there is no CPU path")
        self.device_index = torch.cuda.current_device() if device is None else int(device)
        self.device = torch.device("cuda", self.device_index)
        ctx = C.c_void_p()
        _capi.check(self.lib.lc_ctx_create(self.device_index, C.byref(ctx)), self.lib)
        self.lds_tiles_mode = -1      # what set_lds_tiles was last given (-1: the library's default, or LCS_LDS_TILES)
        self.verify_mode = 0          # lc_ctx_set_verify
        self._poison = bool(os.environ.get("LCS_DEBUG_POISON"))
        self._pending = None   # the context's pending pack (PendingPack; prepare_field), until it is complete
        self.ctx = ctx

    def close(self):
        if getattr(self, "ctx", None):
            pack = getattr(self, "_pending", None)
            if pack is not None and pack.live() and pack.moved():
                pack.spoiled = True        # (closing cannot be refused: the field is, wherever it is used next)
            self.lib.lc_ctx_destroy(self.ctx)   # (completes a pending pack: its tensors are alive until here)
            self.ctx = None
            self._pending = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_lds_tiles(self, mode: int):
        """lc_advect float32 kernel choice: -1 default (LDS tiles; at order 1 two seeds per lane from 2^23 seeds per call,
        one below), 1 LDS tiles with two seeds per lane at order 1 whatever the size, 2 one seed per lane, 0 direct gathers."""
        _capi.check(self.lib.lc_ctx_set_lds_tiles(self.ctx, int(mode)), self.lib)
        self.lds_tiles_mode = int(mode)

    def set_sigma_march(self, on: int):
        """lc_sigma float32 kernel choice: -1 default (marching kernel with wavefront shuffles from 2^23 cells per call,
        LDS tiles below), 1 marching kernel whatever the size, 0 LDS tiles."""
        _capi.check(self.lib.lc_ctx_set_sigma_march(self.ctx, int(on)), self.lib)

    def set_level_chunk(self, levels: int):
        """Run every advect call as consecutive launches of at most ``levels`` time levels (0: one launch; -1: by size,
        the default -- 32 levels from 2^18 seeds per call).  Results are bit-identical; it shapes the launches only
        (``lc_ctx_set_level_chunk``)."""
        _capi.check(self.lib.lc_ctx_set_level_chunk(self.ctx, int(levels)), self.lib)

    @property
    def level_chunk(self) -> int:
        """The context's levels-per-launch setting in force (``lc_ctx_get_level_chunk``): what :meth:`set_level_chunk`
        was last given, or what ``LCS_LEVEL_CHUNK`` set when the context was created (-1: by size)."""
        v = C.c_int()
        _capi.check(self.lib.lc_ctx_get_level_chunk(self.ctx, C.byref(v)), self.lib)
        return v.value

    def set_level_grading(self, chunk: int = 0, zone: int = -1, depth: int = -1):
        """Graded level counts of the float32 order-1 two-seed kernel under the by-size level chunk: ``chunk`` levels per
        launch (0: the by-size chunk), the last ``zone`` workgroups of a launch cut short by up to ``depth`` levels, made up
        in the next launch (-1: the defaults; ``depth=0``: uniform chunks).  Results are bit-identical; it shapes the
        launches only (``lc_ctx_set_level_grading``)."""
        _capi.check(self.lib.lc_ctx_set_level_grading(self.ctx, int(chunk), int(zone), int(depth)), self.lib)

    @property
    def level_grading(self):
        """``(chunk, zone, depth)`` as :meth:`set_level_grading` last set them (``lc_ctx_get_level_grading``)."""
        c, z, d = C.c_int(), C.c_int(), C.c_int()
        _capi.check(self.lib.lc_ctx_get_level_grading(self.ctx, C.byref(c), C.byref(z), C.byref(d)), self.lib)
        return c.value, z.value, d.value

    _FIDELITY = {"auto": _capi.LC_F64_AUTO, "exact": _capi.LC_F64_EXACT_ORDER, "fast": _capi.LC_F64_FAST}

    def set_f64_fidelity(self, mode: str):
        """float64 on the reference-shaped surfaces (the drop-in's ``LCS`` / ``parcel_propagation``, the one-call host
        routes): ``'exact'`` = numpy / scipy's operation order (~1e-13 degrees from the reference), ``'fast'`` = the
        fused-level form (rounding-level differences, <= 1e-9 degrees or the flow's own response to a 1e-12 degree seed
        shift, whichever is larger), ``'auto'`` (default) = exact up to 2^18 seeds per call, fast above
        (``lc_ctx_set_f64_fidelity``).  :meth:`prepare_field`'s own ``fuse_levels`` argument is explicit and unaffected."""
        if mode not in self._FIDELITY:
            raise ValueError(f"float64 fidelity {mode!r}: 'auto', 'exact' or 'fast'")
        _capi.check(self.lib.lc_ctx_set_f64_fidelity(self.ctx, self._FIDELITY[mode]), self.lib)

    def f64_fuse_levels(self, dtype, n_seeds: int) -> bool:
        """``fuse_levels`` for a reference-shaped call of ``n_seeds`` seeds in ``dtype`` under the context's fidelity
        setting (the rule of ``lc_lcs_host``: float32 always fuses)."""
        if np.dtype(dtype) != np.dtype(np.float64):
            return True
        m = C.c_int()
        _capi.check(self.lib.lc_ctx_get_f64_fidelity(self.ctx, C.byref(m)), self.lib)
        if m.value == _capi.LC_F64_EXACT_ORDER:
            return False
        return m.value == _capi.LC_F64_FAST or int(n_seeds) > _capi.LC_EXACT_ORDER_MAX_SEEDS

    def set_flag_allreduce(self, group=None, comm=None, enable=True):
        """Row-sharded grids with the reference's non-cyclic clamp (``LC_X_CLAMP_REFERENCE_OUTER``): install the
        MAX all-reduce of the offending-column flags over the ranks that share the seed grid
        (``lc_ctx_set_flag_allreduce``).  ``comm``: the C ABI's RCCL communicator (``lc_comm_flag_allreduce``);
        otherwise ``torch.distributed`` over ``group`` (nccl = RCCL reduces the device buffer in place on the current
        stream; gloo, used when rehearsing on one GPU, goes through the host).  ``enable=False`` removes it."""
        if not enable:
            _capi.check(self.lib.lc_ctx_set_flag_allreduce(self.ctx, None, None), self.lib)
            self._flag_cb = None
            return
        if comm is not None:
            fn = C.cast(self.lib.lc_comm_flag_allreduce, C.c_void_p)
            _capi.check(self.lib.lc_ctx_set_flag_allreduce(self.ctx, fn, comm), self.lib)
            self._flag_cb = None
            return
        torch = self.torch
        import torch.distributed as dist

        class _DeviceWords:     # a raw device pointer as a tensor, through the CUDA array interface
            def __init__(self, ptr, n):
                self.__cuda_array_interface__ = {"shape": (int(n),), "typestr": "<i4", "data": (int(ptr), False), "version": 2}

        def reduce(_user, ptr, count):
            try:
                t = torch.as_tensor(_DeviceWords(ptr, count), device=self.device)     # the flags are 0 / 1: int32 max is the OR
                if dist.get_backend(group) == "gloo":
                    h = t.cpu()
                    dist.all_reduce(h, op=dist.ReduceOp.MAX, group=group)
                    t.copy_(h)
                else:
                    dist.all_reduce(t, op=dist.ReduceOp.MAX, group=group)
                return 0
            except Exception:     # an exception must not unwind through the C frames of lc_advect
                import traceback
                traceback.print_exc()
                return 1
        self._flag_cb = _capi.FLAG_ALLREDUCE_FN(reduce)      # kept alive for as long as the context may call it
        _capi.check(self.lib.lc_ctx_set_flag_allreduce(self.ctx, C.cast(self._flag_cb, C.c_void_p), None), self.lib)

    def last_advect_kernel(self) -> str:
        """Name of the kernel the last :meth:`advect` call launched (as a profiler shows it)."""
        return self.lib.lc_ctx_last_advect_kernel(self.ctx).decode()

    def set_verify(self, mode: int = 1):
        """Wave-state audit of the one-seed order-1 LDS kernel (``lc_ctx_set_verify``): 1 on, 2 on with one injected
        corruption (test hook), 0 off.  Results are bit-identical; :meth:`read_verify` returns the counters."""
        _capi.check(self.lib.lc_ctx_set_verify(self.ctx, int(mode)), self.lib)
        self.verify_mode = int(mode)

    def read_verify(self, reset: bool = True) -> dict:
        """The audit's counters (synchronises): ``tile_changed`` wave-levels whose LDS tile no longer held what the wave
        staged, ``entries_changed`` 16-byte entries, ``slot_changes`` wave-levels at which the wave sat in another hardware
        slot than a level earlier (its context was switched out and back in), ``audited`` wave-levels checked, and the
        first event (workgroup, tile, wave, level, HW_ID before / after, lane mask)."""
        out = (C.c_uint * 16)()
        _capi.check(self.lib.lc_ctx_read_verify(self.ctx, out, int(bool(reset))), self.lib)
        v = [int(x) for x in out]
        d = {"tile_changed": v[0], "entries_changed": v[1], "slot_changes": v[2], "audited": v[3]}
        if v[12]:
            d["first_event"] = {"workgroup": v[4], "tile": v[5], "wave": v[6], "level": v[7], "hw_id_before": hex(v[8]),
                                "hw_id_after": hex(v[9]), "lane_mask": hex(v[10] | (v[11] << 32))}
        return d

    def last_advect_launches(self) -> int:
        """Kernel launches the last :meth:`advect` call made (level chunks)."""
        return int(self.lib.lc_ctx_last_advect_launches(self.ctx))

    TWO_SEED_MIN = 1 << 23   # seeds per call from which lc_advect's default is the two-seeds-per-lane kernel
    # float64 at order 1 with fused levels: build the fused-level image (True), or let the kernels form it from the raw
    # planes (False: no pack at all).  Measured on BASELINE configs[1] (profiles/r04): see DESIGN.md section 4.
    EXT_IMAGE_F64 = True
    # float64 at order 3 with fused levels: build the fused-level COEFFICIENT image ext = 2 cub[t] - cub[t+1] (True), or let
    # the kernels form it from cub node by node (False: the pack neither reads the coefficients back nor writes a second
    # image: 4.56 -> 3.28 ms on BASELINE configs[1]; but the advect kernel then stages two levels per iteration tile and
    # takes 8.22 ms instead of 6.31 -- the step loses 0.6 ms either way, serial and pipelined: profiles/r05/c2_o3_no_ext_image_ab.txt).
    EXT_IMAGE_F64_O3 = True

    class _Concurrent:
        """Context manager for ``n`` advect calls running side by side on different streams: what fills the machine is
        the seeds in flight, so the size rule of the default kernel choice is applied to ``n`` calls' worth."""

        def __init__(self, eng, seeds_per_call, n):
            self.eng, self.force = eng, eng.lds_tiles_mode == -1 and "LCS_LDS_TILES" not in os.environ \
                and seeds_per_call < Engine.TWO_SEED_MIN <= seeds_per_call * n

        def __enter__(self):
            if self.force:
                self.eng.set_lds_tiles(1)
            return self

        def __exit__(self, *exc):
            if self.force:
                self.eng.set_lds_tiles(-1)
            return False

    def concurrent_calls(self, seeds_per_call: int, n: int):
        return Engine._Concurrent(self, int(seeds_per_call), int(n))

    def last_sigma_kernel(self) -> str:
        """Name of the kernel the last :meth:`sigma` / :meth:`flowmap_gradient` call launched."""
        return self.lib.lc_ctx_last_sigma_kernel(self.ctx).decode()

    # ------------------------------------------------------------------ plumbing
    def last_pack_kernel(self) -> str:
        """The kernel the last ``lc_field_pack`` launched for its interleave / prefilter stage (``lc_ctx_last_pack_kernel``)."""
        return self.lib.lc_ctx_last_pack_kernel(self.ctx).decode()

    def _use_current_stream(self):
        """The context works on torch's current stream.  It precedes every call the engine makes into the library, and most
        of those complete a pending pack on their own, from the planes as they are at that moment (a change of stream here,
        ``lc_advect_ex`` of another field, ``lc_sample``, the copies): so this is where the planes' version stamps are looked
        at -- whatever completes the pack next, the planes are still the ones ``prepare_field`` was given."""
        if self._pending is not None:
            self._pending.check()
        s = self.torch.cuda.current_stream(self.device).cuda_stream
        _capi.check(self.lib.lc_ctx_set_stream(self.ctx, C.c_void_p(s)), self.lib)

    STAGED_COPY_FROM = 8 << 20   # bytes from which host <-> device copies go through the context's pinned staging ring

    def to_device(self, a, dtype: np.dtype):
        torch = self.torch
        if isinstance(a, torch.Tensor):
            t = a.to(device=self.device, dtype=getattr(torch, np.dtype(dtype).name))
            return t.contiguous()
        a = np.asarray(a)
        if a.ndim > 1 and not a.flags.c_contiguous and a.dtype == np.dtype(dtype) and a.nbytes >= self.STAGED_COPY_FROM:
            # a transposed VIEW of a contiguous array (the reference's example builds u, v with dims (latitude, longitude,
            # time) and the adapter asks for (time, latitude, longitude): LCS/LCS.py:101-104): making it contiguous on the host
            # is a strided copy at ~1 GB/s.  The buffer travels as it lies in memory, the permutation runs on the device.
            order = sorted(range(a.ndim), key=lambda i: -abs(a.strides[i]))
            base = a.transpose(order)
            if base.flags.c_contiguous:
                inv = [order.index(i) for i in range(a.ndim)]
                return self.to_device(base, dtype).permute(inv).contiguous()
        a = np.ascontiguousarray(a, dtype=dtype)
        if a.nbytes >= self.STAGED_COPY_FROM:
            # a large pageable array (a reanalysis wind series): through the ring of pinned buffers, at the bus rate whatever
            # state its pages are in (lc_copy_to_device; a first-touch pageable copy runs at a quarter of it)
            t = torch.empty(a.shape, dtype=getattr(torch, np.dtype(dtype).name), device=self.device)
            self._use_current_stream()
            _capi.check(self.lib.lc_copy_to_device(self.ctx, C.c_void_p(t.data_ptr()), a.ctypes.data_as(C.c_void_p), a.nbytes), self.lib)
            return t
        return torch.from_numpy(a).to(self.device).contiguous()

    def to_host(self, t) -> np.ndarray:
        """A device tensor as a numpy array (results of the drop-in surface); large ones through the staging ring."""
        t = t.detach()
        if not t.is_cuda or t.numel() * t.element_size() < self.STAGED_COPY_FROM:
            return t.cpu().numpy()
        t = t.contiguous()
        out = np.empty(tuple(t.shape), dtype=np.dtype(str(t.dtype).replace("torch.", "")))
        self._use_current_stream()
        _capi.check(self.lib.lc_copy_to_host(self.ctx, out.ctypes.data_as(C.c_void_p), C.c_void_p(t.data_ptr()), out.nbytes), self.lib)
        return out

    def _empty(self, shape, dtype):
        t = self.torch.empty(shape, dtype=getattr(self.torch, np.dtype(dtype).name), device=self.device)
        if self._poison and t.is_floating_point():
            # LCS_DEBUG_POISON=1 (read once, at Engine creation): every buffer the engine allocates starts as NaN instead of
            # whatever the caching allocator hands back -- typically the previous call's identical results, which would make
            # an element that a kernel forgot to write look right.  The GPU suite runs green with it.
            t.fill_(float("nan"))
        return t

    @staticmethod
    def _ptr(t):
        return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)

    # ------------------------------------------------------------------ field
    def prepare_field(self, u, v, lat_f, lon_f, interp_order: int = 1, dtype=None, fuse_levels=None,
                      lin_image=None, ext_image=None) -> PackedField:
        """Upload (if needed) and pack a wind series.  u, v: (nt, ny_f, nx_f).

        ``lin_image``: build the order-1 image too.  Default (None): only where a kernel reads it -- float32 at
        ``interp_order=1``.  Everywhere else the raw planes themselves are the order-1 source (``lc_advect_ex``: the
        pole seed rows at any order, LCS/tools.py:31-39, and in float64 the Euler sample): the field keeps a reference to
        the device copies of ``u`` and ``v`` instead of a second, interleaved copy, the pack writes a third (order 1) to a
        fifth (order 3) fewer bytes, and results are bit-identical either way.

        ``ext_image`` (float64 at ``interp_order=1`` with ``fuse_levels``): False = do not build the fused-level image
        either -- the kernels form ``2 F[t] - F[t+1]`` from the raw planes node by node (``lc_advect_args.fuse_levels_raw``;
        the same expression, bit-identical results): such a field needs NO pack at all.  Default: see ``EXT_IMAGE_F64``.
        At ``interp_order=3`` (float64): False = the kernels form the fused-level coefficients ``2 cub[t] - cub[t+1]`` from
        the coefficient image node by node (bit-identical too): the pack is the two prefilter sweeps and the pads, nothing
        more.  Default: see ``EXT_IMAGE_F64_O3``.

        ``fuse_levels``: also build ext[t] = 2 F[t] - F[t+1] so each SETTLS iteration takes one
        gather instead of two (interpolation is linear in the field => the same value up to rounding).
        Default: on, for float32 and -- since round 3 -- float64 (orders 1 and 3; float64 positions move by
        <= 1e-10 degrees against the reference's operation order on config 2, inside the 1e-9 degrees the float64
        parity tests state).  ``fuse_levels=False`` keeps numpy / scipy's exact operation order in float64
        (two samples per iteration, true divisions, scipy's tap sum): results equal to the CPU oracle's to
        ~1e-13 degrees, at 1.4x the time."""
        if interp_order not in (1, 2, 3, 4, 5):
            raise ValueError(f"interp_order {interp_order} unsupported (scipy's spline orders 1..5; "
                             "0 fails in the reference too, LCS/tools.py:24-30)")
        lat_f, lon_f = np.asarray(lat_f), np.asarray(lon_f)
        dtype = np.dtype(dtype or common_dtype(u, v, lat_f, lon_f))
        wind_f32 = dtype == np.float64 and common_dtype(u, v) == np.float32 and common_dtype(lat_f, lon_f) != np.float32
        nt, ny_f, nx_f = _check_grid(u, v, lat_f, lon_f, "field")
        plan = field_plan(dtype, wind_f32, interp_order, nt, fuse_levels, lin_image, ext_image, self.EXT_IMAGE_F64, self.EXT_IMAGE_F64_O3)
        if plan.refusal:
            raise ValueError(plan.refusal)
        self._use_current_stream()
        field, ud, vd = self._planned_field(plan, u, v, lat_f, lon_f, dtype, nt, ny_f, nx_f)
        for code, order, image, with_ext in plan.packs:
            if code == _capi.LC_F32 and order == 1 and image == "lin" and with_ext and nt - 1 > self.DEFER_FIRST_LEVELS:
                # the series is longer than the first launch of a fused advect call reaches: the first levels now, the rest
                # inside the launches of that call (PackedField.pending; a context with deferring switched off packs it all)
                if self._pending is not None:
                    self._pending.check()      # (the call below completes it, from its planes as they are now)
                _capi.check(self.lib.lc_field_pack_deferred(self.ctx, self._ptr(ud), self._ptr(vd), nt, ny_f, nx_f,
                                                            self.DEFER_FIRST_LEVELS, self._ptr(field.lin), self._ptr(field.ext)), self.lib)
                self._pending = None
                if self.lib.lc_ctx_pack_pending(self.ctx):
                    field.pending = self._pending = PendingPack(self, ud, vd, field.lin, field.ext)
                continue
            _capi.check(self.lib.lc_field_pack(self.ctx, self._ptr(ud), self._ptr(vd), code, nt, ny_f, nx_f, order,
                                               self._ptr(getattr(field, image) if image else None),
                                               self._ptr(field.ext if with_ext else None)), self.lib)
        return field

    DEFER_FIRST_LEVELS = 32   # the default level chunk (lcplan::chunk_for_k): what launch 0 of a chunked call reads

    def _pack_settled(self, field):
        """After a call that may have completed the pending pack: its tensors are dropped, by the engine and by the field."""
        if self._pending is not None:
            self._pending.live()
        if field.pending is not None and not field.pending.spoiled and not field.pending.live():
            field.pending = None

    def _planned_field(self, plan: FieldPlan, u, v, lat_f, lon_f, dtype, nt, ny_f, nx_f):
        """``(field, u, v)``: the planes on the device and the field of ``plan`` with its images allocated, not yet packed."""
        ud, vd = self.to_device(u, plan.upload), self.to_device(v, plan.upload)
        images = {k: self._empty((self.lib.lc_packed_elems(levels, ny_f, nx_f),), np.float32 if k == "lin32" else dtype)
                  for k, levels in plan.images.items()}
        field = PackedField.on_grid(lat_f, lon_f, dtype, nt, ny_f, nx_f, wind_f32=plan.wind_f32, order=plan.order,
                                    fuse_raw=plan.fuse_raw, **images, **dict(zip(plan.planes, (ud, vd))))
        return field, ud, vd

    # ------------------------------------------------------------------ global pre-processing (LCS.py:105-118)
    def regrid(self, u, lat, lon, lats, lons):
        """``u.interp(linear)`` onto (lats, lons) with nearest fill outside the source range (LCS/LCS.py:107-114).
        u: (nt, nlat, nlon) array or device tensor.  Returns a float64 device tensor (nt, len(lats), len(lons))."""
        dtype = common_dtype(u)
        ud = self.to_device(u, dtype)
        nt, ny_s, nx_s = (int(s) for s in ud.shape)
        c = [np.ascontiguousarray(a, dtype=np.float64) for a in (lat, lon, lats, lons)]
        if c[0].size != ny_s or c[1].size != nx_s:
            raise ValueError("coordinate lengths do not match the field")
        out = self._empty((nt, c[2].size, c[3].size), np.float64)
        self._use_current_stream()
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        _capi.check(self.lib.lc_regrid_common_grid(self.ctx, self._ptr(ud), _NP2LC[dtype], nt, ny_s, nx_s, p(c[0]), p(c[1]),
                                                   p(c[2]), int(c[2].size), p(c[3]), int(c[3].size), self._ptr(out)), self.lib)
        return out

    def spectral_truncate(self, f, T=20, gridtype="regular"):
        """Triangular truncation at total wavenumber T of fields (..., nlat, nlon), latitude ascending, on
        SPHEREPACK's equally spaced grid or (``gridtype='gaussian'``) on Gaussian latitudes (LCS/LCS.py:115-118).
        Same shape and dtype back (device tensor)."""
        dtype = common_dtype(f)
        fd = self.to_device(f, dtype)
        shape = tuple(int(s) for s in fd.shape)
        nlat, nlon = shape[-2], shape[-1]
        nb = int(np.prod(shape[:-2])) if len(shape) > 2 else 1
        out = self._empty(shape, dtype)
        self._use_current_stream()
        gt = {"regular": _capi.LC_GRID_REGULAR, "gaussian": _capi.LC_GRID_GAUSSIAN}[gridtype]
        _capi.check(self.lib.lc_spectral_truncate(self.ctx, self._ptr(fd), _NP2LC[dtype], nb, nlat, nlon, int(T), gt,
                                                  self._ptr(out)), self.lib)
        return out

    # ------------------------------------------------------------------ K1
    def advect(self, field: PackedField, seed_lat, seed_lon, timestep, SETTLS_order=0, interp_order=1,
               cyclic_xboundary=True, t0=0, nsteps=None, return_traj=False, row0=0, ny_global=None, halo=None,
               noncyclic_clamp=None, start=None, out=None, global_rows=None):
        """Departure points of the seed rows given.  Returns (x, y[, traj_x, traj_y]) device tensors.

        ``global_rows`` (instead of ``row0``): the rows given are NOT one contiguous block of the global grid but an
        ascending selection of its rows (``sharded``'s interleaved chunks: several windows concatenated); entry i is the
        global row of ``seed_lat[i]``.  Advection is per seed (LCS/trajectory.py:80-126) and the only thing the kernels
        derive from a seed's global row is whether it is one of the ``interp_order`` rows next to either pole (Q3), so
        the call is expressed through ``row0`` / ``ny_global`` values that mark exactly those rows (:meth:`pole_window`);
        a selection that holds only part of a pole's rows, or holds them anywhere but at its own ends, is refused.

        ``out=(x, y)``: write the results into these ``(ny, nx)`` tensors (may be the ``start`` tensors: in place)
        instead of allocating.

        ``start=(x, y)``: continue from these ``(ny, nx)`` positions instead of the seed grid (``lc_advect_from``):
        levels [t0, t0+a) followed by [t0+a, t0+a+b) from the first call's result equals one call over a+b levels.

        ``noncyclic_clamp`` (only with ``cyclic_xboundary=False``): see :func:`x_boundary_mode`.

        ``halo=(n_lo, n_hi)``: return ``(n_lo + ny + n_hi, nx)`` buffers with the results in the middle
        rows, so a row-sharded caller can receive its neighbours' rows in place (sharded.py)."""
        _check_order(field, interp_order)
        dtype = field.dtype
        slat = self.to_device(seed_lat, dtype)
        slon = self.to_device(seed_lon, dtype)
        ny, nx = int(slat.numel()), int(slon.numel())
        ny_global = ny if ny_global is None else int(ny_global)
        whole = int(row0) == 0 and ny == ny_global
        if global_rows is not None:
            if int(row0) != 0 or halo:
                raise ValueError("global_rows replaces row0 (and carries its own halo rows)")
            row0, ny_global = self.pole_window(global_rows, ny, ny_global, int(interp_order))
            whole = False
        nsteps = field.nt - 1 - t0 if nsteps is None else int(nsteps)
        n_lo, n_hi = halo if halo else (0, 0)
        if out is not None:
            if halo:
                raise ValueError("out= and halo= cannot be combined")
            x_buf, y_buf = out
            want = getattr(self.torch, np.dtype(dtype).name)
            for b in (x_buf, y_buf):
                if tuple(b.shape) != (ny, nx) or b.dtype != want or not b.is_contiguous() or b.device != self.device:
                    raise ValueError(f"out tensors must be contiguous ({ny}, {nx}) {np.dtype(dtype).name} tensors on {self.device}")
        else:
            x_buf = self._empty((n_lo + ny + n_hi, nx), dtype)
            y_buf = self._empty((n_lo + ny + n_hi, nx), dtype)
        x, y = x_buf[n_lo:n_lo + ny], y_buf[n_lo:n_lo + ny]
        if halo:  # rows to be received: NaN until the exchange fills them, so a skipped exchange cannot pass unnoticed
            for buf in (x_buf, y_buf):
                buf[:n_lo].fill_(float("nan"))
                buf[n_lo + ny:].fill_(float("nan"))
        traj = (self._empty((nsteps + 1, ny, nx), dtype), self._empty((nsteps + 1, ny, nx), dtype)) if return_traj else None
        if start is not None:
            start = sx, sy = tuple(self.to_device(a, dtype) for a in start)
            if tuple(sx.shape) != (ny, nx) or tuple(sy.shape) != (ny, nx):
                raise ValueError(f"start positions must be two ({ny}, {nx}) arrays")
        self._use_current_stream()
        a = self._advect_args(field, interp_order, slat, ny, slon, nx, timestep, SETTLS_order,
                              x_boundary_mode(cyclic_xboundary, noncyclic_clamp, whole), row0=row0, ny_global=ny_global,
                              start=start, t0=t0, nsteps=nsteps, out=(x, y), traj=traj)
        _capi.check(self.lib.lc_advect_ex(self.ctx, C.byref(a)), self.lib)
        self._pack_settled(field)
        if halo:
            x, y = x_buf, y_buf
        return (x, y, *traj) if return_traj else (x, y)

    @staticmethod
    def pole_window(global_rows, ny: int, ny_global: int, order: int):
        """``(row0, ny_global)`` to hand ``lc_advect`` for an ascending SELECTION of the global grid's rows, such that the
        kernels' pole rule -- local row i is a pole row iff ``row0 + i < order`` or ``row0 + i >= ny_global - order`` (Q3: the
        ``order`` rows next to either pole take the order-1 / 'constant' sample) -- marks exactly the selected rows that are
        pole rows of the real grid.  The selection must hold a pole's rows completely and as its own first / last rows, or
        not at all (``sharded.interleaved_chunks`` does: the first chunk starts at row 0, the last one ends at the last row)."""
        g = np.asarray(global_rows, dtype=np.int64)
        if g.shape != (ny,) or (ny > 1 and not np.all(np.diff(g) > 0)) or g[0] < 0 or g[-1] >= ny_global:
            raise ValueError(f"global_rows: {ny} ascending row indices inside [0, {ny_global})")
        is_pole = (g < order) | (g >= ny_global - order)
        row0 = 0 if g[0] < order else order
        nyg = row0 + ny + (0 if g[-1] >= ny_global - order else order)
        i = np.arange(ny) + row0
        if not np.array_equal((i < order) | (i >= nyg - order), is_pole):
            raise ValueError("global_rows: the selection holds part of a pole's rows, or holds them elsewhere than at its ends")
        return int(row0), int(nyg)

    def advect_batch(self, field: PackedField, seed_lat, seed_lon, timestep, n_members: int, nsteps: int, SETTLS_order=0,
                     interp_order=1, cyclic_xboundary=True, t0=0, t0_stride=1, start=None, out=None):
        """Departure points of an ENSEMBLE of start times over one seed grid (``lc_advect_batch``): member ``m`` runs
        ``nsteps`` steps from time level ``t0 + m * t0_stride``.  Returns ``(x, y)`` of shape ``(n_members, ny, nx)``.
        One launch per level chunk covers every member (:meth:`set_level_chunk`); each member's result equals
        ``advect(t0=t0 + m * t0_stride, nsteps=nsteps)`` bit for bit.  ``start`` / ``out``: ``(n_members, ny, nx)``
        tensors to continue from / write into (may be the same)."""
        _check_order(field, interp_order)
        if not cyclic_xboundary:
            raise ValueError("advect_batch: the reference's non-cyclic clamp is decided per member; call advect for each")
        dtype = field.dtype
        slat, slon = self.to_device(seed_lat, dtype), self.to_device(seed_lon, dtype)
        ny, nx, n = int(slat.numel()), int(slon.numel()), int(n_members)
        want = getattr(self.torch, np.dtype(dtype).name)

        def chk(t, what):
            if tuple(t.shape) != (n, ny, nx) or t.dtype != want or not t.is_contiguous() or t.device != self.device:
                raise ValueError(f"{what} tensors must be contiguous ({n}, {ny}, {nx}) {np.dtype(dtype).name} tensors on {self.device}")
            return t
        x, y = (chk(t, "out") for t in out) if out is not None else (self._empty((n, ny, nx), dtype), self._empty((n, ny, nx), dtype))
        sx, sy = (chk(t, "start") for t in start) if start is not None else (None, None)
        self._use_current_stream()
        a = self._advect_args(field, interp_order, slat, ny, slon, nx, timestep, SETTLS_order, _capi.LC_X_CYCLIC,
                              start=(sx, sy), t0=t0, nsteps=nsteps, n_members=n, t0_stride=t0_stride, out=(x, y))
        _capi.check(self.lib.lc_advect_ex(self.ctx, C.byref(a)), self.lib)
        return x, y

    def _advect_args(self, field, interp_order, slat, ny, slon, nx, timestep, K, xmode, *, row0=0, ny_global=None, start=None,
                     t0=0, nsteps, n_members=1, t0_stride=0, out, traj=None) -> "_capi.AdvectArgs":
        """``lc_advect_args`` of one call on ``field``: the borrowed planes checked, what the call's source (:func:`call_source`)
        needs made, then the structure, filled here and nowhere else.  ``start``, ``out``, ``traj``: ``(x, y)`` pairs of tensors."""
        self._check_planes(field)
        pack = field.pending
        if pack is not None and pack.engine is self and pack.live():
            pack.check()           # this context's own pending pack: lc_advect_ex carries or completes it
        elif pack is not None:
            pack.complete()        # another engine's: whole images before this context reads them (refused if it was spoiled)
            field.pending = None
        src = call_source(field, interp_order, xmode)
        if src.planes64:
            self._planes64(field)
        if src.lin:
            self._ensure_lin(field, interp_order)
        p = lambda t: t.data_ptr() if t is not None else None
        (sx, sy), (tx, ty) = start or (None, None), traj or (None, None)
        return _capi.AdvectArgs(
            struct_size=C.sizeof(_capi.AdvectArgs), **{arg: p(field.image(name)) for arg, name in src.buffers.items()},
            dtype=src.dtype, nt=field.nt, ny_f=field.ny_f, nx_f=field.nx_f, lat_min=field.lat_min, lat_max=field.lat_max,
            lon_min=field.lon_min, lon_max=field.lon_max, seed_lat_dev=p(slat), ny=int(ny), seed_lon_dev=p(slon), nx=int(nx),
            row0=int(row0), ny_global=int(ny if ny_global is None else ny_global), x_start=p(sx), y_start=p(sy),
            timestep=float(timestep), settls_order=int(K), interp_order=int(interp_order), cyclic_x=int(xmode), t0=int(t0),
            nsteps=int(nsteps), n_members=int(n_members), t0_stride=int(t0_stride), x_out=p(out[0]), y_out=p(out[1]),
            traj_x=p(tx), traj_y=p(ty), fuse_levels_raw=src.fuse_levels_raw)

    def _planes64(self, field: PackedField):
        """A wind_f32 field prepared at order 1 keeps its wind float32; the float64 planes (the order-1 source of every other
        call form: lc_advect's LC_F64_WIND_F32 with the reference's outer-product clamp, :meth:`sample`) are made here, once."""
        if field.u is None and field.u32 is not None:
            field.u, field.v = self.to_device(field.u32, field.dtype), self.to_device(field.v32, field.dtype)
            field.planes_version = (field.u._version, field.v._version)

    @staticmethod
    def _check_planes(field: PackedField):
        """The borrowed wind planes (``u`` / ``v``, and the float32 ``u32`` / ``v32`` of a float32 wind on float64 coordinates)
        must not have been written in place since ``prepare_field`` (a time loop refilling its buffers): the kernels read them
        live (pole rows, Euler samples) next to images packed from their old values; refused by the tensors' version counters.  The first thing :meth:`_advect_args` and :meth:`sample` do."""
        for a, b, stamp in ((field.u, field.v, field.planes_version), (field.u32, field.v32, field.planes32_version)):
            if a is not None and stamp is not None and (a._version, b._version) != stamp:
                raise RuntimeError("the wind tensors given to prepare_field were modified in place afterwards: the field's packed "
                                   "images no longer match them (prepare the field again, or pass copies)")

    def _ensure_lin(self, field: PackedField, interp_order: int):
        """The order-1 source of a call on ``field``, checked (:meth:`_check_planes`) and -- where it is an image that does not
        exist yet -- built.  A float32 field prepared for another order and now used at order 1 ("order 1 is always
        available"): its kernels read the order-1 image's 16-byte node pairs, so the image is packed here, once, and kept on
        the field (``advect`` and ``sample`` alike).  Everywhere else the raw planes ``field.u`` / ``field.v`` are the source."""
        self._check_planes(field)
        if field.image("lin") is None and field.dtype == np.dtype(np.float32) and interp_order == 1:
            field.lin = self._empty((self.lib.lc_packed_elems(field.nt, field.ny_f, field.nx_f),), field.dtype)
            self._use_current_stream()
            _capi.check(self.lib.lc_field_pack(self.ctx, self._ptr(field.u), self._ptr(field.v), _NP2LC[field.dtype], field.nt,
                                               field.ny_f, field.nx_f, 1, self._ptr(field.lin), None), self.lib)

    def sample(self, field: PackedField, pos_x, pos_y, level=0, interp_order=1, row0=0, ny_global=None):
        """tools.xr_map_coordinates for (u, v) of one time level at positions (ny, nx) in degrees.

        Positions that are not finite (``lc_sample`` in include/lcs_hip.h; every order, both dtypes): on an interior
        ('wrap') row a NaN or infinite coordinate gives NaN; on one of the first / last ``interp_order`` global rows
        ('constant') an infinite coordinate is outside the field and gives exactly 0, a NaN coordinate gives NaN unless the
        other coordinate is outside.  The finite positions of the same call are not affected.  scipy itself answers 0 for a
        NaN coordinate (an undefined float-to-integer cast); this departs from it on purpose."""
        _check_order(field, interp_order)
        self._check_planes(field)
        self._planes64(field)
        self._ensure_lin(field, interp_order)
        dtype = field.dtype
        px, py = self.to_device(pos_x, dtype), self.to_device(pos_y, dtype)
        ny, nx = (int(s) for s in px.shape)
        ny_global = ny if ny_global is None else int(ny_global)
        ou, ov = self._empty((ny, nx), dtype), self._empty((ny, nx), dtype)
        self._use_current_stream()
        _capi.check(self.lib.lc_sample_raw(
            self.ctx, self._ptr(field.lin), self._ptr(field.cub if interp_order != 1 else None), self._ptr(field.u),
            self._ptr(field.v), _NP2LC[dtype],
            field.nt, field.ny_f, field.nx_f, field.lat_min, field.lat_max, field.lon_min, field.lon_max, int(level),
            self._ptr(px), self._ptr(py), ny, nx, int(row0), ny_global, int(interp_order), self._ptr(ou),
            self._ptr(ov)), self.lib)
        return ou, ov

    # ------------------------------------------------------------------ tracers along trajectories
    TRACER_RING_BYTES = 2 << 30   # cap of advect_tracer's scratch ring of positions (mean-only cyclic calls)

    def last_tracer_kernel(self) -> str:
        """Name of the kernel the last tracer sample launched (``lc_ctx_last_tracer_kernel``)."""
        return self.lib.lc_ctx_last_tracer_kernel(self.ctx).decode()

    def prepare_tracer(self, c1, c2=None, lat_f=None, lon_f=None, interp_order: int = 1, dtype=None) -> PackedTracer:
        """Upload (if needed) and pack one or two tracers ``(nt, ny_f, nx_f)`` on the wind's grid for sampling along
        trajectories.  Only what sampling reads is built: float32 at order 1 the order-1 image, float64 at order 1
        nothing (the planes are sampled), orders 2..5 the coefficient image of that order (the planes serve the pole
        rows).  ``dtype``: the wind field's compute dtype (``PackedField.dtype``); default float32 only if every input is."""
        if interp_order not in (1, 2, 3, 4, 5):
            raise ValueError(f"interp_order {interp_order} unsupported (scipy's spline orders 1..5)")
        lat_f, lon_f = np.asarray(lat_f), np.asarray(lon_f)
        dtype = np.dtype(dtype or common_dtype(c1, c2, lat_f, lon_f))
        nt, ny_f, nx_f = _check_grid(c1, c2, lat_f, lon_f, "tracer")
        d1 = self.to_device(c1, dtype)
        d2 = self.to_device(c2, dtype) if c2 is not None else d1
        img = None
        self._use_current_stream()
        if interp_order != 1 or dtype == np.dtype(np.float32):
            img = self._empty((self.lib.lc_packed_elems(nt, ny_f, nx_f),), dtype)
            _capi.check(self.lib.lc_field_pack(self.ctx, self._ptr(d1), self._ptr(d2), _NP2LC[dtype], nt, ny_f, nx_f,
                                               int(interp_order), self._ptr(img), None), self.lib)
        return PackedTracer.on_grid(lat_f, lon_f, dtype, nt, ny_f, nx_f, c1=d1, c2=d2, two=c2 is not None, order=int(interp_order),
                                    lin=img if interp_order == 1 else None, cub=img if interp_order != 1 else None)

    def sample_tracer(self, tracer: PackedTracer, traj_x, traj_y, level0=0, interp_order=1, row0=0, ny_global=None,
                      values=True, sums=None, mean_count=None):
        """``lc_tracer_sample`` on trajectory entries ``traj_x / traj_y`` ``(n_levels, ny, nx)`` (device tensors of the
        tracer's dtype): entry j at field level ``level0 + j``.  Returns ``(c1, c2)`` per-entry values (``values``; c2
        None for one tracer) and ``(mean1, mean2)`` (when ``mean_count`` is given: sum / mean_count).  ``sums``: float64
        ``(ntracers, ny, nx)`` running sums the entries are added to (carried between calls)."""
        _check_order(tracer, interp_order)
        dtype = tracer.dtype
        want = getattr(self.torch, dtype.name)
        if traj_x.dtype != want or traj_y.dtype != want or tuple(traj_x.shape) != tuple(traj_y.shape) or traj_x.dim() != 3 \
                or not (traj_x.is_contiguous() and traj_y.is_contiguous()):
            raise ValueError(f"trajectories must be two contiguous (n_levels, ny, nx) {dtype.name} device tensors")
        nl, ny, nx = (int(s) for s in traj_x.shape)
        ny_global = ny if ny_global is None else int(ny_global)
        c1 = self._empty((nl, ny, nx), dtype) if values else None
        c2 = self._empty((nl, ny, nx), dtype) if values and tracer.two else None
        m1 = m2 = None
        if mean_count is not None:
            m1 = self._empty((ny, nx), dtype)
            m2 = self._empty((ny, nx), dtype) if tracer.two else None
        p = lambda t: t.data_ptr() if t is not None else None
        a = _capi.TracerArgs(
            struct_size=C.sizeof(_capi.TracerArgs), tracer_lin=p(tracer.lin), tracer_cub=p(tracer.cub if interp_order != 1 else None),
            c1_raw=p(tracer.c1), c2_raw=p(tracer.c2), dtype=_NP2LC[dtype], nt=tracer.nt, ny_f=tracer.ny_f, nx_f=tracer.nx_f,
            lat_min=tracer.lat_min, lat_max=tracer.lat_max, lon_min=tracer.lon_min, lon_max=tracer.lon_max, ny=ny, nx=nx,
            row0=int(row0), ny_global=ny_global, interp_order=int(interp_order), traj_x=p(traj_x), traj_y=p(traj_y),
            level0=int(level0), n_levels=nl, c1_out=p(c1), c2_out=p(c2),
            sum1=p(sums[0]) if sums is not None else None, sum2=p(sums[1]) if sums is not None and tracer.two else None,
            mean1_out=p(m1), mean2_out=p(m2), mean_count=int(mean_count or 0))
        if interp_order == 1 and dtype == np.dtype(np.float32) and tracer.lin is None:
            raise ValueError("float32 at interp_order=1 samples the order-1 image: prepare the tracer at order 1")
        self._use_current_stream()
        _capi.check(self.lib.lc_tracer_sample(self.ctx, C.byref(a)), self.lib)
        return (c1, c2), (m1, m2)

    def advect_tracer(self, field: PackedField, tracer: PackedTracer, seed_lat, seed_lon, timestep, SETTLS_order=0,
                      interp_order=1, cyclic_xboundary=True, t0=0, nsteps=None, return_traj=False, tracer_traj=False,
                      row0=0, ny_global=None, noncyclic_clamp=None, ring_bytes=None):
        """:meth:`advect` plus the tracer(s) sampled along the trajectories: entry i (i = 0 .. nsteps, entry 0 = the seed
        grid) is the tracer at field level ``t0 + i`` at trajectory entry i, with the rule of tools.xr_map_coordinates at
        ``interp_order``.  Returns a dict: ``x``, ``y`` (bit-identical to :meth:`advect` without a tracer), ``mean`` (and
        ``mean2`` for two tracers): sum over the nsteps + 1 entries in float64, level order, divided by nsteps + 1 and
        rounded once; with ``return_traj`` ``traj_x`` / ``traj_y``; with ``tracer_traj`` ``c`` (and ``c2``)
        ``(nsteps + 1, ny, nx)``.

        Without trajectories asked for, a cyclic call advects in level chunks into a scratch ring of at most
        ``ring_bytes`` (default :attr:`TRACER_RING_BYTES`, 2 GiB) of positions (``lc_advect`` / ``lc_advect_from``: bit-
        identical to one call) and samples each chunk, carrying float64 sums of 8 bytes per seed and tracer.  The
        reference's non-cyclic clamp (``LC_X_CLAMP_REFERENCE_OUTER``) is decided over the whole series and cannot resume
        from given positions, so such a call materialises all nsteps + 1 entries once."""
        if tracer.dtype != field.dtype:
            raise ValueError(f"tracer dtype {tracer.dtype} differs from the field's compute dtype {field.dtype}")
        if (tracer.nt, tracer.ny_f, tracer.nx_f) != (field.nt, field.ny_f, field.nx_f) or \
                (tracer.lat_min, tracer.lat_max, tracer.lon_min, tracer.lon_max) != (field.lat_min, field.lat_max, field.lon_min, field.lon_max):
            raise ValueError("the tracer must lie on the wind's grid and time levels")
        _check_order(tracer, interp_order)
        torch = self.torch
        dtype = field.dtype
        nsteps = field.nt - 1 - t0 if nsteps is None else int(nsteps)
        slat = self.to_device(seed_lat, dtype)
        slon = self.to_device(seed_lon, dtype)
        ny, nx = int(slat.numel()), int(slon.numel())
        ny_global = ny if ny_global is None else int(ny_global)
        xmode = x_boundary_mode(cyclic_xboundary, noncyclic_clamp, int(row0) == 0 and ny == ny_global)
        ring_bytes = self.TRACER_RING_BYTES if ring_bytes is None else int(ring_bytes)
        entry_bytes = 2 * ny * nx * dtype.itemsize
        chunk = max(ring_bytes // entry_bytes - 1, 1)          # steps per ring fill
        res = {}
        kw = dict(level0=t0, interp_order=interp_order, row0=row0, ny_global=ny_global)
        if return_traj or tracer_traj or xmode == _capi.LC_X_CLAMP_REFERENCE_OUTER or nsteps <= chunk:
            x, y, tx, ty = self.advect(field, slat, slon, timestep, SETTLS_order, interp_order, cyclic_xboundary, t0, nsteps,
                                       return_traj=True, row0=row0, ny_global=ny_global, noncyclic_clamp=noncyclic_clamp)
            (c1, c2), (m1, m2) = self.sample_tracer(tracer, tx, ty, values=tracer_traj, mean_count=nsteps + 1, **kw)
            res.update(x=x, y=y, mean=m1, mean2=m2)
            if return_traj:
                res.update(traj_x=tx, traj_y=ty)
            if tracer_traj:
                res.update(c=c1, c2=c2)
            return res
        # mean only, cyclic: chunks of `chunk` steps through the ring; entry 0 of a later chunk is the previous chunk's
        # last entry (its start positions), already counted
        x, y = self._empty((ny, nx), dtype), self._empty((ny, nx), dtype)
        ring_x, ring_y = self._empty((chunk + 1, ny, nx), dtype), self._empty((chunk + 1, ny, nx), dtype)
        sums = torch.zeros((2 if tracer.two else 1, ny, nx), dtype=torch.float64, device=self.device)
        s = 0
        while s < nsteps:
            k = min(chunk, nsteps - s)
            self._use_current_stream()
            a = self._advect_args(field, interp_order, slat, ny, slon, nx, timestep, SETTLS_order, xmode, row0=row0,
                                  ny_global=ny_global, start=(x, y) if s else None, t0=t0 + s, nsteps=k, out=(x, y),
                                  traj=(ring_x[:k + 1], ring_y[:k + 1]))
            _capi.check(self.lib.lc_advect_ex(self.ctx, C.byref(a)), self.lib)
            first = 0 if s == 0 else 1
            last = s + k == nsteps
            kw["level0"] = t0 + s + first
            _, (m1, m2) = self.sample_tracer(tracer, ring_x[first:k + 1], ring_y[first:k + 1], values=False, sums=sums,
                                             mean_count=nsteps + 1 if last else None, **kw)
            s += k
        res.update(x=x, y=y, mean=m1, mean2=m2)
        return res

    # ------------------------------------------------------------------ K3
    def sigma(self, x_dep, y_dep, seed_lat_rows, dlat, dlon, ny_global=None, in_row0=0, out_row0=None,
              n_out_rows=None, fd_fp32_cast=True, tensor_layout="reference"):
        """sigma_max for rows [out_row0, out_row0+n_out_rows) of a global grid, from the
        departure rows [in_row0, in_row0+x_dep.shape[0]) (which must include the 2-row halo)."""
        torch = self.torch
        dtype = np.dtype(str(x_dep.dtype).replace("torch.", "")) if isinstance(x_dep, torch.Tensor) \
            else common_dtype(x_dep, y_dep)
        xd = self.to_device(x_dep, dtype)
        yd = self.to_device(y_dep, dtype)
        n_in, nx = (int(s) for s in xd.shape)
        slat = self.to_device(seed_lat_rows, dtype)
        if slat.numel() != n_in:
            raise ValueError("seed_lat_rows must have one latitude per input row")
        ny_global = n_in if ny_global is None else int(ny_global)
        out_row0 = in_row0 if out_row0 is None else int(out_row0)
        n_out_rows = n_in if n_out_rows is None else int(n_out_rows)
        sig = self._empty((n_out_rows, nx), dtype)
        self._use_current_stream()
        _capi.check(self.lib.lc_sigma(self.ctx, self._ptr(xd), self._ptr(yd), _NP2LC[dtype], int(in_row0), n_in, nx,
                                      ny_global, self._ptr(slat), float(dlat), float(dlon), int(bool(fd_fp32_cast)),
                                      _LAYOUTS[tensor_layout], out_row0, n_out_rows, self._ptr(sig)), self.lib)
        return sig

    def flowmap_gradient(self, x_dep, y_dep, seed_lat, dlat, dlon, fd_fp32_cast=True):
        """The (9, ny, nx) def_tensor of LCS.flowmap_gradient (LCS/LCS.py:195-223) as a device tensor."""
        torch = self.torch
        dtype = np.dtype(str(x_dep.dtype).replace("torch.", "")) if isinstance(x_dep, torch.Tensor) \
            else common_dtype(x_dep, y_dep)
        xd = self.to_device(x_dep, dtype)
        yd = self.to_device(y_dep, dtype)
        ny, nx = (int(s) for s in xd.shape)
        slat = self.to_device(seed_lat, dtype)
        out = self._empty((9, ny, nx), dtype)
        self._use_current_stream()
        _capi.check(self.lib.lc_flowmap_gradient(self.ctx, self._ptr(xd), self._ptr(yd), _NP2LC[dtype], ny, nx,
                                                 self._ptr(slat), float(dlat), float(dlon), int(bool(fd_fp32_cast)),
                                                 self._ptr(out)), self.lib)
        return out

    def index_derivative(self, a, dim, isglobal=True):
        """tools.fourth_order_derivative(a, dim, isglobal) (LCS/tools.py:190-245); dtype preserved."""
        torch = self.torch
        dtype = np.dtype(str(a.dtype).replace("torch.", ""))
        if dtype not in _NP2LC:
            raise ValueError(f"dtype {dtype} unsupported (float32 / float64)")
        ad = self.to_device(a, dtype)
        ny, nx = (int(s) for s in ad.shape)
        out = self._empty((ny, nx), dtype)
        self._use_current_stream()
        _capi.check(self.lib.lc_fourth_order_derivative(self.ctx, self._ptr(ad), _NP2LC[dtype], ny, nx, int(dim),
                                                        int(bool(isglobal)), self._ptr(out)), self.lib)
        return out

    def ridge_classify(self, hxx, hxy, hyy, gx, gy, tolerance, return_eigvec=False):
        """Per-point step of tools.find_ridges_spherical_hessian (LCS/tools.py:99-138).
        Returns (mask, eigmin, dt) float64 device tensors shaped like the inputs, plus -- with
        ``return_eigvec`` -- the reference's row-indexed eigenvector as a ``(2, *shape)`` tensor."""
        t = [self.to_device(a, np.float64) for a in (hxx, hxy, hyy, gx, gy)]
        shape = tuple(t[0].shape)
        n = int(t[0].numel())
        mask, eigmin, dt = (self._empty(shape, np.float64) for _ in range(3))
        vec = self._empty((2,) + shape, np.float64) if return_eigvec else None
        self._use_current_stream()
        _capi.check(self.lib.lc_ridge_classify(self.ctx, *(self._ptr(a) for a in t), n, float(tolerance),
                                               self._ptr(mask), self._ptr(eigmin), self._ptr(dt),
                                               self._ptr(vec) if return_eigvec else None), self.lib)
        return (mask, eigmin, dt, vec) if return_eigvec else (mask, eigmin, dt)

    _RIDGE_PLANES = ("mask", "eigmin", "dt", "eigvec", "grad")

    @staticmethod
    def ridge_metric(lat, lon):
        """``(dx, dy)`` of tools.derivative_spherical_coords (LCS/tools.py:254-256) for ascending coordinates in degrees: metres
        per longitude step of every row (an array, in the coordinates' dtype as numpy evaluates it) and per latitude step."""
        y = lat * np.pi / 180                                                   # tools.py:254
        dx = (np.pi / 180) * (lon[1] - lon[0]) * 6371000 * np.cos(y)            # tools.py:255
        dy = (np.pi / 180) * (lat[1] - lat[0]) * 6371000                        # tools.py:256
        return dx, float(dy)

    def last_ridges_kernel(self) -> str:
        """Names of the kernels the last :meth:`ridges_batch` call launched (``lc_ctx_last_ridges_kernel``), joined by ``+``."""
        return self.lib.lc_ctx_last_ridges_kernel(self.ctx).decode()

    def ridges_batch(self, f, lat, lon, sigma=.5, tolerance=0.0005e-3, isglobal=True, want=("mask", "eigmin")) -> dict:
        """tools.find_ridges_spherical_hessian (LCS/tools.py:52-155) for a stack of planes in one call (``lc_ridges_batch``:
        two Gaussian launches and one fused Hessian / classification launch for all of them).  ``f``: ``(ny, nx)`` or
        ``(n, ny, nx)``, an array or a device tensor (used where it lies: nothing goes to the host), ``lat`` / ``lon`` its
        ascending coordinates in degrees (tools.py:70-71 sorts before it gets here).  ``sigma``: the Gaussian's width in grid
        steps, applied to every plane on its own; ``None`` or ``<= 0``: no smoothing.  ``isglobal``: cyclic longitude stencil.

        Returns a dict of float64 device tensors for the names in ``want``: ``mask`` (1 on a ridge, else 0), ``eigmin`` (the
        Hessian eigenvalue of largest magnitude) and ``dt`` (the raw eigenvector / gradient product) shaped like ``f``;
        ``eigvec`` (the row-indexed eigenvector, unmasked) and ``grad`` (``ddadx, ddady``) with a dimension of 2 in front of
        ``(ny, nx)``.  Plane ``m`` of each equals the per-plane chain (:meth:`gaussian_filter`, :meth:`index_derivative`,
        :meth:`ridge_classify`) on plane ``m`` bit for bit."""
        want = tuple(want)
        bad = [w for w in want if w not in self._RIDGE_PLANES]
        if bad or not want:
            raise ValueError(f"want {want!r}: a non-empty subset of {self._RIDGE_PLANES}")
        torch = self.torch
        fd = self.to_device(f, np.float64)
        if fd.dim() not in (2, 3) or fd.numel() == 0:
            raise ValueError("f: a plane (ny, nx) or a stack of planes (n, ny, nx), none of them empty")
        shape = tuple(int(s) for s in fd.shape)
        ny, nx = shape[-2:]
        n = shape[0] if len(shape) == 3 else 1
        lat, lon = np.asarray(lat), np.asarray(lon)
        if lat.shape != (ny,) or lon.shape != (nx,):
            raise ValueError("lat / lon: one latitude per row and one longitude per column of f")
        dx, dy = self.ridge_metric(lat, lon)
        dx = self.to_device(dx, np.float64)
        smooth = sigma is not None and float(sigma) > 0
        out = {}
        for k in want:
            out[k] = self._empty((*shape[:-2], 2, ny, nx) if k in ("eigvec", "grad") else shape, np.float64)
        a = _capi.RidgesArgs(struct_size=C.sizeof(_capi.RidgesArgs))
        a.f, a.ny, a.nx, a.n_members = fd.data_ptr(), ny, nx, n
        a.dx_dev, a.dy, a.sigma, a.tolerance = dx.data_ptr(), dy, float(sigma) if smooth else 0.0, float(tolerance)
        a.isglobal = int(bool(isglobal))
        work = None
        if smooth:
            work = torch.empty((max(1, int(self.lib.lc_ridges_work_elems(ny, nx, n))),), dtype=torch.float64, device=self.device)
            a.work_dev = work.data_ptr()
        for k in self._RIDGE_PLANES:
            setattr(a, k + "_out", out[k].data_ptr() if k in out else None)
        self._use_current_stream()
        _capi.check(self.lib.lc_ridges_batch(self.ctx, C.byref(a)), self.lib)
        return out

    # ------------------------------------------------------------------ connected components of a mask (filter_ridges)
    COMPONENT_PROPS =("area", "mean_intensity", "max_intensity", "min_intensity", "major_axis_length", "minor_axis_length")

    def _planes(self, a, dtype=None):
        """``a`` (2-D, or 3-D with a leading member dimension) on the device as ``(n_members, ny, nx)``; ``dtype`` None: its own
        (float32 / float64 kept, anything else float64)."""
        if dtype is None:
            dtype = np.dtype(str(a.dtype).replace("torch.", ""))
            dtype = dtype if dtype in _NP2LC else np.dtype(np.float64)
        t = self.to_device(a, dtype)
        if t.dim() not in (2, 3) or t.numel() == 0:
            raise ValueError("a plane (ny, nx) or a stack of planes (n_members, ny, nx), none of them empty")
        return t if t.dim() == 3 else t[None]

    def label_components(self, mask, connectivity=2, cyclic=False):
        """Connected components of ``mask`` (``lc_label_components``): ``(labels, counts)``.

        A pixel is foreground when it is ``!= 0`` and not NaN.  ``labels``: int32 device tensor shaped like ``mask`` --
        ``(ny, nx)``, or ``(n_members, ny, nx)``, every plane labelled on its own in the same launches -- 0 on background,
        else ``1..N`` in the order of each component's first pixel in raster order: ``scipy.ndimage.label(mask,
        generate_binary_structure(2, connectivity))``'s numbering.  ``counts``: int32 ``(n_members,)``, N of each plane.
        ``cyclic``: the last column is the western neighbour of the first (a global longitude axis)."""
        m = self._planes(mask)
        n, ny, nx = (int(s) for s in m.shape)
        labels = self.torch.empty((n, ny, nx), dtype=self.torch.int32, device=self.device)
        counts = self.torch.empty((n,), dtype=self.torch.int32, device=self.device)
        work = self.torch.empty((max(1, int(self.lib.lc_label_work_elems(ny, nx, n))),), dtype=self.torch.int32, device=self.device)
        self._use_current_stream()
        _capi.check(self.lib.lc_label_components(self.ctx, self._ptr(m), _NP2LC[np.dtype(str(m.dtype).replace("torch.", ""))], ny, nx, n,
                                                 int(connectivity), int(bool(cyclic)), self._ptr(labels), self._ptr(counts),
                                                 self._ptr(work)), self.lib)
        return (labels if len(mask.shape) == 3 else labels[0]), counts

    def component_sums(self, labels, counts, intensity=None, cyclic=False, n_max=None):
        """``lc_component_sums``: the exact per-component sums :meth:`component_props` is computed from, as a dict of device
        tensors ``(n_members, n_max)`` -- ``root`` (int32, first pixel), ``area`` (int64), ``moments`` (int64, ``(5, n_members,
        n_max)``: sums of dr, dc, dr^2, dr dc, dc^2 about the root pixel) and, with an ``intensity``, ``sum``, ``max``, ``min``
        (float64).  ``n_max`` None: the largest count, read back from the device (one synchronisation)."""
        torch = self.torch
        lab = labels if labels.dim() == 3 else labels[None]
        if lab.dtype != torch.int32 or not lab.is_contiguous():
            raise ValueError("labels: the int32 tensor label_components returned")
        n, ny, nx = (int(s) for s in lab.shape)
        if n_max is None:
            n_max = int(counts.max().item())
        n_max = max(1, int(n_max))
        inten = None
        if intensity is not None:
            inten = self._planes(intensity)
            if tuple(inten.shape) != (n, ny, nx):
                raise ValueError("intensity and labels differ in shape")
        out = {"root": torch.empty((n, n_max), dtype=torch.int32, device=self.device),
               "area": torch.empty((n, n_max), dtype=torch.int64, device=self.device),
               "moments": torch.empty((5, n, n_max), dtype=torch.int64, device=self.device)}
        if inten is not None:
            out.update({k: self._empty((n, n_max), np.float64) for k in ("sum", "max", "min")})
        a = _capi.ComponentSumsArgs(struct_size=C.sizeof(_capi.ComponentSumsArgs))
        a.labels, a.counts, a.intensity = lab.data_ptr(), counts.data_ptr(), inten.data_ptr() if inten is not None else None
        a.dtype = _NP2LC[np.dtype(str(inten.dtype).replace("torch.", ""))] if inten is not None else _capi.LC_F64
        a.ny, a.nx, a.n_members, a.cyclic_x, a.n_max = ny, nx, n, int(bool(cyclic)), n_max
        a.root_out, a.area_out, a.moments_out = (out[k].data_ptr() for k in ("root", "area", "moments"))
        if inten is not None:
            a.sum_out, a.max_out, a.min_out = (out[k].data_ptr() for k in ("sum", "max", "min"))
        self._use_current_stream()
        _capi.check(self.lib.lc_component_sums(self.ctx, C.byref(a)), self.lib)
        return out

    def component_props(self, labels, counts, intensity=None, cyclic=False):
        """Properties of every component of :meth:`label_components`' result, as a dict of float64 device tensors ``(n_max,)``
        (``(n_members, n_max)`` for a stack; ``n_max`` = the largest count; entries past a plane's own count are NaN, area 0):

        ``area`` (int64), ``mean_intensity``, ``max_intensity``, ``min_intensity`` (NaN for all three where the component holds
        a NaN; present with an ``intensity``), ``centroid`` (``(..., 2)``: row, column), ``major_axis_length``,
        ``minor_axis_length`` and ``axis_moments`` (``(..., 2)``: the ``l1, l2`` below).

        The axis lengths are DEFINED here by formula -- the one ``skimage.measure.regionprops`` documents; skimage is not at
        hand to check against: with the central moments per pixel ``a = mu_rr / area, b = mu_rc / area, c = mu_cc / area``,
        ``l1, l2 = (a + c) / 2 +- sqrt(((a - c) / 2)^2 + b^2)``, ``major = 4 sqrt(l1)``, ``minor = 4 sqrt(max(l2, 0))``, in index
        units.  The moments come from exact integer sums about each component's first pixel (``mu_rr = sum dr^2 -
        (sum dr)^2 / area``): nothing large is subtracted from anything large.  ``cyclic``: column offsets are taken the shorter
        way round, so a component that straddles the seam is measured as the one piece it is."""
        torch = self.torch
        s = self.component_sums(labels, counts, intensity, cyclic)
        nx = int(labels.shape[-1])
        area = s["area"]
        valid = area > 0
        nan = torch.full(area.shape, float("nan"), dtype=torch.float64, device=self.device)
        n = torch.where(valid, area, torch.ones_like(area)).to(torch.float64)
        sr, sc, srr, src, scc = (m.to(torch.float64) for m in s["moments"])
        a = (srr - sr * sr / n) / n
        b = (src - sr * sc / n) / n
        c = (scc - sc * sc / n) / n
        mid, rad = (a + c) / 2, torch.sqrt(((a - c) / 2) ** 2 + b * b)
        l1, l2 = mid + rad, mid - rad
        root = s["root"].clamp(min=0)
        row = torch.div(root, nx, rounding_mode="floor")
        col = (root - row * nx).to(torch.float64) + sc / n
        if cyclic:
            col = torch.remainder(col, float(nx))
        props = {"area": area,
                 "centroid": torch.where(valid[..., None], torch.stack([row.to(torch.float64) + sr / n, col], dim=-1), nan[..., None]),
                 "major_axis_length": torch.where(valid, 4 * torch.sqrt(l1), nan),
                 "minor_axis_length": torch.where(valid, 4 * torch.sqrt(l2.clamp(min=0)), nan),
                 "axis_moments": torch.where(valid[..., None], torch.stack([l1, l2], dim=-1), nan[..., None])}
        if intensity is not None:
            props.update(mean_intensity=torch.where(valid, s["sum"] / n, nan), max_intensity=s["max"], min_intensity=s["min"])
        return props if labels.dim() == 3 else {k: v[0] for k, v in props.items()}

    # ------------------------------------------------------------------ the same on the sphere
    SPHERE_PROPS = ("area", "major_axis_length", "minor_axis_length", "centroid_latitude", "centroid_longitude", "orientation",
                    "mean_intensity", "total_intensity")      # the planes of lc_component_sphere_sums' props_out, in order
    METRICS = ("index", "sphere")

    @staticmethod
    def sphere_cell_tables(lat, lon, cyclic=False):
        """``(row_weight, col_weight)``: the exact areas of the cells of a latitude-longitude grid in steradians, in separable
        form -- cell ``(r, c)`` has the area ``row_weight[r] * col_weight[c]`` on the unit sphere.  numpy on the host; no device
        is touched.  ``lat`` / ``lon``: degrees, at least two each, finite, strictly ascending, ``|lat| <= 90``.

        Latitude: the band edges are the midpoints between neighbouring latitudes, the two outer edges lie half the
        neighbouring spacing beyond the first and last latitude, and all edges are clipped to ``[-90, 90]``; ``row_weight =
        sin(top edge) - sin(bottom edge)``.  Longitude: the edges are the midpoints; without ``cyclic`` the outer edges lie half
        the neighbouring spacing out, with ``cyclic`` the first and last cell share the gap ``lon[0] + 360 - lon[-1]`` (which
        must be positive); ``col_weight`` is the width in radians.  On a global grid the weights sum to ``4 pi``."""
        lat, lon = np.asarray(lat, dtype=np.float64), np.asarray(lon, dtype=np.float64)
        if lat.ndim != 1 or lon.ndim != 1 or lat.size < 2 or lon.size < 2:
            raise ValueError("lat and lon: one-dimensional, at least two values each (a cell needs a neighbour to have a width)")
        if not (np.isfinite(lat).all() and np.isfinite(lon).all()):
            raise ValueError("lat and lon: finite degrees")
        if np.abs(lat).max() > 90.0:
            raise ValueError(f"lat: within [-90, 90] degrees, got {lat.min()!r} .. {lat.max()!r}")
        if not ((np.diff(lat) > 0).all() and (np.diff(lon) > 0).all()):
            raise ValueError("lat and lon: strictly ascending")

        def edges(x, first, last):
            e = np.empty(x.size + 1)
            e[1:-1] = (x[:-1] + x[1:]) / 2
            e[0], e[-1] = x[0] - first / 2, x[-1] + last / 2
            return e
        ey = np.clip(edges(lat, lat[1] - lat[0], lat[-1] - lat[-2]), -90.0, 90.0)
        sy = np.sin(ey * np.pi / 180)
        if cyclic:
            gap = lon[0] + 360.0 - lon[-1]
            if not gap > 0:
                raise ValueError(f"lon: with cyclic the axis must leave a gap before it closes: lon[0] + 360 - lon[-1] = {gap!r} (> 0)")
            ex = edges(lon, gap, gap)
        else:
            ex = edges(lon, lon[1] - lon[0], lon[-1] - lon[-2])
        return sy[1:] - sy[:-1], (ex[1:] - ex[:-1]) * np.pi / 180

    def component_sphere_props(self, labels, counts, lat, lon, intensity=None, cyclic=False, radius=6371000.0, n_max=None,
                               return_sums=False):
        """Properties of every label of a label map measured ON THE SPHERE (``lc_component_sphere_sums``), as a dict of
        float64 device tensors ``(n_max,)`` (``(n_members, n_max)`` for a stack; ``n_max`` None: the largest count, read back
        from the device).  ``labels``: int32, as :meth:`label_components` returns them, or any other label map with values in
        ``0..counts[m]`` -- it need not be connected.  ``lat`` ``(ny,)``, ``lon`` ``(nx,)``: degrees, as
        :meth:`sphere_cell_tables` wants them; ``cyclic`` there decides the width of the outer columns only: on the sphere a
        label that straddles the seam is in one piece without a flag.

        Node ``(r, c)`` is the unit vector ``n = (cos lat cos lon, cos lat sin lon, sin lat)`` and has the cell area ``w =
        row_weight[r] col_weight[c]`` (steradians).  With ``d = n - n(root)`` about the label's first pixel in raster order --
        nothing large is subtracted from anything large -- the device sums ``W = sum w``, ``M1 = sum w d``, ``M2 = sum w d d^T``
        and ``S = sum w v`` per label in float64; then ``m = M1 / W``, ``C = M2 / W - m m^T``, ``e1 >= e2 >= e3`` its
        eigenvalues (cyclic Jacobi, a fixed number of sweeps) and ``v`` the eigenvector of ``e1``:

        ``area`` = ``radius^2 W``; ``major_axis_length`` = ``4 radius sqrt(max(e1, 0))`` and ``minor_axis_length`` likewise of
        ``e2``: for a ridge that is small against the sphere the regionprops formula of :meth:`component_props` in the unit of
        ``radius``.  It measures CHORDS, so it saturates for planet-sized labels.  ``centroid_latitude``,
        ``centroid_longitude``: degrees, of the direction ``c = n(root) + m`` (``asin(c_z / |c|)``, ``atan2(c_y, c_x)``), NaN
        where ``|c| < 1e-6``.  ``orientation``: degrees, ``atan2(v . north, v . east)`` at the centroid folded into ``(-90,
        90]`` -- 0 zonal, 90 meridional, positive from SW to NE; NaN for a single pixel (``e1 == 0``) and where the centroid
        is.  With an ``intensity``: ``mean_intensity`` = ``S / W`` (area-weighted), ``total_intensity`` = ``radius^2 S``,
        ``max_intensity``, ``min_intensity`` (exact); a NaN in the label makes all four NaN.  Entries past a plane's count
        and labels without a pixel in the plane: ``area`` 0, everything else NaN.

        The sums are float64 atomic adds whose order is not fixed: the last bits can differ from run to run (as those of
        ``mean_intensity`` of :meth:`component_props` do).  ``return_sums``: also the raw ``root`` (int32), ``W``, ``M1``
        ``(..., 3)``, ``M2`` ``(..., 6)``: xx, xy, xz, yy, yz, zz) and, with an intensity, ``S``."""
        torch = self.torch
        cl, sl, cx, sx, radius, _, _ = self.sphere_tables(lat, lon, radius)
        rw, cw = self.sphere_cell_tables(lat, lon, cyclic)
        lab = labels if labels.dim() == 3 else labels[None]
        if lab.dtype != torch.int32 or not lab.is_contiguous():
            raise ValueError("labels: a contiguous int32 tensor (what label_components returns)")
        n, ny, nx = (int(s) for s in lab.shape)
        if (ny, nx) != (cl.size, cx.size):
            raise ValueError(f"labels {tuple(lab.shape)}: ny = len(lat) = {cl.size} and nx = len(lon) = {cx.size}")
        if n_max is None:
            n_max = int(counts.max().item())
        n_max = max(1, int(n_max))
        inten = None
        if intensity is not None:
            inten = self._planes(intensity)
            if tuple(inten.shape) != (n, ny, nx):
                raise ValueError("intensity and labels differ in shape")
        root = torch.empty((n, n_max), dtype=torch.int32, device=self.device)
        sums = self._empty((11, n, n_max), np.float64)
        props = self._empty((len(self.SPHERE_PROPS), n, n_max), np.float64)
        ext = self._empty((2, n, n_max), np.float64) if inten is not None else None
        tables = [self.to_device(t, np.float64) for t in (cl, sl, rw, cx, sx, cw)]
        a = _capi.ComponentSphereSumsArgs(struct_size=C.sizeof(_capi.ComponentSphereSumsArgs))
        a.labels, a.counts, a.intensity = lab.data_ptr(), counts.data_ptr(), inten.data_ptr() if inten is not None else None
        a.dtype = _NP2LC[np.dtype(str(inten.dtype).replace("torch.", ""))] if inten is not None else _capi.LC_F64
        a.ny, a.nx, a.n_members, a.n_max = ny, nx, n, n_max
        a.cos_lat, a.sin_lat, a.row_weight, a.cos_lon, a.sin_lon, a.col_weight = (t.data_ptr() for t in tables)
        a.radius = radius
        a.root_out, a.sums_out, a.props_out = root.data_ptr(), sums.data_ptr(), props.data_ptr()
        if inten is not None:
            a.max_out, a.min_out = ext[0].data_ptr(), ext[1].data_ptr()
        self._use_current_stream()
        _capi.check(self.lib.lc_component_sphere_sums(self.ctx, C.byref(a)), self.lib)
        out = {k: props[i] for i, k in enumerate(self.SPHERE_PROPS) if inten is not None or not k.endswith("_intensity")}
        if inten is not None:
            out.update(max_intensity=ext[0], min_intensity=ext[1])
        if return_sums:
            out.update(root=root, W=sums[0], M1=sums[1:4].permute(1, 2, 0), M2=sums[4:10].permute(1, 2, 0))
            if inten is not None:
                out["S"] = sums[10]
        return out if labels.dim() == 3 else {k: v[0] for k, v in out.items()}

    def filter_components(self, mask, intensity, criteria, thresholds, connectivity=2, cyclic=False, fill=0.0, metric='index',
                          lat=None, lon=None, radius=6371000.0):
        """``mask`` with every connected component that fails a threshold replaced by ``fill`` (background becomes ``fill``
        too): a component is kept when ``prop >= threshold`` for every ``(criterion, threshold)`` pair -- criteria from
        :attr:`COMPONENT_PROPS`, measured on ``intensity`` -- and a NaN property fails.  Label, sums and apply run on the
        device (``lc_label_components``, ``lc_component_sums``, ``lc_component_apply``); the counts are read back once in
        between, to size the per-component arrays.  Returns a device tensor shaped and typed like ``mask``.

        ``metric='index'`` (the default) measures in index units (:meth:`component_props`); ``metric='sphere'`` takes the same
        criteria names from :meth:`component_sphere_props` on the grid ``lat``, ``lon`` (degrees): ``area`` in ``radius^2``,
        the axis lengths in the unit of ``radius``, ``mean_intensity`` area-weighted."""
        criteria, thresholds = list(criteria), list(thresholds)
        if len(criteria) != len(thresholds):
            raise ValueError("criteria and thresholds differ in length")
        for k in criteria:
            if k not in self.COMPONENT_PROPS:
                raise ValueError(f"criterion {k!r}: one of {', '.join(self.COMPONENT_PROPS)}")
            if intensity is None and k.endswith("_intensity"):
                raise ValueError(f"criterion {k!r} needs an intensity")
        if metric not in self.METRICS:
            raise ValueError(f"metric {metric!r}: 'index' or 'sphere'")
        if metric == 'sphere' and (lat is None or lon is None):
            raise ValueError("metric='sphere' needs lat and lon")
        torch = self.torch
        m = self._planes(mask)
        n, ny, nx = (int(s) for s in m.shape)
        labels, counts = self.label_components(m, connectivity, cyclic)
        if metric == 'sphere':
            props = self.component_sphere_props(labels, counts, lat, lon, intensity, cyclic, radius)
        else:
            props = self.component_props(labels, counts, intensity, cyclic)
        keep = props["area"] > 0
        for k, th in zip(criteria, thresholds):
            keep = keep & (props[k] >= float(th))          # a NaN compares False
        keep = keep.to(torch.uint8).contiguous()
        out = self._empty((n, ny, nx), np.dtype(str(m.dtype).replace("torch.", "")))
        self._use_current_stream()
        _capi.check(self.lib.lc_component_apply(self.ctx, self._ptr(labels), self._ptr(m), _NP2LC[np.dtype(str(m.dtype).replace("torch.", ""))],
                                                ny, nx, n, self._ptr(keep), int(keep.shape[1]), float(fill), self._ptr(out)), self.lib)
        return out if len(mask.shape) == 3 else out[0]

    # ------------------------------------------------------------------ ridges followed through time (track_ridges)
    MAX_TRACK_REACH = _capi.LC_TRACK_MAX_REACH

    @classmethod
    def checked_track_options(cls, connectivity, reach):
        """``(connectivity, reach)`` as ints, or ``ValueError``: what ``lc_label_tracks`` would refuse, without a device."""
        if connectivity not in (1, 2):
            raise ValueError(f"connectivity {connectivity!r}: 1 (edges) or 2 (edges and corners)")
        if isinstance(reach, bool) or not isinstance(reach, (int, np.integer)) or not 0 <= reach <= cls.MAX_TRACK_REACH:
            raise ValueError(f"reach {reach!r}: an integer in 0 .. {cls.MAX_TRACK_REACH} (pixels per time step)")
        return int(connectivity), int(reach)

    def _record(self, mask):
        """``mask`` on the device as a ``(n_times, ny, nx)`` record (float32 / float64 kept, anything else float64)."""
        dtype = np.dtype(str(mask.dtype).replace("torch.", ""))
        t = self.to_device(mask, dtype if dtype in _NP2LC else np.dtype(np.float64))
        if t.dim() != 3 or t.numel() == 0:
            raise ValueError("a record (n_times, ny, nx), not empty")
        return t

    def label_tracks(self, mask, connectivity=2, cyclic=False, reach=1):
        """Space-time labels of a record of ridge masks (``lc_label_tracks``): ``(labels, count)``.

        ``mask``: ``(n_times, ny, nx)``, float32 or float64, planes in the order given; a voxel is foreground when it is
        ``!= 0`` and not NaN.  Two foreground voxels are linked when they are neighbours in one plane (``connectivity`` and
        ``cyclic`` as in :meth:`label_components`), or lie in adjacent planes at most ``reach`` pixels apart in both row and
        column (``cyclic``: the column offset the shorter way round).  A track is a connected component of that relation, so
        ridges that merge or split are ONE track.  ``labels``: int32 device tensor shaped like ``mask``, 0 on background, else
        ``1..N`` in the order of each track's first voxel in raster order -- ``scipy.ndimage.label``'s numbering on the 3-D
        array (``reach=1, connectivity=2`` is its ``generate_binary_structure(3, 3)``, ``reach=0, connectivity=1`` its
        ``(3, 1)``).  ``count``: int32 ``(1,)``, N.  One plane gives :meth:`label_components` of that plane."""
        connectivity, reach = self.checked_track_options(connectivity, reach)
        m = self._record(mask)
        n, ny, nx = (int(s) for s in m.shape)
        labels = self.torch.empty((n, ny, nx), dtype=self.torch.int32, device=self.device)
        count = self.torch.empty((1,), dtype=self.torch.int32, device=self.device)
        work = self.torch.empty((max(1, int(self.lib.lc_track_work_elems(ny, nx, n))),), dtype=self.torch.int32, device=self.device)
        self._use_current_stream()
        _capi.check(self.lib.lc_label_tracks(self.ctx, self._ptr(m), _NP2LC[np.dtype(str(m.dtype).replace("torch.", ""))], ny, nx, n,
                                             connectivity, int(bool(cyclic)), reach, self._ptr(labels), self._ptr(count),
                                             self._ptr(work)), self.lib)
        return labels, count

    def track_spans(self, labels, count, n_max=None):
        """``lc_track_spans``: per track of :meth:`label_tracks`' result, as a dict of device tensors ``(n_max,)`` -- ``first``
        and ``last`` (int32: the smallest and largest plane index the track occupies), ``duration`` (int32, ``last - first +
        1``) and ``volume`` (int64, voxels).  Entries past the count hold ``first = last = -1`` and ``duration = volume = 0``.
        ``n_max`` None: the count, read back from the device (one synchronisation)."""
        torch = self.torch
        if labels.dim() != 3 or labels.dtype != torch.int32 or not labels.is_contiguous():
            raise ValueError("labels: the int32 tensor label_tracks returned")
        n, ny, nx = (int(s) for s in labels.shape)
        if n_max is None:
            n_max = int(count[0].item())
        n_max = max(1, int(n_max))
        out = {"first": torch.empty((n_max,), dtype=torch.int32, device=self.device),
               "last": torch.empty((n_max,), dtype=torch.int32, device=self.device),
               "volume": torch.empty((n_max,), dtype=torch.int64, device=self.device)}
        a = _capi.TrackSpansArgs(struct_size=C.sizeof(_capi.TrackSpansArgs))
        a.labels, a.count = labels.data_ptr(), count.data_ptr()
        a.ny, a.nx, a.n_times, a.n_max = ny, nx, n, n_max
        a.first_out, a.last_out, a.volume_out = (out[k].data_ptr() for k in ("first", "last", "volume"))
        self._use_current_stream()
        _capi.check(self.lib.lc_track_spans(self.ctx, C.byref(a)), self.lib)
        out["duration"] = torch.where(out["first"] >= 0, out["last"] - out["first"] + 1, torch.zeros_like(out["first"]))
        return out

    def filter_tracks(self, mask, min_duration=1, min_volume=1, connectivity=2, cyclic=False, reach=1, fill=0.0):
        """``mask`` with the voxels of every track that lasts fewer than ``min_duration`` planes or holds fewer than
        ``min_volume`` voxels replaced by ``fill`` (background becomes ``fill`` too).  Label, spans and apply run on the device
        (``lc_label_tracks``, ``lc_track_spans``, and ``lc_component_apply`` on the record viewed as one plane of ``n_times *
        ny`` rows); the count is read back once in between.  Returns a device tensor shaped and typed like ``mask``."""
        torch = self.torch
        m = self._record(mask)
        n, ny, nx = (int(s) for s in m.shape)
        labels, count = self.label_tracks(m, connectivity, cyclic, reach)
        spans = self.track_spans(labels, count)
        keep = (spans["volume"] >= max(1, int(min_volume))) & (spans["duration"] >= int(min_duration))
        keep = keep.to(torch.uint8).contiguous()
        dtype = np.dtype(str(m.dtype).replace("torch.", ""))
        out = self._empty((n, ny, nx), dtype)
        self._use_current_stream()
        _capi.check(self.lib.lc_component_apply(self.ctx, self._ptr(labels), self._ptr(m), _NP2LC[dtype], n * ny, nx, 1,
                                                self._ptr(keep), int(keep.shape[0]), float(fill), self._ptr(out)), self.lib)
        return out

    # ------------------------------------------------------------------ distance to the nearest pixel of a mask
    def distance_transform(self, mask, cyclic=False, sampling=None, max_distance=None, return_nearest=False):
        """Exact Euclidean distance from every pixel to the nearest foreground pixel of ``mask`` (``lc_distance_transform``):
        ``scipy.ndimage.distance_transform_edt(~foreground, sampling=sampling)`` bit for bit, as a float64 device tensor shaped
        like ``mask`` -- ``(ny, nx)``, or ``(n_members, ny, nx)``, every plane on its own in the same launches.

        A pixel is foreground when it is ``!= 0`` and not NaN (float32 / float64 kept, any other dtype converted to float64).
        ``sampling``: the pixel spacing, a scalar or ``(sy, sx)``, default 1.  ``cyclic``: the column offset is taken the
        shorter way round a global longitude axis.  ``max_distance`` (> 0): pixels further away than that are ``+inf`` and
        nobody searches beyond it; None: unbounded.  A plane without foreground is ``+inf`` everywhere.
        ``return_nearest``: also the int32 linear index, into its plane, of the nearest foreground pixel (the smallest index
        among equally near ones; -1 where the distance is ``+inf``)."""
        if sampling is None:
            sampling = 1.0
        sy, sx = (float(s) for s in (np.broadcast_to(np.asarray(sampling, dtype=np.float64), (2,))))
        if max_distance is not None and not float(max_distance) > 0:
            raise ValueError(f"max_distance {max_distance!r}: a positive number, or None for no bound")
        m = self._planes(mask)
        n, ny, nx = (int(s) for s in m.shape)
        torch = self.torch
        dist = self._empty((n, ny, nx), np.float64)
        nearest = torch.empty((n, ny, nx), dtype=torch.int32, device=self.device) if return_nearest else None
        elems = int(self.lib.lc_distance_work_elems(ny, nx, n))
        # the call's own checks refuse what cannot be sized (a plane too large or too wide) before they touch the buffer
        work = torch.empty((max(1, elems if nx <= 16384 and ny * nx < 2 ** 31 else 1),), dtype=torch.int32, device=self.device)
        a = _capi.DistanceArgs(struct_size=C.sizeof(_capi.DistanceArgs))
        a.mask, a.dtype = m.data_ptr(), _NP2LC[np.dtype(str(m.dtype).replace("torch.", ""))]
        a.ny, a.nx, a.n_members, a.cyclic_x = ny, nx, n, int(bool(cyclic))
        a.sampling_y, a.sampling_x = sy, sx
        a.max_distance = 0.0 if max_distance is None else float(max_distance)
        a.dist_out, a.nearest_out, a.work_dev = dist.data_ptr(), nearest.data_ptr() if return_nearest else None, work.data_ptr()
        self._use_current_stream()
        _capi.check(self.lib.lc_distance_transform(self.ctx, C.byref(a)), self.lib)
        if len(mask.shape) != 3:
            dist, nearest = dist[0], nearest[0] if return_nearest else None
        return (dist, nearest) if return_nearest else dist

    # ------------------------------------------------------------------ great-circle distance to the nearest pixel of a mask
    @staticmethod
    def sphere_tables(lat, lon, radius=6371000.0, max_distance=None):
        """What :meth:`sphere_distance` hands to the device, computed with numpy on the host and checked there (no device is
        touched): ``(cos lat, sin lat, cos lon, sin lon, radius, max_chord2, max_distance)``.  ``lat`` / ``lon`` in degrees;
        ``max_chord2 = fl(c c)`` with ``c = 2 sin(max_distance / (2 radius))``, 0 where there is no bound (None, or a bound
        of half the sphere's circumference or more)."""
        lat, lon = np.asarray(lat, dtype=np.float64), np.asarray(lon, dtype=np.float64)
        if lat.ndim != 1 or lon.ndim != 1 or lat.size == 0 or lon.size == 0:
            raise ValueError("lat and lon: one-dimensional and not empty")
        if not (np.isfinite(lat).all() and np.isfinite(lon).all()):
            raise ValueError("lat and lon: finite degrees")
        if np.abs(lat).max() > 90.0:
            raise ValueError(f"lat: within [-90, 90] degrees, got {lat.min()!r} .. {lat.max()!r}")
        radius = float(radius)
        if not (radius > 0 and np.isfinite(radius)):
            raise ValueError(f"radius {radius!r}: a positive, finite number")
        chord2, bound = 0.0, 0.0
        if max_distance is not None:
            if not float(max_distance) > 0:
                raise ValueError(f"max_distance {max_distance!r}: a positive number, or None for no bound")
            if float(max_distance) < np.pi * radius:
                bound = float(max_distance)
                c = np.float64(2.0) * np.sin(np.float64(bound) / (np.float64(2.0) * np.float64(radius)))
                chord2 = float(c * c)
                if not chord2 > 0.0:
                    raise ValueError(f"max_distance {max_distance!r}: its squared chord on a sphere of radius {radius!r} underflows")
        y, x = lat * np.pi / 180, lon * np.pi / 180
        return np.cos(y), np.sin(y), np.cos(x), np.sin(x), radius, chord2, bound

    def sphere_distance(self, mask, lat, lon, radius=6371000.0, max_distance=None, return_nearest=False, return_cost=False):
        """Great-circle distance from every node of a latitude-longitude grid to the nearest foreground pixel of ``mask``
        (``lc_sphere_distance``), as a float64 device tensor shaped like ``mask`` -- ``(ny, nx)``, or ``(n_members, ny, nx)``,
        every plane on its own in the same launches -- in the unit of ``radius`` (metres by default).

        A pixel is foreground when it is ``!= 0`` and not NaN (float32 / float64 kept, any other dtype converted to float64).
        ``lat`` ``(ny,)`` and ``lon`` ``(nx,)`` are degrees, finite, ``|lat| <= 90``; the grid need be neither uniform nor
        global nor sorted.  Their cosines and sines are numpy's, computed here; node ``(r, c)`` is the unit vector ``(cos lat
        cos lon, cos lat sin lon, sin lat)`` and the cost of a pair the squared chord ``((dX dX + dY dY) + dZ dZ)``, every
        operation rounded once to float64: a pixel gets the smallest cost over its plane's foreground, the smallest linear
        index among the pixels of that cost, and ``dist = 2 radius asin(min(1, sqrt(cost) / 2))``.  The seam and the poles
        need no flag.  ``max_distance`` (> 0, in the unit of ``radius``): pixels further away -- ``cost > (2 sin(max_distance /
        (2 radius)))^2`` -- are ``+inf``, and a row is searched against the rows within that bound only; the result is exactly
        the unbounded one under that mask.  None, or ``>= pi radius``: unbounded.  A plane without foreground is ``+inf``.

        ``return_nearest``: also the int32 linear index, into its plane, of the nearest foreground pixel (-1 where the
        distance is ``+inf``).  ``return_cost``: also the float64 squared chord.  Returns ``dist``, then ``nearest``, then
        ``cost``, as asked for.  Every pixel is compared with every foreground pixel of its band."""
        cl, sl, cx, sx, radius, chord2, bound = self.sphere_tables(lat, lon, radius, max_distance)
        shape = tuple(int(s) for s in mask.shape) if hasattr(mask, "shape") else np.shape(mask)
        if len(shape) not in (2, 3) or shape[-2:] != (cl.size, cx.size):
            raise ValueError(f"mask {shape}: (ny, nx) or (n_members, ny, nx) with ny = len(lat) = {cl.size} and nx = len(lon) = {cx.size}")
        m = self._planes(mask)
        n, ny, nx = (int(s) for s in m.shape)
        torch = self.torch
        elems = int(self.lib.lc_sphere_distance_work_elems(ny, nx, n))
        # int64 elements: the list's float64 parts come first and want 8-byte alignment whatever the allocator does; the
        # call's own checks refuse what cannot be sized (a plane too large) before they touch the buffer
        work = torch.empty((max(1, (elems + 1) // 2),), dtype=torch.int64, device=self.device)
        dist = self._empty((n, ny, nx), np.float64)
        nearest = torch.empty((n, ny, nx), dtype=torch.int32, device=self.device) if return_nearest else None
        cost = self._empty((n, ny, nx), np.float64) if return_cost else None
        tables = [self.to_device(t, np.float64) for t in (cl, sl, cx, sx)]
        a = _capi.SphereDistanceArgs(struct_size=C.sizeof(_capi.SphereDistanceArgs))
        a.mask, a.dtype = m.data_ptr(), _NP2LC[np.dtype(str(m.dtype).replace("torch.", ""))]
        a.ny, a.nx, a.n_members = ny, nx, n
        a.cos_lat, a.sin_lat, a.cos_lon, a.sin_lon = (t.data_ptr() for t in tables)
        a.radius, a.max_chord2, a.max_distance = radius, chord2, bound
        a.dist_out, a.work_dev = dist.data_ptr(), work.data_ptr()
        a.nearest_out = nearest.data_ptr() if return_nearest else None
        a.cost_out = cost.data_ptr() if return_cost else None
        self._use_current_stream()
        _capi.check(self.lib.lc_sphere_distance(self.ctx, C.byref(a)), self.lib)
        out = [t if len(shape) == 3 else t[0] for t in (dist, nearest, cost) if t is not None]
        return out[0] if len(out) == 1 else tuple(out)

    # ------------------------------------------------------------------ inverse-distance weighting of scattered values
    IDW_MAX_POWER = 16.0

    @property
    def last_idw_kernel(self) -> str:
        """Names of the kernels the last :meth:`idw_interp` call launched (``lc_ctx_last_idw_kernel``), joined by ``+``."""
        return self.lib.lc_ctx_last_idw_kernel(self.ctx).decode()

    @staticmethod
    def _host_degrees(a):
        """Coordinates in degrees as a float64 numpy array, from a numpy array or a tensor (positions are small beside the
        all-pairs work, and their cosines and sines are numpy's by definition)."""
        if hasattr(a, "detach"):
            a = a.detach().cpu().numpy()
        return np.asarray(a, dtype=np.float64)

    @staticmethod
    def sphere_points(lon, lat, grid=False):
        """Unit vectors ``(X, Y, Z)`` of points given in degrees: ``X = fl(cos lat cos lon)``, ``Y = fl(cos lat sin lon)``, ``Z =
        sin lat`` with numpy's cos / sin of ``degrees * pi / 180``, as :meth:`sphere_tables` forms its tables.  ``lon`` and
        ``lat`` have one shape, which the vectors take; ``grid=True``: ``lat`` is ``(ny,)``, ``lon`` is ``(nx,)`` and the
        vectors are ``(ny, nx)``, one rounded product of the row and column tables each, as ``lc_sphere_distance`` defines its
        nodes.  A point with a coordinate that is not finite or with ``|lat| > 90`` has NaN components: it is left out."""
        lon, lat = np.asarray(lon, dtype=np.float64), np.asarray(lat, dtype=np.float64)
        with np.errstate(invalid="ignore"):
            y, x = lat * np.pi / 180, lon * np.pi / 180
            cl, sl, cx, sx = np.cos(y), np.sin(y), np.cos(x), np.sin(x)
            bad_lat, bad_lon = ~(np.isfinite(lat) & (np.abs(lat) <= 90.0)), ~np.isfinite(lon)
            if grid:
                cl, sl, bad_lat, cx, sx, bad_lon = cl[:, None], sl[:, None], bad_lat[:, None], cx[None, :], sx[None, :], bad_lon[None, :]
            X, Y, bad = cl * cx, cl * sx, bad_lat | bad_lon
        return tuple(np.where(bad, np.nan, v) for v in (X, Y, np.broadcast_to(sl, X.shape)))

    @staticmethod
    def idw_plan(src_lon, src_lat, values_shape, tgt_lon, tgt_lat, grid=False, power=2, radius=6371000.0, max_distance=None):
        """Every check of :meth:`idw_interp` and what it hands to the device, computed with numpy on the host (no device is
        touched): a dict of the source vectors ``src`` and target vectors ``tgt`` (tuples of flat float64 arrays), the targets'
        ``shape``, ``n_planes`` (None for one-dimensional values), ``power``, ``radius``, ``max_chord2`` and ``max_distance``
        (both 0 without a bound) and ``order`` -- with a bound, the permutation that sorts the sources by latitude (``src`` is
        in that order), else None."""
        power, radius = float(power), float(radius)
        if not (0.0 < power <= Engine.IDW_MAX_POWER):
            raise ValueError(f"power {power!r}: in (0, {Engine.IDW_MAX_POWER:g}]")
        if not (radius > 0 and np.isfinite(radius)):
            raise ValueError(f"radius {radius!r}: a positive, finite number")
        chord2, bound = 0.0, 0.0
        if max_distance is not None:
            if not float(max_distance) > 0:
                raise ValueError(f"max_distance {max_distance!r}: a positive number, or None for no bound")
            if float(max_distance) < np.pi * radius:
                bound = float(max_distance)
                c = np.float64(2.0) * np.sin(np.float64(bound) / (np.float64(2.0) * np.float64(radius)))
                chord2 = float(c * c)
                if not chord2 > 0.0:
                    raise ValueError(f"max_distance {max_distance!r}: its squared chord on a sphere of radius {radius!r} underflows")
        shapes = [tuple(int(s) for s in (a.shape if hasattr(a, "shape") else np.shape(a))) for a in (src_lon, src_lat, tgt_lon, tgt_lat)]
        values_shape = tuple(int(s) for s in values_shape)
        if len(shapes[0]) != 1 or shapes[0] != shapes[1] or shapes[0][0] == 0:
            raise ValueError(f"src_lon {shapes[0]} and src_lat {shapes[1]}: one-dimensional, equal and not empty")
        if len(values_shape) not in (1, 2) or values_shape[-1] != shapes[0][0] or 0 in values_shape:
            raise ValueError(f"values {values_shape}: (n_src,) or (n_planes, n_src) with n_src = {shapes[0][0]}")
        if grid:
            if len(shapes[2]) != 1 or len(shapes[3]) != 1 or shapes[2][0] == 0 or shapes[3][0] == 0:
                raise ValueError(f"grid=True: tgt_lon {shapes[2]} is (nx,) and tgt_lat {shapes[3]} is (ny,), neither empty")
            shape = (shapes[3][0], shapes[2][0])
        else:
            if shapes[2] != shapes[3] or 0 in shapes[2]:
                raise ValueError(f"grid=False: tgt_lon {shapes[2]} and tgt_lat {shapes[3]} have equal shapes and are not empty")
            shape = shapes[2]
        n_tgt = int(np.prod(shape, dtype=np.int64))
        if max(shapes[0][0], n_tgt) >= 1 << 31 or (len(values_shape) == 2 and values_shape[0] >= 1 << 31):
            raise ValueError("sources, targets and planes: fewer than 2^31 each")
        slon, slat, tlon, tlat = (Engine._host_degrees(a) for a in (src_lon, src_lat, tgt_lon, tgt_lat))
        src = Engine.sphere_points(slon, slat)
        tgt = tuple(np.ascontiguousarray(v).reshape(-1) for v in Engine.sphere_points(tlon, tlat, grid))
        order = None
        if chord2 > 0.0:
            order = np.argsort(src[2], kind="stable")     # ascending latitude; the points left out (NaN) last
            src = tuple(v[order] for v in src)
        return {"src": tuple(np.ascontiguousarray(v) for v in src), "tgt": tgt, "shape": shape,
                "n_planes": values_shape[0] if len(values_shape) == 2 else None,
                "power": power, "radius": radius, "max_chord2": chord2, "max_distance": bound, "order": order}

    def idw_interp(self, src_lon, src_lat, values, tgt_lon, tgt_lat, grid=False, power=2, radius=6371000.0, max_distance=None,
                   return_weight=False, return_count=False):
        """Values known at scattered points of the sphere, gridded by inverse-distance weighting with great-circle distances
        (``lc_idw_interp``; LCS/tools.py:285-299): ``u = sum(w z) / sum(w)`` with ``w = 1 / d**power`` over the sources.

        ``src_lon``, ``src_lat`` ``(n_src,)`` in degrees; ``values`` ``(n_src,)``, or ``(n_planes, n_src)`` -- several fields
        on the same positions, for which the geometry of a pair is evaluated once -- float32 or float64 (anything else is
        converted to float64), and the result has their dtype.  ``grid=False``: ``tgt_lon`` and ``tgt_lat`` have equal shapes,
        which the result takes; ``grid=True``: ``tgt_lat`` is ``(ny,)``, ``tgt_lon`` is ``(nx,)`` and the result is ``(ny,
        nx)``, in the order given (sorted or not).  With planes the result is ``(n_planes, ...)``.  Numpy arrays or device
        tensors; the result is a device tensor.

        A point is the unit vector ``(cos lat cos lon, cos lat sin lon, sin lat)``, formed here with numpy (:meth:`sphere_points`);
        the cost of a pair is the squared chord ``((dX dX + dY dY) + dZ dZ)``, ``d = 2 radius asin(min(1, sqrt(cost) / 2))`` as
        in :meth:`sphere_distance`, all arithmetic and every sum in float64.  ``0 < power <= 16``; powers 2 and 1 take forms
        without ``pow``.  Where sources coincide with a target (cost 0) the result is the mean of their values, the limit of
        the weighting (the reference divides ``inf`` by ``inf`` there).  A source whose value is NaN is left out of that
        plane; a source with a coordinate that is not finite or ``|lat| > 90`` out of every plane.  Without a bound the result
        does not depend on ``radius``.

        ``max_distance`` (> 0, in the unit of ``radius``; None or ``>= pi radius``: no bound): a source contributes where ``cost
        <= (2 sin(max_distance / (2 radius)))^2``; a target without a contributing source is NaN.  The sources are then sorted
        by latitude and every 256 targets walk only the sources within the bound of their latitudes.

        ``return_weight``: also ``sum(w)`` (float64, shaped like the result; ``+inf`` on an exact hit, 0 where nothing
        contributes).  ``return_count``: also the int32 number of sources within reach of each target (shaped like the
        targets), whatever their values are.  Returns ``u``, then the weight, then the count, as asked for.  The order of
        summation depends on the sizes only: two calls on the same inputs agree bit for bit."""
        vshape = tuple(int(s) for s in values.shape) if hasattr(values, "shape") else np.shape(values)
        plan = self.idw_plan(src_lon, src_lat, vshape, tgt_lon, tgt_lat, grid, power, radius, max_distance)
        torch = self.torch
        dtype = np.dtype(str(values.dtype).replace("torch.", "")) if hasattr(values, "dtype") else np.asarray(values).dtype
        dtype = dtype if dtype in _NP2LC else np.dtype(np.float64)
        v = self.to_device(values, dtype).reshape(-1, vshape[-1])
        if plan["order"] is not None:
            v = v.index_select(1, torch.as_tensor(plan["order"], device=self.device)).contiguous()
        n, n_src = (int(s) for s in v.shape)
        n_tgt = plan["tgt"][0].size
        elems = int(self.lib.lc_idw_work_elems(n_src, n_tgt, n))
        work = torch.empty((max(1, elems),), dtype=torch.float64, device=self.device)
        out = self._empty((n, n_tgt), dtype)
        weight = self._empty((n, n_tgt), np.float64) if return_weight else None
        count = torch.empty((n_tgt,), dtype=torch.int32, device=self.device) if return_count else None
        vectors = [self.to_device(t, np.float64) for t in (*plan["src"], *plan["tgt"])]
        a = _capi.IdwArgs(struct_size=C.sizeof(_capi.IdwArgs))
        a.src_x, a.src_y, a.src_z, a.tgt_x, a.tgt_y, a.tgt_z = (t.data_ptr() for t in vectors)
        a.values, a.dtype = v.data_ptr(), _NP2LC[dtype]
        a.n_src, a.n_tgt, a.n_planes = n_src, n_tgt, n
        a.power, a.radius, a.max_chord2, a.max_distance = plan["power"], plan["radius"], plan["max_chord2"], plan["max_distance"]
        a.out, a.work_dev = out.data_ptr(), work.data_ptr()
        a.weight_out = weight.data_ptr() if return_weight else None
        a.count_out = count.data_ptr() if return_count else None
        self._use_current_stream()
        _capi.check(self.lib.lc_idw_interp(self.ctx, C.byref(a)), self.lib)
        shape = plan["shape"] if plan["n_planes"] is None else (n, *plan["shape"])
        res = [out.reshape(shape)]
        if return_weight:
            res.append(weight.reshape(shape))
        if return_count:
            res.append(count.reshape(plan["shape"]))
        return res[0] if len(res) == 1 else tuple(res)

    # ------------------------------------------------------------------ adaptive local threshold
    _THRESHOLD_PLANES = ("threshold", "mask")

    @property
    def last_threshold_kernel(self) -> str:
        """Names of the kernels the last :meth:`local_threshold` call launched (``lc_ctx_last_threshold_kernel``), joined by
        ``+``."""
        return self.lib.lc_ctx_last_threshold_kernel(self.ctx).decode()

    def local_threshold(self, f, sigma, offset=0.0, cyclic=False, want=("threshold",)) -> dict:
        """The Gaussian local threshold of ``skimage.filters.threshold_local`` and its comparison in one call
        (``lc_local_threshold``; LCS/area_of_influence.py:194-199): ``threshold = scipy.ndimage.gaussian_filter(f, sigma,
        mode='reflect') - offset`` and ``mask = f > threshold``.

        ``f``: ``(ny, nx)`` or ``(n_members, ny, nx)``, an array or a device tensor (float32 / float64 kept, anything else
        converted to float64; float32 is widened on the device), every plane smoothed on its own in the same launches.
        ``sigma``: the Gaussian's width in grid steps, a scalar or ``(latitude, longitude)``; an axis with ``sigma <= 1e-15``
        is not filtered; a radius ``int(4 sigma + 0.5)`` above 256 is refused.  ``cyclic``: longitude is periodic instead of
        reflected.  Returns a dict of device tensors shaped like ``f`` for the names in ``want``: ``threshold`` (float64) and /
        or ``mask`` (uint8: 1 where ``f > threshold``, 0 elsewhere and wherever either side is NaN).  With only the mask
        wanted no threshold plane is written."""
        want = tuple(want)
        if not want or any(w not in self._THRESHOLD_PLANES for w in want):
            raise ValueError(f"want {want!r}: a non-empty subset of {self._THRESHOLD_PLANES}")
        sigma = np.asarray(sigma, dtype=np.float64)
        if sigma.shape not in ((), (2,)):
            raise ValueError("sigma: a scalar or (latitude, longitude)")
        sy, sx = (float(s) for s in np.broadcast_to(sigma, (2,)))
        m = self._planes(f)
        n, ny, nx = (int(s) for s in m.shape)
        torch = self.torch
        out = {}
        if "threshold" in want:
            out["threshold"] = self._empty((n, ny, nx), np.float64)
        if "mask" in want:
            out["mask"] = torch.empty((n, ny, nx), dtype=torch.uint8, device=self.device)
        a = _capi.LocalThresholdArgs(struct_size=C.sizeof(_capi.LocalThresholdArgs))
        a.f, a.dtype = m.data_ptr(), _NP2LC[np.dtype(str(m.dtype).replace("torch.", ""))]
        a.ny, a.nx, a.n_members = ny, nx, n
        a.sigma_y, a.sigma_x, a.offset, a.cyclic = sy, sx, float(offset), int(bool(cyclic))
        work = None
        if sy > 1e-15 and sx > 1e-15:     # the planes between the two passes
            work = self._empty((max(1, int(self.lib.lc_local_threshold_work_elems(ny, nx, n))),), np.float64)
            a.work = work.data_ptr()
        a.threshold_out = out["threshold"].data_ptr() if "threshold" in out else None
        a.mask_out = out["mask"].data_ptr() if "mask" in out else None
        self._use_current_stream()
        _capi.check(self.lib.lc_local_threshold(self.ctx, C.byref(a)), self.lib)
        return out if len(f.shape) == 3 else {k: v[0] for k, v in out.items()}

    # ------------------------------------------------------------------ thinning and dilating a mask
    THINNING_METHODS = ("guohall", "zhang")
    STRUCTURES = {1: 2 + 8 + 32 + 128, 2: 255}   # connectivity -> the neighbours of lc_morph_args.structure (N, E, S, W; all eight)

    @staticmethod
    def thinning_table(method):
        """The 256 codes of a shipped thinning rule as a ``numpy.uint8`` array: entry ``NW + 2 N + 4 NE + 8 E + 16 SE + 32 S +
        64 SW + 128 W`` is 1 where the pixel is deleted in the first sub-iteration, 2 in the second, 3 in both, 0 in neither.

        ``'zhang'``: Zhang & Suen 1984.  With P2..P9 = N, NE, E, SE, S, SW, W, NW, B their sum and A the 0 -> 1 steps round
        the cycle: deletable when 2 <= B <= 6 and A = 1; first sub-iteration N E S = 0 and E S W = 0, second N E W = 0 and
        N S W = 0.  ``'guohall'``: Guo & Hall 1989, the rule ``bwmorph('thin')`` documents.  With x1..x8 = E, NE, N, NW, W, SW,
        S, SE: G1 exactly one k in {1, 3, 5, 7} with ``not x_k and (x_{k+1} or x_{k+2})``; G2 min(n1, n2) in {2, 3} for
        n1 = sum (x_{2k-1} or x_{2k}), n2 = sum (x_{2k} or x_{2k+1}); first sub-iteration ``not ((x2 or x3 or not x8) and x1)``,
        second ``not ((x6 or x7 or not x4) and x5)``."""
        if method not in Engine.THINNING_METHODS:
            raise ValueError(f"method {method!r}: one of {', '.join(Engine.THINNING_METHODS)}")
        table = np.zeros(256, dtype=np.uint8)
        for i in range(256):
            nw, n, ne, e, se, s, sw, w = ((i >> k) & 1 for k in range(8))
            if method == "zhang":
                p = [n, ne, e, se, s, sw, w, nw]
                b, a = sum(p), sum(1 for k in range(8) if not p[k] and p[(k + 1) % 8])
                ok = 2 <= b <= 6 and a == 1
                first, second = ok and not n * e * s and not e * s * w, ok and not n * e * w and not n * s * w
            else:
                x = [None, e, ne, n, nw, w, sw, s, se, e, ne]                 # x[1..8], x[9] = x[1], x[10] = x[2]
                g1 = sum(1 for k in (1, 3, 5, 7) if not x[k] and (x[k + 1] or x[k + 2])) == 1
                n1 = sum(1 for k in (1, 2, 3, 4) if x[2 * k - 1] or x[2 * k])
                n2 = sum(1 for k in (1, 2, 3, 4) if x[2 * k] or x[2 * k + 1])
                ok = g1 and min(n1, n2) in (2, 3)
                first = ok and not ((x[2] or x[3] or not x[8]) and x[1])
                second = ok and not ((x[6] or x[7] or not x[4]) and x[5])
            table[i] = (1 if first else 0) | (2 if second else 0)
        return table

    @staticmethod
    def checked_thinning_table(table):
        """``table`` as the contiguous ``numpy.uint8`` array the library reads, or ``ValueError``: 256 integer codes 0 .. 3."""
        table = np.asarray(table)
        if table.shape != (256,) or table.dtype.kind not in "iub" or (table.astype(np.int64) < 0).any() or (table.astype(np.int64) > 3).any():
            raise ValueError("table: 256 integer codes 0 .. 3")
        return np.ascontiguousarray(table, dtype=np.uint8)

    def _morphology(self, mask, op, table, structure, cyclic, iterations, iterations_per_launch):
        m = self._planes(mask)
        n, ny, nx = (int(s) for s in m.shape)
        torch = self.torch
        out = torch.empty((n, ny, nx), dtype=torch.uint8, device=self.device)
        elems = int(self.lib.lc_morph_work_elems(ny, nx, n))
        # (a plane the call refuses for its size is refused before the buffer is touched)
        work = torch.empty((max(1, elems if ny * nx < 2 ** 31 else 1),), dtype=torch.int32, device=self.device)
        launches = C.c_int(0)
        a = _capi.MorphArgs(struct_size=C.sizeof(_capi.MorphArgs))
        a.mask, a.dtype = m.data_ptr(), _NP2LC[np.dtype(str(m.dtype).replace("torch.", ""))]
        a.ny, a.nx, a.n_members, a.op, a.cyclic_x = ny, nx, n, op, int(bool(cyclic))
        a.table = table.ctypes.data if table is not None else None
        a.structure, a.max_iterations, a.iterations_per_launch = structure, iterations, int(iterations_per_launch or 0)
        a.out, a.launches_out, a.work_dev = out.data_ptr(), C.pointer(launches), work.data_ptr()
        self._use_current_stream()
        _capi.check(self.lib.lc_mask_morphology(self.ctx, C.byref(a)), self.lib)
        self.last_morphology_launches = launches.value
        return out if len(mask.shape) == 3 else out[0]

    @staticmethod
    def _per_launch(iterations_per_launch):
        if iterations_per_launch is not None and int(iterations_per_launch) < 1:
            raise ValueError(f"iterations_per_launch {iterations_per_launch!r}: >= 1, or None for the library's default")

    def thin(self, mask, table, cyclic=False, max_iterations=None, iterations_per_launch=None):
        """``mask`` thinned by the parallel two-sub-iteration rule ``table`` encodes (``lc_mask_morphology``, LC_MORPH_THIN): a
        ``torch.uint8`` device tensor of 0 / 1 shaped like ``mask`` -- ``(ny, nx)``, or ``(n_members, ny, nx)``, every plane on
        its own in the same launches.

        A pixel is foreground when it is ``!= 0`` and not NaN (float32 / float64 kept, any other dtype converted to float64);
        pixels outside a plane are background; ``cyclic``: the last column is the western neighbour of the first.  ``table``:
        256 codes as :meth:`thinning_table` returns them (bit 0: delete in the first sub-iteration, bit 1: in the second).
        Thinning ends when an iteration deletes nothing or after ``max_iterations``.  ``iterations_per_launch`` (default 4, the
        most a launch can do) only changes how the sub-iterations are cut into launches, never the result; after each launch
        one word is read back to see whether anything changed (one synchronisation per launch).
        ``last_morphology_launches`` holds the number of step launches of the last call."""
        table = self.checked_thinning_table(table)
        if max_iterations is not None and int(max_iterations) < 1:
            raise ValueError(f"max_iterations {max_iterations!r}: >= 1, or None for no bound")
        self._per_launch(iterations_per_launch)
        return self._morphology(mask, _capi.LC_MORPH_THIN, table, 0, cyclic,
                                0 if max_iterations is None else int(max_iterations), iterations_per_launch)

    def dilate(self, mask, iterations=1, connectivity=1, cyclic=False, iterations_per_launch=None):
        """``mask`` dilated ``iterations`` times (``lc_mask_morphology``, LC_MORPH_DILATE): a background pixel becomes foreground
        when one of its four edge neighbours (``connectivity=1``) or eight neighbours (``2``) is foreground --
        ``scipy.ndimage.binary_dilation(foreground, generate_binary_structure(2, connectivity), iterations)``.  A ``torch.uint8``
        device tensor of 0 / 1 shaped like ``mask``; foreground, planes, ``cyclic`` and ``iterations_per_launch`` (default 8) as
        for :meth:`thin`."""
        if connectivity not in self.STRUCTURES:
            raise ValueError(f"connectivity {connectivity!r}: 1 (edges) or 2 (edges and corners)")
        if int(iterations) < 1:
            raise ValueError(f"iterations {iterations!r}: >= 1")
        self._per_launch(iterations_per_launch)
        return self._morphology(mask, _capi.LC_MORPH_DILATE, None, self.STRUCTURES[connectivity], cyclic, int(iterations),
                                iterations_per_launch)

    # ------------------------------------------------------------------ thinned ridges as ordered lines
    LINE_STEPS = ((-1, -1), (-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1), (0, -1))   # direction codes 0 .. 7: NW N NE E SE S SW W

    @staticmethod
    def checked_line_options(shape, cyclic, metric, lat, lon, radius, sampling):
        """Every refusal of :meth:`trace_lines`' arguments (``ValueError``), on the host: no device is touched.  Returns
        ``(tables or None, radius, sy, sx)``: the four tables of :meth:`sphere_tables` for ``metric='sphere'``."""
        if metric not in Engine.METRICS:
            raise ValueError(f"metric {metric!r}: 'index' or 'sphere'")
        shape = tuple(int(s) for s in shape)
        if len(shape) not in (2, 3) or min(shape) < 1:
            raise ValueError("a plane (ny, nx) or a stack of planes (n_members, ny, nx), none of them empty")
        ny, nx = shape[-2:]
        if ny * nx >= 2 ** 28:
            raise ValueError(f"plane too large: {ny} x {nx} pixels, dart ids 8 p + k are int32 (< 2^28 pixels)")
        if cyclic and nx < 3:
            raise ValueError(f"cyclic needs at least 3 columns, got {nx}: a pixel would neighbour itself or one pixel twice")
        if metric == 'sphere':
            if sampling is not None:
                raise ValueError("sampling belongs to metric='index': on the sphere the coordinates are the metric")
            if lat is None or lon is None:
                raise ValueError("metric='sphere' needs lat and lon (degrees)")
            cl, sl, cx, sx, radius, _, _ = Engine.sphere_tables(lat, lon, radius)
            if (cl.size, cx.size) != (ny, nx):
                raise ValueError(f"mask {shape}: ny = len(lat) = {cl.size} and nx = len(lon) = {cx.size}")
            return (cl, sl, cx, sx), radius, 1.0, 1.0
        s = np.asarray(1.0 if sampling is None else sampling, dtype=np.float64)
        if s.shape not in ((), (2,)) or not (np.isfinite(s).all() and (s > 0).all()):
            raise ValueError(f"sampling {sampling!r}: a positive finite scalar or (latitude step, longitude step)")
        sy, sx = (float(v) for v in np.broadcast_to(s, (2,)))
        return None, float(radius), sy, sx

    def last_lines_rounds(self) -> int:
        """Pointer-doubling rounds of the last :meth:`trace_lines` call (``lc_lines_args.rounds_out``)."""
        return self._lines_rounds

    _lines_rounds = 0

    def trace_lines(self, mask, cyclic=False, metric='sphere', lat=None, lon=None, radius=6371000.0, sampling=None):
        """The lines of a one-pixel-wide mask as ordered lists of pixels (``lc_trace_lines``; include/lcs_hip.h states the
        definition, tests/lines.py restates it as a pixel walk).  ``mask``: ``(ny, nx)`` or ``(n_members, ny, nx)``, every plane
        on its own in the same launches; a pixel is foreground when it is ``!= 0`` and not NaN; ``cyclic``: the last column is
        the western neighbour of the first (at least 3 columns).

        A foreground pixel is linked to its foreground edge neighbours, and to a foreground corner neighbour only if neither
        of the two pixels edge-adjacent to both is foreground.  Pixels of degree 2 are interior, all others nodes; links that
        meet in an interior pixel belong to one line.  A line starts with its canonical first dart (``pixel * 8 + direction
        code``, codes NW N NE E SE S SW W): of an open line the smaller of the two darts that leave its end nodes along it, of
        a ring the smallest of all its darts.  Lines are numbered by plane, then by that dart.

        Returns a dict of device tensors.  Per line: ``plane``, ``offset``, ``count`` (its points are ``offset .. offset +
        count``), ``closed`` (uint8: a ring, whose first pixel is not repeated), ``first``, ``last`` (int32 pixel indices into
        the plane), ``first_degree``, ``last_degree`` (1 a free end, >= 3 a junction, 0 a lone pixel, 2 a ring), ``n_edge``,
        ``n_diag`` (edge and corner links, a ring's closing link included), ``key`` (the canonical first dart) and ``length``
        (float64).  Per point, ordered by line and position: ``line``, ``pixel`` (int32), ``distance`` (float64: along the line
        from its first point) and ``step`` (the length of the link that leads to the point, 0 at a first point).  Per plane:
        ``links`` (uint8 shaped like ``mask``: bit k set per link) and ``counts`` (int32 ``(n_members, 4)``: foreground,
        interior pixels, nodes, links).

        ``metric='sphere'``: a link is ``2 radius asin(min(1, sqrt(cost) / 2))`` long, with the node vectors and squared chord
        of :meth:`sphere_distance` from ``lat`` / ``lon`` in degrees; ``length`` and ``distance`` are sums of those (float64,
        in no stated order).  ``metric='index'``: ``length = n_edge * sy + n_diag * sqrt(sy * sy + sx * sx)``, every operation
        rounded once, likewise ``distance`` from the counts before a point; ``sampling`` a scalar or ``(sy, sx)``, default 1
        -- meant for uniform sampling, where an edge link is ``sy`` long whichever way it runs.

        The ranking runs on the device (pointer doubling over the interior pixels, :meth:`last_lines_rounds` rounds, one word
        read back per round); selection, one sort and the per-line gathers are torch on the device."""
        torch = self.torch
        shape = tuple(int(s) for s in mask.shape) if hasattr(mask, "shape") else np.shape(mask)
        tables, radius, sy, sx = self.checked_line_options(shape, cyclic, metric, lat, lon, radius, sampling)
        m = self._planes(mask)
        n, ny, nx = (int(s) for s in m.shape)
        npix, dev, i32, i64 = ny * nx, self.device, torch.int32, torch.int64
        links = torch.empty((n, ny, nx), dtype=torch.uint8, device=dev)
        counts = torch.empty((n, 4), dtype=i32, device=dev)
        key, pos, ndiag, head = (torch.empty((n * 2 * npix,), dtype=i32, device=dev) for _ in range(4))
        flags = torch.empty((n * 2 * npix,), dtype=torch.uint8, device=dev)
        a = _capi.LinesArgs(struct_size=C.sizeof(_capi.LinesArgs))
        a.mask, a.dtype = m.data_ptr(), _NP2LC[np.dtype(str(m.dtype).replace("torch.", ""))]
        a.ny, a.nx, a.n_members, a.cyclic_x, a.radius = ny, nx, n, int(bool(cyclic)), radius
        dist = link_len = dev_tables = None
        if tables is not None:
            dev_tables = [self.to_device(t, np.float64) for t in tables]
            a.cos_lat, a.sin_lat, a.cos_lon, a.sin_lon = (t.data_ptr() for t in dev_tables)
            dist, link_len = self._empty((n * 2 * npix,), np.float64), self._empty((n * 2 * npix,), np.float64)
            a.dist_out, a.link_length_out = dist.data_ptr(), link_len.data_ptr()
        work = torch.empty((max(1, (int(self.lib.lc_lines_work_elems(ny, nx, n)) + 1) // 2),), dtype=i64, device=dev)
        rounds = C.c_int(0)
        a.links_out, a.counts_out, a.flags_out = links.data_ptr(), counts.data_ptr(), flags.data_ptr()
        a.key_out, a.pos_out, a.ndiag_out, a.head_out = key.data_ptr(), pos.data_ptr(), ndiag.data_ptr(), head.data_ptr()
        a.rounds_out, a.work_dev = C.pointer(rounds), work.data_ptr()
        self._use_current_stream()
        _capi.check(self.lib.lc_trace_lines(self.ctx, C.byref(a)), self.lib)
        self._lines_rounds = rounds.value
        del work

        F = _capi
        S = 2 * npix
        zero_f = torch.zeros((), dtype=torch.float64, device=dev)

        def has(f, bit):
            return (f & bit) != 0
        # (a) every interior pixel, from its canonical state g; the link that leads to it is the one its other state leaves by
        g = torch.nonzero(has(flags, F.LC_LINE_CANONICAL)).squeeze(1)
        fg_, ring = flags[g], has(flags[g], F.LC_LINE_RING)
        closing = ring & has(fg_, F.LC_LINE_HEAD_IS_END)          # the last point of a ring: its link closes it
        corner = has(fg_, F.LC_LINE_CORNER_LINK).to(i64)
        parts = [dict(plane=g // S, key=key[g].to(i64), pos=pos[g].to(i64), pixel=(g % S) // 2, nd=ndiag[g].to(i64), ring=ring,
                      close_nd=torch.where(closing, corner, torch.zeros_like(corner)))]
        if tables is not None:
            parts[0].update(dist=dist[g], step=torch.where(pos[g] > 0, link_len[g ^ 1], zero_f),
                            close_len=torch.where(closing, link_len[g], zero_f))
        # (b) the end nodes of the open lines that have an interior pixel: the heads of the states that end at once
        e = torch.nonzero(has(flags, F.LC_LINE_HEAD_IS_END) & ~has(flags, F.LC_LINE_RING)).squeeze(1)
        fe = flags[e]
        fwd = has(fe, F.LC_LINE_CANONICAL)
        zero_i = torch.zeros_like(e)
        parts.append(dict(plane=e // S, key=key[e].to(i64), pos=torch.where(fwd, pos[e].to(i64) + 1, zero_i), pixel=head[e].to(i64),
                          nd=torch.where(fwd, ndiag[e].to(i64) + has(fe, F.LC_LINE_CORNER_LINK).to(i64), zero_i),
                          ring=torch.zeros_like(fwd), close_nd=zero_i))
        if tables is not None:
            parts[1].update(dist=torch.where(fwd, dist[e] + link_len[e], zero_f), step=torch.where(fwd, link_len[e], zero_f),
                            close_len=torch.zeros_like(dist[e]))
        # (c) what has no interior pixel: isolated pixels, and nodes next to nodes (from the end with the smaller dart)
        flat = links.reshape(-1)
        popcount = torch.tensor([bin(i).count("1") for i in range(256)], dtype=i64, device=dev)
        degree = popcount[flat.to(i64)]
        lone = torch.nonzero(((m != 0) & ~torch.isnan(m)).reshape(-1) & (flat == 0)).squeeze(1)
        zero_l = torch.zeros_like(lone)
        parts.append(dict(plane=lone // npix, key=(lone % npix) * 8, pos=zero_l, pixel=lone % npix, nd=zero_l,
                          ring=torch.zeros_like(lone, dtype=torch.bool), close_nd=zero_l))
        if tables is not None:
            z = torch.zeros(lone.shape, dtype=torch.float64, device=dev)
            parts[2].update(dist=z, step=z, close_len=z)
        nodes = torch.nonzero((flat != 0) & (degree != 2)).squeeze(1)
        codes = torch.arange(8, device=dev, dtype=i64)
        at, k = torch.nonzero(((flat[nodes].to(i64)[:, None] >> codes[None, :]) & 1) != 0, as_tuple=True)
        p_all = nodes[at]
        plane, p = p_all // npix, p_all % npix
        steps = torch.tensor(self.LINE_STEPS, dtype=i64, device=dev)
        h = (p // nx + steps[k, 0]) * nx + torch.remainder(p % nx + steps[k, 1], nx)       # a link: inside the plane, or across the seam
        own = (degree[plane * npix + h] != 2) & (p * 8 + k < h * 8 + (k + 4) % 8)
        plane, p, h, k = plane[own], p[own], h[own], k[own]
        diag = 1 - k % 2
        zero_n = torch.zeros_like(p)
        parts.append(dict(plane=torch.cat([plane, plane]), key=torch.cat([p * 8 + k] * 2), pos=torch.cat([zero_n, zero_n + 1]),
                          pixel=torch.cat([p, h]), nd=torch.cat([zero_n, diag]), ring=torch.zeros((2 * p.numel(),), dtype=torch.bool, device=dev),
                          close_nd=torch.cat([zero_n, zero_n])))
        if tables is not None:
            length = self._empty((int(p.numel()),), np.float64)
            if p.numel():
                b = _capi.LinkLengthsArgs(struct_size=C.sizeof(_capi.LinkLengthsArgs))
                p32, h32 = p.to(i32).contiguous(), h.to(i32).contiguous()
                b.from_, b.to, b.n_pairs, b.ny, b.nx, b.radius = p32.data_ptr(), h32.data_ptr(), int(p.numel()), ny, nx, radius
                b.cos_lat, b.sin_lat, b.cos_lon, b.sin_lon = (t.data_ptr() for t in dev_tables)
                b.length_out = length.data_ptr()
                _capi.check(self.lib.lc_line_link_lengths(self.ctx, C.byref(b)), self.lib)
            z = torch.zeros_like(length)
            parts[3].update(dist=torch.cat([z, length]), step=torch.cat([z, length]), close_len=torch.cat([z, z]))

        pt = {name: torch.cat([part[name] for part in parts]) for name in parts[0]}
        total = int(pt["pos"].numel())
        span = int(pt["pos"].max().item()) + 1 if total else 1
        if n * 8 * npix * span >= 2 ** 63:
            raise ValueError(f"{n} planes of {ny} x {nx} with lines of up to {span} points: the sort key passes int64; trace fewer planes per call")
        line_key = pt["plane"] * (8 * npix) + pt["key"]
        order = torch.argsort(line_key * span + pt["pos"])
        pt = {name: v[order] for name, v in pt.items()}
        _, count = torch.unique_consecutive(line_key[order], return_counts=True)
        offset = torch.cumsum(count, 0) - count
        n_lines = int(count.numel())
        line = torch.repeat_interleave(torch.arange(n_lines, device=dev, dtype=i64), count, output_size=total) if total else pt["pos"]
        end = offset + count - 1
        closed = pt["ring"][offset]
        n_diag = pt["nd"][end] + pt["close_nd"][end]
        n_edge = count - 1 + closed.to(i64) - n_diag
        if tables is not None:
            distance, step, length = pt["dist"], pt["step"], pt["dist"][end] + pt["close_len"][end]
        else:
            dg = float(np.sqrt(np.float64(sy) * np.float64(sy) + np.float64(sx) * np.float64(sx)))

            def index_length(ne, nd):
                return ne.to(torch.float64) * sy + nd.to(torch.float64) * dg      # three kernels: nothing is fused
            distance, length = index_length(pt["pos"] - pt["nd"], pt["nd"]), index_length(n_edge, n_diag)
            before = torch.cat([pt["nd"][:1] * 0, pt["nd"][:-1]]) if total else pt["nd"]
            corner_step = pt["nd"] - before          # of the link that leads to the point (not read at a first point)
            step = torch.where(pt["pos"] > 0, index_length(1 - corner_step, corner_step), zero_f)
        first, last = pt["pixel"][offset], pt["pixel"][end]
        planes_of = pt["plane"][offset]
        out = {"plane": planes_of, "offset": offset, "count": count, "closed": closed.to(torch.uint8),
               "first": first.to(i32), "last": last.to(i32),
               "first_degree": degree[planes_of * npix + first].to(i32), "last_degree": degree[planes_of * npix + last].to(i32),
               "n_edge": n_edge, "n_diag": n_diag, "key": pt["key"][offset], "length": length,
               "line": line, "pixel": pt["pixel"].to(i32), "distance": distance, "step": step,
               "links": links if len(shape) == 3 else links[0], "counts": counts}
        return out

    # ------------------------------------------------------------------ great-circle transects across ridge lines
    ORIENTS = {"left": _capi.LC_ORIENT_LEFT, "north": _capi.LC_ORIENT_NORTH, "east": _capi.LC_ORIENT_EAST}
    TRANSECT_METHODS = {"linear": _capi.LC_TRANSECT_LINEAR, "nearest": _capi.LC_TRANSECT_NEAREST}

    @property
    def last_transects_kernel(self) -> str:
        """Names of the kernels the last :meth:`ridge_transects` call launched (``lc_ctx_last_transects_kernel``), joined by
        ``+``."""
        return self.lib.lc_ctx_last_transects_kernel(self.ctx).decode()

    @staticmethod
    def checked_transect_options(shape, lat, lon, half_width, spacing, smooth=3, orient='left', method='linear', cyclic=False,
                                 radius=6371000.0, n_points=0, n_lines=0):
        """Every refusal of :meth:`ridge_transects`' arguments (``ValueError``), on the host: no device is touched.  ``shape``
        is the planes' ``(ny, nx)`` or ``(n_planes, ny, nx)``; ``n_points`` and ``n_lines`` are the sizes of the trace, where
        they are known.  Returns what the call hands to the device: a dict of ``tables`` (:meth:`sphere_tables`' four), ``lat``,
        ``lon`` (float64 degrees), ``offset`` (``s_k = k spacing``, ``k = -K .. K``, ``K = floor(half_width / spacing)``),
        ``cos_off`` / ``sin_off`` (numpy's ``cos(s_k / radius)`` and ``sin(s_k / radius)``), ``K``, ``M = 2 K + 1``,
        ``smooth``, ``orient`` and ``method`` (the library's codes) and ``radius``."""
        if orient not in Engine.ORIENTS:
            raise ValueError(f"orient {orient!r}: 'left', 'north' or 'east'")
        if method not in Engine.TRANSECT_METHODS:
            raise ValueError(f"method {method!r}: 'linear' or 'nearest'")
        spacing, half_width = float(spacing), float(half_width)
        if not (spacing > 0 and np.isfinite(spacing)):
            raise ValueError(f"spacing {spacing!r}: a positive, finite number")
        if not (half_width >= 0 and np.isfinite(half_width)):
            raise ValueError(f"half_width {half_width!r}: >= 0 and finite")
        if int(smooth) != smooth or int(smooth) < 1 or int(smooth) >= 2 ** 30:
            raise ValueError(f"smooth {smooth!r}: a whole number >= 1 (points before and after, below 2^30)")
        shape = tuple(int(s) for s in shape)
        if len(shape) not in (2, 3) or min(shape) < 1:
            raise ValueError("a plane (ny, nx) or a stack of planes (n_planes, ny, nx), none of them empty")
        ny, nx = shape[-2:]
        cl, sl, cx, sx, radius, _, _ = Engine.sphere_tables(lat, lon, radius)
        lat, lon = np.asarray(lat, dtype=np.float64), np.asarray(lon, dtype=np.float64)
        if (lat.size, lon.size) != (ny, nx):
            raise ValueError(f"planes {shape}: ny = len(lat) = {lat.size} and nx = len(lon) = {lon.size}")
        if ny < 2 or nx < 2:
            raise ValueError("lat and lon: at least two values each (a cell needs a neighbour)")
        if not ((np.diff(lat) > 0).all() and (np.diff(lon) > 0).all()):
            raise ValueError("lat and lon: distinct and ascending (tools.ridge_transects sorts them)")
        if not half_width / radius < np.pi / 2:
            raise ValueError(f"half_width {half_width!r} on a sphere of radius {radius!r}: below a quarter of the circumference "
                             "(half_width / radius < pi / 2)")
        if cyclic and nx < 3:
            raise ValueError(f"cyclic needs at least 3 columns, got {nx}: a pixel would neighbour itself or one pixel twice")
        if cyclic and not lon[-1] - lon[0] < 360.0:
            raise ValueError(f"cyclic: the longitudes span {lon[-1] - lon[0]!r} degrees, which must be less than 360 (the seam cell "
                             "lies between the last one and the first one + 360)")
        K = int(np.floor(half_width / spacing))
        M = 2 * K + 1
        if ny * nx >= 2 ** 31 or M >= 2 ** 31 or int(n_points) * M >= 2 ** 31 or int(n_lines) * M >= 2 ** 31:
            raise ValueError(f"too large: {ny} x {nx} pixels, {int(n_points)} points and {int(n_lines)} lines with {M} offsets "
                             "(ny nx, n_points M and n_lines M stay below 2^31)")
        offset = np.arange(-K, K + 1, dtype=np.float64) * np.float64(spacing)
        angle = offset / np.float64(radius)
        return {"tables": (cl, sl, cx, sx), "lat": lat, "lon": lon, "offset": offset, "cos_off": np.cos(angle), "sin_off": np.sin(angle),
                "K": K, "M": M, "smooth": int(smooth), "orient": Engine.ORIENTS[orient], "method": Engine.TRANSECT_METHODS[method],
                "radius": radius}

    def ridge_transects(self, trace, fields, lat, lon, half_width, spacing, smooth=3, orient='left', method='linear', cyclic=False,
                        radius=6371000.0):
        """Fields sampled along great circles across the lines of a thinned mask, and the samples averaged per line
        (``lc_ridge_transects``; include/lcs_hip.h states the definition, tests/transects.py restates it in numpy).

        ``trace`` is what :meth:`trace_lines` returned for the mask (its ``line``, ``pixel``, ``plane``, ``offset``, ``count``
        and ``closed`` are read).  ``fields``: ``(n_fields, ny, nx)``, or ``(n_fields, n_planes, ny, nx)`` for a trace of a stack
        -- the points of plane ``m`` read plane ``m`` of every field --, float32 or float64 (anything else is converted to
        float64), numpy or device tensor.  ``lat`` ``(ny,)`` and ``lon`` ``(nx,)`` are degrees, ascending and distinct (they
        need not be uniform); ``cyclic``: the cell after the last longitude ends at ``lon[0] + 360``.

        Through every point a great circle at right angles to the line -- to the chord between the points ``smooth`` before and
        after it, clamped at the ends of an open line and wrapped on a ring -- is sampled at the signed distances ``k spacing``,
        ``|k| <= floor(half_width / spacing)``, in the unit of ``radius``; positive offsets lie to the left of the direction of
        travel (``orient='left'``), or on the side whose normal points north (``'north'``) or east (``'east'``).
        ``method``: ``'linear'`` (bilinear in degrees, NaN where a corner is NaN) or ``'nearest'``.  Positions outside the grid
        give NaN; so do points without a tangent (lines of one point).

        Returns a dict of device tensors: ``offset`` ``(M,)``; per point ``normal`` ``(n_points, 3)``, ``normal_east``,
        ``normal_north``, ``tangent_east``, ``tangent_north``; ``latitude``, ``longitude`` ``(n_points, M)`` float64 degrees;
        ``values`` ``(n_fields, n_points, M)`` in the fields' dtype; ``line_mean`` (that dtype) and ``line_count`` (int32)
        ``(n_fields, n_lines, M)``: the mean of the finite values of a line's points, offset by offset, NaN where there are
        none.  Two calls agree bit for bit."""
        torch = self.torch
        fshape = tuple(int(s) for s in fields.shape) if hasattr(fields, "shape") else np.shape(fields)
        if len(fshape) not in (3, 4) or min(fshape, default=0) < 1:
            raise ValueError(f"fields {fshape}: (n_fields, ny, nx) or (n_fields, n_planes, ny, nx), none of them empty")
        n_points, n_lines = int(trace["pixel"].numel()), int(trace["count"].numel())
        opt = self.checked_transect_options(fshape[1:], lat, lon, half_width, spacing, smooth, orient, method, cyclic, radius,
                                            n_points, n_lines)
        links = tuple(int(s) for s in trace["links"].shape)
        if links != fshape[1:]:
            raise ValueError(f"fields {fshape}: their planes {fshape[1:]} are not the traced mask's {links}")
        if fshape[0] > 65535:
            raise ValueError(f"{fshape[0]} fields: at most 65535 per call")
        dtype = np.dtype(str(fields.dtype).replace("torch.", "")) if hasattr(fields, "dtype") else np.asarray(fields).dtype
        dtype = dtype if dtype in _NP2LC else np.dtype(np.float64)
        f = self.to_device(fields, dtype)
        n_fields, (ny, nx) = fshape[0], fshape[-2:]
        n_planes = fshape[1] if len(fshape) == 4 else 1
        M, dev, i32 = opt["M"], self.device, torch.int32
        normal = self._empty((7, n_points), np.float64)
        latitude, longitude = self._empty((n_points, M), np.float64), self._empty((n_points, M), np.float64)
        values = self._empty((n_fields, n_points, M), dtype)
        mean = self._empty((n_fields, n_lines, M), dtype)
        count = torch.zeros((n_fields, n_lines, M), dtype=i32, device=dev)
        if n_points:
            keep = [trace[k].to(i32).contiguous() for k in ("pixel", "line", "offset", "count", "plane")]
            closed = trace["closed"].to(torch.uint8).contiguous()
            tables = [self.to_device(t, np.float64) for t in (*opt["tables"], opt["lat"], opt["lon"], opt["cos_off"], opt["sin_off"])]
            a = _capi.TransectsArgs(struct_size=C.sizeof(_capi.TransectsArgs))
            a.pixel, a.point_line, a.line_offset, a.line_count, a.line_plane = (t.data_ptr() for t in keep)
            a.line_closed = closed.data_ptr()
            a.cos_lat, a.sin_lat, a.cos_lon, a.sin_lon, a.lat_deg, a.lon_deg, a.cos_off, a.sin_off = (t.data_ptr() for t in tables)
            a.fields, a.dtype = f.data_ptr(), _NP2LC[dtype]
            a.ny, a.nx, a.n_planes, a.n_points, a.n_lines, a.n_offsets, a.n_fields = ny, nx, n_planes, n_points, n_lines, M, n_fields
            a.smooth, a.orient, a.method, a.cyclic_x = opt["smooth"], opt["orient"], opt["method"], int(bool(cyclic))
            a.normal_out, a.lat_out, a.lon_out = normal.data_ptr(), latitude.data_ptr(), longitude.data_ptr()
            a.values_out, a.mean_out, a.count_out = values.data_ptr(), mean.data_ptr(), count.data_ptr()
            self._use_current_stream()
            _capi.check(self.lib.lc_ridge_transects(self.ctx, C.byref(a)), self.lib)
        return {"offset": self.to_device(opt["offset"], np.float64), "normal": normal[:3].T, "normal_east": normal[3],
                "normal_north": normal[4], "tangent_east": normal[5], "tangent_north": normal[6], "latitude": latitude,
                "longitude": longitude, "values": values, "line_mean": mean, "line_count": count}

    # ------------------------------------------------------------------ multi-GPU (RCCL through the C ABI)
    COMM_ID_BYTES = 128

    def comm_unique_id(self) -> bytes:
        """The id rank 0 creates and every rank passes to :meth:`comm_create` (``lc_comm_unique_id``)."""
        buf = C.create_string_buffer(self.COMM_ID_BYTES)
        _capi.check(self.lib.lc_comm_unique_id(buf, self.COMM_ID_BYTES), self.lib)
        return buf.raw

    def comm_create(self, nranks: int, rank: int, unique_id: bytes):
        """RCCL communicator over ``nranks`` processes, this one on this engine's GPU (collective call)."""
        comm = C.c_void_p()
        buf = C.create_string_buffer(bytes(unique_id), self.COMM_ID_BYTES)
        _capi.check(self.lib.lc_comm_create(self.ctx, int(nranks), int(rank), buf, self.COMM_ID_BYTES, C.byref(comm)),
                    self.lib)
        return comm

    def comm_count(self, comm):
        """(nranks, rank) as RCCL itself reports them for the communicator (``lc_comm_count``)."""
        n, r = C.c_int(), C.c_int()
        _capi.check(self.lib.lc_comm_count(comm, C.byref(n), C.byref(r)), self.lib)
        return n.value, r.value

    def comm_destroy(self, comm):
        if comm:
            self.lib.lc_comm_destroy(comm)

    def halo_exchange(self, comm, x_ext, y_ext, n_lo: int, n_hi: int):
        """In-place 2-row halo exchange of the departure points with the previous / next rank
        (``lc_halo_exchange``: RCCL send/recv on the current stream, no staging copies)."""
        if x_ext.shape != y_ext.shape or x_ext.dtype != y_ext.dtype or not (x_ext.is_contiguous() and y_ext.is_contiguous()):
            raise ValueError("x_ext and y_ext must be contiguous (rows, nx) tensors of one dtype")
        dtype = np.dtype(str(x_ext.dtype).replace("torch.", ""))
        self._use_current_stream()
        _capi.check(self.lib.lc_halo_exchange(self.ctx, comm, self._ptr(x_ext), self._ptr(y_ext), _NP2LC[dtype],
                                              int(x_ext.shape[0]), int(x_ext.shape[1]), int(n_lo), int(n_hi)), self.lib)

    def gaussian_filter(self, a, sigma):
        """scipy.ndimage.gaussian_filter(a, sigma) on the device (LCS/LCS.py:187-190)."""
        torch = self.torch
        dtype = np.dtype(str(a.dtype).replace("torch.", "")) if isinstance(a, torch.Tensor) else common_dtype(a)
        ad = self.to_device(a, dtype)
        ny, nx = (int(s) for s in ad.shape)
        tmp = self._empty((ny, nx), dtype)
        out = self._empty((ny, nx), dtype)
        self._use_current_stream()
        _capi.check(self.lib.lc_gaussian_filter(self.ctx, self._ptr(ad), _NP2LC[dtype], ny, nx, float(sigma),
                                                self._ptr(tmp), self._ptr(out)), self.lib)
        return out

    # ------------------------------------------------------------------ pack and advect, pipelined
    PIPELINE_CHUNK = 24      # time levels per pack / advect stage of the pipelined form (measured: profiles/r04/pipelined_pack_ab.txt)

    def pipeline_pays(self, dtype, interp_order, fuse_levels, nsteps, n_seeds, cyclic_xboundary, return_traj=False) -> bool:
        """Where packing chunk k+1 on a side stream while chunk k is advected is the default: nowhere since round 5.  Until
        then float64 at order 3 in the fused-level form took it (the pack's two prefilter sweeps ran at half the HBM rate
        next to a latency-bound advect kernel: 10.9 -> 9.75 ms per step on BASELINE configs[1]); with both sweeps in one
        pass (``prefilter_fused_stream_kernel``: pack 4.6 -> 2.95 ms) the serial form takes 9.0 ms and the pipelined one
        9.1-9.5 at any chunk length (``profiles/r05/c2_o3_fused_prefilter_ab.txt``): the two kernels now want the same
        CUs.  float32 (its advect kernels saturate the VALU) and float64 at order 1 never gained from it.  The pipelined
        form stays available (``pack_and_advect(pipeline=True)``, bit-identical)."""
        return False

    @staticmethod
    def _pack_options(dtype, SETTLS_order, fuse_levels, ext_image):
        """``(fuse_levels, ext_image)`` that :meth:`pack_and_advect` hands :meth:`prepare_field` for a call of this SETTLS order."""
        if fuse_levels is None:
            fuse_levels = True
        if int(SETTLS_order) == 0 and fuse_levels and ext_image is None:
            # SETTLS_order = 0 (the library default, LCS/trajectory.py:14) takes one Euler sample per level and never reads the
            # fused-level image: it is not built.  float64: the kernels' no-image forms (the same Euler sample, bit for bit --
            # at order 1 no packed image at all, at order 3 the coefficients only); float32: the order-1 / coefficient image only.
            # configs[1] at K = 0: pack 1.29 -> 0 ms (order 1), 3.17 -> 1.85 ms (order 3).  The field returned holds what THIS
            # call needed: advected again with SETTLS_order > 0 it takes the two-sample form.
            if np.dtype(dtype) != np.dtype(np.float32):
                ext_image = False
            else:
                fuse_levels = False
        return fuse_levels, ext_image

    def pack_and_advect(self, u, v, lat_f, lon_f, seed_lat, seed_lon, timestep, SETTLS_order=0, interp_order=1,
                        cyclic_xboundary=True, fuse_levels=None, pipeline=None, chunk=None, return_traj=False,
                        noncyclic_clamp=None, ext_image=None):
        """:meth:`prepare_field` + :meth:`advect` of the whole series in one call.  Returns ``(field, x, y[, traj_x, traj_y])``.

        ``pipeline`` (None: where it pays, :meth:`pipeline_pays`): the series is cut into chunks of ``chunk`` time levels;
        the images of chunk k+1 are packed on a side HIP stream while the advect kernel works through chunk k on the
        current stream (an event per chunk), each advect continuing in place from the previous one (``lc_advect_from``:
        bit-identical to one call, LCS/trajectory.py:80-126 carries only positions from level to level).  The level shared
        by two chunks is packed by both (same values; the earlier chunk's advect never reads it).  Results are
        bit-identical to the serial form; the field returned is reusable (with ``SETTLS_order=0`` it holds no fused-level image)."""
        torch = self.torch
        lat_f, lon_f = np.asarray(lat_f), np.asarray(lon_f)
        dtype = common_dtype(u, v, lat_f, lon_f)
        fuse_levels, ext_image = self._pack_options(dtype, SETTLS_order, fuse_levels, ext_image)
        nt = int(u.shape[0])
        ny, nx = len(seed_lat), len(seed_lon)
        if pipeline is None:
            pipeline = self.pipeline_pays(dtype, interp_order, fuse_levels, nt - 1, ny * nx, cyclic_xboundary, return_traj)
        chunk = self.PIPELINE_CHUNK if chunk is None else int(chunk)
        f32 = np.dtype(np.float32)
        wind_f32 = dtype != f32 and common_dtype(u, v) == f32
        can = (cyclic_xboundary and not return_traj and interp_order in (1, 3) and fuse_levels and not wind_f32 and nt - 1 > chunk >= 1
               and not (dtype == f32 and interp_order == 1))      # (float32 at order 1 carries a lin image too: serial form)
        if not (pipeline and can):
            field = self.prepare_field(u, v, lat_f, lon_f, interp_order, fuse_levels=fuse_levels, ext_image=ext_image)
            res = self.advect(field, seed_lat, seed_lon, timestep, SETTLS_order, interp_order, cyclic_xboundary,
                              return_traj=return_traj, noncyclic_clamp=noncyclic_clamp)
            return (field, *res)
        nt, ny_f, nx_f = _check_grid(u, v, lat_f, lon_f, "field")
        # prepare_field's plan, its one pack call made chunk by chunk (order 1: the ext image IS that pack, whatever ext_image)
        plan = field_plan(dtype, False, interp_order, nt, True, None, ext_image if interp_order == 3 else True,
                          self.EXT_IMAGE_F64, self.EXT_IMAGE_F64_O3)
        (code, order, image, with_ext), = plan.packs
        field, ud, vd = self._planned_field(plan, u, v, lat_f, lon_f, dtype, nt, ny_f, nx_f)
        img, ext, no_ext = getattr(field, image) if image else None, field.ext if with_ext else None, plan.fuse_raw
        le = self.lib.lc_packed_elems(1, ny_f, nx_f)
        slat, slon = self.to_device(seed_lat, dtype), self.to_device(seed_lon, dtype)
        x, y = self._empty((ny, nx), dtype), self._empty((ny, nx), dtype)
        cur = torch.cuda.current_stream(self.device)
        if getattr(self, "_side_stream", None) is None:
            self._side_stream = torch.cuda.Stream(self.device)
        side = self._side_stream
        side.wait_stream(cur)                  # the wind, the seeds and the buffers above belong to the current stream
        # (no record_stream on the images: every pack on the side stream is awaited by the current stream below, so by the
        #  time the field can be freed -- in the current stream's order -- the side stream is done with it; recording the
        #  6.8 GB of images instead made the caching allocator hold the blocks back and cudaMalloc new ones every step)
        events, starts = [], list(range(0, nt - 1, chunk))
        try:
            with torch.cuda.stream(side):
                self._use_current_stream()
                for t0 in starts:
                    n = min(chunk, nt - 1 - t0)         # image levels [t0, t0 + n], ext levels [t0, t0 + n)
                    # Without the ext image the advect of chunk k itself reads level t0 + n (as the "next" level of its last
                    # step), so chunk k+1 must NOT pack that level again behind its back (the sweeps work in place: a reader
                    # would see half-filtered values): each level is packed once, by the chunk that first needs it.
                    l0 = t0 + 1 if (no_ext and t0 > 0) else t0
                    _capi.check(self.lib.lc_field_pack(
                        self.ctx, self._ptr(ud[l0:]), self._ptr(vd[l0:]), code, t0 + n + 1 - l0, ny_f, nx_f, order,
                        self._ptr(img[le * l0:] if img is not None else None),
                        self._ptr(ext[le * t0:] if ext is not None else None)), self.lib)
                    e = torch.cuda.Event()
                    e.record(side)
                    events.append(e)
            for e, t0 in zip(events, starts):
                cur.wait_event(e)
                n = min(chunk, nt - 1 - t0)
                self.advect(field, slat, slon, timestep, SETTLS_order, interp_order, True, t0=t0, nsteps=n,
                            start=(x, y) if t0 else None, out=(x, y))
        finally:
            # whatever happened above -- a pack refused half way through the loop included -- nothing of this call is left
            # running behind the current stream: the images were allocated on it and deliberately not record_stream'd
            cur.wait_stream(side)
        return field, x, y

    # ------------------------------------------------------------------ whole path
    def lcs_wind(self, u, v, lat_f, lon_f, seed_lat, seed_lon, timestep, SETTLS_order=0, interp_order=1, cyclic_xboundary=True,
                 fuse_levels=None, gauss_sigma=None, fd_fp32_cast=True, tensor_layout="reference", return_traj=False,
                 noncyclic_clamp=None, pipeline=None):
        """:meth:`pack_and_advect` -> (smooth) -> sigma: the whole path from the raw wind series (what the drop-in surface
        calls).  Returns the dict of :meth:`lcs` plus ``"field"``."""
        dtype = common_dtype(u, v, np.asarray(lat_f), np.asarray(lon_f))
        seed_lat, seed_lon = np.asarray(seed_lat, dtype=dtype), np.asarray(seed_lon, dtype=dtype)
        res = self.pack_and_advect(u, v, lat_f, lon_f, seed_lat, seed_lon, timestep, SETTLS_order, interp_order,
                                   cyclic_xboundary, fuse_levels, pipeline, None, return_traj, noncyclic_clamp)
        out = self._sigma_of(res[1], res[2], seed_lat, seed_lon, gauss_sigma, fd_fp32_cast, tensor_layout)
        out["field"] = res[0]
        if return_traj:
            out["traj_x"], out["traj_y"] = res[3], res[4]
        return out

    def _sigma_of(self, x, y, seed_lat, seed_lon, gauss_sigma, fd_fp32_cast, tensor_layout):
        xs, ys = x, y
        # scipy's gaussian_filter returns an unsmoothed copy for sigma = 0 (LCS/LCS.py:187-190): skip the filter
        if _smoothing_width(gauss_sigma) > 1e-15:
            xs = self.gaussian_filter(x, gauss_sigma)
            ys = self.gaussian_filter(y, gauss_sigma)
        # spacing evaluated in the coordinate dtype, as lat[1]-lat[0] is in numpy (tools.py:255-256)
        dlat = float(seed_lat[1] - seed_lat[0])
        dlon = float(seed_lon[1] - seed_lon[0])
        sig = self.sigma(xs, ys, seed_lat, dlat, dlon, fd_fp32_cast=fd_fp32_cast, tensor_layout=tensor_layout)
        return {"sigma": sig, "x_dep": x, "y_dep": y}

    def lcs(self, field: PackedField, seed_lat, seed_lon, timestep, SETTLS_order=0, interp_order=1,
            cyclic_xboundary=True, t0=0, nsteps=None, gauss_sigma=None, fd_fp32_cast=True,
            tensor_layout="reference", return_traj=False, noncyclic_clamp=None):
        """advect -> (smooth) -> sigma on one GPU.  Returns dict of device tensors."""
        dtype = field.dtype
        seed_lat = np.asarray(seed_lat, dtype=dtype)
        seed_lon = np.asarray(seed_lon, dtype=dtype)
        res = self.advect(field, seed_lat, seed_lon, timestep, SETTLS_order, interp_order, cyclic_xboundary, t0,
                          nsteps, return_traj, noncyclic_clamp=noncyclic_clamp)
        out = self._sigma_of(res[0], res[1], seed_lat, seed_lon, gauss_sigma, fd_fp32_cast, tensor_layout)
        if return_traj:
            out["traj_x"], out["traj_y"] = res[2], res[3]
        return out

    # device memory one group of windows may hold (positions, saved positions and Euler samples of the outer rule, results)
    SERIES_MEM_CAP = 2 << 30

    def series_group(self, dtype, n_seeds: int, n_windows: int, cyclic_xboundary=True, extra_planes: int = 0) -> int:
        """Windows per group of :meth:`lcs_series`, :meth:`lcs_bidirectional` and :meth:`lcs_strain`: as many as fit
        ``SERIES_MEM_CAP`` (at least one).  Per window: x, y and sigma, plus -- under the reference's non-cyclic clamp -- the
        positions saved before each chunk and the Euler sample of the sub-step phase (two planes each), and the smoothing's two
        scratch planes.  ``extra_planes``: the result planes of a window beyond the first (:meth:`lcs_strain`: three)."""
        planes = (5 if cyclic_xboundary else 9) + int(extra_planes)
        per = planes * int(n_seeds) * np.dtype(dtype).itemsize
        return max(1, min(int(n_windows), int(self.SERIES_MEM_CAP) // max(per, 1)))

    def _windowed(self, name, reduce, field: PackedField, seed_lat, seed_lon, timestep, nsteps, n_windows, t0, t0_stride,
                  SETTLS_order, interp_order, cyclic_xboundary, gauss_sigma, fd_fp32_cast, noncyclic_clamp, n_dirs=1,
                  extra_planes=0):
        """The loop of :meth:`lcs_series`, :meth:`lcs_bidirectional` and :meth:`lcs_strain` (``name``: the caller, for its
        errors): the argument checks, the seeds on the device, then per memory group (:meth:`series_group`) one advect call
        over the group's windows -- ``lc_advect_series``, or ``lc_advect_series_dirs`` for ``n_dirs = 2`` --, the optional
        smoothing plane by plane, and one reduction of the group's departure planes.

        ``reduce(head, planes, outs)`` calls the library and returns its status: ``head`` is the argument list that
        ``lc_sigma_batch`` and ``lc_strain`` begin with (context, x, y, dtype, ny, nx, seed latitudes, dlat, dlon,
        fd_fp32_cast) for ``planes`` whole grids, ``outs`` the group's part of each of the ``1 + extra_planes`` results.
        Returns ``(x_dep, y_dep, results)``, every tensor ``(n_windows, ny, nx)``, or ``(n_windows, 2, ny, nx)`` for
        ``n_dirs = 2``."""
        _check_order(field, interp_order)
        if n_dirs == 2:
            timestep = float(timestep)
            if not timestep or not np.isfinite(timestep):
                raise ValueError(f"{name}: timestep {timestep} (non-zero: its sign is taken from the direction)")
            timestep = -abs(timestep)
        n_windows, nsteps, t0, t0_stride = int(n_windows), int(nsteps), int(t0), int(t0_stride)
        if n_windows < 1 or nsteps < 0 or t0 < 0 or t0_stride < 0:
            raise ValueError(f"{name}: n_windows {n_windows}, nsteps {nsteps}, t0 {t0}, t0_stride {t0_stride}")
        dtype = field.dtype
        seed_lat = np.asarray(seed_lat, dtype=dtype)
        seed_lon = np.asarray(seed_lon, dtype=dtype)
        slat, slon = self.to_device(seed_lat, dtype), self.to_device(seed_lon, dtype)
        ny, nx = int(slat.numel()), int(slon.numel())
        # two directions in the library's plane order: window-major, [n_windows][2][ny][nx], plane 2w + d with -timestep for d = 1
        shape = (n_windows, ny, nx) if n_dirs == 1 else (n_windows, n_dirs, ny, nx)
        x, y, *outs = (self._empty(shape, dtype) for _ in range(3 + extra_planes))
        xmode = x_boundary_mode(cyclic_xboundary, noncyclic_clamp, True)
        smooth = _smoothing_width(gauss_sigma) > 1e-15      # as _sigma_of
        dlat = float(seed_lat[1] - seed_lat[0])     # as _sigma_of: the spacing in the coordinate dtype (tools.py:255-256)
        dlon = float(seed_lon[1] - seed_lon[0])
        g = self.series_group(dtype, n_dirs * ny * nx, n_windows, cyclic_xboundary, extra_planes)
        for m0 in range(0, n_windows, g):
            n = min(g, n_windows - m0)
            xg, yg = x[m0:m0 + n], y[m0:m0 + n]
            self._use_current_stream()
            a = self._advect_args(field, interp_order, slat, ny, slon, nx, timestep, SETTLS_order, xmode,
                                  t0=t0 + m0 * t0_stride, nsteps=nsteps, n_members=n, t0_stride=t0_stride, out=(xg, yg))
            _capi.check(self.lib.lc_advect_series(self.ctx, C.byref(a)) if n_dirs == 1 else
                        self.lib.lc_advect_series_dirs(self.ctx, C.byref(a), n_dirs), self.lib)
            planes = n_dirs * n
            xs, ys = xg.reshape(planes, ny, nx), yg.reshape(planes, ny, nx)
            if smooth:     # scipy's gaussian_filter of each plane's departure points (LCS/LCS.py:187-190), as _sigma_of
                xs = self.torch.stack([self.gaussian_filter(xs[i], gauss_sigma) for i in range(planes)])
                ys = self.torch.stack([self.gaussian_filter(ys[i], gauss_sigma) for i in range(planes)])
            self._use_current_stream()
            head = (self.ctx, self._ptr(xs), self._ptr(ys), _NP2LC[dtype], ny, nx, self._ptr(slat), dlat, dlon, int(bool(fd_fp32_cast)))
            _capi.check(reduce(head, planes, [self._ptr(t[m0:m0 + n]) for t in outs]), self.lib)
        return x, y, outs

    def _sigma_planes(self, tensor_layout):
        """:meth:`_windowed`'s reduction to sigma_max (``lc_sigma_batch``)."""
        return lambda head, planes, outs: self.lib.lc_sigma_batch(*head, _LAYOUTS[tensor_layout], planes, *outs)

    def lcs_series(self, field: PackedField, seed_lat, seed_lon, timestep, nsteps: int, n_windows: int, t0=0, t0_stride=1,
                   SETTLS_order=0, interp_order=1, cyclic_xboundary=True, gauss_sigma=None, fd_fp32_cast=True,
                   tensor_layout="reference", noncyclic_clamp=None):
        """:meth:`lcs` over ``n_windows`` sliding windows of one packed field: window ``m`` runs ``nsteps`` steps from level
        ``t0 + m * t0_stride``.  Returns ``{"sigma", "x_dep", "y_dep"}`` as ``(n_windows, ny, nx)`` device tensors; entry ``m``
        equals ``lcs(field, ..., t0=t0 + m * t0_stride, nsteps=nsteps)`` bit for bit.

        One ``lc_advect_series`` call (every window in one launch per level chunk; with the reference's non-cyclic clamp each
        window decides on its own whether and from which chunk it re-runs sub-step by sub-step) and one ``lc_sigma_batch``
        call per group of windows; groups are as large as ``SERIES_MEM_CAP`` allows (:meth:`series_group`), and the results
        do not depend on the grouping."""
        x, y, (sig,) = self._windowed("lcs_series", self._sigma_planes(tensor_layout), field, seed_lat, seed_lon, timestep, nsteps,
                                      n_windows, t0, t0_stride, SETTLS_order, interp_order, cyclic_xboundary, gauss_sigma,
                                      fd_fp32_cast, noncyclic_clamp)
        return {"sigma": sig, "x_dep": x, "y_dep": y}

    def lcs_bidirectional(self, field: PackedField, seed_lat, seed_lon, timestep, nsteps: int, n_windows: int = 1, t0=0,
                          t0_stride=1, SETTLS_order=0, interp_order=1, cyclic_xboundary=True, gauss_sigma=None,
                          fd_fp32_cast=True, tensor_layout="reference", noncyclic_clamp=None):
        """:meth:`lcs_series` in both directions of time: the attracting (backward, ``-|timestep|``) and the repelling
        (forward, ``+|timestep|``) field of every window.  Returns ``{"sigma", "x_dep", "y_dep"}`` as ``(2, n_windows, ny, nx)``
        device tensors; entry ``[d, w]`` equals ``lcs(field, ..., timestep=(-1, +1)[d] * |timestep|, t0=t0 + w * t0_stride,
        nsteps=nsteps)`` bit for bit.

        One ``lc_advect_series_dirs`` call (both directions of every window in one launch per level chunk) and one
        ``lc_sigma_batch`` call per group of windows; a group counts two planes per window against ``SERIES_MEM_CAP``, and the
        results do not depend on the grouping."""
        x, y, (sig,) = self._windowed("lcs_bidirectional", self._sigma_planes(tensor_layout), field, seed_lat, seed_lon, timestep,
                                      nsteps, n_windows, t0, t0_stride, SETTLS_order, interp_order, cyclic_xboundary, gauss_sigma,
                                      fd_fp32_cast, noncyclic_clamp, n_dirs=2)
        return {k: t.transpose(0, 1).contiguous() for k, t in (("sigma", sig), ("x_dep", x), ("y_dep", y))}

    def sigma_batch(self, x_dep, y_dep, seed_lat, dlat, dlon, fd_fp32_cast=True, tensor_layout="reference"):
        """sigma_max of ``n`` whole grids at once (``lc_sigma_batch``): ``x_dep``, ``y_dep`` ``(n, ny, nx)``; plane ``m`` of the
        result equals :meth:`sigma` of plane ``m`` bit for bit."""
        torch = self.torch
        dtype = np.dtype(str(x_dep.dtype).replace("torch.", "")) if isinstance(x_dep, torch.Tensor) else common_dtype(x_dep, y_dep)
        xd, yd = self.to_device(x_dep, dtype), self.to_device(y_dep, dtype)
        if xd.dim() != 3 or tuple(yd.shape) != tuple(xd.shape):
            raise ValueError("x_dep and y_dep must both be (n, ny, nx)")
        n, ny, nx = (int(s) for s in xd.shape)
        slat = self.to_device(seed_lat, dtype)
        if slat.numel() != ny:
            raise ValueError("seed_lat must have one latitude per row")
        sig = self._empty((n, ny, nx), dtype)
        self._use_current_stream()
        _capi.check(self.lib.lc_sigma_batch(self.ctx, self._ptr(xd), self._ptr(yd), _NP2LC[dtype], ny, nx, self._ptr(slat), float(dlat),
                                            float(dlon), int(bool(fd_fp32_cast)), _LAYOUTS[tensor_layout], n, self._ptr(sig)), self.lib)
        return sig

    # ------------------------------------------------------------------ stretch factors and direction
    _STRAIN_PLANES = ("s1", "s2", "e_lon", "e_lat")

    def last_strain_kernel(self) -> str:
        """Name of the kernel the last :meth:`strain` call launched (``lc_ctx_last_strain_kernel``)."""
        return self.lib.lc_ctx_last_strain_kernel(self.ctx).decode()

    def strain(self, x_dep, y_dep, seed_lat, dlat, dlon, fd_fp32_cast=True, want=("s1", "s2", "e_lon", "e_lat")) -> dict:
        """Both singular values ``s1 >= s2`` of the 3 x 2 flow-map Jacobian (the physical layout, not the reference's 3 x 3
        reshape: ``s1`` is :meth:`sigma` with ``tensor_layout="physical"``, bit for bit in float64) and the unit direction
        ``(e_lon, e_lat)`` at the seed that is stretched by ``s1`` (east, north components; ``e_lon > 0``, or ``e_lon == 0``
        and ``e_lat > 0``; ``(1, 0)`` in an isotropic cell), in one launch (``lc_strain``).  ``x_dep``, ``y_dep``: ``(ny, nx)``
        or ``(n, ny, nx)`` whole grids; the result maps each name in ``want`` (``"s1"`` is always computed) to a device tensor
        of the input's shape and dtype.  ``s1 * s2`` is the area change of the flow map."""
        torch = self.torch
        want = tuple(want)
        bad = [w for w in want if w not in self._STRAIN_PLANES]
        if bad or not want:
            raise ValueError(f"want {want!r}: a non-empty subset of {self._STRAIN_PLANES}")
        dtype = np.dtype(str(x_dep.dtype).replace("torch.", "")) if isinstance(x_dep, torch.Tensor) else common_dtype(x_dep, y_dep)
        xd, yd = self.to_device(x_dep, dtype), self.to_device(y_dep, dtype)
        if xd.dim() not in (2, 3) or tuple(yd.shape) != tuple(xd.shape):
            raise ValueError("x_dep and y_dep must both be (ny, nx) or (n, ny, nx)")
        shape = tuple(int(s) for s in xd.shape)
        ny, nx = shape[-2:]
        n = shape[0] if len(shape) == 3 else 1
        slat = self.to_device(seed_lat, dtype)
        if slat.numel() != ny:
            raise ValueError("seed_lat must have one latitude per row")
        out = {k: self._empty(shape, dtype) for k in self._STRAIN_PLANES if k in want or k == "s1"}
        self._use_current_stream()
        _capi.check(self.lib.lc_strain(self.ctx, self._ptr(xd), self._ptr(yd), _NP2LC[dtype], ny, nx, self._ptr(slat), float(dlat),
                                       float(dlon), int(bool(fd_fp32_cast)), n,
                                       *(self._ptr(out.get(k)) for k in self._STRAIN_PLANES)), self.lib)
        return {k: out[k] for k in want}

    def lcs_strain(self, field: PackedField, seed_lat, seed_lon, timestep, nsteps: int, n_windows: int = 1, t0=0, t0_stride=1,
                   SETTLS_order=0, interp_order=1, cyclic_xboundary=True, gauss_sigma=None, fd_fp32_cast=True,
                   noncyclic_clamp=None):
        """:meth:`lcs_series`' advection (same arguments, same kernels: window ``m`` runs ``nsteps`` steps from level
        ``t0 + m * t0_stride``) followed by :meth:`strain` instead of sigma: one ``lc_advect_series`` call and one ``lc_strain``
        call per memory group.  Returns ``{"s1", "s2", "e_lon", "e_lat", "x_dep", "y_dep"}`` as ``(n_windows, ny, nx)`` device
        tensors; ``x_dep`` / ``y_dep`` equal :meth:`lcs_series`' bit for bit.  ``gauss_sigma`` smooths the departure fields
        first, as there."""
        x, y, outs = self._windowed("lcs_strain", lambda head, planes, outs: self.lib.lc_strain(*head, planes, *outs), field, seed_lat,
                                    seed_lon, timestep, nsteps, n_windows, t0, t0_stride, SETTLS_order, interp_order, cyclic_xboundary,
                                    gauss_sigma, fd_fp32_cast, noncyclic_clamp, extra_planes=len(self._STRAIN_PLANES) - 1)
        return {**dict(zip(self._STRAIN_PLANES, outs)), "x_dep": x, "y_dep": y}

    # ------------------------------------------------------------------ auxiliary-grid gradient
    _AUX_OUTPUTS = ("sigma", "s1", "s2", "e_lon", "e_lat")
    _AUX_PLANES = ("x_e", "y_e", "x_w", "y_w", "x_n", "y_n", "x_s", "y_s")     # lc_aux_gradient_args' order

    @staticmethod
    def aux_seeds(seed_lat, seed_lon, delta, field_box, dtype) -> "AuxSeeds":
        """The four shifted seed coordinate arrays of an auxiliary grid and what the gradient divides by (:class:`AuxSeeds`).

        ``delta``: the offset in degrees, a positive float or ``(dlat, dlon)``.  ``field_box``: ``(lat_min, lat_max, lon_min,
        lon_max)`` of the wind field.  Everything is evaluated in ``dtype``, as the advect kernels will read it: ``lat + d``
        is rounded, so the separations ``lat_n - lat_s`` and ``lon_e - lon_w`` are taken from the rounded arrays (in float32
        the nominal ``2 d`` is wrong by up to 8e-4 relative at ``d = 0.01``).  A row is valid iff ``lat - d >= lat_min`` and
        ``lat + d <= lat_max``, a column iff ``lon -+ d`` lies inside ``[lon_min, lon_max]`` -- for a cyclic field too: the
        seam columns of a global field are invalid.  Shifted coordinates are clipped into the box, so no seed starts outside
        the field; invalid rows and columns get a NaN separation, which is how ``lc_aux_gradient`` learns of them."""
        dtype = np.dtype(dtype)
        if dtype not in _NP2LC:
            raise ValueError(f"aux_seeds: dtype {dtype} (float32 or float64)")
        try:
            dlat, dlon = (float(d) for d in (delta if np.ndim(delta) else (delta, delta)))
        except (TypeError, ValueError):
            raise ValueError(f"aux_seeds: delta {delta!r}: a positive number of degrees, or (dlat, dlon)") from None
        if not (np.isfinite(dlat) and np.isfinite(dlon) and dlat > 0 and dlon > 0):
            raise ValueError(f"aux_seeds: delta {delta!r}: a positive number of degrees, or (dlat, dlon)")
        lat_min, lat_max, lon_min, lon_max = (dtype.type(b) for b in field_box)
        if not (lat_min <= lat_max and lon_min <= lon_max):
            raise ValueError(f"aux_seeds: field_box {tuple(field_box)!r}: (lat_min, lat_max, lon_min, lon_max)")
        lat, lon = np.asarray(seed_lat, dtype=dtype), np.asarray(seed_lon, dtype=dtype)
        if lat.ndim != 1 or lon.ndim != 1 or not lat.size or not lon.size:
            raise ValueError("aux_seeds: seed_lat and seed_lon must be non-empty 1-D arrays")

        def shifted(c, d, lo, hi):
            plus, minus = c + dtype.type(d), c - dtype.type(d)                 # rounded in the dtype
            with np.errstate(invalid="ignore"):
                valid = (minus >= lo) & (plus <= hi)                           # (a NaN coordinate is invalid)
            plus, minus = np.clip(plus, lo, hi), np.clip(minus, lo, hi)
            sep = np.where(valid, plus - minus, dtype.type("nan")).astype(dtype)
            return plus, minus, sep, valid
        lat_n, lat_s, sep_lat, row_valid = shifted(lat, dlat, lat_min, lat_max)
        lon_e, lon_w, sep_lon, col_valid = shifted(lon, dlon, lon_min, lon_max)
        return AuxSeeds(lat_n, lat_s, lon_e, lon_w, sep_lat, sep_lon, row_valid, col_valid)

    def last_aux_kernel(self) -> str:
        """Name of the kernel the last :meth:`aux_gradient` call launched (``lc_ctx_last_aux_kernel``)."""
        return self.lib.lc_ctx_last_aux_kernel(self.ctx).decode()

    def _aux_call(self, planes, dtype, ny, nx, n, slat, sep_lat, sep_lon, tensor_layout, outs):
        """One ``lc_aux_gradient`` call: ``planes`` the eight device tensors in ``_AUX_PLANES``' order, ``outs`` name -> tensor."""
        a = _capi.AuxGradientArgs(struct_size=C.sizeof(_capi.AuxGradientArgs), dtype=_NP2LC[np.dtype(dtype)], ny=int(ny), nx=int(nx),
                                  n_members=int(n), seed_lat_dev=slat.data_ptr(), sep_lat_dev=sep_lat.data_ptr(),
                                  sep_lon_dev=sep_lon.data_ptr(), tensor_layout=_LAYOUTS[tensor_layout],
                                  **{k: t.data_ptr() for k, t in zip(self._AUX_PLANES, planes)},
                                  **{k + "_out": t.data_ptr() for k, t in outs.items()})
        self._use_current_stream()
        _capi.check(self.lib.lc_aux_gradient(self.ctx, C.byref(a)), self.lib)

    def _aux_want(self, want):
        want = tuple(want)
        if not want or any(w not in self._AUX_OUTPUTS for w in want):
            raise ValueError(f"want {want!r}: a non-empty subset of {self._AUX_OUTPUTS}")
        return want

    def aux_gradient(self, planes, seed_lat, sep_lat, sep_lon, want=("sigma", "s1", "s2", "e_lon", "e_lat"),
                     tensor_layout="reference") -> dict:
        """sigma, both stretch factors and the stretching direction from the departure points of an auxiliary grid, in one
        launch (``lc_aux_gradient``).  ``planes``: the eight planes ``x_e, y_e, x_w, y_w, x_n, y_n, x_s, y_s`` (a mapping by
        these names, or a sequence in this order), each ``(ny, nx)`` or ``(n, ny, nx)``: the departure points of the parcels
        seeded east, west, north and south of every output point.  ``seed_lat``: the output rows' latitudes; ``sep_lat``
        ``(ny,)`` and ``sep_lon`` ``(nx,)``: the separations of the shifted seed coordinates (:meth:`aux_seeds`; NaN marks a row
        or column as invalid).  Returns each name in ``want`` as a device tensor of the input's shape and dtype: ``s1``,
        ``s2``, ``e_lon``, ``e_lat`` as :meth:`strain` defines them, ``sigma`` in ``tensor_layout`` (``"physical"``: equal to
        ``s1``).  A NaN input gives NaN in that cell's outputs only."""
        torch = self.torch
        want = self._aux_want(want)
        if tensor_layout not in _LAYOUTS:
            raise ValueError(f"tensor_layout {tensor_layout!r}")
        seq = [planes[k] for k in self._AUX_PLANES] if hasattr(planes, "keys") else list(planes)
        if len(seq) != 8:
            raise ValueError(f"planes: the eight planes {self._AUX_PLANES}")
        dtype = (np.dtype(str(seq[0].dtype).replace("torch.", "")) if all(isinstance(p, torch.Tensor) for p in seq)
                 else common_dtype(*seq))
        dev = [self.to_device(p, dtype) for p in seq]
        shape = tuple(int(s) for s in dev[0].shape)
        if len(shape) not in (2, 3) or any(tuple(p.shape) != shape for p in dev):
            raise ValueError("planes must all be (ny, nx) or all (n, ny, nx)")
        ny, nx = shape[-2:]
        n = shape[0] if len(shape) == 3 else 1
        slat, dla, dlo = self.to_device(seed_lat, dtype), self.to_device(sep_lat, dtype), self.to_device(sep_lon, dtype)
        if slat.numel() != ny or dla.numel() != ny or dlo.numel() != nx:
            raise ValueError("seed_lat and sep_lat must have one entry per row, sep_lon one per column")
        out = {k: self._empty(shape, dtype) for k in self._AUX_OUTPUTS if k in want}
        self._aux_call(dev, dtype, ny, nx, n, slat, dla, dlo, tensor_layout, out)
        return {k: out[k] for k in want}

    def aux_group(self, dtype, n_seeds: int, n_windows: int, cyclic_xboundary=True, n_outputs: int = 1, centre=False) -> int:
        """Windows per group of :meth:`lcs_aux`: as many as fit ``SERIES_MEM_CAP`` (at least one).  Per window: the eight
        position planes, the ``n_outputs`` result planes, the centre grid's two, and -- under the reference's non-cyclic clamp --
        the four scratch planes of the advect call that is running (:meth:`series_group`).  ``n_seeds`` counts both directions."""
        planes = 8 + int(n_outputs) + (2 if centre else 0) + (0 if cyclic_xboundary else 4)
        per = planes * int(n_seeds) * np.dtype(dtype).itemsize
        return max(1, min(int(n_windows), int(self.SERIES_MEM_CAP) // max(per, 1)))

    def lcs_aux(self, field: PackedField, seed_lat, seed_lon, timestep, nsteps: int, n_windows: int = 1, t0=0, t0_stride=1,
                SETTLS_order=0, interp_order=1, cyclic_xboundary=True, gauss_sigma=None, tensor_layout="reference",
                noncyclic_clamp=None, *, aux_delta, n_dirs=1, want=("sigma",), centre=False, return_planes=False) -> dict:
        """FTLE from an auxiliary grid (Haller): four parcels per output point, seeded ``aux_delta`` degrees east, west, north
        and south of it, are advected through the windows of :meth:`lcs_series` (same arguments: window ``m`` runs ``nsteps``
        steps from level ``t0 + m * t0_stride``), and the flow-map gradient at the point is the centred difference of their
        departure points (:meth:`aux_gradient`).  The gradient is local: its accuracy is set by ``aux_delta``, not by the output
        spacing; there is no neighbour stencil, so no cyclic seam, no one-sided rows and no NaN halo.

        Per memory group (:meth:`aux_group`; results do not depend on the grouping) four ``lc_advect_series`` calls -- for
        ``n_dirs = 2`` four ``lc_advect_series_dirs`` calls, ``timestep``'s sign then ignored as in :meth:`lcs_bidirectional`
        --, one per shifted grid (:meth:`aux_seeds` on the field's box: shifted seeds are clipped into it), each exactly what
        :meth:`advect` returns for that seed grid, then one ``lc_aux_gradient`` call.  ``centre=True``: a fifth advect call on
        the unshifted grid, returned as ``x_dep`` / ``y_dep`` (:meth:`lcs_series`' bits).

        Returns the names in ``want`` (``sigma`` in ``tensor_layout``, ``s1``, ``s2``, ``e_lon``, ``e_lat``) as ``(n_windows, ny,
        nx)`` device tensors, ``(2, n_windows, ny, nx)`` for ``n_dirs = 2`` (backward first); ``"seeds"``: the :class:`AuxSeeds`
        (rows and columns it marks invalid -- within ``aux_delta`` of the field's edge, the seam columns of a global field
        included -- are NaN); with ``return_planes`` the eight position planes by name.  ``gauss_sigma`` is refused: smoothing
        departure fields across seeds contradicts a local gradient."""
        if _smoothing_width(gauss_sigma) > 1e-15:
            raise ValueError("lcs_aux: gauss_sigma smooths the departure fields across seeds, which contradicts the auxiliary grid's "
                             "local gradient; use one or the other")
        _check_order(field, interp_order)
        want = self._aux_want(want)
        if tensor_layout not in _LAYOUTS:
            raise ValueError(f"tensor_layout {tensor_layout!r}")
        if n_dirs not in (1, 2):
            raise ValueError(f"lcs_aux: n_dirs {n_dirs!r} (1 or 2)")
        if n_dirs == 2:
            timestep = float(timestep)
            if not timestep or not np.isfinite(timestep):
                raise ValueError(f"lcs_aux: timestep {timestep} (non-zero: its sign is taken from the direction)")
            timestep = -abs(timestep)
        n_windows, nsteps, t0, t0_stride = int(n_windows), int(nsteps), int(t0), int(t0_stride)
        if n_windows < 1 or nsteps < 0 or t0 < 0 or t0_stride < 0:
            raise ValueError(f"lcs_aux: n_windows {n_windows}, nsteps {nsteps}, t0 {t0}, t0_stride {t0_stride}")
        dtype = field.dtype
        seed_lat, seed_lon = np.asarray(seed_lat, dtype=dtype), np.asarray(seed_lon, dtype=dtype)
        seeds = self.aux_seeds(seed_lat, seed_lon, aux_delta, (field.lat_min, field.lat_max, field.lon_min, field.lon_max), dtype)
        dev = lambda a: self.to_device(a, dtype)
        slat, slon = dev(seed_lat), dev(seed_lon)
        ny, nx = int(slat.numel()), int(slon.numel())
        # the seed grids in _AUX_PLANES' order: east, west, north, south
        grids = ((slat, dev(seeds.lon_e)), (slat, dev(seeds.lon_w)), (dev(seeds.lat_n), slon), (dev(seeds.lat_s), slon))
        sep_lat, sep_lon = dev(seeds.sep_lat), dev(seeds.sep_lon)
        xmode = x_boundary_mode(cyclic_xboundary, noncyclic_clamp, True)
        tail = (ny, nx) if n_dirs == 1 else (n_dirs, ny, nx)      # the library's plane order: window-major, plane 2w + d
        g = self.aux_group(dtype, n_dirs * ny * nx, n_windows, cyclic_xboundary, len(want), centre)
        outs = {k: self._empty((n_windows, *tail), dtype) for k in self._AUX_OUTPUTS if k in want}
        # the position planes: of every window if they are returned, else of one group (reused by the next)
        pos = [self._empty((n_windows if return_planes else g, *tail), dtype) for _ in self._AUX_PLANES]
        x = y = None
        if centre:
            x, y = self._empty((n_windows, *tail), dtype), self._empty((n_windows, *tail), dtype)

        def advect(la, lo, m0, n, xg, yg):
            self._use_current_stream()
            a = self._advect_args(field, interp_order, la, ny, lo, nx, timestep, SETTLS_order, xmode,
                                  t0=t0 + m0 * t0_stride, nsteps=nsteps, n_members=n, t0_stride=t0_stride, out=(xg, yg))
            _capi.check(self.lib.lc_advect_series(self.ctx, C.byref(a)) if n_dirs == 1 else
                        self.lib.lc_advect_series_dirs(self.ctx, C.byref(a), n_dirs), self.lib)
        for m0 in range(0, n_windows, g):
            n = min(g, n_windows - m0)
            p0 = m0 if return_planes else 0
            group = [p[p0:p0 + n] for p in pos]
            for i, (la, lo) in enumerate(grids):
                advect(la, lo, m0, n, group[2 * i], group[2 * i + 1])
            if centre:
                advect(slat, slon, m0, n, x[m0:m0 + n], y[m0:m0 + n])
            self._aux_call(group, dtype, ny, nx, n_dirs * n, slat, sep_lat, sep_lon, tensor_layout,
                           {k: t[m0:m0 + n] for k, t in outs.items()})
        # two directions: (n_windows, 2, ...) -> (2, n_windows, ...), as lcs_bidirectional
        shape_out = (lambda t: t) if n_dirs == 1 else (lambda t: t.transpose(0, 1).contiguous())
        res = {k: shape_out(outs[k]) for k in want}
        res["seeds"] = seeds
        if centre:
            res["x_dep"], res["y_dep"] = shape_out(x), shape_out(y)
        if return_planes:
            res.update({k: shape_out(p) for k, p in zip(self._AUX_PLANES, pos)})
        return res

    # ------------------------------------------------------------------ finite-size Lyapunov exponents
    _FSLE_MODES = {"ratio": _capi.LC_FSLE_RATIO, "distance": _capi.LC_FSLE_DISTANCE}
    FSLE_MAX_THRESHOLDS = 8

    def last_fsle_kernel(self) -> str:
        """Name of the kernel the last :meth:`fsle_update` call launched (``lc_ctx_last_fsle_kernel``)."""
        return self.lib.lc_ctx_last_fsle_kernel(self.ctx).decode()

    @classmethod
    def checked_fsle_options(cls, thresholds, mode, timestep, radius=6371000.0, dtype=None):
        """``(thresholds, mode, timestep, radius)`` as :meth:`fsle_update` hands them to the library, or ``ValueError``: 1 to 8
        finite thresholds (a scalar is one), each ``> 1`` for ``mode='ratio'`` and ``> 0`` (metres) for ``mode='distance'`` --
        with ``dtype`` also once rounded to it, as the kernel sees them (a float32 ratio of ``1 + 1e-9`` is 1) --; a non-zero
        finite ``timestep`` (its sign only names the direction the record was advected in); a positive finite radius."""
        if mode not in cls._FSLE_MODES:
            raise ValueError(f"fsle: mode {mode!r} ('ratio' or 'distance')")
        try:
            thr = np.atleast_1d(np.asarray(thresholds, dtype=np.float64))
        except (TypeError, ValueError):
            raise ValueError(f"fsle: thresholds {thresholds!r}: 1 to {cls.FSLE_MAX_THRESHOLDS} numbers") from None
        if thr.ndim != 1 or not 1 <= thr.size <= cls.FSLE_MAX_THRESHOLDS:
            raise ValueError(f"fsle: {thr.size} thresholds (1 to {cls.FSLE_MAX_THRESHOLDS}, one-dimensional)")
        with np.errstate(over="ignore"):
            seen = thr if dtype is None else thr.astype(dtype).astype(np.float64)
        if not np.all(np.isfinite(seen)) or np.any(seen <= (1.0 if mode == "ratio" else 0.0)):
            raise ValueError(f"fsle: thresholds {thr.tolist()}: finite, and > 1 as ratios / > 0 metres as distances"
                             + ("" if dtype is None else f" once rounded to {np.dtype(dtype).name}"))
        try:
            timestep, radius = float(timestep), float(radius)
        except (TypeError, ValueError):
            raise ValueError(f"fsle: timestep {timestep!r}, radius {radius!r}") from None
        if not np.isfinite(timestep) or timestep == 0:
            raise ValueError(f"fsle: timestep {timestep} (non-zero and finite)")
        if not np.isfinite(radius) or radius <= 0:
            raise ValueError(f"fsle: radius {radius} (positive and finite)")
        return thr, mode, timestep, radius

    def fsle_update(self, traj_x, traj_y, seed_lat, seed_lon, thresholds, mode, timestep, level0, tau=None, fsle=None, cyclic=False,
                    radius=6371000.0):
        """One block of trajectory levels folded into the finite-size Lyapunov exponent (``lc_fsle_update``; the definition is in
        include/lcs_hip.h and restated in tests/fsle.py).  ``traj_x``, ``traj_y``: ``(n_levels, ny, nx)`` positions in degrees
        after ``level0``, ``level0 + 1``, ... steps (:meth:`advect` with ``return_traj=True``), ``n_levels >= 2``; entry 0 of a
        continued block (``level0 > 0``) is the last entry of the block before.  ``thresholds``: 1 to 8 ratios (``mode='ratio'``:
        a pair crosses when its separation reaches that multiple of its initial one) or final separations in metres
        (``mode='distance'``).  ``tau``, ``fsle``: the ``(n_thr, ny, nx)`` tensors the previous block returned -- they are updated
        in place and returned; with ``level0 == 0`` they may be omitted (or are overwritten).  ``cyclic``: column ``nx - 1`` pairs
        with column 0.  Returns ``(tau, fsle)``: per threshold and cell the time its first neighbour pair takes to separate to
        the threshold (seconds, positive) and ``ln(T / d0) / tau``, NaN where none does within the levels seen so far."""
        thr, mode, timestep, radius = self.checked_fsle_options(thresholds, mode, timestep, radius)
        level0 = int(level0)
        if level0 < 0:
            raise ValueError(f"fsle_update: level0 {level0}")
        if np.ndim(traj_x) != 3 or tuple(np.shape(traj_x)) != tuple(np.shape(traj_y)):
            raise ValueError("fsle_update: traj_x and traj_y must both be (n_levels, ny, nx)")
        n_levels, ny, nx = (int(s) for s in np.shape(traj_x))
        if n_levels < 2 or ny < 1 or nx < 1 or ny * nx == 1:
            raise ValueError(f"fsle_update: {n_levels} levels of a {ny} x {nx} grid (at least two levels and two seeds)")
        count = lambda a: int(a.numel()) if hasattr(a, "numel") else int(np.size(a))
        if count(seed_lat) != ny or count(seed_lon) != nx:
            raise ValueError("fsle_update: seed_lat must have one entry per row, seed_lon one per column")
        if (tau is None) != (fsle is None) or (tau is None and level0 != 0):
            raise ValueError("fsle_update: tau and fsle go together, and a continued block (level0 > 0) needs both")
        dtype = (np.dtype(str(traj_x.dtype).replace("torch.", "")) if hasattr(traj_x, "data_ptr") and hasattr(traj_y, "data_ptr")
                 else common_dtype(traj_x, traj_y))
        if dtype not in _NP2LC:
            raise ValueError(f"fsle_update: dtype {dtype} (float32 or float64)")
        self.checked_fsle_options(thr, mode, timestep, radius, dtype)
        torch = self.torch
        tx, ty = self.to_device(traj_x, dtype), self.to_device(traj_y, dtype)
        slat, slon = self.to_device(seed_lat, dtype).reshape(-1), self.to_device(seed_lon, dtype).reshape(-1)
        if tau is None:
            tau, fsle = self._empty((thr.size, ny, nx), dtype), self._empty((thr.size, ny, nx), dtype)
        want = getattr(torch, dtype.name)
        for t in (tau, fsle):
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != (thr.size, ny, nx) or t.dtype != want or not t.is_contiguous() \
                    or t.device != self.device:
                raise ValueError(f"fsle_update: tau and fsle must be contiguous ({thr.size}, {ny}, {nx}) {dtype.name} tensors on {self.device}")
        a = _capi.FsleArgs(struct_size=C.sizeof(_capi.FsleArgs), traj_x=tx.data_ptr(), traj_y=ty.data_ptr(), dtype=_NP2LC[dtype],
                           ny=ny, nx=nx, n_levels=n_levels, level0=level0, seed_lat_dev=slat.data_ptr(), seed_lon_dev=slon.data_ptr(),
                           mode=self._FSLE_MODES[mode], n_thr=int(thr.size), thresholds=(C.c_double * 8)(*thr.tolist()),
                           radius=radius, timestep=timestep, cyclic_x=int(bool(cyclic)), tau=tau.data_ptr(), fsle=fsle.data_ptr())
        self._use_current_stream()
        _capi.check(self.lib.lc_fsle_update(self.ctx, C.byref(a)), self.lib)
        return tau, fsle

    def fsle(self, field: PackedField, seed_lat, seed_lon, timestep, thresholds, mode="ratio", t0=0, nsteps=None, level_chunk=16,
             SETTLS_order=0, interp_order=1, cyclic_xboundary=True, noncyclic_clamp=None, radius=6371000.0) -> dict:
        """Finite-size Lyapunov exponents of the seed grid's neighbour pairs over ``nsteps`` steps from level ``t0`` of a packed
        field: ``{'tau', 'fsle'}`` as ``(n_thr, ny, nx)`` device tensors (:meth:`fsle_update`) and the departure points ``'x_dep'``,
        ``'y_dep'`` of :meth:`advect`.  The record is streamed: ``advect(start=(x, y), out=(x, y), nsteps=chunk,
        return_traj=True)`` continues in place (bit for bit what one call gives) and each block of ``level_chunk`` steps is folded
        into tau / fsle and dropped, so at most ``level_chunk + 1`` trajectory planes per coordinate are alive at a time; the
        result does not depend on ``level_chunk``.  Pairs close across the ±180 seam with ``cyclic_xboundary``.

        ``cyclic_xboundary=False`` with the default ``reference_outer`` clamp cannot be continued (``lc_advect_from`` refuses it):
        that case makes ONE advect over all levels and one update, and needs the full record -- ``2 (nsteps + 1)`` planes -- in
        device memory.  ``noncyclic_clamp='pointwise'`` streams."""
        thr, mode, timestep, radius = self.checked_fsle_options(thresholds, mode, timestep, radius, field.dtype)
        _check_order(field, interp_order)
        t0 = int(t0)
        nsteps = field.nt - 1 - t0 if nsteps is None else int(nsteps)
        level_chunk = int(level_chunk)
        if t0 < 0 or nsteps < 1 or t0 + nsteps > field.nt - 1:
            raise ValueError(f"fsle: t0 {t0}, nsteps {nsteps} on a record of {field.nt} levels (at least one step, inside the record)")
        if level_chunk < 1:
            raise ValueError(f"fsle: level_chunk {level_chunk} (at least 1)")
        count = lambda a: int(a.numel()) if hasattr(a, "numel") else int(np.size(a))
        if np.ndim(seed_lat) != 1 or np.ndim(seed_lon) != 1 or count(seed_lat) * count(seed_lon) < 2:
            raise ValueError("fsle: seed_lat and seed_lon must be 1-D and hold at least two seeds between them")
        xmode = x_boundary_mode(cyclic_xboundary, noncyclic_clamp, True)
        kw = dict(SETTLS_order=SETTLS_order, interp_order=interp_order, cyclic_xboundary=cyclic_xboundary, noncyclic_clamp=noncyclic_clamp)
        if xmode == _capi.LC_X_CLAMP_REFERENCE_OUTER:
            level_chunk = nsteps               # one block: the clamp is decided over the whole grid, level by level, inside one call
        cyclic = xmode == _capi.LC_X_CYCLIC
        x = y = tau = fsle = None
        for done in range(0, nsteps, level_chunk):
            n = min(level_chunk, nsteps - done)
            x, y, tx, ty = self.advect(field, seed_lat, seed_lon, timestep, t0=t0 + done, nsteps=n, return_traj=True,
                                       start=None if done == 0 else (x, y), out=None if done == 0 else (x, y), **kw)
            tau, fsle = self.fsle_update(tx, ty, seed_lat, seed_lon, thr, mode, timestep, done, tau, fsle, cyclic=cyclic, radius=radius)
            del tx, ty
        return {"tau": tau, "fsle": fsle, "x_dep": x, "y_dep": y}

    # ------------------------------------------------------------------ vorticity, LAVD, rotation and path length
    _VORT_DEVIATIONS = {"domain": _capi.LC_VORT_DEVIATION_DOMAIN, "none": _capi.LC_VORT_DEVIATION_NONE}
    GRID_UNIFORM_RTOL = 1e-3     # a coordinate step may differ from the mean step by this fraction (float32 coordinates round)

    def last_vorticity_kernel(self) -> str:
        """Names of the kernels the last :meth:`vorticity` call launched (``lc_ctx_last_vorticity_kernel``)."""
        return self.lib.lc_ctx_last_vorticity_kernel(self.ctx).decode()

    def last_lavd_kernel(self) -> str:
        """Name of the kernel the last :meth:`lavd_update` call launched (``lc_ctx_last_lavd_kernel``)."""
        return self.lib.lc_ctx_last_lavd_kernel(self.ctx).decode()

    @classmethod
    def checked_deviation(cls, deviation, nt=None):
        """``(mode, given)`` of a ``deviation`` argument, or ``ValueError``: ``'domain'`` (subtract each level's area-weighted
        mean), ``'none'``, or one finite number per time level (``given``: float64, 1-D; checked against ``nt`` when it is
        known)."""
        if isinstance(deviation, str):
            if deviation not in cls._VORT_DEVIATIONS:
                raise ValueError(f"vorticity: deviation {deviation!r} ('domain', 'none' or one value per time level)")
            return cls._VORT_DEVIATIONS[deviation], None
        try:
            given = np.asarray(deviation, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"vorticity: deviation {deviation!r} ('domain', 'none' or one value per time level)") from None
        if given.ndim != 1 or given.size < 1 or not np.all(np.isfinite(given)):
            raise ValueError("vorticity: a given deviation is one finite value per time level, one-dimensional")
        if nt is not None and given.size != int(nt):
            raise ValueError(f"vorticity: {given.size} deviation values for {int(nt)} time levels")
        return _capi.LC_VORT_DEVIATION_GIVEN, np.ascontiguousarray(given)

    @classmethod
    def checked_vorticity_options(cls, u_shape, v_shape, lat_f, lon_f, deviation="domain", radius=6371000.0):
        """``(nt, ny_f, nx_f, mode, given, radius)`` as :meth:`vorticity` hands them to the library, or ``ValueError``: ``u`` and
        ``v`` of one ``(time, latitude, longitude)`` shape with at least 4 rows and 4 columns; finite, ascending, uniformly
        spaced coordinates of those lengths, latitudes within -90 .. 90; a ``deviation`` :meth:`checked_deviation` accepts for
        that many levels; a positive finite radius."""
        u_shape, v_shape = tuple(int(s) for s in u_shape), tuple(int(s) for s in v_shape)
        if len(u_shape) != 3 or u_shape != v_shape:
            raise ValueError("vorticity: u and v must both be (time, latitude, longitude)")
        nt, ny_f, nx_f = u_shape
        if nt < 1 or ny_f < 4 or nx_f < 4:
            raise ValueError(f"vorticity: a record of {nt} x {ny_f} x {nx_f} (at least one level of 4 x 4 nodes)")
        try:
            lat, lon = np.asarray(lat_f, dtype=np.float64), np.asarray(lon_f, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("vorticity: latitude and longitude must be numbers") from None
        if lat.shape != (ny_f,) or lon.shape != (nx_f,):
            raise ValueError("vorticity: coordinate lengths do not match the wind")
        for c, what in ((lat, "latitude"), (lon, "longitude")):
            d = np.diff(c)
            if not np.all(np.isfinite(c)) or not np.all(d > 0):
                raise ValueError(f"vorticity: {what} must be finite and ascending (sort first)")
            if np.max(np.abs(d - d.mean())) > cls.GRID_UNIFORM_RTOL * d.mean():
                raise ValueError(f"vorticity: {what} must be uniformly spaced (regrid first)")
        if lat[0] < -90.0 or lat[-1] > 90.0:
            raise ValueError(f"vorticity: latitudes {lat[0]} .. {lat[-1]} outside -90 .. 90")
        mode, given = cls.checked_deviation(deviation, nt)
        try:
            radius = float(radius)
        except (TypeError, ValueError):
            raise ValueError(f"vorticity: radius {radius!r}") from None
        if not np.isfinite(radius) or radius <= 0:
            raise ValueError(f"vorticity: radius {radius} (positive and finite)")
        return nt, ny_f, nx_f, mode, given, radius

    def vorticity(self, u, v, lat_f, lon_f, cyclic=False, deviation="domain", radius=6371000.0, dtype=None) -> dict:
        """Relative vorticity of a wind record on the sphere (``lc_vorticity``; the definition is in include/lcs_hip.h and
        restated in tests/lavd.py): ``{'omega': (nt, ny_f, nx_f) device tensor of the compute dtype, 'level_mean': (nt,) float64
        device tensor}``.  ``omega = (dv/dlambda - d(u cos phi)/dphi) / (R cos phi)`` with centred differences, second-order
        one-sided ones at the first and last row (and column, unless ``cyclic``: then centred across the seam), the adjacent row's
        mean on a pole row, NaN where a stencil holds a non-finite wind.  ``level_mean[t]`` is the ``cos phi``-weighted mean of
        level ``t`` over its finite nodes.  ``deviation='domain'`` subtracts it from level ``t``, ``'none'`` leaves ``omega`` as it
        is, an array subtracts one given value per level; ``level_mean`` is returned in every case.  The grid must be uniform and
        ascending.  ``dtype``: the compute dtype; default float32 only if every input is."""
        nt, ny_f, nx_f, mode, given, radius = self.checked_vorticity_options(np.shape(u), np.shape(v), lat_f, lon_f, deviation, radius)
        lat, lon = np.asarray(lat_f), np.asarray(lon_f)
        dtype = np.dtype(dtype or common_dtype(u, v, lat, lon))
        if dtype not in _NP2LC:
            raise ValueError(f"vorticity: dtype {dtype} (float32 or float64)")
        elems = int(self.lib.lc_vorticity_work_elems(nt, ny_f, nx_f))
        if elems == 0:
            raise ValueError(f"vorticity: a record of {nt} x {ny_f} x {nx_f} is too large for one call")
        du, dv = self.to_device(u, dtype), self.to_device(v, dtype)
        omega = self._empty((nt, ny_f, nx_f), dtype)
        mean = self._empty((nt,), np.float64)
        work = self._empty((elems,), np.float64)
        gdev = self.to_device(given, np.float64) if given is not None else None
        a = _capi.VorticityArgs(struct_size=C.sizeof(_capi.VorticityArgs), u=du.data_ptr(), v=dv.data_ptr(), dtype=_NP2LC[dtype], nt=nt,
                                ny_f=ny_f, nx_f=nx_f, lat_min=float(lat[0]), lat_max=float(lat[-1]), lon_min=float(lon[0]),
                                lon_max=float(lon[-1]), cyclic_x=int(bool(cyclic)), deviation=mode, radius=radius,
                                given_dev=gdev.data_ptr() if gdev is not None else None, omega=omega.data_ptr(),
                                level_mean=mean.data_ptr(), work_dev=work.data_ptr())
        self._use_current_stream()
        _capi.check(self.lib.lc_vorticity(self.ctx, C.byref(a)), self.lib)
        return {"omega": omega, "level_mean": mean}

    def lavd_update(self, traj_x, traj_y, c, timestep, level0, acc=None, final=False, radius=6371000.0) -> dict:
        """One block of trajectory levels folded into the running integrals of LAVD, rotation and path length
        (``lc_lavd_update``; the definition is in include/lcs_hip.h and restated in tests/lavd.py).  ``traj_x``, ``traj_y``:
        ``(n_levels, ...)`` positions in degrees after ``level0``, ``level0 + 1``, ... steps, ``n_levels >= 2``; entry 0 of a
        continued block (``level0 > 0``) is the last entry of the block before.  ``c``: the vorticity deviation sampled at the
        same entries (:meth:`sample_tracer`), or None for the path length alone.  ``acc``: the ``(3, ...)`` float64 tensor the
        previous block returned -- updated in place; with ``level0 == 0`` it may be omitted (or is overwritten).  Returns
        ``{'acc'}`` and, with ``final``, ``'lavd'`` (the integral of ``|c|`` over time, trapezoid rule), ``'rotation'`` (the signed
        integral) -- both None without ``c`` -- and ``'length'`` (metres), each of the trajectories' dtype and shape
        ``traj_x.shape[1:]``."""
        try:
            timestep, radius = float(timestep), float(radius)
        except (TypeError, ValueError):
            raise ValueError(f"lavd_update: timestep {timestep!r}, radius {radius!r}") from None
        if not np.isfinite(timestep) or timestep == 0:
            raise ValueError(f"lavd_update: timestep {timestep} (non-zero and finite)")
        if not np.isfinite(radius) or radius <= 0:
            raise ValueError(f"lavd_update: radius {radius} (positive and finite)")
        level0 = int(level0)
        if level0 < 0:
            raise ValueError(f"lavd_update: level0 {level0}")
        shape = tuple(int(s) for s in np.shape(traj_x))
        if len(shape) < 2 or shape != tuple(int(s) for s in np.shape(traj_y)) or (c is not None and tuple(int(s) for s in np.shape(c)) != shape):
            raise ValueError("lavd_update: traj_x, traj_y and c must have one shape, (n_levels, ...)")
        n_levels, n = shape[0], int(np.prod(shape[1:]))
        if n_levels < 2 or n < 1 or n >= 1 << 31:
            raise ValueError(f"lavd_update: {n_levels} levels of {n} parcels (at least two levels and one parcel, fewer than 2^31)")
        if acc is None and level0 != 0:
            raise ValueError("lavd_update: a continued block (level0 > 0) needs the acc of the block before")
        on_dev = all(hasattr(a, "data_ptr") for a in (traj_x, traj_y) + (() if c is None else (c,)))
        dtype = np.dtype(str(traj_x.dtype).replace("torch.", "")) if on_dev else common_dtype(traj_x, traj_y, c)
        if dtype not in _NP2LC:
            raise ValueError(f"lavd_update: dtype {dtype} (float32 or float64)")
        torch = self.torch
        tx, ty = self.to_device(traj_x, dtype), self.to_device(traj_y, dtype)
        cd = self.to_device(c, dtype) if c is not None else None
        if acc is None:
            acc = self._empty((3,) + shape[1:], np.float64)
        if not isinstance(acc, torch.Tensor) or tuple(acc.shape) != (3,) + shape[1:] or acc.dtype != torch.float64 \
                or not acc.is_contiguous() or acc.device != self.device:
            raise ValueError(f"lavd_update: acc must be a contiguous {(3,) + shape[1:]} float64 tensor on {self.device}")
        out = [self._empty(shape[1:], dtype) if final and (cd is not None or k == 2) else None for k in range(3)]
        p = lambda t: t.data_ptr() if t is not None else None
        a = _capi.LavdArgs(struct_size=C.sizeof(_capi.LavdArgs), traj_x=tx.data_ptr(), traj_y=ty.data_ptr(), c=p(cd), dtype=_NP2LC[dtype],
                           n=n, n_levels=n_levels, level0=level0, timestep=timestep, radius=radius, acc=acc.data_ptr(), lavd=p(out[0]),
                           rotation=p(out[1]), length=p(out[2]))
        self._use_current_stream()
        _capi.check(self.lib.lc_lavd_update(self.ctx, C.byref(a)), self.lib)
        res = {"acc": acc}
        if final:
            res.update(lavd=out[0], rotation=out[1], length=out[2])
        return res

    def lavd(self, field: PackedField, tracer, seed_lat, seed_lon, timestep, t0=0, nsteps=None, level_chunk=16, SETTLS_order=0,
             interp_order=1, cyclic_xboundary=True, noncyclic_clamp=None, radius=6371000.0) -> dict:
        """LAVD, rotation and path length of the seed grid's parcels over ``nsteps`` steps from level ``t0`` of a packed field:
        ``{'lavd', 'rotation', 'length'}`` as ``(ny, nx)`` device tensors (:meth:`lavd_update`) and the departure points
        ``'x_dep'``, ``'y_dep'`` of :meth:`advect`.  ``tracer``: the vorticity deviation on the wind's grid and time levels
        (:meth:`vorticity`, then :meth:`prepare_tracer`); trajectory entry i is sampled at field level ``t0 + i`` whatever the
        sign of ``timestep``, as :meth:`advect_tracer` samples.  ``tracer=None``: the path length alone (``'lavd'`` and
        ``'rotation'`` are None).

        The record is streamed as :meth:`fsle` streams it: each block of ``level_chunk`` steps is advected from where the last
        one ended (bit for bit what one call gives), sampled and folded, then dropped, so ``2 (level_chunk + 1)`` position planes
        and ``level_chunk + 1`` value planes are alive at a time; the result does not depend on ``level_chunk``.
        ``cyclic_xboundary=False`` with the default ``reference_outer`` clamp cannot be continued and takes one block over all
        levels; ``noncyclic_clamp='pointwise'`` streams."""
        try:
            timestep, radius = float(timestep), float(radius)
        except (TypeError, ValueError):
            raise ValueError(f"lavd: timestep {timestep!r}, radius {radius!r}") from None
        if not np.isfinite(timestep) or timestep == 0:
            raise ValueError(f"lavd: timestep {timestep} (non-zero and finite)")
        if not np.isfinite(radius) or radius <= 0:
            raise ValueError(f"lavd: radius {radius} (positive and finite)")
        _check_order(field, interp_order)
        if tracer is not None:
            if tracer.dtype != field.dtype:
                raise ValueError(f"lavd: tracer dtype {tracer.dtype} differs from the field's compute dtype {field.dtype}")
            if (tracer.nt, tracer.ny_f, tracer.nx_f) != (field.nt, field.ny_f, field.nx_f) or \
                    (tracer.lat_min, tracer.lat_max, tracer.lon_min, tracer.lon_max) != (field.lat_min, field.lat_max, field.lon_min, field.lon_max):
                raise ValueError("lavd: the tracer must lie on the wind's grid and time levels")
            _check_order(tracer, interp_order)
        t0 = int(t0)
        nsteps = field.nt - 1 - t0 if nsteps is None else int(nsteps)
        level_chunk = int(level_chunk)
        if t0 < 0 or nsteps < 1 or t0 + nsteps > field.nt - 1:
            raise ValueError(f"lavd: t0 {t0}, nsteps {nsteps} on a record of {field.nt} levels (at least one step, inside the record)")
        if level_chunk < 1:
            raise ValueError(f"lavd: level_chunk {level_chunk} (at least 1)")
        count = lambda a: int(a.numel()) if hasattr(a, "numel") else int(np.size(a))
        if np.ndim(seed_lat) != 1 or np.ndim(seed_lon) != 1 or count(seed_lat) * count(seed_lon) < 1:
            raise ValueError("lavd: seed_lat and seed_lon must be 1-D and hold at least one seed each")
        xmode = x_boundary_mode(cyclic_xboundary, noncyclic_clamp, True)
        kw = dict(SETTLS_order=SETTLS_order, interp_order=interp_order, cyclic_xboundary=cyclic_xboundary, noncyclic_clamp=noncyclic_clamp)
        if xmode == _capi.LC_X_CLAMP_REFERENCE_OUTER:
            level_chunk = nsteps               # one block: the clamp is decided over the whole grid, level by level, inside one call
        x = y = acc = res = None
        for done in range(0, nsteps, level_chunk):
            n = min(level_chunk, nsteps - done)
            x, y, tx, ty = self.advect(field, seed_lat, seed_lon, timestep, t0=t0 + done, nsteps=n, return_traj=True,
                                       start=None if done == 0 else (x, y), out=None if done == 0 else (x, y), **kw)
            c = None if tracer is None else self.sample_tracer(tracer, tx, ty, level0=t0 + done, interp_order=interp_order)[0][0]
            res = self.lavd_update(tx, ty, c, timestep, done, acc, final=done + n == nsteps, radius=radius)
            acc = res["acc"]
            del tx, ty, c
        return {"lavd": res["lavd"], "rotation": res["rotation"], "length": res["length"], "x_dep": x, "y_dep": y}

    # ------------------------------------------------------------------ footprints: residence-time maps of trajectories
    FOOTPRINT_Q_MAX = 1 << 20       # a parcel's integer weight: 0 .. 2^20 (lc_footprint_update)
    FOOTPRINT_PLANES = ("hits", "mass", "csum", "chits")
    _FOOTPRINT_FORMS = {"auto": _capi.LC_FOOTPRINT_AUTO, "direct": _capi.LC_FOOTPRINT_DIRECT, "tiled": _capi.LC_FOOTPRINT_TILED,
                        "census": _capi.LC_FOOTPRINT_TILED_CENSUS}

    def last_footprint_kernel(self) -> str:
        """Name of the kernel the last :meth:`footprint_update` call launched (``lc_ctx_last_footprint_kernel``)."""
        return self.lib.lc_ctx_last_footprint_kernel(self.ctx).decode()

    def set_footprint_form(self, mode=-1):
        """Which kernel :meth:`footprint_update` launches (``lc_ctx_set_footprint_form``): ``-1`` / ``'auto'`` (the default: the
        library's rule), ``0`` / ``'direct'`` (one thread per parcel, global atomics), ``1`` / ``'tiled'`` (a workgroup sums its
        patch of seeds in an LDS window first), ``2`` / ``'census'`` (tiled; ``stats[2]`` also counts, in half-weights, the valid
        entries that left the window: a measuring aid).  Every form gives the same integers."""
        mode = self._FOOTPRINT_FORMS.get(mode, mode) if isinstance(mode, str) else mode
        if isinstance(mode, bool) or not isinstance(mode, (int, np.integer)) or int(mode) not in (-1, 0, 1, 2):
            raise ValueError(f"footprint form {mode!r}: -1 / 'auto', 0 / 'direct', 1 / 'tiled' or 2 / 'census'")
        _capi.check(self.lib.lc_ctx_set_footprint_form(self.ctx, int(mode)), self.lib)

    @classmethod
    def checked_footprint_grid(cls, lat, lon, cyclic=False):
        """``(ny_t, nx_t, lat0, lat1, lon0, lon1)`` of a footprint's target grid as :meth:`footprint_update` hands it to the
        library, or ``ValueError``: ``lat`` and ``lon`` are the cell centres in degrees, one-dimensional, at least two each,
        finite, strictly ascending and uniformly spaced, ``|lat| <= 90``; with ``cyclic`` the longitudes span 360 degrees minus
        one spacing, so that the cell after the last one is the first.  numpy on the host; no device is touched."""
        try:
            lat, lon = np.asarray(lat, dtype=np.float64), np.asarray(lon, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("footprint grid: lat and lon must be numbers") from None
        if lat.ndim != 1 or lon.ndim != 1 or lat.size < 2 or lon.size < 2:
            raise ValueError("footprint grid: lat and lon: one-dimensional, at least two values each")
        if not (np.isfinite(lat).all() and np.isfinite(lon).all()):
            raise ValueError("footprint grid: lat and lon: finite degrees")
        if np.abs(lat).max() > 90.0:
            raise ValueError(f"footprint grid: lat: within [-90, 90] degrees, got {lat.min()!r} .. {lat.max()!r}")
        for c, what in ((lat, "lat"), (lon, "lon")):
            d = np.diff(c)
            if not (d > 0).all():
                raise ValueError(f"footprint grid: {what}: strictly ascending (sort first)")
            if np.max(np.abs(d - d.mean())) > cls.GRID_UNIFORM_RTOL * d.mean():
                raise ValueError(f"footprint grid: {what}: uniformly spaced (regrid first)")
        if cyclic:
            step = (lon[-1] - lon[0]) / (lon.size - 1)
            gap = lon[0] + 360.0 - lon[-1]
            if abs(gap - step) > cls.GRID_UNIFORM_RTOL * step:
                raise ValueError(f"footprint grid: lon: with cyclic the axis must close after one more step: lon[0] + 360 - lon[-1] = "
                                 f"{gap!r} against a spacing of {step!r}")
        if lat.size * lon.size >= 1 << 31:
            raise ValueError(f"footprint grid: {lat.size} x {lon.size} cells (fewer than 2^31)")
        return int(lat.size), int(lon.size), float(lat[0]), float(lat[-1]), float(lon[0]), float(lon[-1])

    @staticmethod
    def seed_cell_areas(lat, lon, radius=6371000.0):
        """``R^2 cos(lat) dlat dlon`` of every cell of a uniform seed grid, ``(ny, nx)`` float64 in the square of ``radius``'s
        unit: the ``weights='area'`` of ``LCS.footprint``.  ``dlat`` and ``dlon`` are the mean spacings in radians (1 degree for
        an axis of one point); the cosine is clipped at 0."""
        lat, lon = np.asarray(lat, dtype=np.float64), np.asarray(lon, dtype=np.float64)
        k = np.pi / 180.0
        dlat = (lat[-1] - lat[0]) / (lat.size - 1) * k if lat.size > 1 else k
        dlon = (lon[-1] - lon[0]) / (lon.size - 1) * k if lon.size > 1 else k
        return np.repeat((float(radius) ** 2 * np.maximum(np.cos(lat * k), 0.0) * (dlat * dlon))[:, None], lon.size, axis=1)

    @classmethod
    def footprint_weights(cls, weights, shape):
        """``(q, wscale)``: parcel weights quantised once, on the host, for :meth:`footprint_update`.  ``weights``: non-negative
        numbers of the seed grid's ``shape``; NaN and 0 exclude the parcel; a negative or infinite weight is refused.  ``q =
        rint(w / max(w) 2^20)`` as int32 and ``wscale = max(w) / 2^20``, so that ``q wscale`` is the weight to within 2^-21 of the
        largest (a weight below that is 0: the parcel is left out).  None: ``(None, 1.0)``, every parcel counts once."""
        if weights is None:
            return None, 1.0
        try:
            w = np.array(weights, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("footprint: weights must be numbers") from None
        if w.shape != tuple(shape):
            raise ValueError(f"footprint: weights of shape {w.shape} for seeds of shape {tuple(shape)}")
        w[np.isnan(w)] = 0.0
        if np.isinf(w).any() or (w < 0).any():
            raise ValueError("footprint: weights must be finite and not negative (NaN and 0 exclude a parcel)")
        top = float(w.max()) if w.size else 0.0
        if top == 0.0:
            return np.zeros(w.shape, np.int32), 0.0
        return np.rint(w / top * cls.FOOTPRINT_Q_MAX).astype(np.int32), top / cls.FOOTPRINT_Q_MAX

    def footprint_update(self, traj_x, traj_y, grid_lat, grid_lon, level0, final, q=None, c=None, c_scale=None, acc=None, cyclic=False,
                         want=("hits", "mass")) -> dict:
        """One block of trajectory levels binned into the cells of a target grid (``lc_footprint_update``; the definition is in
        include/lcs_hip.h and restated in tests/footprint.py).  ``traj_x``, ``traj_y``: ``(n_levels, ...)`` positions in degrees
        after ``level0``, ``level0 + 1``, ... steps, ``n_levels >= 2``; entry 0 of a continued block (``level0 > 0``) is the last
        entry of the block before and is skipped; ``final`` marks the block that ends the record.  ``grid_lat``, ``grid_lon``:
        the centres of the target cells (:meth:`checked_footprint_grid`; ``cyclic``: the columns wrap).  ``q``: integer weights
        ``0 .. 2^20`` of the seeds' shape (:meth:`footprint_weights`), 0 leaving a parcel out altogether; None: all 1.  ``c``:
        values sampled at the same entries (:meth:`sample_tracer`), binned as ``rint(c c_scale)``.

        Returns the accumulators ``{'hits', 'mass', 'csum', 'chits', 'stats'}``: int64 device tensors ``(ny_t, nx_t)`` -- the
        half-weights, the half-weights times ``q``, times the scaled value, and the half-weights of the entries whose value
        counted -- those of ``want`` (and, with ``c``, both value planes), None for the rest; ``stats`` ``(4,)``: the half-weights
        of the entries outside the grid, of the values dropped (not finite, or beyond ``2^31 / c_scale``), 0, 0.  ``acc=None``
        creates and clears them (only with ``level0 == 0``); given the dict an earlier call returned, the block is added into
        it.  Every sum is an integer: any split into blocks, either kernel form and any run give the same bits."""
        ny_t, nx_t, lat0, lat1, lon0, lon1 = self.checked_footprint_grid(grid_lat, grid_lon, cyclic)
        level0 = int(level0)
        if level0 < 0:
            raise ValueError(f"footprint_update: level0 {level0}")
        shape = tuple(int(s) for s in np.shape(traj_x))
        if len(shape) < 2 or shape != tuple(int(s) for s in np.shape(traj_y)) or (c is not None and tuple(int(s) for s in np.shape(c)) != shape):
            raise ValueError("footprint_update: traj_x, traj_y and c must have one shape, (n_levels, ...)")
        n_levels, n = shape[0], int(np.prod(shape[1:]))
        if n_levels < 2 or n < 1 or n >= 1 << 31:
            raise ValueError(f"footprint_update: {n_levels} levels of {n} parcels (at least two levels and one parcel, fewer than 2^31)")
        if n * (level0 + n_levels) * (2 * self.FOOTPRINT_Q_MAX) >= 1 << 63:
            raise ValueError(f"footprint_update: {n} parcels over {level0 + n_levels} levels could overflow a 64-bit sum")
        if acc is None and level0 != 0:
            raise ValueError("footprint_update: a continued block (level0 > 0) needs the acc of the block before")
        want = (want,) if isinstance(want, str) else tuple(want)
        if any(k not in ("hits", "mass") for k in want):
            raise ValueError(f"footprint_update: want {want!r} (of 'hits' and 'mass'; csum and chits come with c)")
        planes = [k for k in ("hits", "mass") if k in want] + (["csum", "chits"] if c is not None else [])
        if not planes:
            raise ValueError("footprint_update: no output (want is empty and there is no c)")
        if c is not None:
            try:
                c_scale = float(c_scale)
            except (TypeError, ValueError):
                raise ValueError(f"footprint_update: c_scale {c_scale!r} (required with c: positive and finite)") from None
            if not np.isfinite(c_scale) or c_scale <= 0:
                raise ValueError(f"footprint_update: c_scale {c_scale} (positive and finite)")
        torch = self.torch
        if q is not None:
            if tuple(int(s) for s in np.shape(q)) != shape[1:]:
                raise ValueError(f"footprint_update: q of shape {tuple(np.shape(q))} for seeds of shape {shape[1:]}")
            if isinstance(q, torch.Tensor):
                if q.dtype.is_floating_point or q.dtype == torch.bool:
                    raise ValueError("footprint_update: q must be integers (Engine.footprint_weights quantises weights)")
                lo, hi = (int(q.min()), int(q.max()))
            else:
                q = np.asarray(q)
                if q.dtype.kind not in "iu":
                    raise ValueError("footprint_update: q must be integers (Engine.footprint_weights quantises weights)")
                lo, hi = int(q.min()), int(q.max())
            if lo < 0 or hi > self.FOOTPRINT_Q_MAX:
                raise ValueError(f"footprint_update: q {lo} .. {hi} (0 to 2^20)")
        on_dev = all(hasattr(a, "data_ptr") for a in (traj_x, traj_y) + (() if c is None else (c,)))
        dtype = np.dtype(str(traj_x.dtype).replace("torch.", "")) if on_dev else common_dtype(traj_x, traj_y, c)
        if dtype not in _NP2LC:
            raise ValueError(f"footprint_update: dtype {dtype} (float32 or float64)")
        tx, ty = self.to_device(traj_x, dtype), self.to_device(traj_y, dtype)
        cd = self.to_device(c, dtype) if c is not None else None
        qd = self.to_device(q, np.int32) if q is not None else None
        zero_first = acc is None
        if acc is None:
            acc = {k: (torch.empty((ny_t, nx_t), dtype=torch.int64, device=self.device) if k in planes else None) for k in self.FOOTPRINT_PLANES}
            acc["stats"] = torch.empty((4,), dtype=torch.int64, device=self.device)
        else:
            if not isinstance(acc, dict) or any(k not in acc for k in self.FOOTPRINT_PLANES + ("stats",)):
                raise ValueError("footprint_update: acc must be the dict an earlier call returned")
            for k, want_shape in [(k, (ny_t, nx_t)) for k in planes] + [("stats", (4,))]:
                t = acc[k]
                if not isinstance(t, torch.Tensor) or tuple(t.shape) != want_shape or t.dtype != torch.int64 or not t.is_contiguous() \
                        or t.device != self.device:
                    raise ValueError(f"footprint_update: acc[{k!r}] must be a contiguous {want_shape} int64 tensor on {self.device}")
        p = lambda t: t.data_ptr() if t is not None else None
        use = {k: (acc[k] if k in planes else None) for k in self.FOOTPRINT_PLANES}
        a = _capi.FootprintArgs(struct_size=C.sizeof(_capi.FootprintArgs), traj_x=tx.data_ptr(), traj_y=ty.data_ptr(), c=p(cd), q=p(qd),
                                dtype=_NP2LC[dtype], ny=n // shape[-1], nx=shape[-1], n=n, n_levels=n_levels, level0=level0,
                                final=int(bool(final)), ny_t=ny_t, nx_t=nx_t, lat0=lat0, lat1=lat1, lon0=lon0, lon1=lon1,
                                cyclic_x=int(bool(cyclic)), c_scale=c_scale if c is not None else 0.0, zero_first=int(zero_first),
                                hits=p(use["hits"]), mass=p(use["mass"]), csum=p(use["csum"]), chits=p(use["chits"]),
                                stats=acc["stats"].data_ptr())
        self._use_current_stream()
        _capi.check(self.lib.lc_footprint_update(self.ctx, C.byref(a)), self.lib)
        return acc

    def footprint(self, field: PackedField, seed_lat, seed_lon, timestep, grid_lat, grid_lon, weights=None, tracer=None, c_scale=None,
                  t0=0, nsteps=None, level_chunk=16, SETTLS_order=0, interp_order=1, cyclic_xboundary=True, noncyclic_clamp=None,
                  into=None) -> dict:
        """Where the parcels of the seed grid have been over ``nsteps`` steps from level ``t0`` of a packed field: the residence-
        time map of their trajectories on the target grid ``grid_lat`` x ``grid_lon`` (cell centres; the columns wrap when
        ``cyclic_xboundary`` and the longitudes close the circle).  ``weights``: ``(ny, nx)`` non-negative parcel weights, NaN
        and 0 leaving a parcel out (a receptor mask), quantised by :meth:`footprint_weights`; None: every parcel counts once.
        ``tracer``: a value on the wind's grid and levels (:meth:`prepare_tracer`), sampled along the trajectories as
        :meth:`lavd` samples and binned as ``rint(c c_scale)``; ``c_scale`` defaults to ``2^30 / max |tracer|``.

        Returns ``'acc'`` -- the integer planes and ``'stats'`` of :meth:`footprint_update`, device tensors -- and, as float64
        numpy arrays ``(ny_t, nx_t)`` formed on the host from those integers: ``'residence' = hits |timestep| / 2`` (seconds: the trapezoid rule in time), ``'mass' = mass wscale
        |timestep| / 2`` (weight x seconds), ``'mean_value' = csum / chits / c_scale`` (NaN where ``chits == 0``; None without a
        tracer); the departure points ``'x_dep'``, ``'y_dep'`` of :meth:`advect`; ``'wscale'``, ``'c_scale'``, ``'half_step'``.
        ``into``: an earlier result whose integers this window (or receptor set) is added into, for climatologies: the same grid,
        ``|timestep|``, ``wscale`` and ``c_scale`` (the earlier ``c_scale`` is the default then).

        The record is streamed as :meth:`lavd` streams it, ``level_chunk`` steps at a time; the result does not depend on
        ``level_chunk``.  ``cyclic_xboundary=False`` with the default ``reference_outer`` clamp takes one block over all levels;
        ``noncyclic_clamp='pointwise'`` streams."""
        try:
            timestep = float(timestep)
        except (TypeError, ValueError):
            raise ValueError(f"footprint: timestep {timestep!r}") from None
        if not np.isfinite(timestep) or timestep == 0:
            raise ValueError(f"footprint: timestep {timestep} (non-zero and finite)")
        _check_order(field, interp_order)
        if tracer is not None:
            if tracer.dtype != field.dtype:
                raise ValueError(f"footprint: tracer dtype {tracer.dtype} differs from the field's compute dtype {field.dtype}")
            if (tracer.nt, tracer.ny_f, tracer.nx_f) != (field.nt, field.ny_f, field.nx_f) or \
                    (tracer.lat_min, tracer.lat_max, tracer.lon_min, tracer.lon_max) != (field.lat_min, field.lat_max, field.lon_min, field.lon_max):
                raise ValueError("footprint: the tracer must lie on the wind's grid and time levels")
            _check_order(tracer, interp_order)
        t0 = int(t0)
        nsteps = field.nt - 1 - t0 if nsteps is None else int(nsteps)
        level_chunk = int(level_chunk)
        if t0 < 0 or nsteps < 1 or t0 + nsteps > field.nt - 1:
            raise ValueError(f"footprint: t0 {t0}, nsteps {nsteps} on a record of {field.nt} levels (at least one step, inside the record)")
        if level_chunk < 1:
            raise ValueError(f"footprint: level_chunk {level_chunk} (at least 1)")
        count = lambda a: int(a.numel()) if hasattr(a, "numel") else int(np.size(a))
        if np.ndim(seed_lat) != 1 or np.ndim(seed_lon) != 1 or count(seed_lat) * count(seed_lon) < 1:
            raise ValueError("footprint: seed_lat and seed_lon must be 1-D and hold at least one seed each")
        glat, glon = np.asarray(grid_lat, dtype=np.float64), np.asarray(grid_lon, dtype=np.float64)
        cyclic = False
        if cyclic_xboundary and glon.ndim == 1 and glon.size >= 2:
            step = (glon[-1] - glon[0]) / (glon.size - 1)
            cyclic = bool(abs((glon[0] + 360.0 - glon[-1]) - step) <= self.GRID_UNIFORM_RTOL * abs(step))
        grid = self.checked_footprint_grid(glat, glon, cyclic)
        q, wscale = self.footprint_weights(weights, (count(seed_lat), count(seed_lon)))
        xmode = x_boundary_mode(cyclic_xboundary, noncyclic_clamp, True)
        half = abs(timestep) / 2
        acc = None
        if into is not None:
            if not isinstance(into, dict) or "acc" not in into or into.get("grid") != grid + (cyclic,):
                raise ValueError("footprint: into must be an earlier result on the same target grid")
            if into["half_step"] != half or into["wscale"] != wscale:
                raise ValueError(f"footprint: into was built with |timestep| / 2 = {into['half_step']} and wscale {into['wscale']}, this call "
                                 f"has {half} and {wscale} (normalise the weights to one largest value)")
            if (tracer is None) != (into["c_scale"] is None):
                raise ValueError("footprint: into and this call must both have a tracer, or neither")
            if c_scale is None:
                c_scale = into["c_scale"]
            elif float(c_scale) != into["c_scale"]:
                raise ValueError(f"footprint: c_scale {c_scale} differs from into's {into['c_scale']}")
            acc = into["acc"]
        if tracer is not None:
            if c_scale is None:
                top = self.torch.nan_to_num(tracer.c1.abs(), nan=0.0, posinf=0.0, neginf=0.0).max().item()
                c_scale = float(1 << 30) / top if top > 0 else 1.0
            c_scale = float(c_scale)
            if not np.isfinite(c_scale) or c_scale <= 0:
                raise ValueError(f"footprint: c_scale {c_scale} (positive and finite)")
        else:
            c_scale = None
        kw = dict(SETTLS_order=SETTLS_order, interp_order=interp_order, cyclic_xboundary=cyclic_xboundary, noncyclic_clamp=noncyclic_clamp)
        if xmode == _capi.LC_X_CLAMP_REFERENCE_OUTER:
            level_chunk = nsteps               # one block: the clamp is decided over the whole grid, level by level, inside one call
        qd = self.to_device(q, np.int32) if q is not None else None
        x = y = None
        for done in range(0, nsteps, level_chunk):
            n = min(level_chunk, nsteps - done)
            x, y, tx, ty = self.advect(field, seed_lat, seed_lon, timestep, t0=t0 + done, nsteps=n, return_traj=True,
                                       start=None if done == 0 else (x, y), out=None if done == 0 else (x, y), **kw)
            c = None if tracer is None else self.sample_tracer(tracer, tx, ty, level0=t0 + done, interp_order=interp_order)[0][0]
            acc = self.footprint_update(tx, ty, glat, glon, done, done + n == nsteps, qd, c, c_scale, acc, cyclic)
            del tx, ty, c
        return self._footprint_result(acc, grid + (cyclic,), half, wscale, c_scale, x, y)

    def _footprint_result(self, acc, grid, half, wscale, c_scale, x=None, y=None) -> dict:
        """The float64 maps of :meth:`footprint` from the integers, formed with numpy on the host -- one rounding per operation,
        in the order written, IEEE division: the same bits wherever it runs (a device division need not round correctly)."""
        host = lambda k: self.to_host(acc[k]).astype(np.float64)
        res = {"acc": acc, "grid": grid, "half_step": half, "wscale": wscale, "c_scale": c_scale, "x_dep": x, "y_dep": y}
        res["residence"] = host("hits") * half if acc["hits"] is not None else None
        res["mass"] = (host("mass") * wscale) * half if acc["mass"] is not None else None
        res["mean_value"] = None
        if acc["csum"] is not None:
            with np.errstate(invalid="ignore", divide="ignore"):
                res["mean_value"] = (host("csum") / host("chits")) / c_scale
        return res

    def synchronize(self):
        self.torch.cuda.synchronize(self.device)


# ---------------------------------------------------------------------------
# torch-free route: host arrays through lc_lcs_host
# ---------------------------------------------------------------------------
def lcs_host(u, v, lat_f, lon_f, timestep, SETTLS_order=0, interp_order=3, cyclic_xboundary=False,
             seed_lat=None, seed_lon=None, t0=0, nsteps=None, gauss_sigma=None, fd_fp32_cast=True,
             tensor_layout="reference", return_traj=False, want_sigma=True, device=0, noncyclic_clamp=None,
             float64_fidelity=None, pipeline=None):
    """numpy in, numpy out, via the one-call C entry point.  Returns a dict.
    ``float64_fidelity``: ``'auto'`` (default) / ``'exact'`` / ``'fast'``, see :meth:`Engine.set_f64_fidelity`.
    ``pipeline`` (default on): the staged, level-chunk pipelined transfers of ``lc_ctx_set_host_pipeline``; ``False`` = the
    serial form (plain copies of the whole series, then the kernels).  Results are bit-identical."""
    lib = _capi.load()
    dtype = common_dtype(u, v, lat_f, lon_f, seed_lat, seed_lon)
    u = np.ascontiguousarray(u, dtype=dtype)
    v = np.ascontiguousarray(v, dtype=dtype)
    if u.shape != v.shape or u.ndim != 3:
        raise ValueError("u and v must both be (time, latitude, longitude)")
    lat_f = np.ascontiguousarray(lat_f, dtype=dtype)
    lon_f = np.ascontiguousarray(lon_f, dtype=dtype)
    seed_lat = lat_f if seed_lat is None else np.ascontiguousarray(seed_lat, dtype=dtype)
    seed_lon = lon_f if seed_lon is None else np.ascontiguousarray(seed_lon, dtype=dtype)
    nt, ny_f, nx_f = u.shape
    ny, nx = seed_lat.size, seed_lon.size
    nsteps = nt - 1 - t0 if nsteps is None else int(nsteps)
    out = {"x_dep": np.empty((ny, nx), dtype), "y_dep": np.empty((ny, nx), dtype)}
    if want_sigma:
        out["sigma"] = np.empty((ny, nx), dtype)
    if return_traj:
        out["traj_x"] = np.empty((nsteps + 1, ny, nx), dtype)
        out["traj_y"] = np.empty((nsteps + 1, ny, nx), dtype)

    def p(a):
        return a.ctypes.data_as(C.c_void_p) if a is not None else C.c_void_p(0)

    ctx = _host_ctx(lib, device)
    with _HOST_LOCK:
        _capi.check(lib.lc_ctx_set_f64_fidelity(ctx, Engine._FIDELITY[float64_fidelity or "auto"]), lib)
        on = (os.environ.get("LCS_HOST_PIPELINE", "1")[:1] != "0") if pipeline is None else bool(pipeline)
        _capi.check(lib.lc_ctx_set_host_pipeline(ctx, int(on)), lib)
        gs = _smoothing_width(gauss_sigma)
        _capi.check(lib.lc_lcs_host(
            ctx, p(u), p(v), _NP2LC[dtype], nt, ny_f, nx_f, p(lat_f), p(lon_f), p(seed_lat), ny, p(seed_lon), nx,
            float(timestep), int(SETTLS_order), int(interp_order), x_boundary_mode(cyclic_xboundary, noncyclic_clamp),
            int(t0), nsteps, gs,
            int(bool(fd_fp32_cast)), _LAYOUTS[tensor_layout], p(out.get("sigma")), p(out["x_dep"]), p(out["y_dep"]),
            p(out.get("traj_x")), p(out.get("traj_y"))), lib)
        marks = (C.c_double * 4)()
        lib.lc_ctx_last_host_marks(ctx, marks)
    out["host_marks_ms"] = {"buffers_allocated": marks[0], "uploads_and_launches_issued": marks[1], "kernels_done": marks[2],
                            "results_down": marks[3]}
    return out


# The one-call routes' context per device, created on first use and kept for the life of the process: it owns the pinned
# staging ring and the copy threads of lc_lcs_host (lc_ctx_set_host_pipeline), which cost far more to set up than a call
# takes.  Calls through it are serialised (a context is not re-entrant).
_HOST_CTX = {}
_HOST_LOCK = __import__("threading").Lock()


def _host_ctx(lib, device):
    with _HOST_LOCK:
        ctx = _HOST_CTX.get(int(device))
        if ctx is None:
            ctx = C.c_void_p()
            _capi.check(lib.lc_ctx_create(int(device), C.byref(ctx)), lib)
            _HOST_CTX[int(device)] = ctx
            import atexit
            atexit.register(lambda c=ctx: lib.lc_ctx_destroy(c))
        return ctx


def lcs_global_host(u, v, lat_f, lon_f, timestep, SETTLS_order=0, interp_order=3, interp_to_common_grid=True,
                    truncation=20, gauss_sigma=None, fd_fp32_cast=True, tensor_layout="reference", device=0,
                    float64_fidelity=None):
    """The reference's default global call form ``LCS(...)(ds, isglobal=True)`` (LCS/LCS.py:105-157) on numpy
    arrays, torch-free, through ``lc_lcs_global_host``: regrid to the common 0.5 degree grid, T-truncation,
    cyclic advection from the grid nodes, sigma.  Returns a dict with ``sigma, x_dep, y_dep, latitude, longitude``."""
    lib = _capi.load()
    dtype = common_dtype(u, v)
    u = np.ascontiguousarray(u, dtype=dtype)
    v = np.ascontiguousarray(v, dtype=dtype)
    if u.shape != v.shape or u.ndim != 3:
        raise ValueError("u and v must both be (time, latitude, longitude)")
    lat_f = np.ascontiguousarray(lat_f, dtype=np.float64)
    lon_f = np.ascontiguousarray(lon_f, dtype=np.float64)
    nt, ny_f, nx_f = u.shape
    if interp_to_common_grid:
        ny, nx = C.c_int(), C.c_int()
        lib.lc_common_grid(C.byref(ny), C.byref(nx), None, None)
        lat, lon = np.empty(ny.value), np.empty(nx.value)
        lib.lc_common_grid(None, None, lat.ctypes.data_as(C.c_void_p), lon.ctypes.data_as(C.c_void_p))
        odt = np.dtype(np.float64)
    else:
        lat, lon, odt = lat_f, lon_f, dtype
    out = {k: np.empty((lat.size, lon.size), odt) for k in ("sigma", "x_dep", "y_dep")}
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    gs = _smoothing_width(gauss_sigma)
    ctx = C.c_void_p()
    _capi.check(lib.lc_ctx_create(int(device), C.byref(ctx)), lib)
    try:
        if float64_fidelity is not None:
            _capi.check(lib.lc_ctx_set_f64_fidelity(ctx, Engine._FIDELITY[float64_fidelity]), lib)
        _capi.check(lib.lc_lcs_global_host(
            ctx, p(u), p(v), _NP2LC[dtype], nt, ny_f, nx_f, p(lat_f), p(lon_f), int(bool(interp_to_common_grid)),
            -1 if truncation is None else int(truncation), float(timestep), int(SETTLS_order), int(interp_order), gs,
            int(bool(fd_fp32_cast)), _LAYOUTS[tensor_layout], p(out["sigma"]), p(out["x_dep"]), p(out["y_dep"])), lib)
    finally:
        lib.lc_ctx_destroy(ctx)
    out["latitude"], out["longitude"] = lat, lon
    return out
