"""What ``Engine.prepare_field`` and ``Engine._advect_args`` DECIDE, recorded on the CPU: an engine made without a context,
a stand-in library that answers ``lc_packed_elems`` and records every ``lc_field_pack``, torch CPU tensors as the device.
``record(call_args)`` drives every case and returns the tables of ``tests/golden/engine_field_plan.json``
(``tests/golden/make_engine_field_plan.py`` wrote them at the parent of the engine's field plan; ``tests/test_engine_field_plan.py``
replays them against the engine as checked out).  Each table is stored as its distinct outcomes plus one index per case."""
import ctypes as C
import itertools
import json

import numpy as np
import torch

from lagrangiancoherence_amd import _capi
from lagrangiancoherence_amd.engine import Engine

NY_F, NX_F = 6, 8
KINDS = {"float32": (np.float32, np.float32), "float64": (np.float64, np.float64), "wind_f32": (np.float32, np.float64)}
ORDERS, NTS, TRI = (1, 2, 3, 4, 5), (1, 2, 3), (None, True, False)
FIELD_ATTRS = ("lin", "cub", "ext", "u", "v", "lin32", "u32", "v32", "planes_version", "planes32_version")
BUFFERS = ("lin", "lin32", "cub", "ext", "u", "v", "u32", "v32")
POINTERS = [n for n, t in _capi.AdvectArgs._fields_ if t is C.c_void_p]
SCALARS = [n for n, t in _capi.AdvectArgs._fields_ if t is not C.c_void_p]
XMODES = {"cyclic": _capi.LC_X_CYCLIC, "clamp_point": _capi.LC_X_CLAMP_POINT, "clamp_reference_outer": _capi.LC_X_CLAMP_REFERENCE_OUTER}
PREPARE_OPTIONS = {"default": {}, "fuse_levels=False": {"fuse_levels": False}, "ext_image=False": {"ext_image": False}}
SEEDS = (4, 5)
# the call geometries of the _advect_args cases: everything at its default, and everything set
GEOMETRIES = ("plain", "full")
STALE_FIELDS = (("float32", 3), ("float64", 1), ("float64", 3), ("wind_f32", 1), ("wind_f32", 3))   # fields that borrow planes


def _present(p):
    return bool(getattr(p, "value", p))


class StubLib:
    """``lc_packed_elems`` answers a size, ``lc_field_pack`` records (dtype code, nt, order, image present, ext present)."""

    def __init__(self):
        self.packs = []

    def lc_packed_elems(self, nt, ny_f, nx_f):
        return max(int(nt), 0) * (ny_f + 2) * (nx_f + 2) * 2

    def lc_field_pack(self, ctx, u, v, dtype, nt, ny_f, nx_f, order, image, ext):
        assert _present(u) and _present(v) and (ny_f, nx_f) == (NY_F, NX_F)
        self.packs.append([int(dtype), int(nt), int(order), _present(image), _present(ext)])
        return _capi.LC_OK

    def lc_sample_raw(self, *args):
        return _capi.LC_OK


def stub_engine():
    eng = object.__new__(Engine)
    eng.torch, eng.device, eng._poison, eng.ctx, eng.lib = torch, torch.device("cpu"), False, None, StubLib()
    eng._use_current_stream = lambda: None
    return eng


def wind(kind, nt):
    """``u, v`` as torch CPU tensors (so the field borrows them where the dtype already fits) and the coordinates."""
    wdt, cdt = KINDS[kind]
    t = torch.arange(nt * NY_F * NX_F, dtype=torch.float64).reshape(nt, NY_F, NX_F)
    tdt = getattr(torch, np.dtype(wdt).name)
    return (0.25 * t).to(tdt), (3.0 - 0.5 * t).to(tdt), np.linspace(-10, 10, NY_F).astype(cdt), np.linspace(0, 70, NX_F).astype(cdt)


def field_outcome(eng, kind, order, nt, fuse_levels, lin_image, ext_image):
    u, v, lat, lon = wind(kind, nt)
    del eng.lib.packs[:]
    try:
        f = eng.prepare_field(u, v, lat, lon, order, fuse_levels=fuse_levels, lin_image=lin_image, ext_image=ext_image)
    except ValueError as e:
        return {"error": str(e)}
    return {"packs": list(eng.lib.packs), "present": [a for a in FIELD_ATTRS if getattr(f, a) is not None],
            "wind_f32": f.wind_f32, "order": f.order, "fuse_raw": f.fuse_raw, "dtype": f.dtype.name}


def field_cases():
    return list(itertools.product(KINDS, ORDERS, NTS, TRI, TRI, TRI))


def args_cases():
    out = []
    for kind, order, opts in itertools.product(KINDS, (1, 3, 5), PREPARE_OPTIONS):
        for call_order in sorted({1, order}):
            out += [(kind, order, opts, call_order, x, g) for x in XMODES for g in GEOMETRIES]
    return out


def call_buffers(kind, geometry):
    """The tensors of one ``_advect_args`` call, by the name the outcome gives their pointers, and its scalar geometry."""
    dt = torch.float32 if kind == "float32" else torch.float64
    ny, nx = SEEDS
    names = ["seed_lat", "seed_lon", "out_x", "out_y"] + (["start_x", "start_y", "traj_x", "traj_y"] if geometry == "full" else [])
    bufs = {n: torch.zeros(ny if n == "seed_lat" else nx if n == "seed_lon" else 3 * ny * nx, dtype=dt) for n in names}
    scal = dict(timestep=-900.0, K=2, nsteps=2)
    if geometry == "full":
        scal.update(row0=1, ny_global=ny + 5, t0=1, nsteps=1, n_members=2, t0_stride=1)
    return bufs, scal


def args_outcome(eng, call_args, kind, order, opts, call_order, xmode, geometry):
    u, v, lat, lon = wind(kind, 3)
    f = eng.prepare_field(u, v, lat, lon, order, **PREPARE_OPTIONS[opts])
    bufs, scal = call_buffers(kind, geometry)
    before = {a: getattr(f, a) is None for a in ("u", "lin")}
    del eng.lib.packs[:]
    a = call_args(eng, f, call_order, XMODES[xmode], bufs, scal)
    names = {t.data_ptr(): n for n, t in bufs.items()}
    names.update({getattr(f, n).data_ptr(): n for n in BUFFERS if getattr(f, n) is not None})
    assert len(names) == len(bufs) + sum(getattr(f, n) is not None for n in BUFFERS)
    return {"scalars": {n: getattr(a, n) for n in SCALARS},
            "pointers": {n: names[getattr(a, n)] if getattr(a, n) else None for n in POINTERS},
            "made": [n for n, was_none in before.items() if was_none and getattr(f, n) is not None],
            "packs": list(eng.lib.packs)}


def stale_cases():
    out = []
    for kind, order in STALE_FIELDS:
        out += [(kind, order, "args", o, x) for o in sorted({1, order}) for x in XMODES]
        out += [(kind, order, "sample", o, None) for o in sorted({1, order})] + [(kind, order, "ensure_lin", 1, None)]
    return out


def stale_outcome(eng, call_args, kind, order, path, call_order, xmode):
    """A borrowed plane written in place after ``prepare_field``: the RuntimeError's text, or None if the path let it through."""
    u, v, lat, lon = wind(kind, 3)
    f = eng.prepare_field(u, v, lat, lon, order)
    assert (f.u if f.u is not None else f.u32) is u, "the field must borrow the planes for this case to mean anything"
    u.fill_(1.0)
    try:
        if path == "args":
            bufs, scal = call_buffers(kind, "plain")
            call_args(eng, f, call_order, XMODES[xmode], bufs, scal)
        elif path == "sample":
            eng.sample(f, np.full(SEEDS, 30.0), np.full(SEEDS, 1.0), interp_order=call_order)
        else:
            eng._ensure_lin(f, call_order)
    except RuntimeError as e:
        return str(e)
    return None


def _table(cases, outcome):
    distinct, index = [], []
    for c in cases:
        o = outcome(*c)
        if o not in distinct:
            distinct.append(o)
        index.append(distinct.index(o))
    return {"outcomes": distinct, "cases": index}


def record(call_args):
    """``call_args(eng, field, interp_order, xmode, bufs, scal)`` -> the filled ``AdvectArgs`` (the one thing whose spelling
    differs between the engine as recorded and the engine as replayed)."""
    eng = stub_engine()
    return {"prepare_field": _table(field_cases(), lambda *c: field_outcome(eng, *c)),
            "advect_args": _table(args_cases(), lambda *c: args_outcome(eng, call_args, *c)),
            "stale_wind": _table(stale_cases(), lambda *c: stale_outcome(eng, call_args, *c))}


def dumps(doc):
    """One outcome per line: small, and a change shows as the lines it touches."""
    lines = []
    for key, val in doc.items():
        if isinstance(val, dict):
            rows = ",\n".join("   " + json.dumps(o, separators=(",", ":")) for o in val["outcomes"])
            lines.append(f' {json.dumps(key)}: {{"outcomes": [\n{rows}],\n  "cases": {json.dumps(val["cases"], separators=(",", ":"))}}}')
        else:
            lines.append(f" {json.dumps(key)}: {json.dumps(val)}")
    return "{\n" + ",\n".join(lines) + "\n}\n"
