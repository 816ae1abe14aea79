"""Thinning and dilation without a GPU: the two shipped tables by rule, what the numpy restatement of tests/skeleton.py does on
planes whose answer is known, the properties every named plane has on that restatement alone (the skeleton is a subset of its
input, thinning it again changes nothing, and under 'guohall' it has the input's number of 8-connected components, the seam
included) -- which the GPU test then inherits by equality -- and the entry point in the header, the bindings and the library
with every refusal made before the device is touched."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from lagrangiancoherence_amd import _capi, build
from tests import skeleton as SK
from tests.labelled import DataArray

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMED = [(n, False) for n in {**SK.CASES, **SK.LARGE}] + [(n, True) for n in SK.CYCLIC_CASES]
NAMED_IDS = [f"{n}{'-cyclic' if c else ''}" for n, c in NAMED]


@functools.lru_cache(maxsize=None)
def _thinned(name, method, cyclic=False):
    plane, loops = SK.thin(SK.mask_of(name), SK.table(method), cyclic)
    plane.setflags(write=False)
    return plane, loops


# ------------------------------------------------------------------ the tables
@pytest.mark.parametrize("method", SK.METHODS)
def test_the_table_has_the_histogram_of_its_rule(method):
    t = SK.table(method)
    assert t.dtype == np.uint8 and t.shape == (256,)
    assert tuple(np.bincount(t, minlength=4)) == SK.HISTOGRAMS[method]
    assert t[0] == 0 and t[255] == 0                      # an isolated pixel and an interior pixel stay


@pytest.mark.parametrize("method", SK.METHODS)
def test_the_engines_table_is_the_support_modules(method):
    from lagrangiancoherence_amd.engine import Engine
    t = Engine.thinning_table(method)
    assert isinstance(t, np.ndarray) and t.dtype == np.uint8 and np.array_equal(t, SK.table(method))


def test_the_engine_knows_no_other_method():
    from lagrangiancoherence_amd.engine import Engine
    with pytest.raises(ValueError, match="method"):
        Engine.thinning_table("lee")


# ------------------------------------------------------------------ known answers of the restatement
def test_a_block_of_four_vanishes_under_zhang_and_leaves_a_pixel_under_guohall():
    assert _thinned("block-6x6", "zhang")[0].sum() == 0
    assert _thinned("block-6x6", "guohall")[0].sum() == 1


@pytest.mark.parametrize("method, pixels", [("zhang", 63), ("guohall", 64)])
def test_the_full_plane_takes_34_loops_and_stays_one_piece(method, pixels):
    plane, loops = _thinned("full-67x130", method)
    assert loops == 34 and plane.sum() == pixels and SK.components(plane) == 1
    before = SK.thin(SK.mask_of("full-67x130"), SK.table(method), max_iterations=32)[0]
    assert before.sum() > pixels                           # the 33rd still deletes, the 34th nothing
    assert np.array_equal(SK.thin(SK.mask_of("full-67x130"), SK.table(method), max_iterations=33)[0], plane)


def test_the_bar_under_zhang():
    plane, loops = _thinned("bar-40x150", "zhang")
    assert loops == 12 and plane.sum() == 117


def test_the_neighbourhood_index_and_the_seam():
    m = np.zeros((3, 4), dtype=bool)
    m[0, 1] = m[1, 3] = True
    assert SK.index(m)[1, 2] == 1 + 8 and SK.index(m)[1, 0] == 4 and SK.index(m)[0, 2] == 128 + 16
    assert SK.index(m, cyclic=True)[1, 0] == 4 + 128 and SK.index(m, cyclic=True)[0, 0] == 8 + 64
    assert SK.index(m)[0, 0] == 8                          # without the seam: only the eastern neighbour


def test_the_cyclic_dilation_reference_crosses_the_seam():
    m = np.zeros((3, 6))
    m[1, 0] = 1
    assert SK.dilate(m, 1, 1, cyclic=True)[1].tolist() == [1, 1, 0, 0, 0, 1] and SK.dilate(m, 1, 1)[1].tolist() == [1, 1, 0, 0, 0, 0]
    assert SK.dilate(m, 2, 2, cyclic=True).sum() == 15 and SK.dilate(m, 1, 1, cyclic=True).sum() == 5


# ------------------------------------------------------------------ every named plane, on the restatement alone
@pytest.mark.parametrize("method", SK.METHODS)
@pytest.mark.parametrize("name, cyclic", NAMED, ids=NAMED_IDS)
def test_the_skeleton_is_an_idempotent_subset_with_the_inputs_components(name, cyclic, method):
    mask = SK.mask_of(name)
    plane, _ = _thinned(name, method, cyclic)
    fg = SK.foreground(mask)
    assert not (plane.astype(bool) & ~fg).any()
    again, loops = SK.thin(plane, SK.table(method), cyclic)
    assert loops == 1 and np.array_equal(again, plane)
    if method == "guohall":
        assert SK.components(plane, cyclic) == SK.components(mask, cyclic)


def test_the_named_planes_are_what_their_tests_need():
    m = SK.mask_of("nan-negative")
    assert np.isnan(m).any() and (m < 0).any() and (m > 0).any()
    assert SK.mask_of("smooth-49x113").shape == (49, 113)                        # one more than a tile, both ways
    blob = SK.mask_of("blob-on-column-0")
    assert blob[:, 0].any() and blob[:, -1].any() and not blob[:, 20:30].any()
    for name in ("smooth-67x130", "smooth-130x67", "smooth-150x200", "smooth-515x513"):
        assert _thinned(name, "guohall")[1] > 5, name                            # thicker than one launch (4 iterations) finishes
    assert 3 not in SK.custom_table() and (SK.custom_table() != SK.table("zhang")).sum() == 28


# ------------------------------------------------------------------ header, bindings, library
@pytest.fixture(scope="module")
def lib():
    build.build_library(verbose=False)
    return _capi.load()


def test_the_entry_points_are_declared_prototyped_and_exported(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lcs_hip.h")).read(), flags=re.S)
    for name in ("lc_mask_morphology", "lc_morph_work_elems"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _capi.PROTOTYPES and hasattr(lib, name), name
    assert "morphology.hip" in build.SOURCES
    assert lib.lc_version() == 104 == _capi.LC_VERSION


def test_the_header_states_the_contract():
    text = " ".join(open(os.path.join(ROOT, "include", "lcs_hip.h")).read().split())
    section = text[text.index("thinning and dilating a ridge mask"):text.index("int lc_mask_morphology(")]
    for phrase in ("LCS/area_of_influence.py:207", "without a bump", "!= 0 and not NaN", "NW + 2 N + 4 NE + 8 E + 16 SE + 32 S + 64 SW + 128 W",
                   "one stream synchronisation per launch", "before any HIP call", "No kernel of this call waits for another workgroup"):
        assert phrase in section, phrase


def test_work_elems_is_pure_arithmetic(lib):
    # four words in front, a flag per tile of 48 x 112 pixels, and a byte per pixel
    assert lib.lc_morph_work_elems(1, 1, 1) == 4 + 1 + 1 and lib.lc_morph_work_elems(48, 112, 1) == 4 + 1 + 48 * 28
    assert lib.lc_morph_work_elems(49, 113, 3) == 4 + 3 * 4 + (3 * 49 * 113 + 3) // 4
    assert lib.lc_morph_work_elems(0, 5, 1) == 0 and lib.lc_morph_work_elems(5, -1, 1) == 0 and lib.lc_morph_work_elems(5, 5, 0) == 0


# A context nobody dereferences and pointers nobody follows: every call below is refused by its argument checks.
_BLOCK = C.create_string_buffer(4096)
CTX = PTR = C.cast(_BLOCK, C.c_void_p)
_TABLE = SK.table("guohall")
_BAD_TABLE = _TABLE.copy()
_BAD_TABLE[17] = 4
GOOD = dict(ctx=CTX, dtype=_capi.LC_F64, ny=4, nx=6, n_members=2, op=_capi.LC_MORPH_THIN, table=_TABLE.ctypes.data, structure=0,
            max_iterations=0, iterations_per_launch=0, mask=PTR, out=PTR, work_dev=PTR)
DILATE = dict(op=_capi.LC_MORPH_DILATE, table=None, structure=170, max_iterations=1)
EINVAL = _capi.LC_EINVAL
REFUSALS = [
    (dict(ctx=None), b"null context"),
    (dict(op=2), b"bad op"),
    (dict(op=-1), b"bad op"),
    (dict(dtype=2), b"bad dtype"),
    (dict(ny=0), b"bad size"),
    (dict(nx=-3), b"bad size"),
    (dict(n_members=0), b"bad size"),
    (dict(ny=1 << 17, nx=1 << 14), b"plane too large"),
    (dict(ny=46341, nx=46341), b"plane too large"),
    (dict(ny=1 << 15, nx=1 << 15, n_members=1 << 12), b"too many planes"),
    (dict(iterations_per_launch=-1), b"bad iterations_per_launch"),
    (dict(iterations_per_launch=5), b"bad iterations_per_launch"),
    (dict(table=None), b"null thinning table"),
    (dict(table=_BAD_TABLE.ctypes.data), b"code 4 at index 17"),
    ({**DILATE, "structure": 0}, b"bad structure"),
    ({**DILATE, "structure": 256}, b"bad structure"),
    ({**DILATE, "max_iterations": 0}, b"bad iterations"),
    ({**DILATE, "iterations_per_launch": 9}, b"bad iterations_per_launch"),
    (dict(mask=None), b"null pointer"),
    (dict(out=None), b"null pointer"),
    ({**DILATE, "work_dev": None}, b"null pointer"),
]


def _call(g):
    a = _capi.MorphArgs(struct_size=C.sizeof(_capi.MorphArgs))
    for k, v in g.items():
        if k != "ctx":
            setattr(a, k, v)
    return _capi.load().lc_mask_morphology(g["ctx"], C.byref(a))


def test_the_structure_matches_the_library(lib):
    a = _capi.MorphArgs(struct_size=C.sizeof(_capi.MorphArgs) - 8)
    assert lib.lc_mask_morphology(CTX, C.byref(a)) == EINVAL and b"struct_size" in lib.lc_last_error()
    assert lib.lc_mask_morphology(CTX, None) == EINVAL and b"null argument structure" in lib.lc_last_error()
    assert lib.lc_mask_morphology(None, None) == EINVAL and b"null context" in lib.lc_last_error()


@pytest.mark.parametrize("change, message", REFUSALS, ids=[m.decode().replace(" ", "-") + f"-{i}" for i, (_, m) in enumerate(REFUSALS)])
def test_the_call_refuses_before_it_touches_a_device(lib, change, message):
    assert _call({**GOOD, **change}) == EINVAL
    err = lib.lc_last_error()
    assert message in err and b"lc_mask_morphology" in err


def test_the_kernels_never_wait_for_another_workgroup():
    """The house rule of components.hip and distance.hip: no atomic, no cooperative launch, no grid synchronisation, no loop
    without a counted end -- and no inline assembly."""
    src = build._strip_comments(open(os.path.join(build.CSRC, "morphology.hip")).read())
    for word in ("cooperative", "grid_group", "this_grid", "hipLaunchCooperativeKernel", "__threadfence", "atomic", "while (", "for (;;)", "asm"):
        assert word not in src, word


# ------------------------------------------------------------------ the Python surfaces refuse before any device work
def test_the_engine_refuses_bad_arguments_without_a_device():
    from lagrangiancoherence_amd.engine import Engine
    eng = Engine.__new__(Engine)             # no device: the checks come before anything is touched
    plane, good = np.ones((2, 2)), SK.table("zhang")
    for bad in (good[:255], good.astype(np.float64), np.full(256, 4, np.uint8), -good.astype(np.int8)):
        with pytest.raises(ValueError, match="table"):
            eng.thin(plane, bad)
    with pytest.raises(ValueError, match="max_iterations"):
        eng.thin(plane, good, max_iterations=0)
    with pytest.raises(ValueError, match="iterations_per_launch"):
        eng.thin(plane, good, iterations_per_launch=0)
    with pytest.raises(ValueError, match="connectivity"):
        eng.dilate(plane, connectivity=3)
    with pytest.raises(ValueError, match="iterations"):
        eng.dilate(plane, iterations=0)


def _ridges():
    return DataArray(np.ones((3, 4)), ("latitude", "longitude"), {"latitude": np.arange(3.0), "longitude": np.arange(4.0)})


@pytest.mark.parametrize("kwargs, match", [
    (dict(method="lee"), "method"), (dict(max_iterations=0), "max_iterations"), (dict(max_iterations=-2), "max_iterations"),
    (dict(table=np.zeros(255, np.uint8)), "table"), (dict(table=np.full(256, 4)), "table"), (dict(table=np.zeros(256)), "table"),
], ids=["method", "max_iterations-0", "max_iterations-negative", "table-255", "table-code-4", "table-float"])
def test_skeletonize_ridges_refuses_before_it_asks_for_an_engine(monkeypatch, kwargs, match):
    from lagrangiancoherence_amd import tools
    monkeypatch.setattr(tools, "get_engine", lambda *a, **k: pytest.fail("an engine was asked for"))
    with pytest.raises(ValueError, match=match):
        tools.skeletonize_ridges(_ridges(), **kwargs)


@pytest.mark.parametrize("kwargs, match", [(dict(connectivity=3), "connectivity"), (dict(connectivity=0), "connectivity"),
                                           (dict(iterations=0), "iterations"), (dict(iterations=-1), "iterations")],
                         ids=["connectivity-3", "connectivity-0", "iterations-0", "iterations-negative"])
def test_dilate_ridges_refuses_before_it_asks_for_an_engine(monkeypatch, kwargs, match):
    from lagrangiancoherence_amd import tools
    monkeypatch.setattr(tools, "get_engine", lambda *a, **k: pytest.fail("an engine was asked for"))
    with pytest.raises(ValueError, match=match):
        tools.dilate_ridges(_ridges(), **kwargs)


def test_the_shim_exports_both_functions():
    from LagrangianCoherence.LCS import tools as shim
    from lagrangiancoherence_amd import tools
    assert shim.skeletonize_ridges is tools.skeletonize_ridges and shim.dilate_ridges is tools.dilate_ridges
    assert {"skeletonize_ridges", "dilate_ridges"} <= set(tools.__all__)
    doc = " ".join(tools.skeletonize_ridges.__doc__.split())
    assert "scikit-image's own table is NOT reproduced" in doc and "Guo & Hall" in doc and "Zhang & Suen" in doc
