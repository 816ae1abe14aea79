"""Every case of tests/preprocess_cases.py on the GPU: the kernels of csrc/preprocess.hip at their edges.

The truncation is checked twice.  Against the 30-digit operators of tests/golden/trunc_operators_mp.npz: a batch of unit rows
times one zonal wave reads every entry of every operator the C++ builder made back through the three kernels; the bound per
case is 16 x the float64 oracle's own deviation from the same operators (computed here, on the CPU), at least 1e-14.  And
against ``PO.spectral_truncate`` on standard-normal data at the shapes where the launch arithmetic changes, within the bound
tests/test_preprocess_gpu.py states for the same size class.  ``pytest -s`` prints every measured figure.

NOT YET RUN ON AN MI355X: no GPU slot could be had while this module was written, so no measured maxima stand here.  What is
known from the CPU: the C++ builder's operators (the host code of preprocess.hip compiled into a stand-alone program) deviate
from the 30-digit ones by
  regular (5, 4) 6.7e-16, (9, 8) 2.7e-15, (17, 7) 2.6e-15, (33, 16) 1.9e-14; Gaussian (8, 7) 8.9e-16, (16, 5) 6.7e-16, (32, 16) 6.4e-15
against read-back bounds of 2.8e-14, 5.9e-14, 7.2e-13, 3.4e-12; 6.6e-14, 2.0e-14, 1.2e-12; and a numpy restatement of the three
kernels with those operators is within 1.1e-13 of the oracle on every 5e-13 case, 1.3e-12 on C258 (bound 2e-12), 3e-16 on the
wide rows (bound 5e-12).  The first GPU run's figures (``pytest -s``) belong here in their place.
"""
import os
import re

import numpy as np
import pytest
import torch

from lagrangiancoherence_amd import preprocess as PP
from oracle import preprocess_oracle as PO
from tests import preprocess_cases as PC

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trunc_operators_mp.npz")


@pytest.fixture(scope="module")
def eng():
    from lagrangiancoherence_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _truncate(eng, f, T, gridtype="regular"):
    return PP.spectral_truncate(eng, f, T, gridtype).cpu().numpy()


# ------------------------------------------------------------------ the operators, read back through the kernels
@pytest.mark.parametrize("gridtype,nlat,T", list(PC.GOLDEN), ids=[PC.golden_key(*k) for k in PC.GOLDEN])
def test_every_operator_entry_read_through_the_kernels_is_the_30_digit_one(eng, golden, gridtype, nlat, T):
    P = golden[PC.golden_key(gridtype, nlat, T)]
    ops = PO.truncation_operators_gaussian(nlat, T) if gridtype == "gaussian" else PO.truncation_operators(nlat, T)
    oracle_dev = float(np.abs(np.array(ops) - P).max())
    bound = max(PC.READBACK_MARGIN * oracle_dev, PC.READBACK_FLOOR)
    f = PC.readback_batch(nlat, T)
    got = _truncate(eng, f, T, gridtype)
    err = np.abs(got - PC.readback_expected(P)).reshape(T + 1, nlat, -1).max(axis=2)       # (m, column j)
    worst = np.unravel_index(err.argmax(), err.shape)
    print(f"\nread-back {gridtype} ({nlat}, {T}): {f.shape[0]} members, {PC.column_tiles(f.shape[0])} column tiles; oracle deviation "
          f"{oracle_dev:.2e}, bound {bound:.2e}, measured {err.max():.2e} at (m, column) = {tuple(int(w) for w in worst)}")
    assert err.max() <= bound


# ------------------------------------------------------------------ the kernels' edges against the oracle
@pytest.mark.parametrize("name", list(PC.TRUNC))
def test_truncation_edges_match_the_oracle(eng, name):
    c = PC.TRUNC[name]
    f = PC.trunc_input(c["nb"], c["nlat"], c["nlon"])
    ref = PO.spectral_truncate(f, c["T"], c["gridtype"])
    tol = PC.trunc_tol(c["nlat"], c["nlon"], c["T"])
    got = _truncate(eng, f, c["T"], c["gridtype"])
    assert got.shape == f.shape and got.dtype == np.float64
    err = float(np.abs(got - ref).max())
    print(f"\n{name} ({c['branch']}): nb {c['nb']}, {c['nlat']} x {c['nlon']}, T {c['T']}, {c['gridtype']}: {err:.2e} (bound {tol:.0e})")
    assert err <= tol
    if name in PC.TRUNC_F32:
        f32 = f.astype(np.float32)
        ref32 = PO.spectral_truncate(f32.astype(np.float64), c["T"], c["gridtype"])
        out = PP.spectral_truncate(eng, f32, c["T"], c["gridtype"])
        assert out.dtype == torch.float32
        over = np.abs(out.cpu().numpy().astype(np.float64) - ref32) - (2.0 ** -24 * np.abs(ref32) + tol)
        print(f"{name} float32: max |error| {np.abs(out.cpu().numpy() - ref32).max():.2e}, max over its bound {over.max():.2e} (must be <= 0)")
        assert over.max() <= 0.0


def test_truncation_refusals(eng):
    f = PC.trunc_input(2, 9, 16)
    before = _truncate(eng, f, 3)
    for nlat, nlon, T, piece in PC.TRUNC_REFUSALS:
        with pytest.raises(ValueError, match=re.escape(piece)):              # _capi.check: LC_EINVAL and LC_EUNSUPPORTED -> ValueError
            eng.spectral_truncate(np.zeros((nlat, nlon)), T)
    assert np.array_equal(_truncate(eng, f, 3), before)             # the context and its operators are as they were


def test_a_nonfinite_member_leaves_the_others_untouched(eng):
    c = PC.NONFINITE
    clean, dirty = PC.nonfinite_input()
    with np.errstate(all="ignore"):
        ref = PO.spectral_truncate(dirty, c["T"])
    base, got = _truncate(eng, clean, c["T"]), _truncate(eng, dirty, c["T"])
    bad = (c["nan_member"], c["inf_member"])
    for b in range(c["nb"]):
        if b in bad:
            assert (~np.isfinite(ref[b])).any() and not np.isfinite(got[b][~np.isfinite(ref[b])]).any(), b
        else:
            assert np.isfinite(ref[b]).all() and np.array_equal(got[b], base[b]), b


def test_the_operator_cache_is_keyed_by_every_argument(eng):
    from lagrangiancoherence_amd.engine import Engine
    nlat, nlon = PC.CACHE_SEQUENCE[0][:2]
    f = PC.trunc_input(3, nlat, nlon)
    for nlat, nlon, T, gridtype in PC.CACHE_SEQUENCE:
        got = _truncate(eng, f, T, gridtype)
        fresh = Engine(0)
        try:
            want = _truncate(fresh, f, T, gridtype)
        finally:
            fresh.close()
        assert np.array_equal(got, want), (T, gridtype)
    seen = [_truncate(eng, f, T, g) for _, _, T, g in PC.CACHE_SEQUENCE[:3]]
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[0], seen[2])


# ------------------------------------------------------------------ regrid
@pytest.mark.parametrize("name", list(PC.REGRID))
def test_regrid_cases_match_scipy_and_pandas(eng, name):
    u, lat, lon, lats, lons = PC.regrid_input(name)
    kw = {} if lats is None else dict(lats=lats, lons=lons)
    with np.errstate(all="ignore"):
        ref = PO.regrid_common_grid(u, lat, lon, **kw)[0]
    got, glats, glons = PP.regrid_common_grid(eng, u, lat, lon, **kw)
    assert got.dtype == torch.float64 and tuple(got.shape) == ref.shape
    got = got.cpu().numpy()
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan)
    scale = float(np.abs(u[np.isfinite(u)]).max())
    inf = np.isinf(ref)
    assert np.array_equal(got[inf], ref[inf])
    fin = ~nan & ~inf
    err = float(np.abs(got[fin] - ref[fin]).max()) if fin.any() else 0.0
    same = np.array_equal(got, ref, equal_nan=True)
    print(f"\nregrid {name}: {ref.size} outputs, {int(nan.sum())} NaN, {int(inf.sum())} inf, max |error| {err:.2e} "
          f"(bound {PC.REGRID_ATOL * scale:.2e}), bit-identical: {same}")
    assert err <= PC.REGRID_ATOL * scale
    if name == "nonfinite_source":
        assert nan.any() and inf.any()
    if name == "f32_overflow":
        assert inf.any() and np.isfinite(u).all()
    if PC.REGRID[name]["check"] == "oracle+right_hand_node":
        r, c = PC.TIE_NAN_NODE
        at = lambda la, lo: got[0, int(round(la * 2)), int(round(lo * 2))]
        assert at(r, c + 0.5) == u[0, r, c + 1] and at(r + 0.5, c) == u[0, r + 1, c] and at(r + 0.5, c + 0.5) == u[0, r + 1, c + 1]
        assert np.isnan(at(r, c - 0.5)) and np.isnan(at(r - 0.5, c)) and int(nan.sum()) == 4


def test_regrid_refuses_axes_that_do_not_ascend(eng):
    u = np.zeros((1, 4, 4))
    dst = np.array([0.5, 1.5])
    for lat, lon in PC.REGRID_REFUSALS:
        with pytest.raises(ValueError, match="must ascend"):
            eng.regrid(u, lat, lon, dst, dst)
