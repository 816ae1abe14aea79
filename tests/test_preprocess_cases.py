"""The pre-processing case table (tests/preprocess_cases.py) against csrc/preprocess.hip's own text, against its own promises,
and the float64 oracle against the 30-digit operators of tests/golden/trunc_operators_mp.npz.  No GPU, no build.

The oracle (oracle/preprocess_oracle.py) is the same algorithm as the C++ operator builder in the same precision; the fixture
is the published statement evaluated in 40 digits by other means (tests/golden/make_trunc_operators_mp.py), so an error the two
share shows here.  The deviations this module measures are the float64 rounding level at each case's conditioning; the GPU
module builds its bounds from them (``oracle_deviation``)."""
import os
import re

import numpy as np
import pytest

from oracle import preprocess_oracle as PO
from tests import preprocess_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "lagrangiancoherence_amd", "csrc", "preprocess.hip")
GOLDEN = os.path.join(ROOT, "tests", "golden", "trunc_operators_mp.npz")


def strip_comments(text):
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", code)


@pytest.fixture(scope="module")
def code():
    with open(SOURCE) as fh:
        return strip_comments(fh.read())


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def oracle_operators(gridtype, nlat, T):
    return np.array(PO.truncation_operators_gaussian(nlat, T) if gridtype == "gaussian" else PO.truncation_operators(nlat, T))


def oracle_deviation(golden, gridtype, nlat, T):
    """max |oracle - 30-digit operator| over every entry of every m."""
    return float(np.abs(oracle_operators(gridtype, nlat, T) - golden[PC.golden_key(gridtype, nlat, T)]).max())


# ------------------------------------------------------------------ the table against the source text
def test_the_restated_launch_arithmetic_is_the_sources(code):
    consts = dict(re.findall(r"constexpr int (DFT_ROWS|PT)\s*=\s*(\d+)", code))
    assert int(consts["DFT_ROWS"]) == PC.DFT_ROWS and int(consts["PT"]) == PC.PT
    # forward DFT: rows per block from 64 KB of doubles, capped; the grid and the dynamic LDS from it; one wave per staged row
    assert "int rpb = (int)((size_t)64 * 1024 / ((size_t)nlon * sizeof(double)));" in code and PC.LDS_FORWARD == 64 * 1024
    assert "rpb = rpb > DFT_ROWS ? DFT_ROWS : rpb;" in code
    assert "dim3((rows + rpb - 1) / rpb), dim3(256)" in code and "(size_t)rpb * nlon * sizeof(double)" in code
    assert "const int r = threadIdx.x / 64;" in code and "c < C; c += 64" in code and PC.WAVE * PC.DFT_ROWS == PC.BLOCK
    # projection: column tiles x row tiles x (T + 1)
    assert "dim3((2 * nb + PT - 1) / PT, (nlat + PT - 1) / PT, T1), dim3(256)" in code
    # inverse DFT: one block per row, C doubles of LDS, loaded 256 at a time
    assert "dim3(rows), dim3(256), (size_t)C * sizeof(double)" in code and "c < C; c += blockDim.x" in code
    # regrid: 256 threads, at most 16384 blocks, grid stride
    assert "(n + 255) / 256 < 16384 ? (n + 255) / 256 : 16384" in code and PC.REGRID_MAX_BLOCKS == 16384
    assert "o += (size_t)gridDim.x * blockDim.x" in code
    # the two LDS refusals and the size conditions
    assert "(size_t)2 * (truncation + 1) * sizeof(double) > 48 * 1024" in code and PC.LDS_INVERSE == 48 * 1024
    assert "(size_t)nlon * sizeof(double) > 64 * 1024" in code
    req = re.findall(r"LC_REQUIRE\(([^;]*)\);", code)
    assert any(r.startswith("nbatch >= 1 && nlat >= 3 && nlon >= 4,") for r in req) and (PC.MIN_NLAT, PC.MIN_NLON) == (3, 4)
    assert any(r.startswith("truncation >= 0,") for r in req)
    assert any(r.startswith("truncation <= nlat - 1 && truncation <= (nlon - 1) / 2,") for r in req)
    assert any(r.startswith("nt >= 1 && ny_s >= 2 && nx_s >= 2 && ny_d >= 1 && nx_d >= 1,") for r in req)
    assert sum("must ascend" in r for r in req) == 2
    # every message piece the refusal cases expect is in the source
    with open(SOURCE) as fh:
        text = fh.read()
    for piece in {r[3] for r in PC.TRUNC_REFUSALS} | {"exceeds this build's limit"}:
        assert piece in text, piece


def test_the_arithmetic_at_the_values_the_issue_states():
    assert [PC.rows_per_block(n) for n in (4, 2048, 2049, 2184, 2185, 2730, 2731, 4096, 4097, 8192)] == [4, 4, 3, 3, 3, 3, 2, 2, 1, 1]
    assert PC.rows_per_block(8193) == 0 and PC.truncate_refusal(1, 3, 8193, 1) == "longitudes exceed"
    assert PC.truncate_refusal(1, 3, 8192, 1) is None and 8 * 8192 == PC.LDS_FORWARD
    assert PC.truncate_refusal(1, 4000, 8000, 3071) is None and PC.truncate_refusal(1, 4000, 8000, 3072) == "exceeds this build's limit"
    assert PC.column_tiles(97 * 4) == 25 and PC.column_tiles(16) == 1 and PC.column_tiles(17) == 2 and PC.row_tiles(360) == 12
    assert PC.regrid_passes(4_194_304) == 1 and PC.regrid_passes(4_194_305) == 2 and PC.regrid_blocks(257) == 2
    assert PC.forward_blocks(1, 5, 2200) == 2 and PC.forward_blocks(17, 3, 24) == 13


def test_every_truncation_case_is_legal_and_reaches_its_branch():
    reached = set()
    for name, c in PC.TRUNC.items():
        assert PC.truncate_refusal(c["nb"], c["nlat"], c["nlon"], c["T"]) is None, name
        assert c["gridtype"] in ("regular", "gaussian") and c["dtype"] == "float64" and c["check"] == "oracle", name
        got = PC.reaches(c)
        assert c["branch"] in got, (name, c["branch"], sorted(got))
        reached |= got
        assert c["nb"] * c["nlat"] * c["nlon"] <= 600_000, name          # seconds, not minutes
    want = {"column_tile_past_first", "ragged_column_tile", "one_full_column_tile", "second_column_tile_of_two",
            "row_tile_past_first", "row_tile_ragged", "row_tile_full", "second_row_tile_of_one", "three_row_tiles",
            "rows_per_block_4", "rows_per_block_3", "rows_per_block_2", "rows_per_block_1", "rows_per_block_1_64k",
            "forward_tail_block", "forward_second_trip", "inverse_second_coefficient",
            "smallest_nlat", "smallest_nlon", "odd_nlon", "zonal_mean_only", "full_latitude_band",
            "highest_wavenumber_odd", "highest_wavenumber_even"}
    assert want <= reached, sorted(want - reached)
    T = PC.TRUNC
    # the shapes the issue names
    assert [T[k]["nb"] for k in ("nb16", "nb17", "nb33", "nb50")] == [16, 17, 33, 50]
    assert [T[f"nlat{n}"]["nlat"] for n in (3, 5, 31, 32, 33, 65)] == [3, 5, 31, 32, 33, 65]
    assert all(T[f"nlat{n}"]["nb"] == 17 for n in (3, 5, 31, 32, 33, 65))
    assert (T["C258"]["nb"], T["C258"]["nlat"], T["C258"]["nlon"], T["C258"]["T"]) == (1, 130, 258, 128)
    assert (T["rpb3"]["nb"], T["rpb3"]["nlat"], T["rpb3"]["nlon"], T["rpb3"]["T"]) == (1, 5, 2200, 2)
    assert T["rpb1"]["nlon"] == 4100 and T["rpb1_all_lds"]["nlon"] == 8192
    # rpb 3 on 5 rows: two blocks, one empty slot in the second; a tail block exists for every rows-per-block value above 1
    assert PC.forward_blocks(1, 5, 2200) * 3 - 5 == 1
    for rpb in (2, 3, 4):
        assert any(PC.rows_per_block(c["nlon"]) == rpb and "forward_tail_block" in PC.reaches(c) for c in T.values()), rpb
    assert set(PC.TRUNC_F32) <= set(T) and len(PC.TRUNC_F32) == 4
    for nlat, nlon, Tr, piece in PC.TRUNC_REFUSALS:
        assert PC.truncate_refusal(1, nlat, nlon, Tr) == piece, (nlat, nlon, Tr)
    # the operator read-back drives many column tiles, ragged ones among them
    sizes = [(Tr + 1) * nlat for (_, nlat, Tr) in PC.GOLDEN]
    assert min(sizes) == 25 and max(sizes) == 561
    assert any(PC.column_tiles(n) > 30 for n in sizes) and any((2 * n) % PC.PT for n in sizes)
    c = PC.NONFINITE
    assert c["nb"] == 20 and c["nan_member"] == 7 and c["inf_member"] == 18 and PC.column_tiles(c["nb"]) == 2
    assert PC.CACHE_SEQUENCE[0] == PC.CACHE_SEQUENCE[3] and len({s[3] for s in PC.CACHE_SEQUENCE}) == 2


def test_every_regrid_case_reaches_its_branch():
    common = PO.COMMON_LATS.size * PO.COMMON_LONS.size
    for name, c in PC.REGRID.items():
        u, lat, lon, lats, lons = PC.regrid_input(name)
        assert u.dtype == np.dtype(c["dtype"]) and u.shape == (c["nt"], lat.size, lon.size), name
        assert np.all(np.diff(lat) > 0) and np.all(np.diff(lon) > 0), name
        n = u.shape[0] * (common if lats is None else lats.size * lons.size)
        assert (PC.regrid_passes(n) >= 2) == (c["branch"] == "grid_stride"), name
        u2 = PC.regrid_input(name)[0]
        assert np.array_equal(u, u2, equal_nan=True) and u2 is not u, name                  # seeded, fresh
    assert 17 * common == 4_412_520
    inp = PC.regrid_input
    lat = inp("gaussian_source")[1]
    assert np.ptp(np.diff(lat)) > 0.01 and inp("gaussian_source")[3][0] < lat[0]
    _, lat, lon, lats, lons = inp("targets_on_nodes")
    assert np.array_equal(lat, lats) and np.array_equal(lon, lons)
    _, lat, lon, lats, lons = inp("unsorted_repeated_targets")
    for a in (lats, lons):
        assert np.any(np.diff(a) < 0) and np.unique(a).size < a.size
    assert inp("source_2x2")[0].shape[1:] == (2, 2)
    assert inp("one_node_targets")[3].size == 1 and inp("one_node_targets")[4].size == 1
    _, lat, lon, lats, lons = inp("outside_all_sides")
    assert lats.min() < lat[0] and lats.max() > lat[-1] and lons.min() < lon[0] and lons.max() > lon[-1]
    u = inp("nonfinite_source")[0]
    assert np.isposinf(u).any() and np.isneginf(u).any() and np.isnan(u).any()
    u = inp("f32_overflow")[0]
    with np.errstate(over="ignore"):
        assert np.isinf(u[0, 2, 2] - u[0, 1, 2]) and np.isinf(u[0, 1, 3] - u[0, 1, 2]) and np.isfinite(u).all()
    for lat, lon in PC.REGRID_REFUSALS:
        assert not (np.all(np.diff(lat) > 0) and np.all(np.diff(lon) > 0))


# ------------------------------------------------------------------ the oracle against the 30-digit operators
def test_the_fixture_holds_every_case_and_projectors(golden):
    assert set(golden) == {PC.golden_key(*k) for k in PC.GOLDEN}
    for (gridtype, nlat, T) in PC.GOLDEN:
        P = golden[PC.golden_key(gridtype, nlat, T)]
        assert P.shape == (T + 1, nlat, nlat) and P.dtype == np.float64 and np.abs(P).max() <= 1.0
        # synthesis . analysis of an orthonormal family: idempotent -- while the interpolant can represent the family.  On the
        # regular grid at T = nlat - 1 and odd m it cannot: Pbar^m_N is a sine polynomial of degree N, sin(N theta) vanishes on
        # every row, the sine series stops at N - 1.  There the statement is no projector (P[3] of (5, 4): |P.P - P| = 0.094).
        for m in range(T + 1):
            if gridtype == "regular" and T == nlat - 1 and m % 2:
                continue
            assert np.abs(P[m] @ P[m] - P[m]).max() < 1e-13, (gridtype, nlat, T, m)
    assert os.path.getsize(GOLDEN) < 512 * 1024


def test_the_oracle_agrees_with_the_30_digit_operators(golden):
    """Measured here (max over all entries; entries have magnitude <= 1): regular (5, 4) 1.8e-15, (9, 8) 3.7e-15,
    (17, 7) 4.5e-14, (33, 16) 2.1e-13; Gaussian (8, 7) 4.1e-15, (16, 5) 1.2e-15, (32, 16) 7.5e-14."""
    for (gridtype, nlat, T), recorded in PC.GOLDEN.items():
        dev = oracle_deviation(golden, gridtype, nlat, T)
        print(f"oracle - 30-digit operator, {gridtype} ({nlat}, {T}): {dev:.2e}" + (f"  (recorded {recorded:.1e})" if recorded else ""))
        if recorded is not None:
            assert dev <= 4 * recorded, (gridtype, nlat, T, dev)
        assert dev < 1e-12, (gridtype, nlat, T, dev)


def _regular_operators_f64(nlat, T, halve_last_cosine=True, parity_matched=True):
    """The statement once more in plain float64 with the two defining choices as switches: the halving of the k = N term of the
    cosine interpolant, and the sine series for odd m.  The integrals by a 400-node Gauss-Legendre rule (the cosine series
    against an odd-m Pbar is no polynomial in x; 400 nodes leave about 1e-6 there, far below what the switch changes)."""
    N = nlat - 1
    i = np.arange(nlat)
    xq, wq = np.polynomial.legendre.leggauss(400)
    tq = np.arccos(xq)
    ops = []
    for m in range(T + 1):
        cosine = m % 2 == 0 or not parity_matched
        k = np.arange(0, N + 1) if cosine else np.arange(1, N)
        trig = np.cos if cosine else np.sin
        B = (2.0 / N) * trig(np.outer(k, i) * np.pi / N)
        if cosine:
            B[:, [0, -1]] *= 0.5
            B[0] *= 0.5
            if halve_last_cosine:
                B[-1] *= 0.5
        integ = (PO.legendre_normalized(m, T, xq) * wq) @ trig(np.outer(k, tq)).T
        ops.append(PO.legendre_normalized(m, T, np.cos(i * np.pi / N)).T @ integ @ B)
    return np.array(ops)


def test_a_wrong_operator_is_caught(golden):
    regular = [(nlat, T) for (g, nlat, T) in PC.GOLDEN if g == "regular"]
    dev = lambda **kw: max(np.abs(_regular_operators_f64(nlat, T, **kw) - golden[PC.golden_key("regular", nlat, T)]).max()
                           for nlat, T in regular)
    assert dev() < 1e-11                                           # the switches on: the fixture's operator
    no_halving, cosine_for_odd = dev(halve_last_cosine=False), dev(parity_matched=False)
    print(f"k = N term not halved: {no_halving:.2e}; cosine series for odd m: {cosine_for_odd:.2e}")
    assert no_halving > 1e-6 and cosine_for_odd > 1e-6


def test_the_gaussian_fixture_sees_its_weights_and_row_order(golden):
    for (g, nlat, T) in PC.GOLDEN:
        if g != "gaussian":
            continue
        P = golden[PC.golden_key(g, nlat, T)]
        ops = oracle_operators(g, nlat, T)
        assert np.abs(ops[:, ::-1, ::-1] - P).max() < 1e-12        # symmetric nodes: flipping both axes is the same grid
        assert np.abs(np.swapaxes(ops, 1, 2) - P).max() > 1e-6     # the weights sit on the columns


# ------------------------------------------------------------------ the read-back batch of the GPU module, on the CPU
def test_the_readback_batch_truncated_by_the_oracle_is_the_operators_columns(golden):
    for (g, nlat, T) in (("regular", 5, 4), ("gaussian", 8, 7), ("regular", 9, 8)):
        P = golden[PC.golden_key(g, nlat, T)]
        f = PC.readback_batch(nlat, T)
        assert f.shape == ((T + 1) * nlat, nlat, 2 * T + 2)
        want = PC.readback_expected(P)
        got = PO.spectral_truncate(f, T, g)
        assert np.abs(got - want).max() < 1e-13, (g, nlat, T)
        # an entry of the operator wrong by 1e-9 shows in that member alone
        Q = P.copy()
        Q[T // 2, 1, 2] += 1e-9
        d = np.abs(PC.readback_expected(Q) - want).reshape(T + 1, nlat, -1).max(axis=2)
        assert d[T // 2, 2] > 5e-10 and np.count_nonzero(d) == 1


# ------------------------------------------------------------------ regrid: the tie inside the source range
def test_the_oracle_fills_an_in_range_tie_from_the_right_hand_node():
    """A NaN source node makes the interpolation NaN at the midpoints beside it; those are filled from reindex(method='nearest'),
    where a midpoint is a tie: pandas takes the larger index of an increasing index."""
    u, lat, lon, lats, lons = PC.regrid_input("nan_beside_midpoint")
    r, c = PC.TIE_NAN_NODE
    assert np.isnan(u[0, r, c]) and np.isnan(u).sum() == 1
    out = PO.regrid_common_grid(u, lat, lon, lats, lons)[0][0]
    at = lambda la, lo: out[int(round(la * 2)), int(round(lo * 2))]
    assert at(r, c + 0.5) == u[0, r, c + 1] and at(r + 0.5, c) == u[0, r + 1, c] and at(r + 0.5, c + 0.5) == u[0, r + 1, c + 1]
    # the midpoints on the other side tie too, and their right-hand node is the NaN itself
    assert np.isnan(at(r, c - 0.5)) and np.isnan(at(r - 0.5, c)) and np.isnan(at(r, c))
    assert at(r - 0.5, c + 0.5) == u[0, r, c + 1] and at(r + 0.5, c - 0.5) == u[0, r + 1, c]
    assert np.isnan(out).sum() == 4                                # the node, two midpoints, and (r - 0.5, c - 0.5): all -> the node
    assert not np.isnan(at(r + 1, c)) and not np.isnan(at(r, c + 1))
