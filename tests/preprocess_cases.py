"""Case tables of the global pre-processing kernels (``csrc/preprocess.hip``): ``regrid_kernel<T>`` behind
``lc_regrid_common_grid`` and ``dft_forward_kernel<T>`` -> ``project_kernel`` -> ``dft_inverse_kernel<T>`` behind
``lc_spectral_truncate``, with the operators the host code builds for them (``build_projectors``, ``build_projectors_gaussian``).

Plain data and numpy input builders, imported by ``test_preprocess_cases.py`` (the table against the source text and against its
own promises, the oracle against the 30-digit operators; no GPU) and ``test_preprocess_cases_gpu.py`` (every case on the GPU).
No torch, no engine.

- the launch arithmetic of the two entry points, restated: ``rows_per_block``, ``forward_blocks``, ``column_tiles``,
  ``row_tiles``, ``regrid_blocks``, ``regrid_passes``, ``truncate_refusal``;
- ``GOLDEN``: the (gridtype, nlat, T) of ``tests/golden/trunc_operators_mp.npz`` (generator beside it), and for the regular ones
  the deviation of the float64 oracle from them as first measured;
- ``TRUNC``: name -> one truncation case: ``branch`` (what it is there to reach, a key of ``reaches``), ``nb, nlat, nlon, T``,
  ``gridtype``, ``dtype`` and ``check`` (``oracle``: against ``PO.spectral_truncate`` within ``trunc_tol``);
- ``TRUNC_F32``: the cases that also run with float32 in and out; ``TRUNC_REFUSALS``; ``NONFINITE``; ``CACHE_SEQUENCE``;
- ``REGRID``: name -> one regrid case (``branch``, ``dtype``, the source's ``nt, ny, nx``, ``check``); ``regrid_input`` builds its
  arrays; ``REGRID_REFUSALS``.

Every builder is seeded and returns fresh arrays; the references are computed by the tests, once per case.
"""
import numpy as np

# ------------------------------------------------------------------ the launch arithmetic, restated
DFT_ROWS = 4                     # field rows a forward-DFT block stages at most
PT = 32                          # project_kernel's tile edge: rows of P[m], and columns (batch member, re | im)
BLOCK = 256
WAVE = 64                        # the forward DFT walks the C spectral columns 64 at a time, one wave per staged row
LDS_FORWARD = 64 * 1024          # dynamic LDS of dft_forward_kernel: rows_per_block rows of nlon doubles
LDS_INVERSE = 48 * 1024          # dynamic LDS of dft_inverse_kernel: the C = 2 (T + 1) coefficients of one row
REGRID_MAX_BLOCKS = 16384
MIN_NLAT, MIN_NLON = 3, 4


def rows_per_block(nlon):
    return min(DFT_ROWS, LDS_FORWARD // (8 * nlon))


def forward_blocks(nb, nlat, nlon):
    return -(-nb * nlat // rows_per_block(nlon))


def column_tiles(nb):
    return -(-2 * nb // PT)


def row_tiles(nlat):
    return -(-nlat // PT)


def coefficients(T):
    return 2 * (T + 1)


def regrid_blocks(n):
    return min(-(-n // BLOCK), REGRID_MAX_BLOCKS)


def regrid_passes(n):
    """Elements the busiest thread of the grid-stride loop writes."""
    return -(-n // (regrid_blocks(n) * BLOCK))


def truncate_refusal(nb, nlat, nlon, T):
    """None, or a piece of the message lc_spectral_truncate refuses these sizes with (its checks, in its order)."""
    if nb < 1 or nlat < MIN_NLAT or nlon < MIN_NLON:
        return "bad sizes"
    if T < 0:
        return "truncation must be >= 0"
    if T > nlat - 1 or T > (nlon - 1) // 2:
        return "too high"
    if 8 * coefficients(T) > LDS_INVERSE:
        return "exceeds this build's limit"
    if 8 * nlon > LDS_FORWARD:
        return "longitudes exceed"
    return None


# ------------------------------------------------------------------ the 30-digit operators
# (gridtype, nlat, T) -> max |oracle - golden| over all entries (all of magnitude <= 1) as measured when the fixture was made,
# None where the issue recorded none (the Gaussian grid: the CPU test prints them).  The CPU test holds the oracle to 4 x this.
GOLDEN = {
    ("regular", 5, 4): 1.8e-15,
    ("regular", 9, 8): 3.7e-15,
    ("regular", 17, 7): 4.5e-14,
    ("regular", 33, 16): 2.1e-13,
    ("gaussian", 8, 7): None,
    ("gaussian", 16, 5): None,
    ("gaussian", 32, 16): None,
}
READBACK_MARGIN, READBACK_FLOOR = 16.0, 1e-14     # the GPU bound: 16 x the oracle's deviation on that case, at least 1e-14
READBACK_PHASE = 0.3


def golden_key(gridtype, nlat, T):
    return f"{gridtype}_{nlat}_{T}"


def readback_batch(nlat, T):
    """f[m * nlat + j] = e_j(lat) x cos(m lon + 0.3), j counted from the north, latitude stored ascending; nlon = 2 T + 2.
    Truncated, member (m, j) is column j of P[m] times the same cosine: every entry of every operator, read through the kernels."""
    nlon = 2 * T + 2
    lam = 2 * np.pi * np.arange(nlon) / nlon
    f = np.zeros((T + 1, nlat, nlat, nlon))
    for m in range(T + 1):
        f[m, np.arange(nlat), nlat - 1 - np.arange(nlat)] = np.cos(m * lam + READBACK_PHASE)
    return f.reshape((T + 1) * nlat, nlat, nlon)


def readback_expected(P):
    """The same batch truncated by the operators ``P`` ((T + 1, nlat, nlat), row 0 north)."""
    T1, nlat, _ = P.shape
    nlon = 2 * T1
    lam = 2 * np.pi * np.arange(nlon) / nlon
    wave = np.cos(np.arange(T1)[:, None] * lam + READBACK_PHASE)                     # (m, l)
    out = np.einsum("mij,ml->mjil", P, wave)[:, :, ::-1, :]                          # (m, j, latitude ascending, l)
    return np.ascontiguousarray(out).reshape(T1 * nlat, nlat, nlon)


# ------------------------------------------------------------------ truncation edges against the oracle
def trunc_tol(nlat, nlon, T):
    """The bounds tests/test_preprocess_gpu.py already states against the same oracle on standard-normal data, by size class:
    5e-13 (360 x 721 T20, 91 x 180 T12), 2e-12 past T = 31 (96 x 192 T42 and T63, the Gaussian 64 x 128),
    5e-12 past 2048 longitudes (33 x 2880)."""
    return 5e-12 if nlon > 2048 else 2e-12 if T > 31 else 5e-13


TRUNC = {}


def _t(name, branch, nb, nlat, nlon, T, gridtype="regular"):
    assert name not in TRUNC, name
    TRUNC[name] = dict(branch=branch, nb=nb, nlat=nlat, nlon=nlon, T=T, gridtype=gridtype, dtype="float64", check="oracle")


# project_kernel's column tiles: 2 nb columns in tiles of 32
_t("nb16", "one_full_column_tile", 16, 9, 20, 5)
_t("nb17", "second_column_tile_of_two", 17, 9, 20, 5)
_t("nb33", "ragged_column_tile", 33, 9, 20, 5)
_t("nb50", "ragged_column_tile", 50, 9, 20, 5)
# its row tiles (and the k loop over the same 32): less than one, one, one row over, three
_t("nlat3", "smallest_nlat", 17, 3, 24, 2)
_t("nlat5", "row_tile_ragged", 17, 5, 24, 4)
_t("nlat31", "row_tile_ragged", 17, 31, 24, 10)
_t("nlat32", "row_tile_full", 17, 32, 24, 10)
_t("nlat33", "second_row_tile_of_one", 17, 33, 24, 10)
_t("nlat65", "three_row_tiles", 17, 65, 24, 10)
_t("nlat33_gaussian", "second_row_tile_of_one", 17, 33, 24, 10, "gaussian")
# the shortest rows, the extreme truncations
_t("nlon4", "smallest_nlon", 3, 5, 4, 1)
_t("nlon5", "odd_nlon", 3, 5, 5, 2)
_t("T0", "zonal_mean_only", 3, 9, 16, 0)
_t("T_nlat_minus_1", "full_latitude_band", 3, 9, 20, 8)
_t("T_half_odd_nlon", "highest_wavenumber_odd", 3, 12, 17, 8)        # nlon = 2 T + 1
_t("T_half_even_nlon", "highest_wavenumber_even", 3, 12, 18, 8)      # nlon = 2 T + 2: one below Nyquist
# the spectral columns: a wave's second trip in the forward DFT, a thread's second coefficient in the inverse DFT
_t("C68", "forward_second_trip", 2, 34, 68, 33)
_t("C258", "inverse_second_coefficient", 1, 130, 258, 128)
# rows a forward-DFT block stages: 4, 3, 2, 1; tail blocks with empty slots
_t("rpb3", "rows_per_block_3", 1, 5, 2200, 2)                        # 5 rows: the second block has one empty slot
_t("rpb2", "rows_per_block_2", 1, 3, 2736, 1)
_t("rpb1", "rows_per_block_1", 1, 3, 4100, 1)
_t("rpb1_all_lds", "rows_per_block_1_64k", 1, 3, 8192, 1)            # exactly 64 KB of dynamic LDS

TRUNC_F32 = ("nb17", "nlat33", "nlon5", "rpb3")

# (nlat, nlon, T) -> a piece of the message; each is refused before anything is launched or built
TRUNC_REFUSALS = (
    (3, 8193, 1, "longitudes exceed"),
    (5, 16, 5, "too high"),              # T > nlat - 1
    (2, 16, 1, "bad sizes"),
    (9, 16, -1, "truncation must be >= 0"),
)

NONFINITE = dict(nb=20, nlat=9, nlon=20, T=5, nan_member=7, inf_member=18)

# (nlat, nlon, T, gridtype) in order on one engine: another grid type, another T, then the first again
CACHE_SEQUENCE = ((33, 66, 16, "regular"), (33, 66, 16, "gaussian"), (33, 66, 8, "regular"), (33, 66, 16, "regular"))


def trunc_input(nb, nlat, nlon, dtype="float64"):
    return np.random.default_rng([11, nb, nlat, nlon]).standard_normal((nb, nlat, nlon)).astype(dtype)


def nonfinite_input():
    c = NONFINITE
    clean = trunc_input(c["nb"], c["nlat"], c["nlon"])
    dirty = clean.copy()
    dirty[c["nan_member"], 4, 11] = np.nan
    dirty[c["inf_member"], 0, 0] = np.inf
    return clean, dirty


def reaches(case):
    """The branch names a truncation case reaches, by the launch arithmetic above."""
    nb, nlat, nlon, T = case["nb"], case["nlat"], case["nlon"], case["T"]
    rpb, rows, C, cols = rows_per_block(nlon), nb * nlat, coefficients(T), 2 * nb
    got = {f"rows_per_block_{rpb}"}
    if 8 * nlon == LDS_FORWARD:
        got.add("rows_per_block_1_64k")
    if rows % rpb:
        got.add("forward_tail_block")
    if C > WAVE:
        got.add("forward_second_trip")
    if C > BLOCK:
        got.add("inverse_second_coefficient")
    if cols == PT:
        got.add("one_full_column_tile")
    if column_tiles(nb) > 1:
        got.add("column_tile_past_first")
        if cols % PT == 2 and column_tiles(nb) == 2:
            got.add("second_column_tile_of_two")
    if cols % PT:
        got.add("ragged_column_tile")
    if nlat % PT:
        got.add("row_tile_ragged")
    else:
        got.add("row_tile_full")
    if row_tiles(nlat) > 1:
        got.add("row_tile_past_first")
        if nlat % PT == 1:
            got.add("second_row_tile_of_one")
    if row_tiles(nlat) >= 3:
        got.add("three_row_tiles")
    if nlat == MIN_NLAT:
        got.add("smallest_nlat")
    if nlon == MIN_NLON:
        got.add("smallest_nlon")
    if nlon % 2:
        got.add("odd_nlon")
    if T == 0:
        got.add("zonal_mean_only")
    if T == nlat - 1:
        got.add("full_latitude_band")
    if T == (nlon - 1) // 2:
        got.add("highest_wavenumber_odd" if nlon % 2 else "highest_wavenumber_even")
    return got


# ------------------------------------------------------------------ regrid
# name -> what the case is there for.  ``common``: onto the 0.5 degree grid of LCS.py:107-108 (360 x 721 targets).
REGRID = {
    "stride_f64": dict(branch="grid_stride", dtype="float64", nt=17, ny=19, nx=40, common=True),      # 4,412,520 outputs
    "stride_f32": dict(branch="grid_stride", dtype="float32", nt=17, ny=19, nx=40, common=True),
    "gaussian_source": dict(branch="non_uniform_axis", dtype="float64", nt=2, ny=19, nx=40),
    "targets_on_nodes": dict(branch="target_equals_node", dtype="float64", nt=2, ny=7, nx=9),
    "unsorted_repeated_targets": dict(branch="unsorted_targets", dtype="float64", nt=2, ny=7, nx=9),
    "source_2x2": dict(branch="smallest_source", dtype="float64", nt=3, ny=2, nx=2),
    "one_node_targets": dict(branch="one_node_target_axis", dtype="float64", nt=2, ny=7, nx=9),
    "outside_all_sides": dict(branch="nearest_fill_outside", dtype="float64", nt=2, ny=7, nx=9),
    "nonfinite_source": dict(branch="nonfinite", dtype="float64", nt=2, ny=7, nx=9),
    "f32_overflow": dict(branch="float32_difference_overflows", dtype="float32", nt=1, ny=4, nx=5),
    "nan_beside_midpoint": dict(branch="nearest_tie_in_range", dtype="float64", nt=1, ny=10, nx=10, check="oracle+right_hand_node"),
}
for _c in REGRID.values():
    _c.setdefault("check", "oracle")       # PO.regrid_common_grid: NaN masks, infinities, then values within REGRID_ATOL x scale
TIE_NAN_NODE = (4, 5)             # (row, column) of the NaN in nan_beside_midpoint's 1 degree source, nodes 0 .. 9 on both axes
REGRID_ATOL = 1e-14               # per unit of data scale: the bound tests/test_preprocess_gpu.py states


def _uniform(n, lo, hi):
    return np.linspace(lo, hi, n)


def regrid_input(name):
    """(u, lat, lon, lats, lons) of one REGRID case; lats / lons None for the common grid."""
    c = REGRID[name]
    nt, ny, nx = c["nt"], c["ny"], c["nx"]
    rng = np.random.default_rng([13, nt, ny, nx, sorted(REGRID).index(name)])
    u = rng.standard_normal((nt, ny, nx)).astype(c["dtype"])
    lat, lon = _uniform(ny, -90.0, 90.0), -180.0 + 360.0 / nx * np.arange(nx)
    if c.get("common"):
        return u, lat, lon, None, None
    lats, lons = _uniform(23, -88.0, 88.0), _uniform(31, -179.0, 170.0)
    if name == "gaussian_source":
        lat = np.degrees(np.arcsin(np.polynomial.legendre.leggauss(ny)[0]))            # ascending, uneven, poles excluded
        lats = _uniform(37, -90.0, 90.0)                                               # so both ends are nearest-filled
    elif name == "targets_on_nodes":
        lats, lons = lat.copy(), lon.copy()                                            # first and last node included
    elif name == "unsorted_repeated_targets":
        lats = rng.permutation(np.concatenate([lats, lats[:5], [-95.0, 95.0, lat[2]]]))
        lons = rng.permutation(np.concatenate([lons, lons[-4:], [-200.0, 300.0, lon[3]]]))
    elif name == "source_2x2":
        lat, lon = np.array([-10.0, 30.0]), np.array([5.0, 6.5])
        lats, lons = np.array([-20.0, -10.0, 0.0, 29.0, 30.0, 31.0]), np.array([4.0, 5.0, 5.75, 6.5, 7.0])
    elif name == "one_node_targets":
        lats, lons = np.array([12.5]), np.array([-33.25])
    elif name == "outside_all_sides":
        lat, lon = _uniform(ny, -60.0, 60.0), _uniform(nx, -100.0, 100.0)
        lats, lons = np.array([-90.0, -60.5, -60.0, 0.0, 60.0, 60.5, 90.0]), np.array([-180.0, -100.5, -100.0, 3.0, 100.0, 100.5, 180.0])
    elif name == "nonfinite_source":
        u[0, 2, 3], u[0, 4, 6], u[1, 3, 3] = np.inf, -np.inf, np.nan
        u[1, 0, 0], u[1, ny - 1, nx - 1] = np.inf, np.nan                              # corners: reached by the nearest fill
        lats, lons = _uniform(25, -95.0, 95.0), _uniform(37, -185.0, 185.0)            # some targets on nodes (t = 0: inf * 0)
    elif name == "f32_overflow":
        u[0, 1, 2], u[0, 2, 2], u[0, 1, 3] = 3e38, -3e38, -3e38                        # float32 differences of -6e38: -inf
        lat, lon = np.arange(4.0), np.arange(5.0)
        lats, lons = np.array([0.0, 0.5, 1.0, 1.25, 1.5, 2.0, 2.5, 3.0]), np.array([0.0, 1.5, 2.0, 2.5, 3.0, 3.5, 4.0])
    elif name == "nan_beside_midpoint":
        lat, lon = np.arange(10.0), np.arange(10.0)                                    # 1 degree
        lats, lons = np.arange(19) * 0.5, np.arange(19) * 0.5                          # 0.5 degree: every second target a midpoint
        u[0][TIE_NAN_NODE] = np.nan
    return u, lat, lon, lats, lons


# (lat, lon) source axes lc_regrid_common_grid refuses with "must ascend"
REGRID_REFUSALS = (
    (np.array([3.0, 2.0, 1.0, 0.0]), np.arange(4.0)),            # descending
    (np.arange(4.0), np.array([0.0, 1.0, 1.0, 2.0])),            # repeated
)
