// K3b -- finite-size Lyapunov exponents: a record of trajectory planes reduced, block of levels by block of levels, to the time
// tau every cell's neighbour pairs take to separate to a threshold, and to lambda = ln(T / d(0)) / tau.
//
// The contract (include/lcs_hip.h has it in full; tests/fsle.py restates it in numpy).  Positions are degrees, k = pi / 180.
//   pairs       every horizontally or vertically adjacent couple of seeds; with cyclic_x column nx-1 pairs with column 0.  A cell
//               owns up to four, in the order E, W, N, S; the E pair of (r, c) is the W pair of (r, c+1): same parcels, same numbers
//   separation  h = sin^2(k dphi / 2) + cos(k phi1) cos(k phi2) sin^2(k dlambda / 2),  d = 2 radius asin(min(1, sqrt h)), dlambda the
//               raw difference (the form is periodic: the seam needs no wrap); d(0) from seed_lat / seed_lon
//   threshold   ratio: T = ratio_q d(0); distance: T = delta_q metres.  A pair is eligible when d(0) is finite, > 0 and < T
//   crossing    the first level j >= 1 with both separations finite and d(j-1) < T <= d(j):
//               t = (j-1 + (T - d(j-1)) / (d(j) - d(j-1))) |timestep|
//   cell        tau = the minimum of t over the cell's pairs (ties: E, W, N, S), fsle = ln(T / d(0)) / tau of that pair (ratio mode:
//               ln(ratio_q) / tau); NaN where no pair upcrosses
//   streaming   tau and fsle are the only state between blocks; a cell whose tau[q] is finite is final for q.  A block therefore
//               walks its levels in order and closes a cell at the first level where one of its pairs upcrosses (among the pairs
//               that upcross at that level: the smallest t, ties E, W, N, S) -- which is what makes any split of the levels into
//               blocks give the bits one block gives.  In real arithmetic it equals the minimum over the pairs' first crossings,
//               because a crossing at a later level has a larger t; in floating point j + f with a tiny f can round to j and tie
//               with a pair that crossed one level earlier with f = 1: such a tie across levels goes to the earlier level's pair,
//               whatever the E, W, N, S order says (the streaming rule decides: that cell was already final).
//
// Shape.  One thread per PARCEL of an 8 rows x 64 columns patch, one wavefront per row, patches overlapping by one parcel on
// every side: a cell needs its four neighbours, so a patch yields 6 x 62 cells.  Per level a thread loads its parcel's position (a
// wavefront reads one 256 / 512 B line of the plane: coalesced along longitude; the next level's load is issued before this
// level's arithmetic), takes cos(k phi) once, and forms the separations of its W pair (the west neighbour's position and cosine
// come from lane - 1 by a wavefront shuffle) and of its S pair (the row below through LDS).  Each pair is formed once per level
// in a patch and handed to its other cell: E is the W pair of lane + 1 (shuffle), N is the S pair of the row above (LDS).  Two
// barriers per level; 8 / 16 KB of LDS; no atomics, no inline assembly, nothing between workgroups.  A cell closes once per
// threshold, so tau and fsle go straight to memory at the crossing and the only per-threshold state in registers is one bit.
// The asin is taken at every level, as a short polynomial in float32 (the test on h against sin^2(T / 2 radius) was not built:
// it needs a threshold per pair in ratio mode).  HBM traffic per level and cell: the two positions, read 1.4x for the overlap.
// Measured: the barriers bind, not the arithmetic or the memory -- 16-row patches are a third slower than 8-row ones.
//   fsle_update_kernel<float, 8>    float32, 512 threads
//   fsle_update_kernel<double, 8>   float64, 512 threads
#include "great_circle.h"   // fsle_cos, fsle_sep, fsle_log: shared with lavd.hip

namespace {

constexpr int FSLE_BX = 64;      // parcels of a patch along longitude: one wavefront
constexpr int FSLE_CX = FSLE_BX - 2;  // cells of a patch along longitude
constexpr int FSLE_MAXQ = 8;
constexpr int FSLE_ROWS = 8;     // rows of a patch, both dtypes (16 and 4 were measured in float32: DESIGN.md)

template <typename T>
struct FsleArgs {
    const T *traj_x, *traj_y;      // [n_levels][ny*nx]
    const T *seed_lat, *seed_lon;  // [ny], [nx]
    T *tau, *fsle;                 // [n_thr][ny*nx]
    T thr[FSLE_MAXQ];
    T radius, dt;                  // dt = |timestep|
    int ny, nx, n_levels, level0, n_thr, mode, cyclic, nbx;
};

template <typename T, int BY>
__global__ void __launch_bounds__(FSLE_BX *BY) fsle_update_kernel(const FsleArgs<T> A) {
#pragma clang fp contract(off)
    __shared__ T s_x[BY][FSLE_BX], s_y[BY][FSLE_BX], s_c[BY][FSLE_BX], s_d[BY][FSLE_BX];
    const int lane = threadIdx.x, w = threadIdx.y;
    const int bx = (int)(blockIdx.x % (unsigned)A.nbx), by = (int)(blockIdx.x / (unsigned)A.nbx);
    const int ny = A.ny, nx = A.nx;
    const size_t cells = (size_t)ny * nx;
    const T nan = __builtin_nan("");
    const T two_r = T(2) * A.radius;

    // this thread's parcel: row rr, column cc before the cyclic wrap, col after it
    const int rr = by * (BY - 2) - 1 + w;
    const long long cc = (long long)bx * FSLE_CX - 1 + lane;
    auto wrapped = [&](long long c, int &col) -> bool {  // is column c (one step past either edge at most) a parcel, and which
        if (c >= 0 && c < nx) { col = (int)c; return true; }
        if (A.cyclic && c == -1) { col = nx - 1; return true; }
        if (A.cyclic && c == nx) { col = 0; return true; }
        col = 0;
        return false;
    };
    int col, col_w;
    const bool row_in = rr >= 0 && rr < ny;
    const bool here = wrapped(cc, col) && row_in;
    // the W pair (with lane - 1) and the S pair (with the row below) of this parcel, where both ends exist in this patch
    const bool pair_w = here && lane >= 1 && wrapped(cc - 1, col_w);
    const bool pair_s = here && w >= 1 && rr >= 1;
    const size_t at = here ? (size_t)rr * nx + col : 0;
    // the cell this thread writes: inside the patch's rim and inside the grid
    const bool cell = here && lane >= 1 && lane <= FSLE_CX && w >= 1 && w <= BY - 2 && cc >= 0 && cc < nx;

    // separations of the W and S pairs of this thread's parcel from its position, and the hand-over to the pairs' other cells:
    // returns E, W, N, S of this thread's cell (NaN for a pair that does not exist)
    auto separations = [&](T x, T y, T d[4]) {
        const T c = fsle_cos(y);
        const T xl = __shfl_up(x, 1), yl = __shfl_up(y, 1), cl = __shfl_up(c, 1);
        s_x[w][lane] = x, s_y[w][lane] = y, s_c[w][lane] = c;
        __syncthreads();
        const int wb = w >= 1 ? w - 1 : 0;
        const T xb = s_x[wb][lane], yb = s_y[wb][lane], cb = s_c[wb][lane];
        const T dw = pair_w ? fsle_sep(xl, yl, cl, x, y, c, two_r) : nan;
        const T ds = pair_s ? fsle_sep(xb, yb, cb, x, y, c, two_r) : nan;
        const T de = __shfl_down(dw, 1);
        s_d[w][lane] = ds;
        __syncthreads();
        d[0] = lane < FSLE_BX - 1 ? de : nan;
        d[1] = dw;
        d[2] = w < BY - 1 ? s_d[w + 1][lane] : nan;
        d[3] = ds;
    };

    T d0[4], dprev[4], dcur[4];
    separations(here ? A.seed_lon[col] : nan, here ? A.seed_lat[rr] : nan, d0);
    if (A.level0 == 0) {
#pragma unroll
        for (int p = 0; p < 4; ++p) dprev[p] = d0[p];
    } else {  // a continued block: its entry 0 is the last entry of the block before
        separations(here ? A.traj_x[at] : nan, here ? A.traj_y[at] : nan, dprev);
    }

    // which thresholds this cell is still open for.  A cell closes once per threshold, so tau and fsle are written straight to
    // memory at the crossing and never held in registers; what is still open at the end of the first block gets its NaN there
    // (a later block finds it in place).
    unsigned open = 0;
    if (cell) {
        for (int q = 0; q < A.n_thr; ++q) {
            const T carried = A.level0 == 0 ? nan : A.tau[(size_t)q * cells + at];
            open |= (carried == carried ? 0u : 1u) << q;
        }
    }

    // the next level's position is asked for before this level's arithmetic, which then hides its latency
    T xn = here ? A.traj_x[cells + at] : nan, yn = here ? A.traj_y[cells + at] : nan;
    for (int j = 1; j < A.n_levels; ++j) {
        const T xj = xn, yj = yn;
        if (j + 1 < A.n_levels && here) {
            const size_t o = (size_t)(j + 1) * cells + at;
            xn = A.traj_x[o], yn = A.traj_y[o];
        }
        separations(xj, yj, dcur);
        const T before = (T)(A.level0 + j - 1);  // whole steps before this interval
#pragma unroll 1
        for (int q = 0; q < A.n_thr; ++q) {
            if (!(open >> q & 1u)) continue;
            const T thr_q = A.thr[q];
            // which of the four pairs upcross T in this interval: eligible (d0 finite, > 0, < T) and d(j-1) < T <= d(j); a NaN
            // fails every comparison.  Comparisons only: the divisions wait for a hit
            T thr4[4];
            unsigned hit = 0;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                thr4[p] = A.mode == LC_FSLE_RATIO ? thr_q * d0[p] : thr_q;
                hit |= (unsigned)(d0[p] > T(0) && d0[p] < thr4[p] && dprev[p] < thr4[p] && thr4[p] <= dcur[p]) << p;
            }
            if (!hit) continue;
            T best = nan, best_thr = nan, best_d0 = nan;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                if (hit >> p & 1u) {
                    const T t = (before + (thr4[p] - dprev[p]) / (dcur[p] - dprev[p])) * A.dt;
                    if (!(best == best) || t < best) best = t, best_thr = thr4[p], best_d0 = d0[p];
                }
            }
            if (best == best) {
                A.tau[(size_t)q * cells + at] = best;
                A.fsle[(size_t)q * cells + at] = (A.mode == LC_FSLE_RATIO ? fsle_log(thr_q) : fsle_log(best_thr / best_d0)) / best;
                open &= ~(1u << q);
            }
        }
#pragma unroll
        for (int p = 0; p < 4; ++p) dprev[p] = dcur[p];
    }

    if (A.level0 == 0) {
        for (int q = 0; q < A.n_thr; ++q)
            if (open >> q & 1u) A.tau[(size_t)q * cells + at] = nan, A.fsle[(size_t)q * cells + at] = nan;
    }
}

template <typename T, int BY>
int fsle_impl(lc_ctx *ctx, const lc_fsle_args *a, const char *name) {
    FsleArgs<T> A;
    A.traj_x = (const T *)a->traj_x, A.traj_y = (const T *)a->traj_y;
    A.seed_lat = (const T *)a->seed_lat_dev, A.seed_lon = (const T *)a->seed_lon_dev;
    A.tau = (T *)a->tau, A.fsle = (T *)a->fsle;
    for (int q = 0; q < FSLE_MAXQ; ++q) A.thr[q] = q < a->n_thr ? (T)a->thresholds[q] : (T)0;
    A.radius = (T)a->radius;
    A.dt = (T)fabs(a->timestep);
    A.ny = a->ny, A.nx = a->nx, A.n_levels = a->n_levels, A.level0 = a->level0, A.n_thr = a->n_thr, A.mode = a->mode;
    A.cyclic = a->cyclic_x ? 1 : 0;
    const long long nbx = ((long long)a->nx + FSLE_CX - 1) / FSLE_CX, nby = ((long long)a->ny + (BY - 2) - 1) / (BY - 2);
    A.nbx = (int)nbx;
    ctx->last_fsle_kernel = name;
    hipLaunchKernelGGL((fsle_update_kernel<T, BY>), dim3((unsigned)(nbx * nby)), dim3(FSLE_BX, BY), 0, ctx->stream, A);
    LC_HIP_CHECK(hipGetLastError());
    return LC_OK;
}

}  // namespace

extern "C" int lc_fsle_update(lc_ctx *ctx, const lc_fsle_args *a) {
    const char *who = "lc_fsle_update";
    LC_REQUIRE(ctx, "%s: null context", who);
    LC_REQUIRE(a, "%s: null argument structure", who);
    LC_REQUIRE(a->struct_size == sizeof(lc_fsle_args), "%s: struct_size %zu, this library has %zu", who, (size_t)a->struct_size,
               sizeof(lc_fsle_args));
    LC_REQUIRE(a->dtype == LC_F32 || a->dtype == LC_F64, "%s: bad dtype %d", who, a->dtype);
    LC_REQUIRE(a->mode == LC_FSLE_RATIO || a->mode == LC_FSLE_DISTANCE, "%s: bad mode %d", who, a->mode);
    LC_REQUIRE(a->ny >= 1 && a->nx >= 1 && !(a->ny == 1 && a->nx == 1), "%s: bad grid %dx%d (at least two seeds)", who, a->ny, a->nx);
    LC_REQUIRE((size_t)a->ny * (size_t)a->nx < ((size_t)1 << 31), "%s: a plane of %dx%d cells (2^31 or more)", who, a->ny, a->nx);
    LC_REQUIRE(a->n_levels >= 2, "%s: n_levels %d (a block has at least two trajectory entries)", who, a->n_levels);
    LC_REQUIRE(a->level0 >= 0, "%s: level0 %d", who, a->level0);
    LC_REQUIRE(a->n_thr >= 1 && a->n_thr <= FSLE_MAXQ, "%s: n_thr %d (1 to %d)", who, a->n_thr, FSLE_MAXQ);
    for (int q = 0; q < a->n_thr; ++q) {
        // as the kernel will see it: in float32 a ratio of 1 + 1e-9 is 1, which no pair could ever cross
        const double t = a->dtype == LC_F32 ? (double)(float)a->thresholds[q] : a->thresholds[q];
        LC_REQUIRE(t - t == 0.0 && (a->mode == LC_FSLE_RATIO ? t > 1.0 : t > 0.0),
                   "%s: threshold %d is %g once rounded to the dtype (finite, and > 1 as a ratio, > 0 as a distance)", who, q, t);
    }
    LC_REQUIRE(a->radius - a->radius == 0.0 && a->radius > 0.0, "%s: radius %g (positive and finite)", who, a->radius);
    LC_REQUIRE(a->timestep - a->timestep == 0.0 && a->timestep != 0.0, "%s: timestep %g (non-zero and finite)", who, a->timestep);
    LC_REQUIRE(a->traj_x && a->traj_y && a->seed_lat_dev && a->seed_lon_dev && a->tau && a->fsle, "%s: null pointer", who);
    {  // one launch holds fewer than 2^32 threads: a grid one seed wide or high reaches that long before 2^31 cells
        const long long rows = FSLE_ROWS;
        const long long groups = (((long long)a->nx + FSLE_CX - 1) / FSLE_CX) * (((long long)a->ny + rows - 3) / (rows - 2));
        LC_REQUIRE(groups * rows * FSLE_BX < ((long long)1 << 32), "%s: a %dx%d grid needs %lld workgroups (too many for one launch)", who,
                   a->ny, a->nx, groups);
    }
    LC_HIP_CHECK(hipSetDevice(ctx->device));
    if (a->dtype == LC_F32) return fsle_impl<float, FSLE_ROWS>(ctx, a, "fsle_update_kernel<float, 8>");
    return fsle_impl<double, FSLE_ROWS>(ctx, a, "fsle_update_kernel<double, 8>");
}

extern "C" const char *lc_ctx_last_fsle_kernel(const lc_ctx *ctx) { return ctx ? ctx->last_fsle_kernel : ""; }
