// Footprints: every (parcel, level) entry of a block of trajectory levels scattered into the cell of a target grid it lies in --
// where the air that arrives at the seeds has been, for how long, and what it carried there.
//
// The contract (include/lcs_hip.h has it in full; tests/footprint.py restates it in numpy).  Entry j of parcel i, unless it is
// entry 0 of a continued block, counts with the half-weight h = 1 (the record's first and last entry) or 2 (the trapezoid rule in
// halves), for a parcel of integer weight q > 0:
//   cell       fy = ((double)y - lat0) inv_dy + 0.5, row floor(fy) when 0 <= fy < ny_t; fx likewise, with cyclic_x reduced by
//              floored modulo nx_t when |fx| < 2^31: float64, no contraction, compared before any conversion
//   valid      hits[cell] += h, mass[cell] += h q; with c: v = rint((double)c c_scale), csum[cell] += h v and chits[cell] += h
//              when |v| <= 2^31, else stats[1] += h
//   invalid    stats[0] += h
// Every sum is a 64-bit integer add: whichever kernel, launch shape, split into blocks or run, the bits are the same.
//
// Two forms of one fold.
//   footprint_direct_kernel<T, HAS_C>   one thread per parcel, the level loop inside, FP_BATCH levels' loads in flight, one 64-bit
//                                       global atomic per sum and entry; one add per wave for stats
//   footprint_tile_kernel<T, HAS_C>     a workgroup owns a patch of FP_BY x FP_BX neighbouring seeds for all levels of the block.
//                                       Neighbouring seeds stay near each other, so it holds a window of FP_WY x FP_WX target
//                                       cells in LDS, adds into it with LDS atomics and flushes the non-zero cells, one global
//                                       atomic each.  The window is anchored anew every FP_SEG levels, at the cell of the
//                                       counted parcel nearest the patch's centre, and flushed before it moves.  An entry
//                                       outside it goes straight to global atomics: the window never decides a result.  The LDS
//                                       counters of hits are 32-bit -- between two flushes a cell takes at most 512 parcels x
//                                       4 levels x 2 = 2^12 --, those of h q and h v 64-bit (2^12 x 2^20, 2^12 x 2^31)
// What was measured and why the window is re-anchored as often as every FP_SEG = 4 levels (on a latitude-longitude seed grid a
// third of the parcels sit poleward of 58 degrees, where a few steps carry a patch across many columns): DESIGN.md section 4.
#include <stdint.h>

#include "lcs_common.h"

#pragma clang fp contract(off)

namespace {

typedef unsigned long long u64;

constexpr int FP_THREADS = 256;       // direct form: parcels of a workgroup
constexpr int FP_BATCH = 4;           // levels a thread loads before it bins them
constexpr int FP_BX = 64, FP_BY = 8;  // tiled form: seeds of a patch along longitude (one wavefront) and latitude
// (the window and the anchoring period can be set at compile time, -DLCS_FP_WX= ..., for experiment libraries: build.build_library)
#ifndef LCS_FP_WX
#define LCS_FP_WX 64
#endif
#ifndef LCS_FP_WY
#define LCS_FP_WY 32
#endif
#ifndef LCS_FP_SEG
#define LCS_FP_SEG 4
#endif
constexpr int FP_WX = LCS_FP_WX, FP_WY = LCS_FP_WY; // ... target cells of the LDS window
constexpr int FP_CELLS = FP_WX * FP_WY;
constexpr int FP_SEG = LCS_FP_SEG;    // ... levels between two anchorings of the window
constexpr long long FP_TILE_MIN_SEEDS = 1 << 16;  // auto: below this many seeds the direct form
static_assert((long long)FP_BX * FP_BY * FP_SEG * 2 < (1ll << 32) >> 1, "an LDS hit counter could overflow between two flushes");

template <typename T>
struct FootArgs {
    const T *x, *y, *c;  // [n_levels][n]
    const int *q;        // [n] or NULL
    u64 *hits, *mass, *csum, *chits, *stats;
    double lat0, lon0, inv_dy, inv_dx, ny_td, nx_td, c_scale;
    int n, ny, nx, n_levels, level0, final, ny_t, nx_t, cyclic, nbx, census;
};

// the cell of a position: false when it lies in none
template <typename T>
__device__ __forceinline__ bool fp_cell(const FootArgs<T> &A, T x, T y, int &row, int &col) {
    const double fy = ((double)y - A.lat0) * A.inv_dy + 0.5;
    const double fx = ((double)x - A.lon0) * A.inv_dx + 0.5;
    if (!(fy >= 0.0 && fy < A.ny_td)) return false;
    if (A.cyclic) {
        if (!(fabs(fx) < 2147483648.0)) return false;
        int m = (int)((long long)floor(fx) % A.nx_t);
        col = m < 0 ? m + A.nx_t : m;
    } else {
        if (!(fx >= 0.0 && fx < A.nx_td)) return false;
        col = (int)fx;  // not negative: truncation is the floor
    }
    row = (int)fy;
    return true;
}

template <typename T>
__device__ __forceinline__ bool fp_value(const FootArgs<T> &A, T c, long long &v) {
    const double r = rint((double)c * A.c_scale);
    if (!(fabs(r) <= 2147483648.0)) return false;  // NaN and inf fail the comparison
    v = (long long)r;
    return true;
}

template <typename T>
__device__ __forceinline__ unsigned fp_half_weight(const FootArgs<T> &A, int j) {
    return ((j == 0 && A.level0 == 0) || (j == A.n_levels - 1 && A.final)) ? 1u : 2u;
}

template <typename T, bool HAS_C>
__global__ void __launch_bounds__(FP_THREADS) footprint_direct_kernel(const FootArgs<T> A) {
    const size_t n = (size_t)A.n;
    const size_t i = (size_t)blockIdx.x * FP_THREADS + threadIdx.x;
    const int q = i < n ? (A.q ? A.q[i] : 1) : 0;
    const int last = A.n_levels - 1;
    u64 out = 0, drop = 0;
    if (q > 0) {
        for (int j0 = A.level0 > 0 ? 1 : 0; j0 <= last; j0 += FP_BATCH) {
            T bx[FP_BATCH], by[FP_BATCH], bc[FP_BATCH];
#pragma unroll
            for (int d = 0; d < FP_BATCH; ++d) {
                const size_t e = (size_t)(j0 + d < last ? j0 + d : last) * n + i;
                bx[d] = A.x[e], by[d] = A.y[e];
                bc[d] = HAS_C ? A.c[e] : T(0);
            }
#pragma unroll
            for (int d = 0; d < FP_BATCH; ++d) {
                const int j = j0 + d;
                if (j > last) break;
                const unsigned h = fp_half_weight(A, j);
                int row, col;
                if (!fp_cell(A, bx[d], by[d], row, col)) {
                    out += h;
                    continue;
                }
                const size_t cell = (size_t)row * A.nx_t + col;
                if (A.hits) atomicAdd(A.hits + cell, (u64)h);
                if (A.mass) atomicAdd(A.mass + cell, (u64)h * (u64)q);
                if (HAS_C) {
                    long long v;
                    if (!fp_value(A, bc[d], v)) {
                        drop += h;
                    } else if (A.csum) {
                        atomicAdd(A.csum + cell, (u64)((long long)h * v));
                        atomicAdd(A.chits + cell, (u64)h);
                    }
                }
            }
        }
    }
    // stats: one add per wave
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        out += __shfl_down(out, s, 64);
        drop += __shfl_down(drop, s, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (out) atomicAdd(A.stats, out);
        if (drop) atomicAdd(A.stats + 1, drop);
    }
}

template <typename T, bool HAS_C>
__global__ void __launch_bounds__(FP_BX *FP_BY) footprint_tile_kernel(const FootArgs<T> A) {
    __shared__ unsigned s_hits[FP_CELLS], s_chits[FP_CELLS];
    __shared__ u64 s_mass[FP_CELLS], s_csum[FP_CELLS];
    __shared__ u64 s_key, s_stats[3];
    const int lane = threadIdx.x, w = threadIdx.y, tid = w * FP_BX + lane;
    const int bx = (int)(blockIdx.x % (unsigned)A.nbx), by = (int)(blockIdx.x / (unsigned)A.nbx);
    const int r = by * FP_BY + w, cc = bx * FP_BX + lane;
    const bool here = r < A.ny && cc < A.nx;
    const size_t n = (size_t)A.n, i = here ? (size_t)r * A.nx + cc : 0;
    const int q = here ? (A.q ? A.q[i] : 1) : 0;
    const bool use_mass = A.mass && A.q;  // without q, mass is hits: taken from the hits at the flush
    const bool use_c = HAS_C && A.csum;
    const int last = A.n_levels - 1;
    // nearer the patch's centre is smaller; ties are broken by the cell: any choice gives the same sums
    const u64 prox = (u64)((w < FP_BY / 2 ? FP_BY / 2 - w : w - FP_BY / 2) * FP_BX + (lane < FP_BX / 2 ? FP_BX / 2 - lane : lane - FP_BX / 2));
    for (int k = tid; k < FP_CELLS; k += FP_BX * FP_BY) {
        s_hits[k] = 0, s_mass[k] = 0;
        if (HAS_C) s_chits[k] = 0, s_csum[k] = 0;
    }
    if (tid < 3) s_stats[tid] = 0;
    u64 out = 0, drop = 0, left = 0;
    for (int s0 = A.level0 > 0 ? 1 : 0; s0 <= last; s0 += FP_SEG) {
        const int s1 = s0 + FP_SEG - 1 < last ? s0 + FP_SEG - 1 : last;
        if (tid == 0) s_key = ~0ull;
        __syncthreads();
        if (q > 0) {
            int row, col;
            const size_t e = (size_t)s0 * n + i;
            if (fp_cell(A, A.x[e], A.y[e], row, col)) atomicMin(&s_key, (prox << 32) | (u64)(unsigned)(row * A.nx_t + col));
        }
        __syncthreads();
        const u64 key = s_key;
        int oy = 0, ox = 0;
        if (key != ~0ull) {
            const int cell = (int)(unsigned)key;
            oy = cell / A.nx_t - FP_WY / 2, ox = cell % A.nx_t - FP_WX / 2;
        }
        if (q > 0) {
            for (int j0 = s0; j0 <= s1; j0 += FP_BATCH) {
                T qx[FP_BATCH], qy[FP_BATCH], qc[FP_BATCH];
#pragma unroll
                for (int d = 0; d < FP_BATCH; ++d) {
                    const size_t e = (size_t)(j0 + d < s1 ? j0 + d : s1) * n + i;
                    qx[d] = A.x[e], qy[d] = A.y[e];
                    qc[d] = HAS_C ? A.c[e] : T(0);
                }
#pragma unroll
                for (int d = 0; d < FP_BATCH; ++d) {
                    const int j = j0 + d;
                    if (j > s1) break;
                    const unsigned h = fp_half_weight(A, j);
                    int row, col;
                    if (!fp_cell(A, qx[d], qy[d], row, col)) {
                        out += h;
                        continue;
                    }
                    const int rr = row - oy;
                    int rc = col - ox;
                    if (A.cyclic) {
                        rc %= A.nx_t;
                        rc = rc < 0 ? rc + A.nx_t : rc;
                    }
                    const bool in = (unsigned)rr < (unsigned)FP_WY && (unsigned)rc < (unsigned)FP_WX;
                    const int wi = rr * FP_WX + rc;
                    const size_t cell = (size_t)row * A.nx_t + col;
                    if (in) {
                        atomicAdd(&s_hits[wi], h);
                        if (use_mass) atomicAdd(&s_mass[wi], (u64)h * (u64)q);
                    } else {
                        left += h;
                        if (A.hits) atomicAdd(A.hits + cell, (u64)h);
                        if (A.mass) atomicAdd(A.mass + cell, (u64)h * (u64)q);
                    }
                    if (HAS_C) {
                        long long v;
                        if (!fp_value(A, qc[d], v)) {
                            drop += h;
                        } else if (use_c) {
                            if (in) {
                                atomicAdd(&s_csum[wi], (u64)((long long)h * v));
                                atomicAdd(&s_chits[wi], h);
                            } else {
                                atomicAdd(A.csum + cell, (u64)((long long)h * v));
                                atomicAdd(A.chits + cell, (u64)h);
                            }
                        }
                    }
                }
            }
        }
        __syncthreads();
        // the flush: a window cell that took an entry has hits; it is a cell of the grid, since only valid entries enter
        for (int k = tid; k < FP_CELLS; k += FP_BX * FP_BY) {
            const unsigned hc = s_hits[k];
            if (!hc) continue;
            s_hits[k] = 0;
            const int row = oy + k / FP_WX;
            int col = ox + k % FP_WX;
            if (A.cyclic) {
                col %= A.nx_t;
                col = col < 0 ? col + A.nx_t : col;
            }
            if (row < 0 || row >= A.ny_t || col < 0 || col >= A.nx_t) continue;
            const size_t cell = (size_t)row * A.nx_t + col;
            if (A.hits) atomicAdd(A.hits + cell, (u64)hc);
            if (A.mass) atomicAdd(A.mass + cell, use_mass ? s_mass[k] : (u64)hc);
            if (use_mass) s_mass[k] = 0;
            if (use_c) {
                const unsigned ch = s_chits[k];
                if (ch) {
                    atomicAdd(A.csum + cell, s_csum[k]);
                    atomicAdd(A.chits + cell, (u64)ch);
                    s_csum[k] = 0, s_chits[k] = 0;
                }
            }
        }
    }
    if (out) atomicAdd(&s_stats[0], out);
    if (drop) atomicAdd(&s_stats[1], drop);
    if (left) atomicAdd(&s_stats[2], left);
    __syncthreads();
    if (tid < (A.census ? 3 : 2) && s_stats[tid]) atomicAdd(A.stats + tid, s_stats[tid]);
}

template <typename T>
void launch(lc_ctx *ctx, const lc_footprint_args *a, bool tiled, int census) {
    FootArgs<T> A;
    A.x = (const T *)a->traj_x, A.y = (const T *)a->traj_y, A.c = (const T *)a->c;
    A.q = (const int *)a->q;
    A.hits = (u64 *)a->hits, A.mass = (u64 *)a->mass, A.csum = (u64 *)a->csum, A.chits = (u64 *)a->chits, A.stats = (u64 *)a->stats;
    A.lat0 = a->lat0, A.lon0 = a->lon0;
    A.inv_dy = (double)(a->ny_t - 1) / (a->lat1 - a->lat0), A.inv_dx = (double)(a->nx_t - 1) / (a->lon1 - a->lon0);
    A.ny_td = (double)a->ny_t, A.nx_td = (double)a->nx_t;
    A.c_scale = a->c ? a->c_scale : 1.0;
    A.n = a->n, A.ny = a->ny, A.nx = a->nx, A.n_levels = a->n_levels, A.level0 = a->level0, A.final = a->final != 0;
    A.ny_t = a->ny_t, A.nx_t = a->nx_t, A.cyclic = a->cyclic_x != 0;
    A.nbx = (a->nx + FP_BX - 1) / FP_BX;
    A.census = census;
    if (tiled) {
        const dim3 grid((unsigned)((long long)A.nbx * ((a->ny + FP_BY - 1) / FP_BY))), block(FP_BX, FP_BY);
        if (a->c)
            hipLaunchKernelGGL((footprint_tile_kernel<T, true>), grid, block, 0, ctx->stream, A);
        else
            hipLaunchKernelGGL((footprint_tile_kernel<T, false>), grid, block, 0, ctx->stream, A);
    } else {
        const dim3 grid((unsigned)(((long long)a->n + FP_THREADS - 1) / FP_THREADS)), block(FP_THREADS);
        if (a->c)
            hipLaunchKernelGGL((footprint_direct_kernel<T, true>), grid, block, 0, ctx->stream, A);
        else
            hipLaunchKernelGGL((footprint_direct_kernel<T, false>), grid, block, 0, ctx->stream, A);
    }
}

const char *const FP_NAMES[2][2][2] = {
    {{"footprint_direct_kernel<float, false>", "footprint_direct_kernel<float, true>"},
     {"footprint_direct_kernel<double, false>", "footprint_direct_kernel<double, true>"}},
    {{"footprint_tile_kernel<float, false>", "footprint_tile_kernel<float, true>"},
     {"footprint_tile_kernel<double, false>", "footprint_tile_kernel<double, true>"}}};

}  // namespace

extern "C" int lc_footprint_update(lc_ctx *ctx, const lc_footprint_args *a) {
    const char *who = "lc_footprint_update";
    LC_REQUIRE(ctx, "%s: null context", who);
    LC_REQUIRE(a, "%s: null argument structure", who);
    LC_REQUIRE(a->struct_size == sizeof(lc_footprint_args), "%s: struct_size %zu, this library has %zu", who, (size_t)a->struct_size,
               sizeof(lc_footprint_args));
    LC_REQUIRE(a->dtype == LC_F32 || a->dtype == LC_F64, "%s: bad dtype %d", who, a->dtype);
    LC_REQUIRE(a->n >= 1, "%s: n %d (at least one parcel)", who, a->n);
    LC_REQUIRE(a->ny >= 1 && a->nx >= 1 && (long long)a->ny * a->nx == (long long)a->n, "%s: seed grid %dx%d for n %d (ny nx == n)", who,
               a->ny, a->nx, a->n);
    LC_REQUIRE(a->n_levels >= 2, "%s: n_levels %d (a block has at least two trajectory entries)", who, a->n_levels);
    LC_REQUIRE(a->level0 >= 0, "%s: level0 %d", who, a->level0);
    LC_REQUIRE(a->ny_t >= 2 && a->nx_t >= 2, "%s: target grid %dx%d (at least 2 cells a side)", who, a->ny_t, a->nx_t);
    LC_REQUIRE((long long)a->ny_t * a->nx_t < ((long long)1 << 31), "%s: target grid %dx%d (fewer than 2^31 cells)", who, a->ny_t, a->nx_t);
    LC_REQUIRE(a->lat0 - a->lat0 == 0.0 && a->lat1 - a->lat1 == 0.0 && a->lat0 < a->lat1, "%s: bad latitudes %g .. %g (finite, ascending)",
               who, a->lat0, a->lat1);
    LC_REQUIRE(a->lon0 - a->lon0 == 0.0 && a->lon1 - a->lon1 == 0.0 && a->lon0 < a->lon1, "%s: bad longitudes %g .. %g (finite, ascending)",
               who, a->lon0, a->lon1);
    LC_REQUIRE(!a->c || (a->c_scale - a->c_scale == 0.0 && a->c_scale > 0.0), "%s: c_scale %g (positive and finite, with c)", who, a->c_scale);
    LC_REQUIRE(a->c || (!a->csum && !a->chits), "%s: csum and chits need c", who);
    LC_REQUIRE(!a->csum == !a->chits, "%s: csum and chits come together (both or neither)", who);
    LC_REQUIRE(a->hits || a->mass || a->csum, "%s: no output (hits, mass, or csum with chits)", who);
    LC_REQUIRE(a->traj_x && a->traj_y && a->stats, "%s: null pointer", who);
    const long long groups = (((long long)a->nx + FP_BX - 1) / FP_BX) * (((long long)a->ny + FP_BY - 1) / FP_BY);
    // auto: the tiled form where a patch is filled and the launch is large enough to pay for its flushes
    const bool tile_fits = groups < ((long long)1 << 31);
    const bool tiled = ctx->footprint_form < 0 ? tile_fits && a->ny >= FP_BY && (long long)a->n >= FP_TILE_MIN_SEEDS : ctx->footprint_form >= 1;
    LC_REQUIRE(!tiled || tile_fits, "%s: a %dx%d seed grid needs %lld workgroups in the tiled form (too many for one launch)", who, a->ny,
               a->nx, groups);
    LC_HIP_CHECK(hipSetDevice(ctx->device));
    if (a->zero_first) {
        const size_t bytes = (size_t)a->ny_t * a->nx_t * sizeof(int64_t);
        int64_t *const planes[4] = {a->hits, a->mass, a->csum, a->chits};
        for (int k = 0; k < 4; ++k)
            if (planes[k]) LC_HIP_CHECK(hipMemsetAsync(planes[k], 0, bytes, ctx->stream));
        LC_HIP_CHECK(hipMemsetAsync(a->stats, 0, 4 * sizeof(int64_t), ctx->stream));
    }
    const int census = ctx->footprint_form == 2;
    if (a->dtype == LC_F32)
        launch<float>(ctx, a, tiled, census);
    else
        launch<double>(ctx, a, tiled, census);
    ctx->last_footprint_kernel = FP_NAMES[tiled][a->dtype == LC_F64][a->c != nullptr];
    LC_HIP_CHECK(hipGetLastError());
    return LC_OK;
}

extern "C" const char *lc_ctx_last_footprint_kernel(const lc_ctx *ctx) { return ctx ? ctx->last_footprint_kernel : ""; }

extern "C" int lc_ctx_set_footprint_form(lc_ctx *ctx, int mode) {
    LC_REQUIRE(ctx, "lc_ctx_set_footprint_form: null context");
    LC_REQUIRE(mode >= -1 && mode <= 2, "lc_ctx_set_footprint_form: mode %d (-1 auto, 0 direct, 1 tiled, 2 tiled with the window census)", mode);
    ctx->footprint_form = mode;
    return LC_OK;
}
