// Inverse-distance weighting of scattered values on the sphere: the device side of tools.Inverse_weighted_interpolation and
// tools.xr_idx_interp (LCS/tools.py:285-333, an all-pairs numba loop there).  Checked against the numpy oracle of tests/idw.py in
// tests/test_idw_gpu.py.  Two departures from the reference, both stated in include/lcs_hip.h: the distance is the project's own
// chord form (the reference's haversine calls arctan where it means arctan2), and a source that coincides with a target is the
// limit of the weighting, the mean of the coincident values (inf / inf = NaN there).
//
// The host hands over the unit vectors of sources and targets, X = fl(cos lat cos lon), Y = fl(cos lat sin lon), Z = sin lat
// (numpy's); no kernel evaluates a trigonometric function of a coordinate.  A point that is to be left out has NaN components:
// its cost to anything is NaN, and a NaN is within no reach.  The cost of a pair is sphere_distance.hip's squared chord
//     cost = fl(fl(fl(dX dX) + fl(dY dY)) + fl(dZ dZ)),   dX = fl(Xt - Xs), ...     float64, nothing contracted
// a source is within reach where cost <= max_chord2 (+inf without a bound), d = 2 radius asin(min(1, sqrt(cost) / 2)) and
// w = 1 / d^power.  Per plane and target: numerator sum(w z), denominator sum(w), and for the sources of cost 0 the sum of their
// values and their number; result = hit sum / hit count where there is a hit, numerator / denominator otherwise, NaN without
// a contributing source.  A NaN value leaves its source out of its plane.
//   range    (with a bound) one workgroup per 256 targets: the smallest and the largest Z among its targets, then the first and
//            the last source s that can be within the bound of a latitude in between: Z_lo <= Z_s <= Z_hi, or the same-meridian
//            chord from s to the nearer of the two, (cl - cl_s)^2 + (Z - Z_s)^2 with cl = sqrt(X X + Y Y) -- no pair of points of
//            the two latitudes is nearer --, within the bound plus IDW_BAND_MARGIN.  The margin is a thousand times every
//            rounding of either expression (values <= 4, a few ulp each, the square root among them): no source within the bound
//            is ever left out.  Sources need not be sorted by Z; where they are (the Engine sorts them) the range is a band.
//   search   one thread per target, 256 consecutive targets per workgroup; IDW_PLANES planes per launch, whose four accumulators
//            each (numerator, denominator, hit sum, hit count) stay in registers; the workgroup's sources are staged through LDS
//            IDW_CHUNK at a time, vectors and the planes' values widened to float64, and every thread walks the chunk in
//            ascending order with broadcast reads.  The geometry of a pair -- cost, asin, the weight -- is evaluated once for
//            the planes of the launch.  With fewer than IDW_FILL workgroups of targets the range of each is cut into n_split
//            equal pieces, one workgroup each (n_split from the sizes alone: idw_split), whose partial sums go to the work buffer
//   combine  (n_split > 1) one thread per target: the partial sums of every plane added in ascending piece order, then the
//            same finish as the search kernel's own.
// What bounds it: the search, and within it the weight of a pair within reach -- a float64 square root, asin (a polynomial of
// some 20 terms after its own square root for arguments above 1 / 2), one division (two with pow) and, for powers other than 1
// and 2, pow -- some 100 to 300 float64 vector instructions beside the eight of the cost and one fma and one add per plane.
// Without a bound every pair pays it; with one, a wave whose 64 targets are all out of reach of a source pays the cost and the
// compare only.  Nothing is read from memory twice: targets x sources-in-range pairs at the vector float64 rate.
// No kernel waits for another workgroup: there is no flag, no look-back, no atomic and no grid synchronisation in this file --
// what one stage needs from the stage before is handed over by the end of that launch.
#include <climits>
#include <cmath>
#include <cstdint>

#include "lcs_common.h"

namespace {

constexpr int IDW_THREADS = 256;
constexpr int IDW_CHUNK = 256;               // sources staged per round: one per thread; 6 KiB of LDS and 2 KiB per plane
constexpr int IDW_PLANES = 4;                // planes per launch: 16 float64 accumulators, 32 registers, no scratch
constexpr int IDW_FILL = 256;                // workgroups of targets from which the sources are not split (one per compute unit)
constexpr int IDW_SPLIT_MIN = 512;           // sources a piece holds at least (of the whole list: a band may be shorter)
constexpr double IDW_BAND_MARGIN = 1e-12;    // squared chord; see `range` above

// pieces the sources of a workgroup are cut into: from the sizes alone, so that a call is reproducible
int idw_split(int n_src, int n_tgt) {
    const long long blocks = ((long long)n_tgt + IDW_THREADS - 1) / IDW_THREADS;
    if (blocks >= IDW_FILL) return 1;
    const long long want = (2ll * IDW_FILL + blocks - 1) / blocks, most = (long long)n_src / IDW_SPLIT_MIN;
    const long long s = want < most ? want : most;
    return s < 1 ? 1 : (int)s;
}

struct Geom {
    const double *sx, *sy, *sz;   // [n_src]
    const double *tx, *ty, *tz;   // [n_tgt]
    const int *range;             // [blocks][2]: first source and one past the last of each workgroup of targets, or NULL: all
    int n_src, n_tgt, n_split;
    double max_chord2;            // +inf: unbounded
    double diameter;              // 2 radius
    double power;
    int pmode;                    // 2: 1 / (d d), 1: 1 / d, 0: 1 / pow(d, power)
};

template <typename T>
struct Planes {
    const T *values;    // [n_planes][n_src], at the first plane of this launch
    T *out;             // [n_planes][n_tgt], at the first plane of this launch
    double *weight;     // likewise, or NULL
    int *count;         // [n_tgt], or NULL (the first launch of a call writes it)
    double *partial;    // [n_split][n_planes][4][n_tgt], at the first plane of this launch (n_split > 1)
    int *pcount;        // [n_split][n_tgt], or NULL
    int n_planes;       // of the call
};

__device__ __forceinline__ void finish(double num, double den, double hs, double hc, double &u, double &w) {
    if (hc > 0.0) {
        u = hs / hc;
        w = INFINITY;
    } else if (den > 0.0) {
        u = num / den;
        w = den;
    } else {
        u = NAN;
        w = 0.0;
    }
}

__global__ __launch_bounds__(IDW_THREADS) void idw_range_kernel(Geom g, int *__restrict__ range, double reach2) {
#pragma clang fp contract(off)
    __shared__ double s_zlo[IDW_THREADS], s_clo[IDW_THREADS], s_zhi[IDW_THREADS], s_chi[IDW_THREADS];
    __shared__ int s_lo[IDW_THREADS], s_hi[IDW_THREADS];
    const long long p = (long long)blockIdx.x * IDW_THREADS + threadIdx.x;
    double z = NAN, cl = NAN;
    if (p < g.n_tgt) {
        const double x = g.tx[p], y = g.ty[p];
        z = g.tz[p];
        cl = __dsqrt_rn(x * x + y * y);
        if (!(cl == cl)) z = NAN;   // a target that is left out has no latitude
    }
    // +-inf where this thread has no target: every comparison below then keeps the other side
    s_zlo[threadIdx.x] = z == z ? z : INFINITY;
    s_zhi[threadIdx.x] = z == z ? z : -INFINITY;
    s_clo[threadIdx.x] = cl;
    s_chi[threadIdx.x] = cl;
    __syncthreads();
    for (int half = IDW_THREADS / 2; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half) {
            if (s_zlo[threadIdx.x + half] < s_zlo[threadIdx.x]) {
                s_zlo[threadIdx.x] = s_zlo[threadIdx.x + half];
                s_clo[threadIdx.x] = s_clo[threadIdx.x + half];
            }
            if (s_zhi[threadIdx.x + half] > s_zhi[threadIdx.x]) {
                s_zhi[threadIdx.x] = s_zhi[threadIdx.x + half];
                s_chi[threadIdx.x] = s_chi[threadIdx.x + half];
            }
        }
        __syncthreads();
    }
    const double zlo = s_zlo[0], clo = s_clo[0], zhi = s_zhi[0], chi = s_chi[0];
    int lo = INT_MAX, hi = 0;   // [lo, hi); zlo > zhi (no target at all) keeps it empty
    if (zlo <= zhi) {
        for (long long j = threadIdx.x; j < g.n_src; j += IDW_THREADS) {
            const double x = g.sx[j], y = g.sy[j], zs = g.sz[j];
            const double cs = __dsqrt_rn(x * x + y * y);
            const double dc0 = clo - cs, dz0 = zlo - zs, dc1 = chi - cs, dz1 = zhi - zs;
            const bool above = zs >= zlo || dc0 * dc0 + dz0 * dz0 <= reach2;   // a NaN is neither
            const bool below = zs <= zhi || dc1 * dc1 + dz1 * dz1 <= reach2;
            if (above && below) {
                lo = (int)j < lo ? (int)j : lo;
                hi = (int)j + 1 > hi ? (int)j + 1 : hi;
            }
        }
    }
    s_lo[threadIdx.x] = lo;
    s_hi[threadIdx.x] = hi;
    __syncthreads();
    for (int half = IDW_THREADS / 2; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half) {
            const int l = s_lo[threadIdx.x + half], h = s_hi[threadIdx.x + half];
            if (l < s_lo[threadIdx.x]) s_lo[threadIdx.x] = l;
            if (h > s_hi[threadIdx.x]) s_hi[threadIdx.x] = h;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const bool any = s_lo[0] < s_hi[0];
        range[2 * (size_t)blockIdx.x] = any ? s_lo[0] : 0;
        range[2 * (size_t)blockIdx.x + 1] = any ? s_hi[0] : 0;
    }
}

template <typename T, int NP>
__global__ __launch_bounds__(IDW_THREADS) void idw_search_kernel(Geom g, Planes<T> v) {
#pragma clang fp contract(off)
    __shared__ double s_x[IDW_CHUNK], s_y[IDW_CHUNK], s_z[IDW_CHUNK], s_v[NP][IDW_CHUNK];
    const int b = blockIdx.x / g.n_split, piece = blockIdx.x - b * g.n_split;
    const long long p = (long long)b * IDW_THREADS + threadIdx.x;
    const bool valid = p < g.n_tgt;
    // this workgroup's sources [j_lo, j_hi): uniform
    long long j_lo = 0, j_hi = g.n_src;
    if (g.range) {
        j_lo = g.range[2 * (size_t)b];
        j_hi = g.range[2 * (size_t)b + 1];   // 0 <= j_lo <= j_hi <= n_src
    }
    if (g.n_split > 1) {
        const long long each = (j_hi - j_lo + g.n_split - 1) / g.n_split;
        j_lo += (long long)piece * each;
        j_hi = j_lo + each < j_hi ? j_lo + each : j_hi;   // an empty piece has j_lo >= j_hi
    }
    double xp = NAN, yp = NAN, zp = NAN;   // a thread without a target is within reach of nothing
    if (valid) {
        xp = g.tx[p];
        yp = g.ty[p];
        zp = g.tz[p];
    }
    double num[NP], den[NP], hs[NP];
    int hc[NP], cnt = 0;
#pragma unroll
    for (int q = 0; q < NP; ++q) {
        num[q] = den[q] = hs[q] = 0.0;
        hc[q] = 0;
    }
    for (long long j0 = j_lo; j0 < j_hi; j0 += IDW_CHUNK) {
        const int n = j_hi - j0 < IDW_CHUNK ? (int)(j_hi - j0) : IDW_CHUNK;
        if ((int)threadIdx.x < n) {
            const size_t j = (size_t)j0 + threadIdx.x;   // < n_src
            s_x[threadIdx.x] = g.sx[j];
            s_y[threadIdx.x] = g.sy[j];
            s_z[threadIdx.x] = g.sz[j];
#pragma unroll
            for (int q = 0; q < NP; ++q) s_v[q][threadIdx.x] = (double)v.values[(size_t)q * (size_t)g.n_src + j];
        }
        __syncthreads();
        for (int k = 0; k < n; ++k) {
            const double dx = xp - s_x[k], dy = yp - s_y[k], dz = zp - s_z[k];
            const double cost = (dx * dx + dy * dy) + dz * dz;
            if (cost <= g.max_chord2) {   // false for a NaN
                ++cnt;                    // < 2^31 sources
                if (cost == 0.0) {
#pragma unroll
                    for (int q = 0; q < NP; ++q) {
                        const double z = s_v[q][k];
                        if (z == z) {
                            hs[q] += z;
                            ++hc[q];
                        }
                    }
                } else {
                    const double h = __dsqrt_rn(cost) / 2.0;   // the division by 2 is exact
                    const double d = g.diameter * asin(h < 1.0 ? h : 1.0);
                    const double w = g.pmode == 2 ? 1.0 / (d * d) : g.pmode == 1 ? 1.0 / d : 1.0 / pow(d, g.power);
#pragma unroll
                    for (int q = 0; q < NP; ++q) {
                        const double z = s_v[q][k];
                        if (z == z) {
                            num[q] = fma(w, z, num[q]);
                            den[q] += w;
                        }
                    }
                }
            }
        }
        __syncthreads();   // the chunk is overwritten in the next round
    }
    if (!valid) return;
    if (g.n_split > 1) {
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            double *part = v.partial + (((size_t)piece * (size_t)v.n_planes + (size_t)q) * 4) * (size_t)g.n_tgt + (size_t)p;
            part[0] = num[q];
            part[(size_t)g.n_tgt] = den[q];
            part[2 * (size_t)g.n_tgt] = hs[q];
            part[3 * (size_t)g.n_tgt] = (double)hc[q];
        }
        if (v.pcount) v.pcount[(size_t)piece * (size_t)g.n_tgt + (size_t)p] = cnt;
        return;
    }
#pragma unroll
    for (int q = 0; q < NP; ++q) {
        double u, w;
        finish(num[q], den[q], hs[q], (double)hc[q], u, w);
        v.out[(size_t)q * (size_t)g.n_tgt + (size_t)p] = (T)u;
        if (v.weight) v.weight[(size_t)q * (size_t)g.n_tgt + (size_t)p] = w;
    }
    if (v.count) v.count[p] = cnt;
}

// every plane of the call in one launch: the pieces in ascending order
template <typename T>
__global__ __launch_bounds__(IDW_THREADS) void idw_combine_kernel(const double *__restrict__ partial, const int *__restrict__ pcount,
                                                                  int n_split, int n_planes, int n_tgt, T *__restrict__ out,
                                                                  double *__restrict__ weight, int *__restrict__ count) {
    const long long p = (long long)blockIdx.x * IDW_THREADS + threadIdx.x;
    if (p >= n_tgt) return;
    for (int q = 0; q < n_planes; ++q) {
        double num = 0.0, den = 0.0, hs = 0.0, hc = 0.0;
        for (int s = 0; s < n_split; ++s) {
            const double *part = partial + (((size_t)s * (size_t)n_planes + (size_t)q) * 4) * (size_t)n_tgt + (size_t)p;
            num += part[0];
            den += part[(size_t)n_tgt];
            hs += part[2 * (size_t)n_tgt];
            hc += part[3 * (size_t)n_tgt];
        }
        double u, w;
        finish(num, den, hs, hc, u, w);
        out[(size_t)q * (size_t)n_tgt + (size_t)p] = (T)u;
        if (weight) weight[(size_t)q * (size_t)n_tgt + (size_t)p] = w;
    }
    if (count) {
        int c = 0;
        for (int s = 0; s < n_split; ++s) c += pcount[(size_t)s * (size_t)n_tgt + (size_t)p];   // the pieces are disjoint: < 2^31
        count[p] = c;
    }
}

// elements of the work buffer in float64, 0 where the sizes are bad: the ranges (two int32 per workgroup of targets) and, where
// the sources are split, four partial sums per piece, plane and target and one int32 count per piece and target
size_t work_elems(int n_src, int n_tgt, int n_planes) {
    if (n_src < 1 || n_tgt < 1 || n_planes < 1) return 0;
    const unsigned long long blocks = ((unsigned long long)n_tgt + IDW_THREADS - 1) / IDW_THREADS;
    const unsigned long long split = (unsigned long long)idw_split(n_src, n_tgt);
    unsigned long long total = blocks;
    if (split > 1) {   // n_tgt < 2^16 and split <= 2^9 here: nothing below passes 2^58
        const unsigned long long cells = split * (unsigned long long)n_tgt;
        total += cells * 4ull * (unsigned long long)n_planes + (cells + 1ull) / 2ull;
    }
    if (total > SIZE_MAX / sizeof(double)) return 0;
    return (size_t)total;
}

template <typename T>
void launch(lc_ctx *ctx, const lc_idw_args *a, const Geom &g, int blocks, double *partial, int *pcount) {
    const dim3 block(IDW_THREADS), grid((unsigned)(blocks * g.n_split));
    for (int q0 = 0; q0 < a->n_planes; q0 += IDW_PLANES) {
        const int np = a->n_planes - q0 < IDW_PLANES ? a->n_planes - q0 : IDW_PLANES;
        Planes<T> v;
        v.values = (const T *)a->values + (size_t)q0 * (size_t)a->n_src;
        v.out = (T *)a->out + (size_t)q0 * (size_t)a->n_tgt;
        v.weight = a->weight_out ? (double *)a->weight_out + (size_t)q0 * (size_t)a->n_tgt : nullptr;
        v.count = q0 == 0 ? (int *)a->count_out : nullptr;
        v.partial = partial ? partial + (size_t)q0 * 4 * (size_t)a->n_tgt : nullptr;
        v.pcount = q0 == 0 && a->count_out ? pcount : nullptr;
        v.n_planes = a->n_planes;
        switch (np) {
            case 1: hipLaunchKernelGGL((idw_search_kernel<T, 1>), grid, block, 0, ctx->stream, g, v); break;
            case 2: hipLaunchKernelGGL((idw_search_kernel<T, 2>), grid, block, 0, ctx->stream, g, v); break;
            case 3: hipLaunchKernelGGL((idw_search_kernel<T, 3>), grid, block, 0, ctx->stream, g, v); break;
            default: hipLaunchKernelGGL((idw_search_kernel<T, 4>), grid, block, 0, ctx->stream, g, v); break;
        }
    }
    if (g.n_split > 1)
        hipLaunchKernelGGL(idw_combine_kernel<T>, dim3((unsigned)blocks), block, 0, ctx->stream, (const double *)partial,
                           (const int *)pcount, g.n_split, a->n_planes, a->n_tgt, (T *)a->out, (double *)a->weight_out,
                           (int *)a->count_out);
}

}  // namespace

extern "C" size_t lc_idw_work_elems(int n_src, int n_tgt, int n_planes) { return work_elems(n_src, n_tgt, n_planes); }

extern "C" const char *lc_ctx_last_idw_kernel(const lc_ctx *ctx) { return ctx ? ctx->last_idw_kernel : ""; }

extern "C" int lc_idw_interp(lc_ctx *ctx, const lc_idw_args *a) {
    const char *who = "lc_idw_interp";
    LC_REQUIRE(ctx, "%s: null context", who);
    LC_REQUIRE(a, "%s: null argument structure", who);
    LC_REQUIRE(a->struct_size == sizeof(lc_idw_args), "%s: struct_size %zu, this library has %zu", who, (size_t)a->struct_size,
               sizeof(lc_idw_args));
    LC_REQUIRE(a->dtype == LC_F32 || a->dtype == LC_F64, "%s: bad dtype %d (LC_F32 or LC_F64)", who, a->dtype);
    LC_REQUIRE(a->n_src >= 1 && a->n_tgt >= 1 && a->n_planes >= 1, "%s: bad size n_src=%d n_tgt=%d n_planes=%d (each >= 1)", who,
               a->n_src, a->n_tgt, a->n_planes);
    LC_REQUIRE(work_elems(a->n_src, a->n_tgt, a->n_planes) != 0, "%s: too large: %d planes of %d sources and %d targets", who,
               a->n_planes, a->n_src, a->n_tgt);
    LC_REQUIRE(a->power > 0.0 && a->power <= 16.0, "%s: bad power %g: in (0, 16]", who, a->power);
    LC_REQUIRE(a->radius > 0.0 && std::isfinite(a->radius), "%s: bad radius %g: > 0 and finite", who, a->radius);
    LC_REQUIRE(a->max_chord2 == a->max_chord2, "%s: bad max_chord2: NaN (<= 0 means unbounded)", who);
    const bool bounded = a->max_chord2 > 0.0;
    LC_REQUIRE(!bounded || (a->max_distance > 0.0 && a->max_distance == a->max_distance),
               "%s: bad max_distance %g beside max_chord2 %g: > 0 where there is a bound", who, a->max_distance, a->max_chord2);
    LC_REQUIRE(a->src_x && a->src_y && a->src_z && a->values && a->tgt_x && a->tgt_y && a->tgt_z && a->out && a->work_dev,
               "%s: null pointer", who);
    LC_HIP_CHECK(hipSetDevice(ctx->device));

    const int blocks = (int)(((long long)a->n_tgt + IDW_THREADS - 1) / IDW_THREADS);   // <= 2^23
    int *range = (int *)a->work_dev;
    double *partial = (double *)a->work_dev + blocks;
    Geom g;
    g.sx = a->src_x;
    g.sy = a->src_y;
    g.sz = a->src_z;
    g.tx = a->tgt_x;
    g.ty = a->tgt_y;
    g.tz = a->tgt_z;
    g.range = bounded ? range : nullptr;
    g.n_src = a->n_src;
    g.n_tgt = a->n_tgt;
    g.n_split = idw_split(a->n_src, a->n_tgt);   // blocks * n_split < 2^10 where n_split > 1
    g.max_chord2 = bounded ? a->max_chord2 : INFINITY;
    g.diameter = 2.0 * a->radius;
    g.power = a->power;
    g.pmode = a->power == 2.0 ? 2 : a->power == 1.0 ? 1 : 0;
    const bool split = g.n_split > 1;
    int *pcount = split ? (int *)(partial + (size_t)g.n_split * (size_t)a->n_planes * 4 * (size_t)a->n_tgt) : nullptr;
    if (bounded)
        hipLaunchKernelGGL(idw_range_kernel, dim3((unsigned)blocks), dim3(IDW_THREADS), 0, ctx->stream, g, range,
                           a->max_chord2 + IDW_BAND_MARGIN);
    if (a->dtype == LC_F32)
        launch<float>(ctx, a, g, blocks, split ? partial : nullptr, split ? pcount : nullptr);
    else
        launch<double>(ctx, a, g, blocks, split ? partial : nullptr, split ? pcount : nullptr);
    LC_HIP_CHECK(hipGetLastError());
    ctx->last_idw_kernel = bounded ? (split ? "idw_range_kernel+idw_search_kernel+idw_combine_kernel" : "idw_range_kernel+idw_search_kernel")
                                   : (split ? "idw_search_kernel+idw_combine_kernel" : "idw_search_kernel");
    return LC_OK;
}
