// Great-circle distance to the nearest ridge pixel: the device side of tools.distance_to_ridges(metric='sphere').  Nothing in
// the reference computes it: it is the metric the index-unit transform of distance.hip (LCS/area_of_influence.py:231) cannot
// give on a latitude-longitude grid.  Pinned bit for bit against a numpy oracle in tests/test_sphere_distance_gpu.py.
//
// The metric is not a sum of a row term and a column term, so nothing of distance.hip's separable transform carries over: this
// is an all-pairs search, every query pixel against the compacted list of its plane's foreground pixels, n_members planes per
// launch.  The host hands over cos / sin of every latitude and longitude (numpy's); no kernel evaluates a trigonometric function
// of a coordinate.  Node (r, c) is the unit vector X = fl(cl[r] cx[c]), Y = fl(cl[r] sx[c]), Z = sl[r], and the cost of a pair is
// the squared chord
//     cost = fl(fl(fl(dX dX) + fl(dY dY)) + fl(dZ dZ)),   dX = fl(Xp - Xq), ...     float64, nothing contracted
// of which a pixel keeps the smallest and, among equal costs, the smallest linear index; dist = 2 radius asin(min(1, sqrt(cost) / 2)).
//   count    one workgroup per (plane, row): the row's foreground pixels                          -> row_start[r]
//   scan     one workgroup per plane: the exclusive sum of those counts, in place                 -> row_start[ny + 1]
//   scatter  one workgroup per (plane, row): the row's foreground pixels in ascending column order, their (X, Y, Z) and linear
//            index, at row_start[r] ...: the list is in ascending linear index and a band of rows is one contiguous range of it
//   band     (with a bound) one workgroup per row r: the first and last row q whose same-meridian chord to r,
//            (cl[r] - cl[q])^2 + (sl[r] - sl[q])^2 -- no pair of pixels of the two rows is nearer --, is within the bound plus
//            SD_BAND_MARGIN.  That is |dphi| radius <= max_distance in chord form; the margin is a thousand times every rounding
//            of either expression (values <= 4, a few ulp each), so no pair within the bound is ever left out.  Latitudes need
//            not be monotone: the band is then the smallest range of rows that holds every row within the bound.
//   search   one thread per query pixel, 256 consecutive pixels per workgroup.  The workgroup's band is the union of its rows'
//            bands; its candidates are staged through LDS SD_CHUNK at a time and every thread walks the chunk in ascending
//            order with broadcast reads, keeping (best cost, its position) under a strict <: the smallest index wins a tie by
//            construction.  With a bound a pixel keeps its result where best <= max_chord2.
// What bounds it: the search.  A pair is eight float64 operations (three differences, three products, two sums; no fma, by
// definition) plus the compare and two selects; pixels x candidates-in-band pairs at the vector float64 rate.  The other four
// kernels read the plane once each or less.
// No kernel waits for another workgroup: there is no flag, no look-back, no atomic and no grid synchronisation in this file --
// what one stage needs from the stage before is handed over by the end of that launch.
#include <climits>
#include <cmath>
#include <cstdint>

#include "lcs_common.h"

namespace {

constexpr int SD_THREADS = 256;
constexpr int SD_WAVES = SD_THREADS / 64;
constexpr int SD_CHUNK = 256;                 // candidates staged per round: one per thread, 6 KiB of LDS
constexpr double SD_BAND_MARGIN = 1e-12;      // squared chord; see `band` above

template <typename T>
__device__ __forceinline__ bool foreground(T v) {
    return v != (T)0 && v == v;   // as distance.hip: NaN is background, a negative value is foreground
}

// the parts of the work buffer; every list of a plane has room for all of its pixels
struct List {
    double *x, *y, *z;   // [n_members][ny * nx]: unit vectors of the foreground pixels, ascending linear index
    int *index;          // [n_members][ny * nx]: their linear indices
    int *row_start;      // [n_members][ny + 1]
    int *band;           // [ny][2]: first and last row within the bound of row r (written and read with a bound only)
    int ny, nx;
};

// foreground pixels of this wave's 64 columns in front of this lane, and in all of them
__device__ __forceinline__ int wave_rank(bool fg, int &total) {
    const unsigned long long votes = __ballot(fg);
    total = __popcll(votes);
    return __popcll(votes & ((1ull << (threadIdx.x & 63)) - 1ull));
}

template <typename T>
__global__ __launch_bounds__(SD_THREADS) void sd_count_kernel(const T *__restrict__ mask, List g) {
    __shared__ int s_wave[SD_WAVES];
    const size_t row = blockIdx.x;   // plane * ny + r
    const T *src = mask + row * (size_t)g.nx;
    int mine = 0;                    // of this wave, the same in all its lanes
    for (int c0 = 0; c0 < g.nx; c0 += SD_THREADS) {
        const long long c = (long long)c0 + threadIdx.x;   // may pass 2^31 in the last round of a plane of one long row
        int total;
        wave_rank(c < g.nx && foreground(src[c < g.nx ? c : 0]), total);
        mine += total;
        if (g.nx - c0 <= SD_THREADS) break;   // c0 + SD_THREADS may not be an int
    }
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int m = (int)(row / (size_t)g.ny), r = (int)(row - (size_t)m * g.ny);
        int sum = 0;
        for (int w = 0; w < SD_WAVES; ++w) sum += s_wave[w];
        g.row_start[(size_t)m * ((size_t)g.ny + 1) + r] = sum;
    }
}

// one workgroup per plane; thread t owns the rows [t seg, (t + 1) seg)
__global__ __launch_bounds__(SD_THREADS) void sd_scan_kernel(List g) {
    __shared__ int s_part[SD_THREADS];
    int *rs = g.row_start + (size_t)blockIdx.x * ((size_t)g.ny + 1);
    const long long seg = ((long long)g.ny + SD_THREADS - 1) / SD_THREADS;
    const long long r0 = (long long)threadIdx.x * seg, r1 = r0 + seg < g.ny ? r0 + seg : g.ny;
    int sum = 0;
    for (long long r = r0; r < r1; ++r) sum += rs[r];   // a plane holds < 2^31 pixels: no sum overflows
    s_part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int t = 0; t < SD_THREADS; ++t) {
            const int v = s_part[t];
            s_part[t] = run;
            run += v;
        }
        rs[g.ny] = run;
    }
    __syncthreads();
    int run = s_part[threadIdx.x];
    for (long long r = r0; r < r1; ++r) {
        const int v = rs[r];
        rs[r] = run;
        run += v;
    }
}

template <typename T>
__global__ __launch_bounds__(SD_THREADS) void sd_scatter_kernel(const T *__restrict__ mask, List g, const double *__restrict__ cl,
                                                                const double *__restrict__ sl, const double *__restrict__ cx,
                                                                const double *__restrict__ sx) {
#pragma clang fp contract(off)
    __shared__ int s_wave[SD_WAVES];
    const size_t row = blockIdx.x;   // plane * ny + r
    const int m = (int)(row / (size_t)g.ny), r = (int)(row - (size_t)m * g.ny);
    const T *src = mask + row * (size_t)g.nx;
    const size_t list = (size_t)m * (size_t)g.ny * (size_t)g.nx;
    int at = g.row_start[(size_t)m * ((size_t)g.ny + 1) + r];   // where the next round's first pixel goes
    const double clr = cl[r], slr = sl[r];
    for (int c0 = 0; c0 < g.nx; c0 += SD_THREADS) {
        const long long c = (long long)c0 + threadIdx.x;
        const bool fg = c < g.nx && foreground(src[c < g.nx ? c : 0]);
        int total;
        const int rank = wave_rank(fg, total);
        if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = total;
        __syncthreads();
        int before = 0, all = 0;
        for (int w = 0; w < SD_WAVES; ++w) {
            const int t = s_wave[w];
            if (w < (int)(threadIdx.x >> 6)) before += t;
            all += t;
        }
        if (fg) {   // at + before + rank < row_start[r + 1] <= ny nx: inside the plane's list
            const size_t j = list + (size_t)(at + before + rank);
            g.x[j] = clr * cx[c];
            g.y[j] = clr * sx[c];
            g.z[j] = slr;
            g.index[j] = (int)((long long)r * g.nx + c);   // a pixel of the plane: < 2^31
        }
        at += all;
        __syncthreads();   // s_wave is written again in the next round
        if (g.nx - c0 <= SD_THREADS) break;
    }
}

__global__ __launch_bounds__(SD_THREADS) void sd_band_kernel(List g, const double *__restrict__ cl, const double *__restrict__ sl,
                                                             double reach2) {
#pragma clang fp contract(off)
    __shared__ int s_lo[SD_THREADS], s_hi[SD_THREADS];
    const int r = blockIdx.x;
    const double clr = cl[r], slr = sl[r];
    int lo = r, hi = r;   // a row is within every bound of itself
    for (int q0 = 0; q0 < g.ny; q0 += SD_THREADS) {
        const long long q = (long long)q0 + threadIdx.x;
        if (q < g.ny) {
            const double dc = clr - cl[q], ds = slr - sl[q];
            if (dc * dc + ds * ds <= reach2) {
                lo = (int)q < lo ? (int)q : lo;
                hi = (int)q > hi ? (int)q : hi;
            }
        }
        if (g.ny - q0 <= SD_THREADS) break;   // q0 + SD_THREADS may not be an int
    }
    s_lo[threadIdx.x] = lo;
    s_hi[threadIdx.x] = hi;
    __syncthreads();
    for (int half = SD_THREADS / 2; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half) {
            const int l = s_lo[threadIdx.x + half], h = s_hi[threadIdx.x + half];
            if (l < s_lo[threadIdx.x]) s_lo[threadIdx.x] = l;
            if (h > s_hi[threadIdx.x]) s_hi[threadIdx.x] = h;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        g.band[2 * (size_t)r] = s_lo[0];
        g.band[2 * (size_t)r + 1] = s_hi[0];
    }
}

struct Search {
    double *dist, *cost;   // or NULL
    int *nearest;          // or NULL
    double diameter;       // 2 radius
    double max_chord2;     // <= 0: unbounded
    int blocks_per_plane;
};

__global__ __launch_bounds__(SD_THREADS) void sd_search_kernel(List g, Search a, const double *__restrict__ cl, const double *__restrict__ sl,
                                                               const double *__restrict__ cx, const double *__restrict__ sx) {
#pragma clang fp contract(off)
    __shared__ double s_x[SD_CHUNK], s_y[SD_CHUNK], s_z[SD_CHUNK];
    const int m = blockIdx.x / a.blocks_per_plane, b = blockIdx.x - m * a.blocks_per_plane;
    const long long npix = (long long)g.ny * g.nx;
    const long long p0 = (long long)b * SD_THREADS, p = p0 + threadIdx.x;   // p0 < npix
    const bool valid = p < npix;
    const long long plast = p0 + SD_THREADS - 1 < npix ? p0 + SD_THREADS - 1 : npix - 1;
    // the union of the bands of this workgroup's rows: uniform
    const int r_lo = (int)(p0 / g.nx), r_hi = (int)(plast / g.nx);
    int q_lo = 0, q_hi = g.ny - 1;
    if (a.max_chord2 > 0.0) {
        q_lo = INT_MAX;
        q_hi = -1;
        for (int r = r_lo; r <= r_hi; ++r) {   // at most SD_THREADS rows
            const int lo = g.band[2 * (size_t)r], hi = g.band[2 * (size_t)r + 1];
            q_lo = lo < q_lo ? lo : q_lo;
            q_hi = hi > q_hi ? hi : q_hi;
        }
    }
    const int *rs = g.row_start + (size_t)m * ((size_t)g.ny + 1);
    const int j_lo = rs[q_lo], j_hi = rs[q_hi + 1];   // 0 <= q_lo <= q_hi <= ny - 1
    const size_t list = (size_t)m * (size_t)npix;
    const double *__restrict__ lx = g.x + list, *__restrict__ ly = g.y + list, *__restrict__ lz = g.z + list;

    double xp = 0.0, yp = 0.0, zp = 0.0;
    if (valid) {
        const int r = (int)(p / g.nx), c = (int)(p - (long long)r * g.nx);
        const double clr = cl[r];
        xp = clr * cx[c];
        yp = clr * sx[c];
        zp = sl[r];
    }
    double best = INFINITY;
    int bj = -1;
    for (int j0 = j_lo; j0 < j_hi; j0 += SD_CHUNK) {   // j_hi <= npix < 2^31 and the last j0 is below it: no overflow
        const int n = j_hi - j0 < SD_CHUNK ? j_hi - j0 : SD_CHUNK;
        if ((int)threadIdx.x < n) {
            s_x[threadIdx.x] = lx[j0 + (int)threadIdx.x];
            s_y[threadIdx.x] = ly[j0 + (int)threadIdx.x];
            s_z[threadIdx.x] = lz[j0 + (int)threadIdx.x];
        }
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < n; ++k) {
            const double dx = xp - s_x[k], dy = yp - s_y[k], dz = zp - s_z[k];
            const double cost = (dx * dx + dy * dy) + dz * dz;
            if (cost < best) {   // ascending index and a strict <: the first of equal costs stays
                best = cost;
                bj = j0 + k;
            }
        }
        __syncthreads();   // the chunk is overwritten in the next round
        if (j_hi - j0 <= SD_CHUNK) break;
    }
    if (!valid) return;
    if (a.max_chord2 > 0.0 && !(best <= a.max_chord2)) {
        best = INFINITY;
        bj = -1;
    }
    const size_t o = list + (size_t)p;
    if (a.cost) a.cost[o] = best;
    if (a.nearest) a.nearest[o] = bj < 0 ? -1 : g.index[list + (size_t)bj];
    if (a.dist) {
        double d = INFINITY;
        if (bj >= 0) {
            const double h = __dsqrt_rn(best) / 2.0;   // the division by 2 is exact
            d = a.diameter * asin(h < 1.0 ? h : 1.0);
        }
        a.dist[o] = d;
    }
}

// elements of the work buffer in int32, 0 where the sizes are bad or the count does not fit a size_t
size_t work_elems(int ny, int nx, int n_members) {
    if (ny < 1 || nx < 1 || n_members < 1) return 0;
    const unsigned long long npix = (unsigned long long)ny * (unsigned long long)nx;
    if (npix >= (1ull << 31)) return 0;
    // per plane: three float64 and one int32 per pixel, and the row table; once: the band table
    const unsigned long long per_plane = 7ull * npix + (unsigned long long)ny + 1ull, once = 2ull * (unsigned long long)ny;
    if ((unsigned long long)n_members > (SIZE_MAX - once) / per_plane) return 0;
    return (size_t)(per_plane * (unsigned long long)n_members + once);
}

}  // namespace

extern "C" size_t lc_sphere_distance_work_elems(int ny, int nx, int n_members) { return work_elems(ny, nx, n_members); }

extern "C" int lc_sphere_distance(lc_ctx *ctx, const lc_sphere_distance_args *a) {
    const char *who = "lc_sphere_distance";
    LC_REQUIRE(ctx, "%s: null context", who);
    LC_REQUIRE(a, "%s: null argument structure", who);
    LC_REQUIRE(a->struct_size == sizeof(lc_sphere_distance_args), "%s: struct_size %zu, this library has %zu", who, (size_t)a->struct_size,
               sizeof(lc_sphere_distance_args));
    LC_REQUIRE(a->dtype == LC_F32 || a->dtype == LC_F64, "%s: bad dtype %d (LC_F32 or LC_F64)", who, a->dtype);
    LC_REQUIRE(a->ny >= 1 && a->nx >= 1 && a->n_members >= 1, "%s: bad size ny=%d nx=%d n_members=%d (each >= 1)", who, a->ny, a->nx,
               a->n_members);
    const long long npix = (long long)a->ny * a->nx;
    LC_REQUIRE(npix < (1ll << 31), "%s: plane too large: %d x %d = %lld pixels, nearest indices are int32 (< 2^31)", who, a->ny, a->nx,
               npix);
    const long long blocks = (npix + SD_THREADS - 1) / SD_THREADS;
    LC_REQUIRE(blocks * a->n_members <= (long long)INT_MAX && (long long)a->ny * a->n_members <= (long long)INT_MAX &&
                   work_elems(a->ny, a->nx, a->n_members) != 0,
               "%s: too many planes: %d of %d x %d", who, a->n_members, a->ny, a->nx);
    LC_REQUIRE(a->radius > 0.0 && std::isfinite(a->radius), "%s: bad radius %g: > 0 and finite", who, a->radius);
    LC_REQUIRE(a->max_chord2 == a->max_chord2, "%s: bad max_chord2: NaN (<= 0 means unbounded)", who);
    const bool bounded = a->max_chord2 > 0.0;
    LC_REQUIRE(!bounded || (a->max_distance > 0.0 && a->max_distance == a->max_distance),
               "%s: bad max_distance %g beside max_chord2 %g: > 0 where there is a bound", who, a->max_distance, a->max_chord2);
    LC_REQUIRE(a->mask && a->cos_lat && a->sin_lat && a->cos_lon && a->sin_lon && a->work_dev, "%s: null pointer", who);
    LC_REQUIRE(a->dist_out || a->nearest_out || a->cost_out, "%s: no output: dist_out, nearest_out and cost_out are all NULL", who);
    LC_HIP_CHECK(hipSetDevice(ctx->device));

    const size_t total = (size_t)a->n_members * (size_t)npix;
    List g;
    g.ny = a->ny;
    g.nx = a->nx;
    g.x = (double *)a->work_dev;
    g.y = g.x + total;
    g.z = g.y + total;
    g.index = (int *)(g.z + total);
    g.row_start = g.index + total;
    g.band = g.row_start + (size_t)a->n_members * ((size_t)a->ny + 1);
    const dim3 block(SD_THREADS), rows((unsigned)(a->ny * a->n_members));
    if (a->dtype == LC_F32) {
        hipLaunchKernelGGL(sd_count_kernel<float>, rows, block, 0, ctx->stream, (const float *)a->mask, g);
        hipLaunchKernelGGL(sd_scan_kernel, dim3((unsigned)a->n_members), block, 0, ctx->stream, g);
        hipLaunchKernelGGL(sd_scatter_kernel<float>, rows, block, 0, ctx->stream, (const float *)a->mask, g, a->cos_lat, a->sin_lat, a->cos_lon,
                           a->sin_lon);
    } else {
        hipLaunchKernelGGL(sd_count_kernel<double>, rows, block, 0, ctx->stream, (const double *)a->mask, g);
        hipLaunchKernelGGL(sd_scan_kernel, dim3((unsigned)a->n_members), block, 0, ctx->stream, g);
        hipLaunchKernelGGL(sd_scatter_kernel<double>, rows, block, 0, ctx->stream, (const double *)a->mask, g, a->cos_lat, a->sin_lat, a->cos_lon,
                           a->sin_lon);
    }
    if (bounded)
        hipLaunchKernelGGL(sd_band_kernel, dim3((unsigned)a->ny), block, 0, ctx->stream, g, a->cos_lat, a->sin_lat,
                           a->max_chord2 + SD_BAND_MARGIN);
    Search s;
    s.dist = (double *)a->dist_out;
    s.cost = (double *)a->cost_out;
    s.nearest = (int *)a->nearest_out;
    s.diameter = 2.0 * a->radius;
    s.max_chord2 = bounded ? a->max_chord2 : 0.0;
    s.blocks_per_plane = (int)blocks;
    hipLaunchKernelGGL(sd_search_kernel, dim3((unsigned)(blocks * a->n_members)), block, 0, ctx->stream, g, s, a->cos_lat, a->sin_lat,
                       a->cos_lon, a->sin_lon);
    LC_HIP_CHECK(hipGetLastError());
    return LC_OK;
}
