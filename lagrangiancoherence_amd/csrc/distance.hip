// Exact Euclidean distance to the nearest ridge pixel: the device side of tools.distance_to_ridges, the call
// LCS/area_of_influence.py:231 makes (scipy.ndimage.distance_transform_edt(~ridges_bool)); pinned bit for bit against scipy
// and a brute-force minimum in tests/test_distance_gpu.py.
//
// The transform is separable, n_members planes per launch:
//   columns  for every pixel the signed row offset dr to the nearest foreground pixel of its own column (ties between up and
//            down go to the smaller row; DT_NONE where the column holds none), int32 in the caller's work buffer.  A column is
//            cut into segments of DT_SEG rows so that a plane of few, long columns still fills the device:
//              local    one thread per (segment, column) walks down its DT_SEG rows: the offset to the last foreground pixel
//                       at or above inside the segment, and the segment's first and last foreground row
//              carry    one thread per column walks the segment summaries (ny / DT_SEG steps): every segment learns the last
//                       foreground row above it and the first below it
//              resolve  one thread per (segment, column) walks its rows upwards and settles every pixel between the two
//   rows     one workgroup per (plane, row) stages that row's dr in LDS; a thread owns pixels c, c + DT_THREADS, ... and looks
//            outward from c at offsets k = 0, 1, 2, ... on both sides for the smallest
//              cost = fl(fl(fl(dr sy)^2) + fl(fl(k sx)^2))       scipy's own expression, float64, nothing contracted
//            and, among equal costs, the smallest linear index (r + dr) nx + c'.  It stops at the first k with
//            fl(fl(k sx)^2) > best: every rounding above is monotone in |dr| and in k, so nothing further out can be cheaper
//            or as cheap.  dist = sqrt(best), correctly rounded.
// What bounds each: the columns phase is three passes over the plane (one read of the mask, two of the int32 buffer) whatever
// the mask holds; a pixel of the rows phase costs as many steps as its distance, in units of sx -- and with max_distance no
// more than max_distance / sx + 1.
// No kernel waits for another workgroup: there is no flag, no look-back, no atomic and no grid synchronisation in this file --
// what one stage needs from the stage before is handed over by the end of that launch.
#include <climits>
#include <cmath>

#include "lcs_common.h"

namespace {

constexpr int DT_THREADS = 256;
constexpr int DT_SEG = 64;            // rows of one segment of a column
constexpr int DT_NONE = INT_MIN;      // no foreground pixel in this column: |dr| <= ny - 1 < 2^31 - 1 never reaches it
constexpr int DT_MAX_NX = 16384;      // an int32 row is 64 KiB of LDS: two workgroups per CU

template <typename T>
__device__ __forceinline__ bool foreground(T v) {
    return v != (T)0 && v == v;   // as components.hip: NaN is background, a negative value is foreground
}

// what the (segment, column-tile) workgroups of the columns phase share: the geometry of a launch of
// n_members * nseg * ctiles workgroups, and the three parts of the work buffer
struct Columns {
    int ny, nx, nseg, ctiles;
    int *dr;      // [n_members][ny][nx]
    int *first;   // [n_members][nseg][nx]: local: first foreground row of the segment or -1; carry: first one BELOW the segment
    int *last;    // [n_members][nseg][nx]: local: last foreground row of the segment or -1; carry: last one ABOVE the segment
};

struct Segment {
    int c, r0, r1;       // column, rows [r0, r1)
    size_t plane, sum;   // first element of the plane in dr, of (segment, column) in first / last
    bool valid;
};
__device__ __forceinline__ Segment segment_of_block(const Columns &g) {
    const int per_plane = g.nseg * g.ctiles;
    const int m = blockIdx.x / per_plane, rest = blockIdx.x - m * per_plane;
    const int seg = rest / g.ctiles, ct = rest - seg * g.ctiles;
    Segment s;
    s.c = ct * DT_THREADS + threadIdx.x;
    s.valid = s.c < g.nx;
    s.r0 = seg * DT_SEG;                                        // < ny
    s.r1 = g.ny - s.r0 < DT_SEG ? g.ny : s.r0 + DT_SEG;         // no overflow at ny close to 2^31
    s.plane = (size_t)m * (size_t)g.ny * (size_t)g.nx;
    s.sum = ((size_t)m * g.nseg + seg) * (size_t)g.nx + (s.valid ? s.c : 0);
    return s;
}

template <typename T>
__global__ __launch_bounds__(DT_THREADS) void dt_local_kernel(const T *__restrict__ mask, Columns g) {
    const Segment s = segment_of_block(g);
    if (!s.valid) return;
    int up = -1, first = -1;
    for (int r = s.r0; r < s.r1; ++r) {
        const size_t p = s.plane + (size_t)r * g.nx + s.c;
        if (foreground(mask[p])) {
            up = r;
            if (first < 0) first = r;
        }
        g.dr[p] = up < 0 ? DT_NONE : up - r;   // 0 on foreground
    }
    g.first[s.sum] = first;
    g.last[s.sum] = up;
}

// one thread per (plane, column); in place
__global__ __launch_bounds__(DT_THREADS) void dt_carry_kernel(Columns g, int n_members) {
    const long long i = (long long)blockIdx.x * DT_THREADS + threadIdx.x;
    if (i >= (long long)n_members * g.nx) return;
    const int m = (int)(i / g.nx), c = (int)(i - (long long)m * g.nx);
    int *first = g.first + (size_t)m * g.nseg * (size_t)g.nx + c, *last = g.last + (size_t)m * g.nseg * (size_t)g.nx + c;
    int carry = -1;
    for (int s = 0; s < g.nseg; ++s) {
        const int t = last[(size_t)s * g.nx];
        last[(size_t)s * g.nx] = carry;
        if (t >= 0) carry = t;
    }
    carry = -1;
    for (int s = g.nseg - 1; s >= 0; --s) {
        const int t = first[(size_t)s * g.nx];
        first[(size_t)s * g.nx] = carry;
        if (t >= 0) carry = t;
    }
}

// reach: offsets of more rows than this become DT_NONE (a max_distance: such a pixel cannot be within it)
__global__ __launch_bounds__(DT_THREADS) void dt_resolve_kernel(Columns g, int reach) {
    const Segment s = segment_of_block(g);
    if (!s.valid) return;
    const int above = g.last[s.sum];
    int down = g.first[s.sum];   // nearest foreground row at or below, -1: none
    for (int r = s.r1 - 1; r >= s.r0; --r) {
        const size_t p = s.plane + (size_t)r * g.nx + s.c;
        const int v = g.dr[p];
        if (v == 0) {
            down = r;
            continue;
        }
        const int up = v != DT_NONE ? r + v : above;
        int d = DT_NONE;   // rows are < 2^31, so are their differences
        if (up >= 0 && (down < 0 || r - up <= down - r)) d = up - r;   // the tie goes up: the smaller row
        else if (down >= 0) d = down - r;
        if (d != DT_NONE && (d > reach || -d > reach)) d = DT_NONE;
        g.dr[p] = d;
    }
}

struct Rows {
    const int *dr;     // [n_members][ny][nx]
    double *dist;
    int *nearest;      // or NULL
    int ny, nx, cyclic;
    int kcap;          // the search looks no further than this many columns (a max_distance; INT_MAX without)
    double sy, sx, dmax;   // dmax <= 0: unbounded
};

__global__ __launch_bounds__(DT_THREADS) void dt_rows_kernel(Rows a) {
#pragma clang fp contract(off)
    extern __shared__ int s_dr[];   // the only LDS of this kernel: nx int32
    const size_t row = blockIdx.x;  // plane * ny + r
    const int r = (int)(row % (size_t)a.ny);
    const int *src = a.dr + row * (size_t)a.nx;
    for (int c = threadIdx.x; c < a.nx; c += DT_THREADS) s_dr[c] = src[c];
    __syncthreads();
    const int nx = a.nx;
    for (int c = threadIdx.x; c < nx; c += DT_THREADS) {
        double best = INFINITY;
        int bidx = -1;
        auto look = [&](int cc, double kx2) {   // 0 <= cc < nx
            const int d = s_dr[cc];
            if (d == DT_NONE) return;
            const double y = (double)d * a.sy;
            const double cost = y * y + kx2;
            const int idx = (r + d) * nx + cc;   // a pixel of the plane: < 2^31
            if (cost < best || (cost == best && idx < bidx)) {
                best = cost;
                bidx = idx;
            }
        };
        int kmax = a.cyclic ? nx / 2 : (c > nx - 1 - c ? c : nx - 1 - c);
        if (kmax > a.kcap) kmax = a.kcap;
        for (int k = 0; k <= kmax; ++k) {
            const double x = (double)k * a.sx;
            const double kx2 = x * x;
            if (kx2 > best) break;   // not >=: a pixel of this row at the same cost may still have the smaller index
            int cl = c - k, cr = c + k;
            if (a.cyclic) {          // k <= nx / 2: one wrap
                if (cl < 0) cl += nx;
                if (cr >= nx) cr -= nx;
            }
            if (cl >= 0) look(cl, kx2);
            if (k > 0 && cr < nx && cr != cl) look(cr, kx2);
        }
        double dist = __dsqrt_rn(best);   // +inf stays +inf
        if (a.dmax > 0.0 && !(dist <= a.dmax)) {
            dist = INFINITY;
            bidx = -1;
        }
        a.dist[row * (size_t)nx + c] = dist;
        if (a.nearest) a.nearest[row * (size_t)nx + c] = bidx;
    }
}

// floor(dmax / step) + 1 steps cover everything within dmax (the + 1 also covers the rounding of the quotient); INT_MAX
// when there is no bound or the bound is past every int
int steps_within(double dmax, double step) {
    if (!(dmax > 0.0)) return INT_MAX;
    const double q = dmax / step;
    return q < (double)(INT_MAX - 1) ? (int)q + 1 : INT_MAX;
}

}  // namespace

extern "C" size_t lc_distance_work_elems(int ny, int nx, int n_members) {
    if (ny < 1 || nx < 1 || n_members < 1) return 0;
    const unsigned long long nseg = ((unsigned long long)ny + DT_SEG - 1) / DT_SEG;
    return (size_t)(((unsigned long long)ny + 2 * nseg) * (unsigned long long)nx) * (size_t)n_members;
}

extern "C" int lc_distance_transform(lc_ctx *ctx, const lc_distance_args *a) {
    const char *who = "lc_distance_transform";
    LC_REQUIRE(ctx, "%s: null context", who);
    LC_REQUIRE(a, "%s: null argument structure", who);
    LC_REQUIRE(a->struct_size == sizeof(lc_distance_args), "%s: struct_size %zu, this library has %zu", who, (size_t)a->struct_size,
               sizeof(lc_distance_args));
    LC_REQUIRE(a->dtype == LC_F32 || a->dtype == LC_F64, "%s: bad dtype %d (LC_F32 or LC_F64)", who, a->dtype);
    LC_REQUIRE(a->ny >= 1 && a->nx >= 1 && a->n_members >= 1, "%s: bad size ny=%d nx=%d n_members=%d (each >= 1)", who, a->ny, a->nx,
               a->n_members);
    const long long npix = (long long)a->ny * a->nx;
    LC_REQUIRE(npix < (1ll << 31), "%s: plane too large: %d x %d = %lld pixels, nearest indices are int32 (< 2^31)", who, a->ny, a->nx,
               npix);
    if (a->nx > DT_MAX_NX) {
        lc_set_error("%s: plane too wide: nx=%d, a row of offsets is staged in LDS (nx <= %d)", who, a->nx, DT_MAX_NX);
        return LC_EUNSUPPORTED;
    }
    LC_REQUIRE(a->sampling_y > 0.0 && a->sampling_x > 0.0 && std::isfinite(a->sampling_y) && std::isfinite(a->sampling_x),
               "%s: bad sampling (%g, %g): each > 0 and finite", who, a->sampling_y, a->sampling_x);
    LC_REQUIRE(a->max_distance == a->max_distance, "%s: bad max_distance: NaN (<= 0 means unbounded)", who);
    const int nseg = (int)(((long long)a->ny + DT_SEG - 1) / DT_SEG), ctiles = (a->nx + DT_THREADS - 1) / DT_THREADS;
    LC_REQUIRE((long long)nseg * ctiles * a->n_members <= (long long)INT_MAX && (long long)a->ny * a->n_members <= (long long)INT_MAX,
               "%s: too many planes: %d of %d rows each", who, a->n_members, a->ny);
    LC_REQUIRE(a->mask && a->dist_out && a->work_dev, "%s: null pointer", who);
    LC_HIP_CHECK(hipSetDevice(ctx->device));

    Columns g;
    g.ny = a->ny;
    g.nx = a->nx;
    g.nseg = nseg;
    g.ctiles = ctiles;
    g.dr = (int *)a->work_dev;
    g.first = g.dr + (size_t)a->n_members * (size_t)npix;
    g.last = g.first + (size_t)a->n_members * (size_t)nseg * (size_t)a->nx;
    const dim3 block(DT_THREADS), grid((unsigned)(nseg * ctiles * a->n_members));
    if (a->dtype == LC_F32)
        hipLaunchKernelGGL(dt_local_kernel<float>, grid, block, 0, ctx->stream, (const float *)a->mask, g);
    else
        hipLaunchKernelGGL(dt_local_kernel<double>, grid, block, 0, ctx->stream, (const double *)a->mask, g);
    const long long columns = (long long)a->n_members * a->nx;   // its workgroups: <= ctiles * n_members, checked above
    hipLaunchKernelGGL(dt_carry_kernel, dim3((unsigned)((columns + DT_THREADS - 1) / DT_THREADS)), block, 0, ctx->stream, g, a->n_members);
    hipLaunchKernelGGL(dt_resolve_kernel, grid, block, 0, ctx->stream, g, steps_within(a->max_distance, a->sampling_y));

    Rows w;
    w.dr = g.dr;
    w.dist = (double *)a->dist_out;
    w.nearest = (int *)a->nearest_out;
    w.ny = a->ny;
    w.nx = a->nx;
    w.cyclic = a->cyclic_x ? 1 : 0;
    w.kcap = steps_within(a->max_distance, a->sampling_x);
    w.sy = a->sampling_y;
    w.sx = a->sampling_x;
    w.dmax = a->max_distance > 0.0 ? a->max_distance : 0.0;
    hipLaunchKernelGGL(dt_rows_kernel, dim3((unsigned)(a->ny * a->n_members)), block, (size_t)a->nx * sizeof(int), ctx->stream, w);
    LC_HIP_CHECK(hipGetLastError());
    return LC_OK;
}
