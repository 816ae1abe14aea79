// Adaptive local threshold: the device side of tools.threshold_local / tools.above_local_threshold, the step
// LCS/area_of_influence.py:194-199 makes (skimage.filters.threshold_local(ftle, block_size=301, offset=-.8) and the comparison
// ftle > threshold).  With skimage's defaults that is scipy.ndimage.gaussian_filter(f, (block_size - 1) / 6, mode='reflect')
// minus offset: a separable Gaussian whose radius is in the hundreds (block 301: sigma 50, radius 200), where gauss_kernel's
// two modulos and two global loads per tap are the wrong tool.
//
// gauss_line_kernel<AXIS> smooths n_members planes [ny][nx] along one axis (0: latitude, 1: longitude).  A workgroup of
// TL_THREADS = 256 threads owns a run of TL_RUN = 256 outputs along the axis for a bundle of TL_LINES = 8 neighbouring lines:
//   staging  run + 2 radius samples of every line go to LDS as float64 (float32 input is widened here), the boundary rule --
//            scipy's 'reflect', or a periodic index along longitude with `cyclic` -- resolved per sample at any distance, so
//            a radius many times the plane is legal.  This is the only place with a division or a modulo.
//   taps     a thread owns 8 outputs and walks the taps once for all of them out of LDS (gauss_taps.h: gauss_taps_lds, node
//            for node the sum of gauss_taps): per tap one weight, 16 LDS reads, 8 additions and 8 multiply-adds.  At a ragged
//            edge a workgroup walks them for the 1, 2 or 4 outputs per thread that lie inside the plane.
//   tile     one image of TL_LINES * TL_PITCH = 8 * 768 float64 = 48 KiB whatever the radius (TL_PITCH = TL_RUN + 2 *
//            GAUSS_W_CAPACITY): three workgroups fit the 160 KiB of a CU, and every stride of the tap loop is a constant that
//            goes into the offset field of the LDS read.
//            AXIS 1  tile[line][sample], TL_PITCH words per line.  Thread t owns sample t of each of the 8 lines.
//            AXIS 0  tile[sample][column], 8 words per sample: the bundle is 8 columns wide, the narrow bundle that keeps a run
//                    of 256 rows at radius 256 inside the tile.  Thread t owns column t % 8 and the rows t / 8 + 32 k, k < 8.
//            Either way lane t of a workgroup reads word (constant + t): consecutive lanes, consecutive 8-byte words, which
//            the two 32-lane groups of a 64-bit LDS read take without a bank conflict.
// The last pass to run subtracts the offset (one rounding) and compares with the caller's field; an earlier pass writes the
// smoothed planes to the work buffer.  No kernel waits for another workgroup.
#include <cmath>
#include <cstdint>
#include <climits>

#include "gauss_taps.h"

namespace {

constexpr int TL_THREADS = 256;
constexpr int TL_RUN = 256;                              // outputs along the axis per workgroup
constexpr int TL_LINES = 8;                              // neighbouring lines per workgroup (AXIS 0: columns, AXIS 1: rows)
constexpr int TL_PITCH = TL_RUN + 2 * GAUSS_W_CAPACITY;  // samples of one staged line at the largest radius
constexpr int TL_OUTPUTS = TL_RUN * TL_LINES / TL_THREADS;   // per thread
constexpr double TL_SKIP_SIGMA = 1e-15;                  // scipy: an axis with sigma <= 1e-15 is not filtered
static_assert(TL_LINES * TL_PITCH * sizeof(double) <= 64 * 1024, "the tile stays within 64 KiB at every radius");
static_assert(TL_OUTPUTS == 8 && TL_LINES == 8 && TL_THREADS / TL_LINES * TL_OUTPUTS == TL_RUN, "8 outputs per thread cover the run on both axes");

struct Line {
    const void *in;       // [n_members][ny][nx]: float32 when in_f32, else float64
    const void *f;        // the caller's field, for the mask (last pass); float32 when f_f32
    double *smooth;       // not the last pass: the smoothed planes
    double *threshold;    // last pass: smooth - offset, or NULL
    unsigned char *mask;  // last pass: f > threshold, or NULL
    double offset;
    int ny, nx;
    int in_f32, f_f32, periodic, last;
    unsigned runs, bundles;   // workgroups of one plane: runs along the axis x bundles of lines
};

// where sample q of a line of n lies: inside as it is, outside by scipy's 'reflect' (d c b a | a b c d | d c b a) or
// periodically, at any distance (reflect_index in 64 bits: q is up to 2^31 + 767, the period up to 2^32)
__device__ __forceinline__ int fold_index(long long q, int n, bool periodic) {
    if (q >= 0 && q < n) return (int)q;
    if (n == 1) return 0;
    const long long period = periodic ? (long long)n : 2ll * n;
    long long i = q % period;
    if (i < 0) i += period;
    return (int)(i < n ? i : period - 1 - i);
}

__device__ __forceinline__ double load_f64(const void *p, size_t i, int f32) {
    return f32 ? (double)((const float *)p)[i] : ((const double *)p)[i];
}

// the first N of a thread's TL_OUTPUTS outputs: the taps out of the staged tile, then the store -- the smoothed value on the way
// to the next pass, or the threshold and the comparison of the last one
template <int AXIS, int N>
__device__ __forceinline__ void line_outputs(const Line &a, const GaussW &G, const double *tile, size_t plane, long long line0,
                                             long long pos0) {
    const int t = threadIdx.x, r = G.radius;
    double acc[N];
    if (AXIS == 1)
        gauss_taps_lds<N, 1, TL_PITCH>(tile + r + t, G, acc);
    else
        gauss_taps_lds<N, TL_LINES, TL_THREADS>(tile + r * TL_LINES + t, G, acc);   // 32 rows on: TL_THREADS words
#pragma unroll
    for (int k = 0; k < N; ++k) {
        long long y, x;
        if (AXIS == 1) {
            y = line0 + k;
            x = pos0 + t;
        } else {
            y = pos0 + t / TL_LINES + (TL_THREADS / TL_LINES) * k;
            x = line0 + t % TL_LINES;
        }
        if (y >= a.ny || x >= a.nx) continue;
        const size_t i = plane + (size_t)y * (size_t)a.nx + (size_t)x;
        if (!a.last) {
            a.smooth[i] = acc[k];
            continue;
        }
        const double thr = acc[k] - a.offset;
        if (a.threshold) a.threshold[i] = thr;
        if (a.mask) a.mask[i] = load_f64(a.f, i, a.f_f32) > thr ? 1 : 0;   // a NaN on either side: 0
    }
}

template <int AXIS>
__global__ __launch_bounds__(TL_THREADS) void gauss_line_kernel(const Line a, const GaussW G) {
    __shared__ double tile[TL_LINES * TL_PITCH];
    const int t = threadIdx.x, r = G.radius, span = TL_RUN + 2 * r;
    const unsigned per_plane = a.runs * a.bundles;
    const unsigned m = blockIdx.x / per_plane, rest = blockIdx.x - m * per_plane;
    const unsigned bundle = rest / a.runs, run = rest - bundle * a.runs;
    const long long line0 = (long long)bundle * TL_LINES, pos0 = (long long)run * TL_RUN;   // both inside the plane
    const size_t plane = (size_t)m * (size_t)a.ny * (size_t)a.nx;

    // a line past the plane's edge is staged as the last one: every word the taps read is a sample of the plane
    if (AXIS == 1) {
        for (int l = 0; l < TL_LINES; ++l) {
            const long long row = line0 + l < a.ny ? line0 + l : a.ny - 1;
            const size_t base = plane + (size_t)row * (size_t)a.nx;
            for (int p = t; p < span; p += TL_THREADS)
                tile[l * TL_PITCH + p] = load_f64(a.in, base + (size_t)fold_index(pos0 - r + p, a.nx, a.periodic != 0), a.in_f32);
        }
    } else {
        for (int e = t; e < span * TL_LINES; e += TL_THREADS) {
            const int p = e / TL_LINES, c = e % TL_LINES;   // (a shift and a mask)
            const long long col = line0 + c < a.nx ? line0 + c : a.nx - 1;
            tile[e] = load_f64(a.in, plane + (size_t)fold_index(pos0 - r + p, a.ny, false) * (size_t)a.nx + (size_t)col, a.in_f32);
        }
    }
    __syncthreads();

    // A ragged edge costs what it holds.  A thread whose first output lies outside the plane has none inside and leaves; the
    // others walk the taps for 1, 2, 4 or 8 outputs: as many as the workgroup's last line (AXIS 1) or last 32 rows (AXIS 0)
    // inside the plane need, the same for every thread.
    int live;
    if (AXIS == 1) {
        if (pos0 + t >= a.nx) return;
        live = a.ny - line0 < TL_LINES ? (int)(a.ny - line0) : TL_LINES;
    } else {
        if (line0 + t % TL_LINES >= a.nx || pos0 + t / TL_LINES >= a.ny) return;
        const int rows = a.ny - pos0 < TL_RUN ? (int)(a.ny - pos0) : TL_RUN, step = TL_THREADS / TL_LINES;
        live = (rows + step - 1) / step;
    }
    if (live > 4)
        line_outputs<AXIS, 8>(a, G, tile, plane, line0, pos0);
    else if (live > 2)
        line_outputs<AXIS, 4>(a, G, tile, plane, line0, pos0);
    else if (live > 1)
        line_outputs<AXIS, 2>(a, G, tile, plane, line0, pos0);
    else
        line_outputs<AXIS, 1>(a, G, tile, plane, line0, pos0);
}

struct Range {
    const char *name;
    const void *p;
    unsigned long long bytes;
};

// the weights of one axis, or the reason the call is refused; *skip: scipy does not filter this axis
int axis_weights(const char *who, const char *axis, double sigma, GaussW &G, bool *skip) {
    LC_REQUIRE(sigma == sigma, "%s: bad sigma_%s: NaN", who, axis);
    *skip = sigma <= TL_SKIP_SIGMA;
    G.radius = 0;
    G.w[0] = 1.0;   // the identity: what the one pass of a call that filters neither axis multiplies by
    if (*skip) return LC_OK;
    if (!(4.0 * sigma + 0.5 < (double)(GAUSS_W_CAPACITY + 1))) {   // as lc_gaussian_filter; in double: any sigma, inf too
        lc_set_error("%s: sigma_%s %g needs radius %.0f > %d", who, axis, sigma, floor(4.0 * sigma + 0.5), GAUSS_W_CAPACITY);
        return LC_EUNSUPPORTED;
    }
    G.radius = gauss_radius(sigma);
    gauss_fill_weights(G, sigma);
    return LC_OK;
}

}  // namespace

extern "C" size_t lc_local_threshold_work_elems(int ny, int nx, int n_members) {
    if (ny < 1 || nx < 1 || n_members < 1) return 0;
    return (size_t)ny * (size_t)nx * (size_t)n_members;   // the planes between the two passes
}

extern "C" const char *lc_ctx_last_threshold_kernel(const lc_ctx *ctx) { return ctx ? ctx->last_threshold_kernel : ""; }

extern "C" int lc_local_threshold(lc_ctx *ctx, const lc_local_threshold_args *a) {
    const char *who = "lc_local_threshold";
    LC_REQUIRE(ctx, "%s: null context", who);
    LC_REQUIRE(a, "%s: null argument structure", who);
    LC_REQUIRE(a->struct_size == sizeof(lc_local_threshold_args), "%s: struct_size %zu, this library has %zu", who,
               (size_t)a->struct_size, sizeof(lc_local_threshold_args));
    LC_REQUIRE(a->dtype == LC_F32 || a->dtype == LC_F64, "%s: bad dtype %d (LC_F32 or LC_F64)", who, a->dtype);
    LC_REQUIRE(a->ny >= 1 && a->nx >= 1 && a->n_members >= 1, "%s: bad size ny=%d nx=%d n_members=%d (each >= 1)", who, a->ny, a->nx,
               a->n_members);
    const long long npix = (long long)a->ny * a->nx;
    LC_REQUIRE(npix < (1ll << 31), "%s: plane too large: %d x %d = %lld points (< 2^31)", who, a->ny, a->nx, npix);
    LC_REQUIRE(std::isfinite(a->offset), "%s: bad offset %g: finite", who, a->offset);
    GaussW Gy, Gx;
    bool skip_y, skip_x;
    if (int st = axis_weights(who, "y", a->sigma_y, Gy, &skip_y)) return st;
    if (int st = axis_weights(who, "x", a->sigma_x, Gx, &skip_x)) return st;
    LC_REQUIRE(a->threshold_out || a->mask_out, "%s: nothing to compute: threshold_out and mask_out are both NULL", who);
    const bool two = !skip_y && !skip_x;
    LC_REQUIRE(a->f, "%s: null pointer (f)", who);
    LC_REQUIRE(!two || a->work, "%s: both axes are filtered: work must hold lc_local_threshold_work_elems float64", who);
    const unsigned long long points = (unsigned long long)npix * (unsigned long long)a->n_members;
    const Range ranges[] = {{"f", a->f, points * (a->dtype == LC_F32 ? 4 : 8)},
                            {"work", two ? a->work : nullptr, points * 8},
                            {"threshold_out", a->threshold_out, points * 8},
                            {"mask_out", a->mask_out, points}};
    constexpr int n_ranges = (int)(sizeof(ranges) / sizeof(ranges[0]));
    for (int i = 0; i < n_ranges; ++i)
        for (int j = i + 1; j < n_ranges; ++j) {
            if (!ranges[i].p || !ranges[j].p) continue;
            const uintptr_t pi = (uintptr_t)ranges[i].p, pj = (uintptr_t)ranges[j].p;
            LC_REQUIRE(pi + ranges[i].bytes <= pj || pj + ranges[j].bytes <= pi, "%s: %s and %s overlap", who, ranges[i].name,
                       ranges[j].name);
        }
    // workgroups of one plane: pass along y, pass along x
    const long long runs_y = ((long long)a->ny + TL_RUN - 1) / TL_RUN, bundles_y = ((long long)a->nx + TL_LINES - 1) / TL_LINES;
    const long long runs_x = ((long long)a->nx + TL_RUN - 1) / TL_RUN, bundles_x = ((long long)a->ny + TL_LINES - 1) / TL_LINES;
    LC_REQUIRE(runs_y * bundles_y * a->n_members <= (long long)INT_MAX && runs_x * bundles_x * a->n_members <= (long long)INT_MAX,
               "%s: too many planes: %d of %d x %d", who, a->n_members, a->ny, a->nx);
    LC_HIP_CHECK(hipSetDevice(ctx->device));

    Line l = {};
    l.f = a->f;
    l.f_f32 = a->dtype == LC_F32;
    l.threshold = (double *)a->threshold_out;
    l.mask = (unsigned char *)a->mask_out;
    l.offset = a->offset;
    l.ny = a->ny;
    l.nx = a->nx;
    l.in = a->f;
    l.in_f32 = l.f_f32;
    const dim3 block(TL_THREADS);
    if (!skip_y) {
        l.runs = (unsigned)runs_y;
        l.bundles = (unsigned)bundles_y;
        l.last = !two;
        l.smooth = (double *)a->work;
        l.periodic = 0;
        hipLaunchKernelGGL(gauss_line_kernel<0>, dim3((unsigned)(runs_y * bundles_y * a->n_members)), block, 0, ctx->stream, l, Gy);
        l.in = a->work;
        l.in_f32 = 0;
    }
    if (!skip_x || skip_y) {   // neither axis filtered: one pass along x with the identity's single weight
        l.runs = (unsigned)runs_x;
        l.bundles = (unsigned)bundles_x;
        l.last = 1;
        l.smooth = nullptr;
        l.periodic = a->cyclic ? 1 : 0;
        hipLaunchKernelGGL(gauss_line_kernel<1>, dim3((unsigned)(runs_x * bundles_x * a->n_members)), block, 0, ctx->stream, l, Gx);
    }
    ctx->last_threshold_kernel = two ? "gauss_line_kernel<0>+gauss_line_kernel<1>" : !skip_y ? "gauss_line_kernel<0>" : "gauss_line_kernel<1>";
    LC_HIP_CHECK(hipGetLastError());
    return LC_OK;
}
