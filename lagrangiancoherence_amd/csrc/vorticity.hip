// Relative vorticity of a wind record on the sphere, its area-weighted domain mean per level, and the deviation from it: the
// field LCS.lavd integrates along trajectories (Haller et al. 2016), and tools.relative_vorticity on its own.
//
// The contract (include/lcs_hip.h has it in full; tests/lavd.py restates it in numpy).  k = pi / 180, the grid is uniform and
// ascending: row r lies at lat_r = lat_min + r dlat degrees (float64), dphi = k dlat, dlambda = k (lon_max - lon_min) / (nx_f - 1).
//   omega       (dv/dlambda - d(u cos phi)/dphi) / (R cos phi) in T; u cos phi is formed in T before it is differenced
//   stencils    centred in the interior, second-order one-sided (-3 f0 + 4 f1 - f2) / 2d on the first and last row and, without
//               cyclic_x, on the first and last column; with cyclic_x centred across the seam at spacing dlambda
//   pole rows   90 - |lat_r| <= 1e-6: every column holds the mean over the finite nodes of the adjacent row; weight 0 in the mean
//   NaN         a non-finite u or v in a node's stencil gives NaN there and only there
//   mean        level_mean[t] = sum w omega / sum w over the finite nodes off the pole rows, w = cos phi, in float64
//   deviation   DOMAIN subtracts level_mean[t], GIVEN the caller's values, NONE nothing; omega = (T)((double)omega - value)
//
// Shape.  One thread per node, one wavefront along longitude (a row read is one 256 / 512 B line), four rows per workgroup;
// the neighbours come straight from L2 (the stencil's reuse is in cache; LDS holds only the eight row cosines of the
// workgroup, formed in float64 by its first eight threads).  Launches:
//   vorticity_kernel<T>            omega, and one float64 partial (sum w omega, sum w) per workgroup: wavefront shuffles, then
//                                  the four wavefronts through LDS, a fixed tree
//   vorticity_finish_kernel<T>     one workgroup per level adds that level's partials in index order (staged through LDS,
//                                  one thread adds); further workgroups fill the pole rows (a fixed tree over the columns)
//   vorticity_subtract_kernel<T>   the deviation, one thread per node (not launched for LC_VORT_DEVIATION_NONE)
// No floating-point atomics anywhere: two runs give the same bits.
#include <cmath>

#include "lcs_common.h"

namespace {

constexpr int VORT_BX = 64;   // nodes of a workgroup along longitude: one wavefront
constexpr int VORT_BY = 4;    // rows of a workgroup
constexpr int VORT_COS = 8;   // row cosines a workgroup holds: rows j0 - 2 .. j0 + 5 (the one-sided stencils reach two rows back)
constexpr int VORT_FIN = 256; // threads of a finish / subtract workgroup
constexpr double VORT_POLE_TOL = 1e-6;  // degrees

template <typename T>
struct VortArgs {
    const T *u, *v;       // [nt][ny][nx]
    T *omega;             // [nt][ny][nx]
    double *partial;      // [nt][nblk][2]
    double lat_min, dlat; // degrees
    T two_dphi, two_dlam, radius;
    int nt, ny, nx, nbx, nby, cyclic, pole_first, pole_last;
};

template <typename T>
__device__ __forceinline__ bool vort_finite(T a) { return a - a == T(0); }

// the numerator of a first derivative over three samples: centred (side 0: b is not used), one-sided forward (side -1: a, b, c
// are the edge sample and the two after it) or backward (side +1: a, b, c are the edge sample and the two before it)
template <typename T>
__device__ __forceinline__ T vort_diff(int side, T a, T b, T c) {
#pragma clang fp contract(off)
    if (side == 0) return c - a;
    if (side < 0) return (T(-3) * a + T(4) * b) - c;
    return (T(3) * a - T(4) * b) + c;
}

template <typename T>
__global__ void __launch_bounds__(VORT_BX *VORT_BY) vorticity_kernel(const VortArgs<T> A) {
#pragma clang fp contract(off)
    __shared__ double s_cos[VORT_COS];
    __shared__ double s_part[VORT_BY][2];
    const int lane = threadIdx.x, w = threadIdx.y;
    const unsigned per_level = (unsigned)A.nbx * (unsigned)A.nby;
    const int t = (int)(blockIdx.x / per_level);
    const unsigned b = blockIdx.x % per_level;
    const int bx = (int)(b % (unsigned)A.nbx), by = (int)(b / (unsigned)A.nbx);
    const int ny = A.ny, nx = A.nx;
    const int j0 = by * VORT_BY;
    const int tid = w * VORT_BX + lane;
    if (tid < VORT_COS) {
        int r = j0 - 2 + tid;
        r = r < 0 ? 0 : (r > ny - 1 ? ny - 1 : r);
        const double lat = A.lat_min + (double)r * A.dlat;
        s_cos[tid] = cos((3.141592653589793 / 180.0) * lat);
    }
    __syncthreads();
    const int i = bx * VORT_BX + lane, j = j0 + w;
    const bool in = i < nx && j < ny;
    double sw = 0.0, s1 = 0.0;
    if (in) {
        const size_t plane = (size_t)ny * (size_t)nx;
        const T *u = A.u + (size_t)t * plane, *v = A.v + (size_t)t * plane;
        const bool pole = (j == 0 && A.pole_first) || (j == ny - 1 && A.pole_last);
        auto cosr = [&](int r) { return s_cos[r - j0 + 2]; };   // rows j0 - 2 .. j0 + 5 clamped into the grid
        // d(u cos phi)/dphi: rows j - 1, j + 1, or the edge row and the two next to it
        int ra, rb, rc, side_y = 0;
        if (j == 0) ra = 0, rb = 1, rc = 2, side_y = -1;
        else if (j == ny - 1) ra = ny - 1, rb = ny - 2, rc = ny - 3, side_y = 1;
        else ra = j - 1, rb = j, rc = j + 1;
        const T ua = u[(size_t)ra * nx + i], ub = side_y ? u[(size_t)rb * nx + i] : T(0), uc = u[(size_t)rc * nx + i];
        const T fa = ua * (T)cosr(ra), fb = side_y ? ub * (T)cosr(rb) : T(0), fc = uc * (T)cosr(rc);
        // dv/dlambda: columns i - 1, i + 1 (across the seam with cyclic_x), or the edge column and the two next to it
        int ca, cb, cc, side_x = 0;
        if (i == 0 && !A.cyclic) ca = 0, cb = 1, cc = 2, side_x = -1;
        else if (i == nx - 1 && !A.cyclic) ca = nx - 1, cb = nx - 2, cc = nx - 3, side_x = 1;
        else ca = i == 0 ? nx - 1 : i - 1, cb = i, cc = i == nx - 1 ? 0 : i + 1;
        const T *vr = v + (size_t)j * nx;
        const T va = vr[ca], vb = side_x ? vr[cb] : T(0), vc = vr[cc];
        const bool ok = vort_finite(ua) && vort_finite(ub) && vort_finite(uc) && vort_finite(va) && vort_finite(vb) && vort_finite(vc);
        const T dv = vort_diff(side_x, va, vb, vc) / A.two_dlam;
        const T du = vort_diff(side_y, fa, fb, fc) / A.two_dphi;
        const double cj = cosr(j);
        T om = (dv - du) / (A.radius * (T)cj);
        if (!ok || pole) om = __builtin_nan("");   // (a pole row is filled by vorticity_finish_kernel)
        A.omega[(size_t)t * plane + (size_t)j * nx + i] = om;
        if (!pole && vort_finite(om)) sw = cj * (double)om, s1 = cj;
    }
    // the workgroup's partial: a fixed tree over the wavefront, then the wavefronts in order
#pragma unroll
    for (int off = VORT_BX / 2; off >= 1; off >>= 1) {
        sw += __shfl_down(sw, off);
        s1 += __shfl_down(s1, off);
    }
    if (lane == 0) s_part[w][0] = sw, s_part[w][1] = s1;
    __syncthreads();
    if (tid == 0) {
        double a = s_part[0][0], c = s_part[0][1];
#pragma unroll
        for (int k = 1; k < VORT_BY; ++k) a += s_part[k][0], c += s_part[k][1];
        double *p = A.partial + ((size_t)t * per_level + b) * 2;
        p[0] = a, p[1] = c;
    }
}

// Workgroups [0, nt): level_mean.  Workgroups [nt, 3 nt): the first and the last row of a level, where they are pole rows.
template <typename T>
__global__ void __launch_bounds__(VORT_FIN) vorticity_finish_kernel(const double *__restrict__ partial, int per_level, int nt, int ny,
                                                                     int nx, int pole_first, int pole_last, T *__restrict__ omega,
                                                                     double *__restrict__ level_mean) {
#pragma clang fp contract(off)
    __shared__ double s_a[VORT_FIN], s_b[VORT_FIN];
    const int tid = threadIdx.x;
    if ((int)blockIdx.x < nt) {
        const int t = blockIdx.x;
        const double *p = partial + (size_t)t * (size_t)per_level * 2;
        double sw = 0.0, s1 = 0.0;   // thread 0's
        for (int base = 0; base < per_level; base += VORT_FIN) {
            const int k = base + tid;
            s_a[tid] = k < per_level ? p[2 * (size_t)k] : 0.0;
            s_b[tid] = k < per_level ? p[2 * (size_t)k + 1] : 0.0;
            __syncthreads();
            if (tid == 0) {
                const int m = per_level - base < VORT_FIN ? per_level - base : VORT_FIN;
                for (int q = 0; q < m; ++q) sw += s_a[q], s1 += s_b[q];
            }
            __syncthreads();
        }
        if (tid == 0) level_mean[t] = s1 > 0.0 ? sw / s1 : __builtin_nan("");
        return;
    }
    const int idx = (int)blockIdx.x - nt, t = idx >> 1, last = idx & 1;
    if (!(last ? pole_last : pole_first)) return;
    T *lvl = omega + (size_t)t * (size_t)ny * (size_t)nx;
    const T *src = lvl + (size_t)(last ? ny - 2 : 1) * nx;
    T *dst = lvl + (size_t)(last ? ny - 1 : 0) * nx;
    double s = 0.0, c = 0.0;
    for (int i = tid; i < nx; i += VORT_FIN) {
        const T a = src[i];
        if (vort_finite(a)) s += (double)a, c += 1.0;
    }
    s_a[tid] = s, s_b[tid] = c;
    __syncthreads();
    for (int off = VORT_FIN / 2; off >= 1; off >>= 1) {
        if (tid < off) s_a[tid] += s_a[tid + off], s_b[tid] += s_b[tid + off];
        __syncthreads();
    }
    const T m = s_b[0] > 0.0 ? (T)(s_a[0] / s_b[0]) : (T)__builtin_nan("");
    for (int i = tid; i < nx; i += VORT_FIN) dst[i] = m;
}

template <typename T>
__global__ void __launch_bounds__(VORT_FIN) vorticity_subtract_kernel(T *__restrict__ omega, const double *__restrict__ value,
                                                                       size_t plane, size_t total) {
#pragma clang fp contract(off)
    const size_t e = (size_t)blockIdx.x * VORT_FIN + threadIdx.x;
    if (e >= total) return;
    omega[e] = (T)((double)omega[e] - value[e / plane]);
}

long long vort_groups(int ny, int nx) {
    return (((long long)nx + VORT_BX - 1) / VORT_BX) * (((long long)ny + VORT_BY - 1) / VORT_BY);
}

// float64 elements of the work buffer, 0 where the sizes are bad: two per workgroup of vorticity_kernel
size_t work_elems(int nt, int ny, int nx) {
    if (nt < 1 || ny < 4 || nx < 4) return 0;
    const long long groups = vort_groups(ny, nx) * (long long)nt;
    if (groups >= ((long long)1 << 31)) return 0;
    if (((long long)nt * ny * (long long)nx + VORT_FIN - 1) / VORT_FIN >= ((long long)1 << 31)) return 0;
    return (size_t)groups * 2;
}

template <typename T>
void launch(lc_ctx *ctx, const lc_vorticity_args *a, bool pole_first, bool pole_last, double dlat) {
    const double K = 3.141592653589793 / 180.0;
    VortArgs<T> A;
    A.u = (const T *)a->u, A.v = (const T *)a->v, A.omega = (T *)a->omega;
    A.partial = (double *)a->work_dev;
    A.lat_min = a->lat_min, A.dlat = dlat;
    A.two_dphi = (T)(2.0 * (K * dlat));
    A.two_dlam = (T)(2.0 * (K * ((a->lon_max - a->lon_min) / (double)(a->nx_f - 1))));
    A.radius = (T)a->radius;
    A.nt = a->nt, A.ny = a->ny_f, A.nx = a->nx_f;
    A.nbx = (a->nx_f + VORT_BX - 1) / VORT_BX, A.nby = (a->ny_f + VORT_BY - 1) / VORT_BY;
    A.cyclic = a->cyclic_x ? 1 : 0, A.pole_first = pole_first, A.pole_last = pole_last;
    const int per_level = A.nbx * A.nby;
    hipLaunchKernelGGL(vorticity_kernel<T>, dim3((unsigned)((long long)per_level * a->nt)), dim3(VORT_BX, VORT_BY), 0, ctx->stream, A);
    hipLaunchKernelGGL(vorticity_finish_kernel<T>, dim3((unsigned)(3 * a->nt)), dim3(VORT_FIN), 0, ctx->stream,
                       (const double *)A.partial, per_level, a->nt, a->ny_f, a->nx_f, (int)pole_first, (int)pole_last, A.omega,
                       (double *)a->level_mean);
    if (a->deviation != LC_VORT_DEVIATION_NONE) {
        const size_t plane = (size_t)a->ny_f * (size_t)a->nx_f, total = plane * (size_t)a->nt;
        const double *value = a->deviation == LC_VORT_DEVIATION_GIVEN ? (const double *)a->given_dev : (const double *)a->level_mean;
        hipLaunchKernelGGL(vorticity_subtract_kernel<T>, dim3((unsigned)((total + VORT_FIN - 1) / VORT_FIN)), dim3(VORT_FIN), 0,
                           ctx->stream, A.omega, value, plane, total);
    }
}

}  // namespace

extern "C" size_t lc_vorticity_work_elems(int nt, int ny_f, int nx_f) { return work_elems(nt, ny_f, nx_f); }

extern "C" const char *lc_ctx_last_vorticity_kernel(const lc_ctx *ctx) { return ctx ? ctx->last_vorticity_kernel : ""; }

extern "C" int lc_vorticity(lc_ctx *ctx, const lc_vorticity_args *a) {
    const char *who = "lc_vorticity";
    LC_REQUIRE(ctx, "%s: null context", who);
    LC_REQUIRE(a, "%s: null argument structure", who);
    LC_REQUIRE(a->struct_size == sizeof(lc_vorticity_args), "%s: struct_size %zu, this library has %zu", who, (size_t)a->struct_size,
               sizeof(lc_vorticity_args));
    LC_REQUIRE(a->dtype == LC_F32 || a->dtype == LC_F64, "%s: bad dtype %d", who, a->dtype);
    LC_REQUIRE(a->nt >= 1 && a->ny_f >= 4 && a->nx_f >= 4, "%s: bad record %dx%dx%d (nt >= 1, ny_f >= 4, nx_f >= 4)", who, a->nt,
               a->ny_f, a->nx_f);
    LC_REQUIRE((size_t)a->ny_f * (size_t)a->nx_f < ((size_t)1 << 31), "%s: a plane of %dx%d nodes (2^31 or more)", who, a->ny_f, a->nx_f);
    LC_REQUIRE(work_elems(a->nt, a->ny_f, a->nx_f) != 0, "%s: too large: %d levels of %dx%d nodes", who, a->nt, a->ny_f, a->nx_f);
    LC_REQUIRE(std::isfinite(a->lat_min) && std::isfinite(a->lat_max) && a->lat_min >= -90.0 - VORT_POLE_TOL &&
                   a->lat_max <= 90.0 + VORT_POLE_TOL && a->lat_min < a->lat_max,
               "%s: bad latitudes %g .. %g (ascending, within -90 .. 90)", who, a->lat_min, a->lat_max);
    LC_REQUIRE(std::isfinite(a->lon_min) && std::isfinite(a->lon_max) && a->lon_min < a->lon_max, "%s: bad longitudes %g .. %g (ascending)",
               who, a->lon_min, a->lon_max);
    LC_REQUIRE(a->radius - a->radius == 0.0 && a->radius > 0.0, "%s: radius %g (positive and finite)", who, a->radius);
    LC_REQUIRE(a->deviation == LC_VORT_DEVIATION_DOMAIN || a->deviation == LC_VORT_DEVIATION_NONE ||
                   a->deviation == LC_VORT_DEVIATION_GIVEN, "%s: bad deviation mode %d", who, a->deviation);
    LC_REQUIRE(a->u && a->v && a->omega && a->level_mean && a->work_dev, "%s: null pointer", who);
    LC_REQUIRE(a->deviation != LC_VORT_DEVIATION_GIVEN || a->given_dev, "%s: LC_VORT_DEVIATION_GIVEN without given_dev", who);
    LC_HIP_CHECK(hipSetDevice(ctx->device));
    const double dlat = (a->lat_max - a->lat_min) / (double)(a->ny_f - 1);
    const bool pole_first = 90.0 - fabs(a->lat_min) <= VORT_POLE_TOL;
    const bool pole_last = 90.0 - fabs(a->lat_min + (double)(a->ny_f - 1) * dlat) <= VORT_POLE_TOL;
    const bool sub = a->deviation != LC_VORT_DEVIATION_NONE;
    if (a->dtype == LC_F32) {
        launch<float>(ctx, a, pole_first, pole_last, dlat);
        ctx->last_vorticity_kernel = sub ? "vorticity_kernel<float>+vorticity_finish_kernel<float>+vorticity_subtract_kernel<float>"
                                         : "vorticity_kernel<float>+vorticity_finish_kernel<float>";
    } else {
        launch<double>(ctx, a, pole_first, pole_last, dlat);
        ctx->last_vorticity_kernel = sub ? "vorticity_kernel<double>+vorticity_finish_kernel<double>+vorticity_subtract_kernel<double>"
                                         : "vorticity_kernel<double>+vorticity_finish_kernel<double>";
    }
    LC_HIP_CHECK(hipGetLastError());
    return LC_OK;
}
