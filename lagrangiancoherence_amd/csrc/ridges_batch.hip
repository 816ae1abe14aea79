// tools.find_ridges_spherical_hessian (LCS/tools.py:52-155) for a whole stack of FTLE planes in two kernels: what the
// per-plane route does in about thirty launches per plane (two Gaussian passes, five times cast / index stencil / cast /
// metric, the classification), for n_members planes [n_members][ny*nx] at once.  A plane never reads another plane.
//
//   gauss_planes_kernel   the separable Gaussian of gauss_taps.h per plane (tools.py:74-75): api.hip's gauss_kernel with a
//                         plane index, same taps in the same order, so a plane has lc_gaussian_filter's bits.
//   hessian_ridge_kernel  everything after the smoothing (tools.py:77-138).  One workgroup of RB_THREADS threads per tile of
//                         RB_TH x RB_TW output points and plane:
//                           level 0  the float32 cast of the tile + a halo of 4 in LDS (tools.py:258, the cast of D());
//                           level 1  ddadx, ddady on the tile + a halo of 2: float32 stencil (flowmap_gradient.h's centred /
//                                    one_sided, the numba typing of tools.py:204-217), widened to float64, divided by the row's
//                                    dx / scaled by 1 / dy in float64 (tools.py:260-264), cast to float32 again in LDS;
//                           level 2  d2x2 = D(ddadx, 1), d2y2 = D(ddady, 0), dxdy = D(ddadx, 0) the same way (tools.py:79-81),
//                                    then ridge_point.h's per-point step (tools.py:92-138).
//                         The edge rules follow the GLOBAL row and column of a point, never its place in the tile: one-sided
//                         differences on the two first / last rows (tools.py:210-217); in longitude the cyclic wrap when
//                         isglobal (:220-228, the halo columns are staged from the wrapped column), else one-sided on the two
//                         first / last columns (:229-244).  Halo points outside the plane hold 0 and are never read by a
//                         point inside it: the one-sided rules look inwards only.
//                         The float64 gradient a point returns is recomputed from level 0 at the point (the same operations
//                         on the same values as the level-1 entry it was rounded to float32 from).
// The tile: 16 x 64 points, 256 threads, 4 points per thread along a row of 64 (coalesced 512-byte rows of every output);
// LDS 24 x 72 + 2 x 20 x 68 floats + 20 doubles = 17,952 bytes, rows read at consecutive addresses (no bank conflict).
// What bounds it: the float64 eigen step per point (VALU), then the seven float64 output planes (56 bytes per point) against
// 8 x 1.69 bytes read.  No inline asm, no atomics, no kernel waits for another workgroup.
#include <climits>
#include <cstdint>

#include "flowmap_gradient.h"
#include "gauss_taps.h"
#include "ridge_point.h"

namespace {

constexpr int RB_THREADS = 256;
constexpr int RB_TW = 64, RB_TH = 16;                 // the tile (longitude x latitude)
constexpr int RB_H0 = 4, RB_H1 = 2;                   // halo of level 0 (the field) and of level 1 (the first derivatives)
constexpr int RB_W0 = RB_TW + 2 * RB_H0, RB_R0 = RB_TH + 2 * RB_H0;   // 72 x 24
constexpr int RB_W1 = RB_TW + 2 * RB_H1, RB_R1 = RB_TH + 2 * RB_H1;   // 68 x 20
constexpr int RB_MAX_PLANES_Y = 65535;                // gridDim.y; more planes than that are walked by a stride

template <int AXIS>
__global__ void __launch_bounds__(RB_THREADS) gauss_planes_kernel(const double *__restrict__ in, double *__restrict__ out, int ny,
                                                                  int nx, int n_members, const GaussW G) {
    const size_t total = (size_t)ny * nx;
    for (int m = blockIdx.y; m < n_members; m += gridDim.y) {
        const double *pin = in + (size_t)m * total;
        double *pout = out + (size_t)m * total;
        for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
            const int y = (int)(i / nx), x = (int)(i - (size_t)y * nx);
            pout[i] = gauss_taps<double, AXIS>(pin, y, x, ny, nx, G);
        }
    }
}

struct Hess {
    const double *f;     // [n_members][ny*nx], smoothed or not
    const double *dx;    // [ny]
    double inv_dy, tol;
    int ny, nx, n_members, isglobal;
    double *mask, *eigmin, *dt, *eigvec, *grad;   // each NULL or [n_members](x2)[ny*nx]
};

// tools.fourth_order_derivative along longitude at LDS position p (row pitch irrelevant), global column gx
__device__ __forceinline__ float stencil_x(const float *p, int gx, int nx, int isglobal) {
    if (!isglobal) {
        if (gx < 2) return one_sided(p[1], p[0]);            // tools.py:229-236
        if (gx >= nx - 2) return one_sided(p[0], p[-1]);      // tools.py:237-244
    }
    return centred(p[1], p[-1], p[2], p[-2]);                // tools.py:220-228 (the wrap is in the staging)
}
// ... and along latitude, global row gy, rows `pitch` floats apart
__device__ __forceinline__ float stencil_y(const float *p, int pitch, int gy, int ny) {
    if (gy < 2) return one_sided(p[pitch], p[0]);            // tools.py:210-213
    if (gy >= ny - 2) return one_sided(p[0], p[-pitch]);      // tools.py:214-217
    return centred(p[pitch], p[-pitch], p[2 * pitch], p[-2 * pitch]);
}
// derivative_spherical_coords' last step (tools.py:260-264) in float64
__device__ __forceinline__ double metric_x(float d, double dx) { return (double)d / dx; }
__device__ __forceinline__ double metric_y(float d, double inv_dy) { return (double)d * inv_dy; }

__global__ void __launch_bounds__(RB_THREADS) hessian_ridge_kernel(const Hess a) {
    __shared__ float s_f[RB_R0 * RB_W0];      // level 0
    __shared__ float s_gx[RB_R1 * RB_W1];     // level 1: ddadx
    __shared__ float s_gy[RB_R1 * RB_W1];     //          ddady
    __shared__ double s_dx[RB_R1];            // dx of the level-1 rows
    const int tid = threadIdx.x;
    const int tiles_x = (a.nx + RB_TW - 1) / RB_TW;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int gy0 = ty * RB_TH, gx0 = tx * RB_TW;    // the tile's first row and column
    const size_t total = (size_t)a.ny * a.nx;

    for (int m = blockIdx.y; m < a.n_members; m += gridDim.y) {
        const double *f = a.f + (size_t)m * total;
        if (tid < RB_R1) {
            const int gy = gy0 - RB_H1 + tid;
            s_dx[tid] = (gy >= 0 && gy < a.ny) ? a.dx[gy] : 1.0;
        }
        for (int i = tid; i < RB_R0 * RB_W0; i += RB_THREADS) {
            const int r = i / RB_W0, c = i - r * RB_W0;
            const int gy = gy0 - RB_H0 + r;
            int gx = gx0 - RB_H0 + c;
            if (a.isglobal) {        // cyclic column (tools.py:225-228); grids narrower than the halo: general modulo
                gx %= a.nx;
                if (gx < 0) gx += a.nx;
            }
            float v = 0.0f;
            if (gy >= 0 && gy < a.ny && gx >= 0 && gx < a.nx) v = (float)f[(size_t)gy * a.nx + gx];   // tools.py:258
            s_f[i] = v;
        }
        __syncthreads();

        for (int i = tid; i < RB_R1 * RB_W1; i += RB_THREADS) {
            const int r = i / RB_W1, c = i - r * RB_W1;
            const int gy = gy0 - RB_H1 + r, gx = gx0 - RB_H1 + c;   // gx: unwrapped; a wrapped column has its own column's value
            float vx = 0.0f, vy = 0.0f;
            if (gy >= 0 && gy < a.ny && (a.isglobal || (gx >= 0 && gx < a.nx))) {
                const float *p = s_f + (r + RB_H0 - RB_H1) * RB_W0 + (c + RB_H0 - RB_H1);
                vx = (float)metric_x(stencil_x(p, gx, a.nx, a.isglobal), s_dx[r]);       // D(a, 1), cast again by the next D()
                vy = (float)metric_y(stencil_y(p, RB_W0, gy, a.ny), a.inv_dy);           // D(a, 0)
            }
            s_gx[i] = vx;
            s_gy[i] = vy;
        }
        __syncthreads();

        for (int i = tid; i < RB_TH * RB_TW; i += RB_THREADS) {
            const int oy = i / RB_TW, ox = i - oy * RB_TW;
            const int gy = gy0 + oy, gx = gx0 + ox;
            if (gy >= a.ny || gx >= a.nx) continue;
            const double dx = s_dx[oy + RB_H1];
            const float *p0 = s_f + (oy + RB_H0) * RB_W0 + (ox + RB_H0);
            const int q = (oy + RB_H1) * RB_W1 + (ox + RB_H1);
            const double ddadx = metric_x(stencil_x(p0, gx, a.nx, a.isglobal), dx);             // tools.py:77
            const double ddady = metric_y(stencil_y(p0, RB_W0, gy, a.ny), a.inv_dy);            // tools.py:78
            const double d2x2 = metric_x(stencil_x(s_gx + q, gx, a.nx, a.isglobal), dx);        // tools.py:79
            const double d2y2 = metric_y(stencil_y(s_gy + q, RB_W1, gy, a.ny), a.inv_dy);       // tools.py:80
            const double dxdy = metric_y(stencil_y(s_gx + q, RB_W1, gy, a.ny), a.inv_dy);       // tools.py:81
            const RidgePoint pt = ridge_point(d2x2, dxdy, d2y2, ddadx, ddady, a.tol);
            const size_t o = (size_t)gy * a.nx + gx, plane = (size_t)m * total;
            if (a.mask) a.mask[plane + o] = pt.mask;
            if (a.eigmin) a.eigmin[plane + o] = pt.eigmin;
            if (a.dt) a.dt[plane + o] = pt.dt;
            if (a.eigvec) {
                a.eigvec[2 * plane + o] = pt.r0;
                a.eigvec[2 * plane + total + o] = pt.r1;
            }
            if (a.grad) {
                a.grad[2 * plane + o] = ddadx;
                a.grad[2 * plane + total + o] = ddady;
            }
        }
        __syncthreads();   // the next plane restages the images
    }
}

struct Range {
    const char *name;
    const void *p;
    unsigned long long bytes;
};

}  // namespace

extern "C" size_t lc_ridges_work_elems(int ny, int nx, int n_members) {
    if (ny < 1 || nx < 1 || n_members < 1) return 0;
    return (size_t)2 * (size_t)ny * (size_t)nx * (size_t)n_members;   // the pass along latitude, then the smoothed planes
}

extern "C" const char *lc_ctx_last_ridges_kernel(const lc_ctx *ctx) { return ctx ? ctx->last_ridges_kernel : ""; }

extern "C" int lc_ridges_batch(lc_ctx *ctx, const lc_ridges_args *a) {
    const char *who = "lc_ridges_batch";
    LC_REQUIRE(ctx, "%s: null context", who);
    LC_REQUIRE(a, "%s: null argument structure", who);
    LC_REQUIRE(a->struct_size == sizeof(lc_ridges_args), "%s: struct_size %zu, this library has %zu", who, (size_t)a->struct_size,
               sizeof(lc_ridges_args));
    LC_REQUIRE(a->ny >= 5 && a->nx >= 5, "%s: grid %dx%d too small for the 5-point stencil", who, a->ny, a->nx);
    LC_REQUIRE(a->n_members >= 1, "%s: bad n_members %d (>= 1)", who, a->n_members);
    const long long npix = (long long)a->ny * a->nx;
    LC_REQUIRE(npix < (1ll << 31), "%s: plane too large: %d x %d = %lld points (< 2^31)", who, a->ny, a->nx, npix);
    const bool smooth = a->sigma > 0.0;   // <= 0 or NaN: no smoothing
    GaussW G;
    G.radius = 0;
    if (smooth) {
        if (!(4.0 * a->sigma + 0.5 < (double)(GAUSS_W_CAPACITY + 1))) {   // as lc_gaussian_filter; in double: any sigma, inf too
            lc_set_error("%s: sigma %g needs radius %.0f > %d", who, a->sigma, floor(4.0 * a->sigma + 0.5), GAUSS_W_CAPACITY);
            return LC_EUNSUPPORTED;
        }
        G.radius = gauss_radius(a->sigma);
    }
    LC_REQUIRE(a->dy == a->dy && a->dy != 0.0, "%s: bad dy %g", who, a->dy);
    LC_REQUIRE(a->f && a->dx_dev, "%s: null pointer (f, dx_dev)", who);
    LC_REQUIRE(!smooth || a->work_dev, "%s: sigma %g smooths: work_dev must hold lc_ridges_work_elems float64", who, a->sigma);
    const unsigned long long plane_bytes = (unsigned long long)npix * (unsigned long long)a->n_members * sizeof(double);
    const Range ranges[] = {{"f", a->f, plane_bytes},
                            {"dx_dev", a->dx_dev, (unsigned long long)a->ny * sizeof(double)},
                            {"work_dev", smooth ? a->work_dev : nullptr, 2 * plane_bytes},
                            {"mask_out", a->mask_out, plane_bytes},
                            {"eigmin_out", a->eigmin_out, plane_bytes},
                            {"dt_out", a->dt_out, plane_bytes},
                            {"eigvec_out", a->eigvec_out, 2 * plane_bytes},
                            {"grad_out", a->grad_out, 2 * plane_bytes}};
    constexpr int n_ranges = (int)(sizeof(ranges) / sizeof(ranges[0]));
    for (int i = 0; i < n_ranges; ++i)
        for (int j = i + 1; j < n_ranges; ++j) {
            if (!ranges[i].p || !ranges[j].p || (i < 2 && j < 2)) continue;   // (two inputs may share memory)
            const uintptr_t pi = (uintptr_t)ranges[i].p, pj = (uintptr_t)ranges[j].p;
            LC_REQUIRE(pi + ranges[i].bytes <= pj || pj + ranges[j].bytes <= pi, "%s: %s and %s overlap", who, ranges[i].name,
                       ranges[j].name);
        }
    LC_HIP_CHECK(hipSetDevice(ctx->device));

    const unsigned planes_y = (unsigned)(a->n_members < RB_MAX_PLANES_Y ? a->n_members : RB_MAX_PLANES_Y);
    const double *field = (const double *)a->f;
    if (smooth) {
        gauss_fill_weights(G, a->sigma);
        double *tmp = (double *)a->work_dev, *smoothed = tmp + (size_t)npix * (size_t)a->n_members;
        const unsigned blocks = (unsigned)((npix + RB_THREADS - 1) / RB_THREADS < 4096 ? (npix + RB_THREADS - 1) / RB_THREADS : 4096);
        hipLaunchKernelGGL(gauss_planes_kernel<0>, dim3(blocks, planes_y), dim3(RB_THREADS), 0, ctx->stream, field, tmp, a->ny, a->nx,
                           a->n_members, G);
        hipLaunchKernelGGL(gauss_planes_kernel<1>, dim3(blocks, planes_y), dim3(RB_THREADS), 0, ctx->stream, (const double *)tmp,
                           smoothed, a->ny, a->nx, a->n_members, G);
        field = smoothed;
    }
    Hess h;
    h.f = field;
    h.dx = (const double *)a->dx_dev;
    h.inv_dy = 1.0 / a->dy;
    h.tol = a->tolerance;
    h.ny = a->ny;
    h.nx = a->nx;
    h.n_members = a->n_members;
    h.isglobal = a->isglobal != 0;
    h.mask = (double *)a->mask_out;
    h.eigmin = (double *)a->eigmin_out;
    h.dt = (double *)a->dt_out;
    h.eigvec = (double *)a->eigvec_out;
    h.grad = (double *)a->grad_out;
    const long long tiles = (((long long)a->ny + RB_TH - 1) / RB_TH) * (((long long)a->nx + RB_TW - 1) / RB_TW);   // < 2^31 / 1024 + ...
    hipLaunchKernelGGL(hessian_ridge_kernel, dim3((unsigned)tiles, planes_y), dim3(RB_THREADS), 0, ctx->stream, h);
    ctx->last_ridges_kernel = smooth ? "gauss_planes_kernel+hessian_ridge_kernel" : "hessian_ridge_kernel";
    LC_HIP_CHECK(hipGetLastError());
    return LC_OK;
}
