// K3s -- both stretch factors of the flow map and its stretching direction, fused.
//
// Per seed, from the departure points of the seed grid:
//   F = [[dXdx, dXdy], [dYdx, dYdy], [dZdx, dZdy]]   the 3 x 2 Jacobian of LCS.flowmap_gradient (LCS/LCS.py:195-208),
//                                                    physically laid out (NOT the reference's 3 x 3 reshape, Q13)
//   s1 >= s2     its singular values: s1 = sqrt(lam), lam the larger eigenvalue of F^T F = [[p, r], [r, q]];
//                s2 = |col1 x col2| / s1 (the product s1 s2 is the area change; the form sqrt(lam_min) cancels)
//   (e_lon, e_lat)  the unit eigenvector of F^T F for lam in local (east, north) components at the seed: the right
//                singular vector, the direction that is stretched by s1.  Sign: e_lon > 0, or e_lon == 0 and e_lat > 0;
//                (1, 0) where F^T F is a multiple of the identity.
// The six derivatives come from flowmap_gradient.h, the code sigma.hip's tile kernels run (lon / lat -> X, Y, Z on the
// sphere, as float when fd_fp32_cast, Q11; 5-point index stencil with numba's typing, cyclic in longitude, one-sided / 2 on
// the 2 first / last rows, Q12; metric division in T), on the whole grid as the row window.  The Gram matrix and its larger
// eigenvalue are that header's too, float64 for both dtypes: float64 s1 equals lc_sigma(LC_LAYOUT_PHYSICAL) bit for bit.
// A NaN departure point gives NaN in all four outputs of every cell whose stencil touches it (Q14).
// HBM traffic: read x_dep, y_dep once (+ halo re-reads served by L2), write up to four planes once.
// Two kernels, both a 64 x 16 tile + 2-cell halo through LDS, blockIdx.y = member (plane):
//   strain_kernel_f32     float32: bounded-argument sincos, float stencil with folded weights (sigma_kernel_f32's)
//   strain_kernel<T, S>   float64: numba's typing of the stencil (S = float when fd_fp32_cast)
#include "flowmap_gradient.h"

namespace {

template <typename T>
struct StrainArgs {
    const T *x_dep, *y_dep, *seed_lat;  // [n_members][ny*nx], [n_members][ny*nx], [ny]
    int ny, nx;
    T dlat, dlon;
    T *s1, *s2, *e_lon, *e_lat;  // [n_members][ny*nx]; all but s1 may be null
};

// the arguments as plane blockIdx.y sees them
template <typename T>
__device__ __forceinline__ StrainArgs<T> strain_member(const StrainArgs<T> &A0) {
    StrainArgs<T> A = A0;
    const size_t off = (size_t)blockIdx.y * ((size_t)A.ny * A.nx);
    A.x_dep += off;
    A.y_dep += off;
    A.s1 += off;
    if (A.s2) A.s2 += off;
    if (A.e_lon) A.e_lon += off;
    if (A.e_lat) A.e_lat += off;
    return A;
}

// Eigen step, float64: a..f = dXdx, dXdy, dYdx, dYdy, dZdx, dZdy.  The Gram step sigma.hip runs (physical layout) and the
// strain step, both flowmap_gradient.h's (stretch_of: aux_gradient.hip reduces its own derivatives with the same).
template <typename T>
__device__ __forceinline__ void strain_store(const StrainArgs<T> &A, size_t o, double a_, double b_, double c_, double d_,
                                             double e_, double f_) {
    const Stretch s = stretch_of(a_, b_, c_, d_, e_, f_, A.s2 != nullptr, A.e_lon || A.e_lat);  // flowmap_gradient.h
    A.s1[o] = (T)s.s1;  // NaN in -> NaN out (Q14)
    if (A.s2) A.s2[o] = (T)s.s2;
    if (A.e_lon) A.e_lon[o] = (T)s.ex;
    if (A.e_lat) A.e_lat[o] = (T)s.ey;
}

// T: arithmetic type of positions; S: type X,Y,Z are differenced in
template <typename T, typename S>
__global__ void __launch_bounds__(SBLOCK) strain_kernel(const StrainArgs<T> A0) {
#pragma clang fp contract(off)
    __shared__ GradientTile<S> tile;
    const StrainArgs<T> A = strain_member(A0);
    int gy0, gx0;
    tile_origin(A.nx, 0, gy0, gx0);
    tile.stage(A.x_dep, A.y_dep, 0, A.ny, A.ny, A.nx, gy0, gx0);
    __syncthreads();

    const T dy = metric_dy(A.dlat);
    for_tile_cells(gy0, gx0, A.ny, A.nx, [&](int oy, int ox, int gy, int gx) {
        T d[6];
        tile.derivatives(oy, ox, gy, A.ny, metric_dx(A.seed_lat[gy], A.dlon), dy, d);
        strain_store(A, (size_t)gy * A.nx + gx, d[0], d[1], d[2], d[3], d[4], d[5]);
    });
}

// float32: sigma_kernel_f32's X, Y, Z and differences (flowmap_gradient.h's float32 arithmetic), then the float64 eigen step
// above on the six float derivatives.
__global__ void __launch_bounds__(SBLOCK) strain_kernel_f32(const StrainArgs<float> A0) {
    __shared__ GradientTileF32 tile;
    const StrainArgs<float> A = strain_member(A0);
    int gy0, gx0;
    tile_origin(A.nx, 0, gy0, gx0);
    tile.stage(A.x_dep, A.y_dep, A.seed_lat, A.dlon, 0, A.ny, A.ny, A.nx, gy0, gx0, A.ny);
    __syncthreads();

    const float inv_dy = inv_dy_f32(A.dlat);
    for_tile_cells(gy0, gx0, A.ny, A.nx, [&](int oy, int ox, int gy, int gx) {
        float d[6];
        tile.derivatives(oy, ox, gy, A.ny, inv_dy, d);
        strain_store(A, (size_t)gy * A.nx + gx, d[0], d[1], d[2], d[3], d[4], d[5]);
    });
}

template <typename T>
int strain_impl(lc_ctx *ctx, const void *x_dep, const void *y_dep, int ny, int nx, const void *seed_lat, double dlat, double dlon,
                int fd_fp32_cast, int n_members, void *s1, void *s2, void *e_lon, void *e_lat) {
    StrainArgs<T> A;
    A.x_dep = (const T *)x_dep;
    A.y_dep = (const T *)y_dep;
    A.seed_lat = (const T *)seed_lat;
    A.ny = ny;
    A.nx = nx;
    A.dlat = (T)dlat;
    A.dlon = (T)dlon;
    A.s1 = (T *)s1;
    A.s2 = (T *)s2;
    A.e_lon = (T *)e_lon;
    A.e_lat = (T *)e_lat;
    const int ntx = (nx + SW - 1) / SW, nty = (ny + SH - 1) / SH;
    const dim3 grid(ntx * nty, n_members);
    if constexpr (sizeof(T) == 4) {
        ctx->last_strain_kernel = "strain_kernel_f32";
        hipLaunchKernelGGL(strain_kernel_f32, grid, dim3(SBLOCK), 0, ctx->stream, A);
    } else if (fd_fp32_cast) {
        ctx->last_strain_kernel = "strain_kernel<double, float>";
        hipLaunchKernelGGL((strain_kernel<T, float>), grid, dim3(SBLOCK), 0, ctx->stream, A);
    } else {
        ctx->last_strain_kernel = "strain_kernel<double, double>";
        hipLaunchKernelGGL((strain_kernel<T, double>), grid, dim3(SBLOCK), 0, ctx->stream, A);
    }
    LC_HIP_CHECK(hipGetLastError());
    return LC_OK;
}

}  // namespace

extern "C" int lc_strain(lc_ctx *ctx, const void *x_dep, const void *y_dep, int dtype, int ny, int nx, const void *seed_lat_dev,
                         double dlat, double dlon, int fd_fp32_cast, int n_members, void *s1_out, void *s2_out, void *e_lon_out,
                         void *e_lat_out) {
    LC_REQUIRE(ctx, "lc_strain: null context");
    LC_REQUIRE(dtype == LC_F32 || dtype == LC_F64, "lc_strain: bad dtype %d", dtype);
    LC_REQUIRE(nx >= 5 && ny >= 5, "lc_strain: grid %dx%d too small for the 5-point stencil", ny, nx);
    LC_REQUIRE(n_members >= 1 && n_members <= 65535, "lc_strain: bad n_members %d", n_members);
    LC_REQUIRE(x_dep && y_dep && seed_lat_dev && s1_out, "lc_strain: null pointer");
    LC_HIP_CHECK(hipSetDevice(ctx->device));
    if (dtype == LC_F32)
        return strain_impl<float>(ctx, x_dep, y_dep, ny, nx, seed_lat_dev, dlat, dlon, fd_fp32_cast, n_members, s1_out, s2_out,
                                  e_lon_out, e_lat_out);
    return strain_impl<double>(ctx, x_dep, y_dep, ny, nx, seed_lat_dev, dlat, dlon, fd_fp32_cast, n_members, s1_out, s2_out,
                               e_lon_out, e_lat_out);
}

extern "C" const char *lc_ctx_last_strain_kernel(const lc_ctx *ctx) { return ctx ? ctx->last_strain_kernel : ""; }
