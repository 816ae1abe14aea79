// Ridge classification of tools.find_ridges_spherical_hessian (LCS/tools.py:99-138): per grid point
// the eigen-decomposition numpy.linalg.eig (LAPACK dgeev) returns for the symmetric 2x2 Hessian, the
// reference's row-indexed "eigenvector" (tools.py:107), its dot product with the gradient, the
// eigenvalue of largest magnitude and the ridge mask.  The reference loops over points in Python.
// The per-point arithmetic is ridge_point.h's (shared with ridges_batch.hip); this file holds the kernel that applies it
// to five derivative planes and its entry point.
#include "ridge_point.h"

namespace {

__global__ void ridge_kernel(const double *__restrict__ hxx, const double *__restrict__ hxy,
                             const double *__restrict__ hyy, const double *__restrict__ gx,
                             const double *__restrict__ gy, size_t n, double tol, double *__restrict__ mask,
                             double *__restrict__ eigmin, double *__restrict__ dt_out,
                             double *__restrict__ eigvec_out) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const RidgePoint p = ridge_point(hxx[i], hxy[i], hyy[i], gx[i], gy[i], tol);
        mask[i] = p.mask;
        eigmin[i] = p.eigmin;
        if (dt_out) dt_out[i] = p.dt;
        if (eigvec_out) {
            eigvec_out[i] = p.r0;
            eigvec_out[n + i] = p.r1;
        }
    }
}

}  // namespace

extern "C" int lc_ridge_classify(lc_ctx *ctx, const void *hxx, const void *hxy, const void *hyy, const void *gx,
                                 const void *gy, size_t n, double tolerance, void *mask_out, void *eigmin_out,
                                 void *dt_out, void *eigvec_out) {
    LC_REQUIRE(ctx, "lc_ridge_classify: null context");
    LC_REQUIRE(hxx && hxy && hyy && gx && gy && mask_out && eigmin_out, "lc_ridge_classify: null pointer");
    LC_HIP_CHECK(hipSetDevice(ctx->device));
    if (n == 0) return LC_OK;
    const int blocks = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    hipLaunchKernelGGL(ridge_kernel, dim3(blocks), dim3(256), 0, ctx->stream, (const double *)hxx, (const double *)hxy,
                       (const double *)hyy, (const double *)gx, (const double *)gy, n, tolerance, (double *)mask_out,
                       (double *)eigmin_out, (double *)dt_out, (double *)eigvec_out);
    LC_HIP_CHECK(hipGetLastError());
    return LC_OK;
}
