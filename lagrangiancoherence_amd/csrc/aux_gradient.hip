// K3a -- the flow-map gradient from an auxiliary grid (Haller's four offset parcels per output point), reduced to sigma, both
// stretch factors and the stretching direction in one pass.
//
// Per output cell (row r, column c) the caller has advected four parcels seeded at (lat[r], lon[c] +- d_lon) and
// (lat[r] +- d_lat, lon[c]); their departure points are the eight planes x_e, y_e, x_w, y_w, x_n, y_n, x_s, y_s.  The chord
// vectors P_e - P_w and P_n - P_s on the reference's sphere (LCS/LCS.py:195-199: a = (y - 90) k, X = R sin a cos l,
// Y = R sin a sin l, Z = R cos a, k = pi / 180) are formed from half-sums and half-differences of the angles, which does not
// cancel (the difference of two X of 6e6 m that are metres apart loses every digit float32 has):
//   am = ((y+ + y-)/2 - 90) k   da = ((y+ - y-)/2) k   lm = ((x+ + x-)/2) k   dl = ((x+ - x-)/2) k
//   dX = 2R (cos am sin da cos lm cos dl - sin am cos da sin lm sin dl)
//   dY = 2R (cos am sin da sin lm cos dl + sin am cos da cos lm sin dl)
//   dZ = -2R sin am sin da
// These are exact identities for any pair of angles: a pair that straddles the +-180 seam gives the chord of the two points.
//   dXdx = dX_ew / (k sep_lon[c] R cos(k seed_lat[r]))     dXdy = dX_ns / (k sep_lat[r] R)     (Y, Z likewise)
// sep_lon / sep_lat are the separations of the shifted seed coordinates as the caller rounded them (not 2 d).  Then the Gram
// step and the strain step of flowmap_gradient.h, float64 for both dtypes, as lc_sigma / lc_strain run them.
//
// Replaces LCS.flowmap_gradient (LCS/LCS.py:171-225) + tools.derivative_spherical_coords (LCS/tools.py:248-267) for callers who
// ask for it; it differs from them on purpose: no neighbour stencil (no cyclic longitude wrap, no one-sided / 2 rows), no
// float32 rounding of X, Y, Z (Q11), and a NaN reaches one cell only.
// NaN: a NaN in any of a cell's eight inputs or in its sep_lat / sep_lon gives NaN in every output of that cell and in no other;
// there is no validity branch, the arithmetic (and the division by the separation) carries it.
// One cell per thread, blockIdx.y = member (plane); no LDS, no neighbour reads.  HBM traffic per cell: eight reads, one to
// five writes of the dtype (float32: 32 B in, 4-20 B out); the three coordinate vectors are served by the caches.
//   aux_gradient_kernel_f32      float32: bounded-argument sincos for the means, a relative-accuracy small-argument path for
//                                the half-differences
//   aux_gradient_kernel<double>  float64: library sincos, no contraction, the operation order of the numpy restatement
//                                (tests/aux_gradient.py)
#include "flowmap_gradient.h"

namespace {

constexpr int ABLOCK = 256;

template <typename T>
struct AuxArgs {
    const T *x_e, *y_e, *x_w, *y_w, *x_n, *y_n, *x_s, *y_s;  // [n_members][ny*nx]
    const T *seed_lat, *sep_lat, *sep_lon;                   // [ny], [ny], [nx]
    int ny, nx, layout;
    T *sigma, *s1, *s2, *e_lon, *e_lat;  // [n_members][ny*nx]; each may be null
};

// sine and cosine of a mean angle (any size) and of a half-difference (small where it matters)
__device__ __forceinline__ void aux_sincos_mean(double a, double *s, double *c) { sincos(a, s, c); }
__device__ __forceinline__ void aux_sincos_half(double a, double *s, double *c) { sincos(a, s, c); }
__device__ __forceinline__ void aux_sincos_mean(float a, float *s, float *c) {
    if (fabsf(a) < 64.0f)
        bounded_sincosf(a, s, c);
    else  // out of the polynomial's range, or NaN: library path
        sincosf(a, s, c);
}
// |a| <= pi/4: the minimax polynomials of bounded_sincosf on the argument itself (no reduction: sin a = a (1 + ...) keeps its
// relative accuracy down to a = 0, which is what the chord's length rests on); larger, or NaN: the library
__device__ __forceinline__ void aux_sincos_half(float a, float *s, float *c) {
    if (fabsf(a) <= 0.785398f) {
        const float z = a * a;
        *s = fmaf(fmaf(fmaf(-1.9515295891e-4f, z, 8.3321608736e-3f), z, -1.6666654611e-1f), z * a, a);
        *c = fmaf(fmaf(fmaf(2.443315711809948e-5f, z, -1.388731625493765e-3f), z, 4.166664568298827e-2f), z * z,
                  fmaf(-0.5f, z, 1.0f));
    } else {
        sincosf(a, s, c);
    }
}

// P+ - P- of two departure points (x+, y+), (x-, y-) in degrees: (dX, dY, dZ) in metres
template <typename T>
__device__ __forceinline__ void chord(T xp, T yp, T xm, T ym, T &dX, T &dY, T &dZ) {
#pragma clang fp contract(off)
    const T K = T(3.141592653589793) / T(180);
    const T R2 = T(2) * T(6371000);
    const T am = ((yp + ym) * T(0.5) - T(90)) * K;
    const T da = ((yp - ym) * T(0.5)) * K;
    const T lm = ((xp + xm) * T(0.5)) * K;
    const T dl = ((xp - xm) * T(0.5)) * K;
    T sa, ca, sda, cda, sl, cl, sdl, cdl;
    aux_sincos_mean(am, &sa, &ca);
    aux_sincos_half(da, &sda, &cda);
    aux_sincos_mean(lm, &sl, &cl);
    aux_sincos_half(dl, &sdl, &cdl);
    const T A = ca * sda, B = sa * cda;
    dX = R2 * ((A * cl) * cdl - (B * sl) * sdl);
    dY = R2 * ((A * sl) * cdl + (B * cl) * sdl);
    dZ = -(R2 * (sa * sda));
}

template <typename T>
__device__ __forceinline__ void aux_cell(const AuxArgs<T> &A0) {
#pragma clang fp contract(off)
    const size_t cells = (size_t)A0.ny * A0.nx;
    const size_t i = (size_t)blockIdx.x * ABLOCK + threadIdx.x;
    if (i >= cells) return;
    const int r = (int)(i / (size_t)A0.nx), c = (int)(i - (size_t)r * A0.nx);
    const size_t o = (size_t)blockIdx.y * cells + i;  // blockIdx.y: the member

    T ex, ey, ez, nx_, ny_, nz_;
    chord(A0.x_e[o], A0.y_e[o], A0.x_w[o], A0.y_w[o], ex, ey, ez);
    chord(A0.x_n[o], A0.y_n[o], A0.x_s[o], A0.y_s[o], nx_, ny_, nz_);
    const T K = T(3.141592653589793) / T(180);
    const T R = T(6371000);
    T sl, cl;
    aux_sincos_mean(A0.seed_lat[r] * K, &sl, &cl);
    const T dx = ((K * A0.sep_lon[c]) * R) * cl;  // NaN separation: NaN in every derivative along it
    const T dy = (K * A0.sep_lat[r]) * R;
    const double a_ = ex / dx, b_ = nx_ / dy, c_ = ey / dx, d_ = ny_ / dy, e_ = ez / dx, f_ = nz_ / dy;  // division in T

    if (A0.sigma) A0.sigma[o] = (T)sqrt(gram_eigen(A0.layout, a_, b_, c_, d_, e_, f_).lam);
    if (A0.s1 || A0.s2 || A0.e_lon || A0.e_lat) {
        const Stretch s = stretch_of(a_, b_, c_, d_, e_, f_, A0.s2 != nullptr, A0.e_lon || A0.e_lat);
        if (A0.s1) A0.s1[o] = (T)s.s1;
        if (A0.s2) A0.s2[o] = (T)s.s2;
        if (A0.e_lon) A0.e_lon[o] = (T)s.ex;
        if (A0.e_lat) A0.e_lat[o] = (T)s.ey;
    }
}

template <typename T>
__global__ void __launch_bounds__(ABLOCK) aux_gradient_kernel(const AuxArgs<T> A) {
    aux_cell<T>(A);
}
__global__ void __launch_bounds__(ABLOCK) aux_gradient_kernel_f32(const AuxArgs<float> A) { aux_cell<float>(A); }

template <typename T>
int aux_impl(lc_ctx *ctx, const lc_aux_gradient_args *a) {
    AuxArgs<T> A;
    A.x_e = (const T *)a->x_e, A.y_e = (const T *)a->y_e, A.x_w = (const T *)a->x_w, A.y_w = (const T *)a->y_w;
    A.x_n = (const T *)a->x_n, A.y_n = (const T *)a->y_n, A.x_s = (const T *)a->x_s, A.y_s = (const T *)a->y_s;
    A.seed_lat = (const T *)a->seed_lat_dev;
    A.sep_lat = (const T *)a->sep_lat_dev;
    A.sep_lon = (const T *)a->sep_lon_dev;
    A.ny = a->ny;
    A.nx = a->nx;
    A.layout = a->tensor_layout;
    A.sigma = (T *)a->sigma_out;
    A.s1 = (T *)a->s1_out;
    A.s2 = (T *)a->s2_out;
    A.e_lon = (T *)a->e_lon_out;
    A.e_lat = (T *)a->e_lat_out;
    const size_t cells = (size_t)a->ny * a->nx;
    const dim3 grid((unsigned)((cells + ABLOCK - 1) / ABLOCK), a->n_members);
    if constexpr (sizeof(T) == 4) {
        ctx->last_aux_kernel = "aux_gradient_kernel_f32";
        hipLaunchKernelGGL(aux_gradient_kernel_f32, grid, dim3(ABLOCK), 0, ctx->stream, A);
    } else {
        ctx->last_aux_kernel = "aux_gradient_kernel<double>";
        hipLaunchKernelGGL(aux_gradient_kernel<T>, grid, dim3(ABLOCK), 0, ctx->stream, A);
    }
    LC_HIP_CHECK(hipGetLastError());
    return LC_OK;
}

}  // namespace

extern "C" int lc_aux_gradient(lc_ctx *ctx, const lc_aux_gradient_args *a) {
    const char *who = "lc_aux_gradient";
    LC_REQUIRE(ctx, "%s: null context", who);
    LC_REQUIRE(a, "%s: null argument structure", who);
    LC_REQUIRE(a->struct_size == sizeof(lc_aux_gradient_args), "%s: struct_size %zu, this library has %zu", who,
               (size_t)a->struct_size, sizeof(lc_aux_gradient_args));
    LC_REQUIRE(a->dtype == LC_F32 || a->dtype == LC_F64, "%s: bad dtype %d", who, a->dtype);
    LC_REQUIRE(a->ny >= 1 && a->nx >= 1, "%s: bad grid %dx%d", who, a->ny, a->nx);
    LC_REQUIRE((size_t)a->ny * (size_t)a->nx < ((size_t)1 << 31), "%s: a plane of %dx%d cells (2^31 or more)", who, a->ny, a->nx);
    LC_REQUIRE(a->n_members >= 1 && a->n_members <= 65535, "%s: bad n_members %d", who, a->n_members);
    LC_REQUIRE(a->tensor_layout == LC_LAYOUT_REFERENCE || a->tensor_layout == LC_LAYOUT_PHYSICAL, "%s: bad tensor_layout %d", who,
               a->tensor_layout);
    LC_REQUIRE(a->x_e && a->y_e && a->x_w && a->y_w && a->x_n && a->y_n && a->x_s && a->y_s && a->seed_lat_dev && a->sep_lat_dev &&
                   a->sep_lon_dev,
               "%s: null input pointer", who);
    LC_REQUIRE(a->sigma_out || a->s1_out || a->s2_out || a->e_lon_out || a->e_lat_out, "%s: no output requested", who);
    LC_HIP_CHECK(hipSetDevice(ctx->device));
    if (a->dtype == LC_F32) return aux_impl<float>(ctx, a);
    return aux_impl<double>(ctx, a);
}

extern "C" const char *lc_ctx_last_aux_kernel(const lc_ctx *ctx) { return ctx ? ctx->last_aux_kernel : ""; }
