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
// Geometry and stencil restate sigma.hip's (which restates LCS/LCS.py:195-199, tools.py:202-228, 254-264): lon / lat ->
// X, Y, Z on the sphere (as float when fd_fp32_cast, Q11), 5-point index stencil with numba's typing, cyclic in longitude,
// one-sided / 2 on the 2 first / last rows (Q12), metric division in T.  The Gram matrix and everything after it are
// float64 for both dtypes, in sigma.hip's operation order: float64 s1 equals lc_sigma(LC_LAYOUT_PHYSICAL) bit for bit.
// A NaN departure point gives NaN in all four outputs of every cell whose stencil touches it (Q14).
// HBM traffic: read x_dep, y_dep once (+ halo re-reads served by L2), write up to four planes once.
// Two kernels, both a 64 x 16 tile + 2-cell halo through LDS, blockIdx.y = member (plane):
//   strain_kernel_f32     float32: bounded-argument sincos, float stencil with folded weights (sigma_kernel_f32's)
//   strain_kernel<T, S>   float64: numba's typing of the stencil (S = float when fd_fp32_cast)
#include "lcs_common.h"

namespace {

constexpr int SW = 64;  // tile width  (longitude)
constexpr int SH = 16;  // tile height (latitude)
constexpr int HALO = 2;
constexpr int LW = SW + 2 * HALO;
constexpr int LH = SH + 2 * HALO;
constexpr int SBLOCK = 256;

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

// Eigen step, float64: a..f = dXdx, dXdy, dYdx, dYdy, dZdx, dZdy.  p, q, r, disc, lam: the operations of sigma.hip's
// physical layout in its order.
template <typename T>
__device__ __forceinline__ void strain_store(const StrainArgs<T> &A, size_t o, double a_, double b_, double c_, double d_,
                                             double e_, double f_) {
#pragma clang fp contract(off)
    const double p = a_ * a_ + c_ * c_ + e_ * e_;
    const double q = b_ * b_ + d_ * d_ + f_ * f_;
    const double r = a_ * b_ + c_ * d_ + e_ * f_;
    const double dpq = p - q;
    const double disc = sqrt(dpq * dpq + 4.0 * r * r);
    const double lam = 0.5 * ((p + q) + disc);
    const double s1 = sqrt(lam);
    A.s1[o] = (T)s1;  // NaN in -> NaN out (Q14)
    if (A.s2) {
        // |col1 x col2| = s1 s2 = sqrt(det F^T F) without the cancellation of (p + q) - disc
        const double cx = c_ * f_ - e_ * d_, cy = e_ * b_ - a_ * f_, cz = a_ * d_ - c_ * b_;
        const double area = sqrt(cx * cx + cy * cy + cz * cz);
        A.s2[o] = (T)(s1 == 0.0 ? 0.0 : area / s1);
    }
    if (A.e_lon || A.e_lat) {
        // (F^T F - lam I) e = 0: the row that does not cancel
        double vx = p >= q ? lam - q : r;
        double vy = p >= q ? r : lam - p;
        const double n = sqrt(vx * vx + vy * vy);
        if (n == 0.0) {  // isotropic cell (disc == 0)
            vx = 1.0;
            vy = 0.0;
        } else {  // (NaN stays NaN: no comparison below holds for it)
            vx = vx / n;
            vy = vy / n;
            if (vx < 0.0 || (vx == 0.0 && vy < 0.0)) {
                vx = -vx;
                vy = -vy;
            }
        }
        if (A.e_lon) A.e_lon[o] = (T)vx;
        if (A.e_lat) A.e_lat[o] = (T)vy;
    }
}

__device__ __forceinline__ void sincos_t(float a, float *s, float *c) { sincosf(a, s, c); }
__device__ __forceinline__ void sincos_t(double a, double *s, double *c) { sincos(a, s, c); }

// T: arithmetic type of positions; S: type X,Y,Z are differenced in
template <typename T, typename S>
__global__ void __launch_bounds__(SBLOCK) strain_kernel(const StrainArgs<T> A0) {
#pragma clang fp contract(off)
    __shared__ S sX[LH][LW + 1];
    __shared__ S sY[LH][LW + 1];
    __shared__ S sZ[LH][LW + 1];
    const StrainArgs<T> A = strain_member(A0);
    const int ntx = (A.nx + SW - 1) / SW;
    const int tyi = blockIdx.x / ntx, txi = blockIdx.x - tyi * ntx;
    const int gy0 = tyi * SH;
    const int gx0 = txi * SW;
    const T PI = T(3.141592653589793);
    const T R = T(6371000);

    // stage X,Y,Z for the tile + halo
    for (int i = threadIdx.x; i < LW * LH; i += SBLOCK) {
        const int ly = i / LW, lx = i - ly * LW;
        const int gy = gy0 - HALO + ly;
        int gx = gx0 - HALO + lx;  // cyclic column (tools.py:225-228)
        gx %= A.nx;
        if (gx < 0) gx += A.nx;
        S vx = S(0), vy = S(0), vz = S(0);
        if (gy >= 0 && gy < A.ny) {
            const size_t o = (size_t)gy * A.nx + gx;
            const T lon = (A.x_dep[o] * PI) / T(180);            // LCS.py:195
            const T lat = ((A.y_dep[o] - T(90)) * PI) / T(180);  // LCS.py:196 (colatitude - pi)
            T sl, cl, so, co;
            sincos_t(lat, &sl, &cl);
            sincos_t(lon, &so, &co);
            vx = (S)((R * sl) * co);  // LCS.py:197
            vy = (S)((R * sl) * so);  // LCS.py:198
            vz = (S)(R * cl);         // LCS.py:199
        }
        sX[ly][lx] = vx;
        sY[ly][lx] = vy;
        sZ[ly][lx] = vz;
    }
    __syncthreads();

    const T dy = ((PI / T(180)) * A.dlat) * R;  // tools.py:256
    for (int i = threadIdx.x; i < SW * SH; i += SBLOCK) {
        const int oy = i / SW, ox = i - oy * SW;
        const int gy = gy0 + oy, gx = gx0 + ox;
        if (gy >= A.ny || gx >= A.nx) continue;
        const int ly = oy + HALO, lx = ox + HALO;
        // numba typing of tools.py:204-207: S differences, double scaling, S store
        auto centred = [](S p1, S m1, S p2, S m2) -> S {
            const S d1 = p1 - m1, d2 = p2 - m2;
            return (S)((4.0 / 3.0) * (double)d1 / 2.0 - (1.0 / 3.0) * (double)d2 / 4.0);
        };
        auto ddx = [&](S(*a)[LW + 1]) -> S {
            return centred(a[ly][lx + 1], a[ly][lx - 1], a[ly][lx + 2], a[ly][lx - 2]);
        };
        auto ddy = [&](S(*a)[LW + 1]) -> S {
            if (gy < 2) return (S)((double)(a[ly + 1][lx] - a[ly][lx]) / 2.0);         // tools.py:210-213
            if (gy >= A.ny - 2) return (S)((double)(a[ly][lx] - a[ly - 1][lx]) / 2.0);  // tools.py:214-217
            return centred(a[ly + 1][lx], a[ly - 1][lx], a[ly + 2][lx], a[ly - 2][lx]);
        };
        const T latr = (A.seed_lat[gy] * PI) / T(180);            // tools.py:254
        const T dx = (((PI / T(180)) * A.dlon) * R) * cos(latr);  // tools.py:255
        // derivative / metric: the division is done in T (float64 / float32 as numpy would)
        const T ta = (T)ddx(sX) / dx, tb = (T)ddy(sX) / dy;  // dXdx, dXdy
        const T tc = (T)ddx(sY) / dx, td = (T)ddy(sY) / dy;  // dYdx, dYdy
        const T te = (T)ddx(sZ) / dx, tf = (T)ddy(sZ) / dy;  // dZdx, dZdy
        strain_store(A, (size_t)gy * A.nx + gx, ta, tb, tc, td, te, tf);
    }
}

// ======================================================================================
// float32: sigma_kernel_f32's X, Y, Z and differences (bounded-argument sincos -- Cody-Waite by pi/2 + cephes minimax
// polynomials, ~1 ulp --, float stencil with the 4th-order weights folded, reciprocal metrics per row), then the float64
// eigen step above on the six float derivatives.
// ======================================================================================
__device__ __forceinline__ void bounded_sincosf(float a, float *sn, float *cs) {  // |a| < 64
    const float n = rintf(a * 0.636619772367581343f);  // 2/pi
    float r = fmaf(n, -1.5703125f, a);
    r = fmaf(n, -4.837512969970703125e-4f, r);
    r = fmaf(n, -7.54978995489188216e-8f, r);
    const float z = r * r;
    const float sp = fmaf(fmaf(fmaf(-1.9515295891e-4f, z, 8.3321608736e-3f), z, -1.6666654611e-1f), z * r, r);
    const float cp = fmaf(fmaf(fmaf(2.443315711809948e-5f, z, -1.388731625493765e-3f), z, 4.166664568298827e-2f),
                          z * z, fmaf(-0.5f, z, 1.0f));
    const int q = (int)n;
    const bool odd = q & 1;  // odd quadrant: sine and cosine swap
    const unsigned s1 = __builtin_bit_cast(unsigned, odd ? cp : sp), c1 = __builtin_bit_cast(unsigned, odd ? sp : cp);
    // signs as bit operations: sine flips in quadrants 2, 3 (bit 1 of q), cosine in quadrants 1, 2 (bit 1 of q + 1)
    *sn = __builtin_bit_cast(float, s1 ^ (((unsigned)q << 30) & 0x80000000u));
    *cs = __builtin_bit_cast(float, c1 ^ (((unsigned)(q + 1) << 30) & 0x80000000u));
}

// X, Y, Z of one departure point (LCS.py:195-199), float
__device__ __forceinline__ void sphere_xyz_f32(float xd, float yd, float &vx, float &vy, float &vz) {
#pragma clang fp contract(off)
    const float D2R = 3.141592653589793f / 180.0f;
    const float R = 6371000.0f;
    const float lon = xd * D2R;            // LCS.py:195
    const float lat = (yd - 90.0f) * D2R;  // LCS.py:196
    float sl, cl, so, co;
    if (fabsf(lat) < 64.0f && fabsf(lon) < 64.0f) {
        bounded_sincosf(lat, &sl, &cl);
        bounded_sincosf(lon, &so, &co);
    } else {  // out of the polynomial's range, or NaN: library path
        sincosf(lat, &sl, &cl);
        sincosf(lon, &so, &co);
    }
    const float rs = R * sl;
    vx = rs * co;  // LCS.py:197
    vy = rs * so;  // LCS.py:198
    vz = R * cl;   // LCS.py:199
}

// 1 / dx of a seed row (tools.py:254-255), float
__device__ __forceinline__ float inv_dx_f32(float seed_lat, float dlon) {
#pragma clang fp contract(off)
    const float latr = (seed_lat * 3.141592653589793f) / 180.0f;                           // tools.py:254
    return 1.0f / ((((3.141592653589793f / 180.0f) * dlon) * 6371000.0f) * cosf(latr));  // tools.py:255
}

// the two stencils with the 4th-order weights folded: (4/3)/2 and -(1/3)/4 of tools.py:204-207
__device__ __forceinline__ float centred_f32(float p1, float m1, float p2, float m2) {
#pragma clang fp contract(off)
    return __builtin_fmaf(2.0f / 3.0f, p1 - m1, (-1.0f / 12.0f) * (p2 - m2));
}
__device__ __forceinline__ float ddy_f32(int gy, int ny, float m2, float m1, float c0, float p1, float p2) {
#pragma clang fp contract(off)
    if (gy < 2) return 0.5f * (p1 - c0);        // tools.py:210-213
    if (gy >= ny - 2) return 0.5f * (c0 - m1);  // tools.py:214-217
    return centred_f32(p1, m1, p2, m2);
}

__global__ void __launch_bounds__(SBLOCK) strain_kernel_f32(const StrainArgs<float> A0) {
    __shared__ float sX[LH][LW + 1];
    __shared__ float sY[LH][LW + 1];
    __shared__ float sZ[LH][LW + 1];
    __shared__ float s_inv_dx[SH];
    const StrainArgs<float> A = strain_member(A0);
    const int ntx = (A.nx + SW - 1) / SW;
    const int tyi = blockIdx.x / ntx, txi = blockIdx.x - tyi * ntx;
    const int gy0 = tyi * SH;
    const int gx0 = txi * SW;

    if (threadIdx.x < SH) {
        const int gy = gy0 + (int)threadIdx.x;
        s_inv_dx[threadIdx.x] = gy < A.ny ? inv_dx_f32(A.seed_lat[gy], A.dlon) : 0.0f;
    }
    for (int i = threadIdx.x; i < LW * LH; i += SBLOCK) {
        const int ly = i / LW, lx = i - ly * LW;
        const int gy = gy0 - HALO + ly;
        int gx = gx0 - HALO + lx;
        gx = gx < 0 ? gx + A.nx : (gx >= A.nx ? gx - A.nx : gx);
        if (gx < 0 || gx >= A.nx) {  // grids narrower than the tile: general modulo
            gx %= A.nx;
            if (gx < 0) gx += A.nx;
        }
        float vx = 0.0f, vy = 0.0f, vz = 0.0f;
        if (gy >= 0 && gy < A.ny) {
            const size_t o = (size_t)gy * A.nx + gx;
            sphere_xyz_f32(A.x_dep[o], A.y_dep[o], vx, vy, vz);
        }
        sX[ly][lx] = vx;
        sY[ly][lx] = vy;
        sZ[ly][lx] = vz;
    }
    __syncthreads();

    const float inv_dy = 1.0f / (((3.141592653589793f / 180.0f) * A.dlat) * 6371000.0f);  // tools.py:256
    for (int i = threadIdx.x; i < SW * SH; i += SBLOCK) {
        const int oy = i / SW, ox = i - oy * SW;
        const int gy = gy0 + oy, gx = gx0 + ox;
        if (gy >= A.ny || gx >= A.nx) continue;
        const int ly = oy + HALO, lx = ox + HALO;
        const float inv_dx = s_inv_dx[oy];
        auto ddx = [&](float(*a)[LW + 1]) -> float {
            return centred_f32(a[ly][lx + 1], a[ly][lx - 1], a[ly][lx + 2], a[ly][lx - 2]) * inv_dx;
        };
        auto ddy = [&](float(*a)[LW + 1]) -> float {
            return ddy_f32(gy, A.ny, a[ly - 2][lx], a[ly - 1][lx], a[ly][lx], a[ly + 1][lx], a[ly + 2][lx]) * inv_dy;
        };
        const float a_ = ddx(sX), b_ = ddy(sX), c_ = ddx(sY), d_ = ddy(sY), e_ = ddx(sZ), f_ = ddy(sZ);
        strain_store(A, (size_t)gy * A.nx + gx, a_, b_, c_, d_, e_, f_);
    }
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
