// The flow-map gradient on chip, shared by sigma.hip and strain.hip: per seed, the six derivatives
//   dXdx, dXdy, dYdx, dYdy, dZdx, dZdy
// of the departure point's X, Y, Z on the sphere along the seed grid, and the 2 x 2 Gram eigenvalue both files reduce them with.
// The Gram step and the strain step (stretch_of) are also what aux_gradient.hip reduces its own six derivatives with.
// Restates
//   LCS.flowmap_gradient               LCS/LCS.py:195-208    lon/lat -> X,Y,Z on the sphere
//   tools.derivative_spherical_coords  LCS/tools.py:254-264  metric dx, dy
//   tools.fourth_order_derivative      LCS/tools.py:202-228  5-point stencil, cyclic in longitude, one-sided/2 on the 2
//                                                            first/last rows (Q12)
// in two arithmetics, each written once:
//   numba's typing   positions and metric in T, X,Y,Z stored and differenced in S (float when fd_fp32_cast, Q11), the
//                    stencil scaled in double and stored as S, the division by the metric in T: GradientTile<S>
//   float32 fast     bounded-argument sincos (Cody-Waite by pi/2 + cephes minimax polynomials, ~1 ulp), the 4th-order
//                    weights folded (2/3, -1/12), reciprocal metrics per row: GradientTileF32, and the same helpers in
//                    the marching kernel of sigma.hip
// A tile is SW x SH output cells + a HALO-cell ring of X, Y, Z in LDS, staged by SBLOCK threads.  A kernel holds the rows
// [in_row0, in_row0 + n_in_rows) of a grid of ny_global rows (x_dep, y_dep and seed_lat start at row in_row0); halo rows
// outside the grid or outside that window are staged as zeros (the entry points admit no output row that would difference
// them).  The whole grid is the window (0, ny, ny).  A NaN departure point gives NaN in every derivative whose stencil
// touches it (Q14).
// `#pragma clang fp contract(off)` is function-scoped: every function here that had it where it came from carries it.
#pragma once
#include "lcs_common.h"

namespace {

constexpr int SW = 64;  // tile width  (longitude)
constexpr int SH = 16;  // tile height (latitude)
constexpr int HALO = 2;
constexpr int LW = SW + 2 * HALO;
constexpr int LH = SH + 2 * HALO;
constexpr int SBLOCK = 256;

// first global row and first column of workgroup blockIdx.x's tile: row-major over the tiles of the output rows from row0
__device__ __forceinline__ void tile_origin(int nx, int row0, int &gy0, int &gx0) {
    const int ntx = (nx + SW - 1) / SW;
    const int tyi = blockIdx.x / ntx, txi = blockIdx.x - tyi * ntx;
    gy0 = row0 + tyi * SH;
    gx0 = txi * SW;
}

// cell(oy, ox, gy, gx) for this thread's cells of the tile at (gy0, gx0) that lie before row_end and column nx
template <typename F>
__device__ __forceinline__ void for_tile_cells(int gy0, int gx0, int row_end, int nx, F cell) {
    for (int i = threadIdx.x; i < SW * SH; i += SBLOCK) {
        const int oy = i / SW, ox = i - oy * SW;
        const int gy = gy0 + oy, gx = gx0 + ox;
        if (gy < row_end && gx < nx) cell(oy, ox, gy, gx);
    }
}

// ======================================================================================
// numba's typing.  T: arithmetic type of positions; S: type X,Y,Z are differenced in
// ======================================================================================
__device__ __forceinline__ void sincos_t(float a, float *s, float *c) { sincosf(a, s, c); }
__device__ __forceinline__ void sincos_t(double a, double *s, double *c) { sincos(a, s, c); }

// X, Y, Z of one departure point (LCS.py:195-199)
template <typename T, typename S>
__device__ __forceinline__ void sphere_xyz(T xd, T yd, S &vx, S &vy, S &vz) {
#pragma clang fp contract(off)
    const T PI = T(3.141592653589793);
    const T R = T(6371000);
    const T lon = (xd * PI) / T(180);            // LCS.py:195
    const T lat = ((yd - T(90)) * PI) / T(180);  // LCS.py:196 (colatitude - pi)
    T sl, cl, so, co;
    sincos_t(lat, &sl, &cl);
    sincos_t(lon, &so, &co);
    vx = (S)((R * sl) * co);  // LCS.py:197
    vy = (S)((R * sl) * so);  // LCS.py:198
    vz = (S)(R * cl);         // LCS.py:199
}

// metric of a seed row and of the rows (tools.py:254-256)
template <typename T>
__device__ __forceinline__ T metric_dx(T seed_lat, T dlon) {
#pragma clang fp contract(off)
    const T PI = T(3.141592653589793);
    const T R = T(6371000);
    const T latr = (seed_lat * PI) / T(180);          // tools.py:254
    return (((PI / T(180)) * dlon) * R) * cos(latr);  // tools.py:255
}
template <typename T>
__device__ __forceinline__ T metric_dy(T dlat) {
#pragma clang fp contract(off)
    return ((T(3.141592653589793) / T(180)) * dlat) * T(6371000);  // tools.py:256
}

// numba typing of tools.py:204-207: S differences, double scaling, S store
template <typename S>
__device__ __forceinline__ S centred(S p1, S m1, S p2, S m2) {
#pragma clang fp contract(off)
    const S d1 = p1 - m1, d2 = p2 - m2;
    return (S)((4.0 / 3.0) * (double)d1 / 2.0 - (1.0 / 3.0) * (double)d2 / 4.0);
}
// and of the one-sided difference / 2 on the two first and two last rows (tools.py:210-217)
template <typename S>
__device__ __forceinline__ S one_sided(S hi, S lo) {
#pragma clang fp contract(off)
    return (S)((double)(hi - lo) / 2.0);
}

template <typename S>
struct GradientTile {
    S X[LH][LW + 1], Y[LH][LW + 1], Z[LH][LW + 1];

    // X,Y,Z of the tile at (gy0, gx0) + halo; the caller synchronises
    template <typename T>
    __device__ __forceinline__ void stage(const T *x_dep, const T *y_dep, int in_row0, int n_in_rows, int ny_global, int nx,
                                          int gy0, int gx0) {
        for (int i = threadIdx.x; i < LW * LH; i += SBLOCK) {
            const int ly = i / LW, lx = i - ly * LW;
            const int gy = gy0 - HALO + ly;  // global row
            int gx = gx0 - HALO + lx;        // cyclic column (tools.py:225-228)
            gx %= nx;
            if (gx < 0) gx += nx;
            const int ry = gy - in_row0;     // row inside the input window
            S vx = S(0), vy = S(0), vz = S(0);
            if (gy >= 0 && gy < ny_global && ry >= 0 && ry < n_in_rows) {
                const size_t o = (size_t)ry * nx + gx;
                sphere_xyz(x_dep[o], y_dep[o], vx, vy, vz);
            }
            X[ly][lx] = vx;
            Y[ly][lx] = vy;
            Z[ly][lx] = vz;
        }
    }

    // d[0..5] = dXdx, dXdy, dYdx, dYdy, dZdx, dZdy of cell (oy, ox) of the tile, global row gy.  derivative / metric: the
    // division is done in T (float64 / float32 as numpy would)
    template <typename T>
    __device__ __forceinline__ void derivatives(int oy, int ox, int gy, int ny_global, T dx, T dy, T (&d)[6]) const {
#pragma clang fp contract(off)
        const int ly = oy + HALO, lx = ox + HALO;
        auto ddx = [&](const S(*a)[LW + 1]) -> S {
            return centred(a[ly][lx + 1], a[ly][lx - 1], a[ly][lx + 2], a[ly][lx - 2]);
        };
        auto ddy = [&](const S(*a)[LW + 1]) -> S {
            if (gy < 2) return one_sided(a[ly + 1][lx], a[ly][lx]);
            if (gy >= ny_global - 2) return one_sided(a[ly][lx], a[ly - 1][lx]);
            return centred(a[ly + 1][lx], a[ly - 1][lx], a[ly + 2][lx], a[ly - 2][lx]);
        };
        d[0] = (T)ddx(X) / dx, d[1] = (T)ddy(X) / dy;
        d[2] = (T)ddx(Y) / dx, d[3] = (T)ddy(Y) / dy;
        d[4] = (T)ddx(Z) / dx, d[5] = (T)ddy(Z) / dy;
    }
};

// ======================================================================================
// float32 fast path.  The float result cannot be bit-identical to the reference (numpy float32 sin/cos, LAPACK sgesdd)
// anyway, so it spends as few VALU cycles per cell as it can.
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
// 1 / dy (tools.py:256), float (products and a quotient: nothing a contraction could change)
__device__ __forceinline__ float inv_dy_f32(float dlat) { return 1.0f / (((3.141592653589793f / 180.0f) * dlat) * 6371000.0f); }

// the two stencils with the 4th-order weights folded: (4/3)/2 and -(1/3)/4 of tools.py:204-207
__device__ __forceinline__ float centred_f32(float p1, float m1, float p2, float m2) {
#pragma clang fp contract(off)
    return __builtin_fmaf(2.0f / 3.0f, p1 - m1, (-1.0f / 12.0f) * (p2 - m2));
}
__device__ __forceinline__ float ddy_f32(int gy, int ny_global, float m2, float m1, float c0, float p1, float p2) {
#pragma clang fp contract(off)
    if (gy < 2) return 0.5f * (p1 - c0);              // tools.py:210-213
    if (gy >= ny_global - 2) return 0.5f * (c0 - m1);  // tools.py:214-217
    return centred_f32(p1, m1, p2, m2);
}

struct GradientTileF32 {
    float X[LH][LW + 1], Y[LH][LW + 1], Z[LH][LW + 1];
    float inv_dx[SH];  // of the tile's rows

    // X,Y,Z of the tile at (gy0, gx0) + halo and 1 / dx of its rows before row_end; the caller synchronises
    __device__ __forceinline__ void stage(const float *x_dep, const float *y_dep, const float *seed_lat, float dlon, int in_row0,
                                          int n_in_rows, int ny_global, int nx, int gy0, int gx0, int row_end) {
        if (threadIdx.x < SH) {
            const int gy = gy0 + (int)threadIdx.x;
            inv_dx[threadIdx.x] = gy < row_end ? inv_dx_f32(seed_lat[gy - in_row0], dlon) : 0.0f;
        }
        for (int i = threadIdx.x; i < LW * LH; i += SBLOCK) {
            const int ly = i / LW, lx = i - ly * LW;
            const int gy = gy0 - HALO + ly;
            int gx = gx0 - HALO + lx;
            gx = gx < 0 ? gx + nx : (gx >= nx ? gx - nx : gx);
            if (gx < 0 || gx >= nx) {  // grids narrower than the tile: general modulo
                gx %= nx;
                if (gx < 0) gx += nx;
            }
            const int ry = gy - in_row0;
            float vx = 0.0f, vy = 0.0f, vz = 0.0f;
            if (gy >= 0 && gy < ny_global && ry >= 0 && ry < n_in_rows) {
                const size_t o = (size_t)ry * nx + gx;
                sphere_xyz_f32(x_dep[o], y_dep[o], vx, vy, vz);
            }
            X[ly][lx] = vx;
            Y[ly][lx] = vy;
            Z[ly][lx] = vz;
        }
    }

    // d[0..5] = dXdx, dXdy, dYdx, dYdy, dZdx, dZdy of cell (oy, ox) of the tile, global row gy.  (No contract(off) here: the
    // products with the reciprocal metrics are compiled as they always were.)
    __device__ __forceinline__ void derivatives(int oy, int ox, int gy, int ny_global, float inv_dy, float (&d)[6]) const {
        const int ly = oy + HALO, lx = ox + HALO;
        const float idx = inv_dx[oy];
        auto ddx = [&](const float(*a)[LW + 1]) -> float {
            return centred_f32(a[ly][lx + 1], a[ly][lx - 1], a[ly][lx + 2], a[ly][lx - 2]) * idx;
        };
        auto ddy = [&](const float(*a)[LW + 1]) -> float {
            return ddy_f32(gy, ny_global, a[ly - 2][lx], a[ly - 1][lx], a[ly][lx], a[ly + 1][lx], a[ly + 2][lx]) * inv_dy;
        };
        d[0] = ddx(X), d[1] = ddy(X), d[2] = ddx(Y), d[3] = ddy(Y), d[4] = ddx(Z), d[5] = ddy(Z);
    }
};

// ======================================================================================
// Gram step, float64 for both arithmetics: [[p, r], [r, q]] of the six derivatives a..f for a layout and its larger
// eigenvalue lam in closed form; the largest singular value is sqrt(lam).
// ======================================================================================
struct Gram {
    double p, q, r, lam;
};
__device__ __forceinline__ Gram gram_eigen(int layout, double a_, double b_, double c_, double d_, double e_, double f_) {
#pragma clang fp contract(off)
    Gram g;
    if (layout == LC_LAYOUT_REFERENCE) {
        // M = [[a,b,c],[d,e,f],[0,0,0]] (LCS.py:153, Q13): Gram matrix of its two non-zero rows
        g.p = a_ * a_ + b_ * b_ + c_ * c_;
        g.q = d_ * d_ + e_ * e_ + f_ * f_;
        g.r = a_ * d_ + b_ * e_ + c_ * f_;
    } else {
        // Jacobian [[a,b],[c,d],[e,f]]: F^T F
        g.p = a_ * a_ + c_ * c_ + e_ * e_;
        g.q = b_ * b_ + d_ * d_ + f_ * f_;
        g.r = a_ * b_ + c_ * d_ + e_ * f_;
    }
    const double dpq = g.p - g.q;
    const double disc = sqrt(dpq * dpq + 4.0 * g.r * g.r);
    g.lam = 0.5 * ((g.p + g.q) + disc);
    return g;
}

// ======================================================================================
// Strain step, float64 for both arithmetics, shared by strain.hip and aux_gradient.hip: both singular values of the 3 x 2
// Jacobian [[a, b], [c, d], [e, f]] (a..f = dXdx, dXdy, dYdx, dYdy, dZdx, dZdy; physical layout) and the unit eigenvector
// (ex, ey) of F^T F for the larger eigenvalue in (east, north) components.  s2 = |col1 x col2| / s1 (0 where s1 == 0).
// Sign: ex > 0, or ex == 0 and ey > 0; (1, 0) where F^T F is a multiple of the identity.  NaN in -> NaN in every member.
// s2 / the direction are only computed where asked for (the others are left 0).
// ======================================================================================
struct Stretch {
    double s1, s2, ex, ey;
};
__device__ __forceinline__ Stretch stretch_of(double a_, double b_, double c_, double d_, double e_, double f_, bool want_s2,
                                              bool want_dir) {
#pragma clang fp contract(off)
    const auto [p, q, r, lam] = gram_eigen(LC_LAYOUT_PHYSICAL, a_, b_, c_, d_, e_, f_);
    Stretch s = {sqrt(lam), 0.0, 0.0, 0.0};  // NaN in -> NaN out (Q14)
    if (want_s2) {
        // |col1 x col2| = s1 s2 = sqrt(det F^T F) without the cancellation of (p + q) - disc
        const double cx = c_ * f_ - e_ * d_, cy = e_ * b_ - a_ * f_, cz = a_ * d_ - c_ * b_;
        const double area = sqrt(cx * cx + cy * cy + cz * cz);
        s.s2 = s.s1 == 0.0 ? 0.0 : area / s.s1;
    }
    if (want_dir) {
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
        s.ex = vx;
        s.ey = vy;
    }
    return s;
}

}  // namespace
