// Great-circle separation of two positions in degrees, in half-angle form: shared by fsle.hip (the separation of a neighbour
// pair) and lavd.hip (the length of one trajectory step).  h = sin^2(k dphi / 2) + cos(k phi1) cos(k phi2) sin^2(k dlambda / 2),
// d = 2 radius asin(min(1, sqrt h)), dlambda the raw difference (the form is periodic: the seam needs no wrap).
#pragma once
#include "flowmap_gradient.h"

namespace {

// float64: the library's functions, in the operation order of the numpy restatement (tests/fsle.py).
__device__ __forceinline__ double fsle_sin_half(double a) { return sin(a); }
__device__ __forceinline__ double fsle_cos_lat(double a) { return cos(a); }
__device__ __forceinline__ double fsle_asin(double s) { return asin(s); }
__device__ __forceinline__ double fsle_sqrt(double h) { return sqrt(h); }
__device__ __forceinline__ double fsle_log(double a) { return log(a); }
// float32: the level loop is bound by these, so each takes the cheapest form that keeps its RELATIVE accuracy (what a pair's
// separation rests on), and the library's where that form does not reach (NaN included: every comparison below fails for it).
//   the sine of half a coordinate difference: small but for the pairs across the seam -- the odd minimax polynomial on the
//   argument itself for |a| <= pi/4 (sin a = a (1 + ...): exact relative accuracy down to 0), else the bounded-argument
//   reduction of flowmap_gradient.h
__device__ __forceinline__ float fsle_sin_half(float a) {
    if (fabsf(a) <= 0.785398f) {
        const float z = a * a;
        return fmaf(fmaf(fmaf(-1.9515295891e-4f, z, 8.3321608736e-3f), z, -1.6666654611e-1f), z * a, a);
    }
    if (fabsf(a) < 64.0f) {
        float sn, cs;
        bounded_sincosf(a, &sn, &cs);
        return sn;
    }
    return sinf(a);
}
__device__ __forceinline__ float fsle_cos_lat(float a) {
    if (fabsf(a) < 64.0f) {
        float sn, cs;
        bounded_sincosf(a, &sn, &cs);
        return cs;
    }
    return cosf(a);
}
//   asin on [0, 1]: s <= 1/2 (a separation up to 60 degrees of arc) by the odd polynomial of Cephes' asinf, else the library
__device__ __forceinline__ float fsle_asin(float s) {
    if (s <= 0.5f) {
        const float z = s * s;
        const float p = fmaf(fmaf(fmaf(fmaf(4.2163199048e-2f, z, 2.4181311049e-2f), z, 4.5470025998e-2f), z, 7.4953002686e-2f), z,
                             1.6666752422e-1f);
        return fmaf(p * z, s, s);
    }
    return asinf(s);
}
__device__ __forceinline__ float fsle_sqrt(float h) { return sqrtf(h); }
__device__ __forceinline__ float fsle_log(float a) { return logf(a); }

template <typename T>
__device__ __forceinline__ T fsle_cos(T lat) {
#pragma clang fp contract(off)
    return fsle_cos_lat((T(3.141592653589793) / T(180)) * lat);
}

// great-circle separation of two parcels (degrees; c = cos(k lat)).  Symmetric in its two parcels bit for bit (every function
// above is odd or even bit for bit); a NaN anywhere gives NaN (the clamp keeps it: NaN > 1 is false).
template <typename T>
__device__ __forceinline__ T fsle_sep(T x1, T y1, T c1, T x2, T y2, T c2, T two_r) {
#pragma clang fp contract(off)
    const T K = T(3.141592653589793) / T(180);
    const T sp = fsle_sin_half(T(0.5) * (K * (y2 - y1)));
    const T sl = fsle_sin_half(T(0.5) * (K * (x2 - x1)));
    const T h = sp * sp + (c1 * c2) * (sl * sl);
    T s = fsle_sqrt(h);
    s = s > T(1) ? T(1) : s;
    return two_r * fsle_asin(s);
}

}  // namespace
