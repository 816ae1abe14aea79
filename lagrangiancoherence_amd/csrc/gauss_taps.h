// The separable Gaussian of scipy.ndimage.gaussian_filter (truncate=4.0, mode='reflect', accumulation in double, the
// symmetric-kernel summation order of ni_filters.c), shared by api.hip (gauss_kernel: one plane, float32 / float64),
// ridges_batch.hip (gauss_planes_kernel: a stack of float64 planes) and threshold.hip (gauss_line_kernel: radii in the
// hundreds, the lines staged in LDS): the weights, the reflection and the tap loop -- out of global memory and out of LDS --
// are written once, here, so a plane smoothed by any of the kernels has the same bits.
#pragma once
#include <cmath>
#include <vector>

#include "lcs_common.h"

namespace {

constexpr int GAUSS_W_CAPACITY = 256;  // the largest radius a GaussW holds (api.hip: GAUSS_MAX_RADIUS)

struct GaussW {
    double w[GAUSS_W_CAPACITY + 1];  // w[0] centre ... w[radius]
    int radius;
};

// scipy: int(truncate * sd + 0.5)
inline int gauss_radius(double sigma) { return (int)(4.0 * sigma + 0.5); }

// scipy _gaussian_kernel1d: phi = exp(-0.5/sigma^2 * x^2); phi /= phi.sum().  G.radius is set (<= GAUSS_W_CAPACITY).
inline void gauss_fill_weights(GaussW &G, double sigma) {
    double sum = 0.0;
    std::vector<double> phi(2 * G.radius + 1);
    for (int k = -G.radius; k <= G.radius; ++k) phi[k + G.radius] = std::exp(-0.5 / (sigma * sigma) * (double)k * k);
    for (double p : phi) sum += p;
    for (int k = 0; k <= G.radius; ++k) G.w[k] = phi[k + G.radius] / sum;
}

__device__ __forceinline__ int reflect_index(int i, int n) {
    // scipy 'reflect' (d c b a | a b c d | d c b a), any distance
    if (n == 1) return 0;
    const int period = 2 * n;
    i %= period;
    if (i < 0) i += period;
    return i < n ? i : period - 1 - i;
}

// one output node (y, x) of the pass along AXIS over the plane `in` [ny][nx]
template <typename T, int AXIS>
__device__ __forceinline__ double gauss_taps(const T *__restrict__ in, int y, int x, int ny, int nx, const GaussW &G) {
    double acc = (double)in[(size_t)y * nx + x] * G.w[0];
    for (int j = G.radius; j >= 1; --j) {  // outermost pair first, as correlate1d does
        double lo, hi;
        if (AXIS == 0) {
            lo = (double)in[(size_t)reflect_index(y - j, ny) * nx + x];
            hi = (double)in[(size_t)reflect_index(y + j, ny) * nx + x];
        } else {
            lo = (double)in[(size_t)y * nx + reflect_index(x - j, nx)];
            hi = (double)in[(size_t)y * nx + reflect_index(x + j, nx)];
        }
        acc += (lo + hi) * G.w[j];
    }
    return acc;
}

// The same sum for N output nodes of lines staged in LDS (threshold.hip: gauss_line_kernel): `centre` is the first node's own
// sample, its neighbours along the axis lie STEP words apart (the boundary rule was resolved when the line was staged), node n
// is NEXT words further on.  Centre first, then the pairs from the outermost inwards: node for node the arithmetic of
// gauss_taps above, so a plane smoothed through LDS has gauss_kernel's bits.  No division, no modulo, no global load.
template <int N, int STEP, int NEXT>
__device__ __forceinline__ void gauss_taps_lds(const double *centre, const GaussW &G, double (&acc)[N]) {
#pragma unroll
    for (int n = 0; n < N; ++n) acc[n] = centre[n * NEXT] * G.w[0];
    for (int j = G.radius; j >= 1; --j) {
        const double w = G.w[j];
        const double *lo = centre - j * STEP, *hi = centre + j * STEP;
#pragma unroll
        for (int n = 0; n < N; ++n) acc[n] += (lo[n * NEXT] + hi[n * NEXT]) * w;
    }
}

}  // namespace
