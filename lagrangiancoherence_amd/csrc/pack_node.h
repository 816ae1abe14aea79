// The order-1 pack of ONE padded node over a run of time levels: the expressions pack_fused_kernel (pack.hip) and the pack
// workgroups inside a fused advect launch (advect.hip: deferred pack, lc_field_pack_deferred) both write the images with, so
// that the two cannot drift apart -- an image is the same bits whichever of them wrote a level.
#pragma once
#include "lcs_common.h"

__device__ __forceinline__ int mirror_index(int i, int n) {
    // scipy ni_interpolation.c tap mirroring; here |i| never exceeds n+1
    if (i < 0) i = -i;
    if (i > n - 1) i = 2 * (n - 1) - i;
    return i;
}

// Non-temporal stores of the images (nothing reads them again before the advect kernel streams them): config 2's float64
// pack 2.07 -> 1.95 ms, C3's 0.54 -> 0.50 (profiles/r03; the plain stores of that A/B: tools/experiments/advect_r06_compile_time_forks.patch).
#define LCS_PACK_STORE(ptr, val) __builtin_nontemporal_store(val, ptr)

// Levels t0 .. t0 + LV - 1 of the node whose mirrored source is element `so` of a raw plane and whose place is node `po` of a
// padded level: lin[t] = {u, v}[t] for lin_from <= t < nt, ext[t] = 2 {u, v}[t] - {u, v}[t+1] for t + 1 < nt.  Level t+1 is
// carried forward, so a raw level is read once (plus one level in LV at the run's end); the loads are issued together, then
// the stores.  nt: the levels that exist as far as this call goes (nothing at or past it is read or written); lin / ext NULL:
// that image is not written.
template <typename T, int LV>
__device__ __forceinline__ void pack_node_levels(const T *__restrict__ u, const T *__restrict__ v, T *__restrict__ lin, T *__restrict__ ext,
                                                 size_t plane, size_t level, size_t so, size_t po, int t0, int nt, int lin_from) {
    typedef T T2 __attribute__((ext_vector_type(2)));
    T a[LV + 1], b[LV + 1];
#pragma unroll
    for (int q = 0; q <= LV; ++q) {
        const size_t t = (size_t)min(t0 + q, nt - 1);          // (past the series: the last level again, never used)
        a[q] = u[t * plane + so];
        b[q] = v[t * plane + so];
    }
#pragma unroll
    for (int q = 0; q < LV; ++q) {
        const int t = t0 + q;
        if (t >= nt) break;
        if (lin && t >= lin_from) LCS_PACK_STORE((T2 *)(lin + ((size_t)t * level + po) * 2), ((T2){a[q], b[q]}));
        if (ext && t + 1 < nt)
            LCS_PACK_STORE((T2 *)(ext + ((size_t)t * level + po) * 2), ((T2){T(2) * a[q] - a[q + 1], T(2) * b[q] - b[q + 1]}));
    }
}
