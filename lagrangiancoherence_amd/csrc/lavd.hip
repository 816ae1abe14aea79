// Lagrangian-averaged vorticity deviation, rotation and path length: a record of trajectory planes and of the vorticity
// deviation sampled along them, folded block of levels by block of levels into three running integrals per parcel.
//
// The contract (include/lcs_hip.h has it in full; tests/lavd.py restates it in numpy).  Per interval j = 1 .. n_levels - 1, in
// level order, in float64:
//   acc_abs += 0.5 (|c[j-1]| + |c[j]|) |timestep|         LAVD: the trapezoid rule on |omega - mean|
//   acc_sgn += 0.5 ( c[j-1]  +  c[j] ) |timestep|         rotation: its sign separates cyclones from anticyclones
//   acc_len += d(j-1, j)                                  path length: the great-circle distance of great_circle.h, formed in T
// acc [3][n] is the only state between blocks and entry 0 of a continued block is the last entry of the block before, so any
// split of the levels into blocks gives the bits one block gives.  A NaN makes the integrals it enters NaN from there on, in
// its own parcel only; a NaN in c does not touch the length.
//
// Shape.  One thread per parcel, nothing shared between parcels.  The record is a pure stream -- 3 T per parcel and level in,
// nothing out until the end -- so, as in advect.hip's tracer_kernel, a ring of LAVD_DEPTH levels is held in registers and every
// slot is refilled, unconditionally and clamped to the last level, as soon as it has been consumed: several levels' loads are in
// flight per lane instead of one HBM latency per level.
//   lavd_update_kernel<T, true>    positions and values: all three integrals
//   lavd_update_kernel<T, false>   c == NULL: the path length only
#include "great_circle.h"

namespace {

constexpr int LAVD_THREADS = 256;
constexpr int LAVD_DEPTH = 4;

template <typename T>
struct LavdArgs {
    const T *x, *y, *c;   // [n_levels][n]
    double *acc;          // [3][n]
    T *lavd, *rotation, *length;
    double dt;            // |timestep|
    T two_r;
    int n, n_levels, level0;
};

template <typename T, bool HAS_C>
__global__ void __launch_bounds__(LAVD_THREADS) lavd_update_kernel(const LavdArgs<T> A) {
#pragma clang fp contract(off)
    const size_t n = (size_t)A.n;
    const size_t i = (size_t)blockIdx.x * LAVD_THREADS + threadIdx.x;
    if (i >= n) return;
    const int last = A.n_levels - 1;
    double s_abs = 0.0, s_sgn = 0.0, s_len = 0.0;
    if (A.level0 != 0) s_abs = A.acc[i], s_sgn = A.acc[n + i], s_len = A.acc[2 * n + i];
    // entry 0, then the ring: slot d holds entry 1 + d, refilled with entry 1 + d + LAVD_DEPTH clamped to the last one
    T xp = A.x[i], yp = A.y[i], cp = HAS_C ? A.c[i] : T(0);
    T qx[LAVD_DEPTH], qy[LAVD_DEPTH], qc[LAVD_DEPTH];
#pragma unroll
    for (int d = 0; d < LAVD_DEPTH; ++d) {
        const size_t e = (size_t)(1 + d < last ? 1 + d : last) * n + i;
        qx[d] = A.x[e], qy[d] = A.y[e];
        qc[d] = HAS_C ? A.c[e] : T(0);
    }
    T kp = fsle_cos(yp);
    auto step = [&](int j, T &sx, T &sy, T &sc) {
        const T x = sx, y = sy, c = sc;
        const size_t e = (size_t)(j + LAVD_DEPTH < last ? j + LAVD_DEPTH : last) * n + i;
        sx = A.x[e], sy = A.y[e];
        if (HAS_C) sc = A.c[e];
        const T k = fsle_cos(y);
        s_len += (double)fsle_sep(xp, yp, kp, x, y, k, A.two_r);
        if (HAS_C) {
            s_abs += (0.5 * (fabs((double)cp) + fabs((double)c))) * A.dt;
            s_sgn += (0.5 * ((double)cp + (double)c)) * A.dt;
        }
        xp = x, yp = y, kp = k, cp = c;
    };
    int j0 = 1;
    for (; j0 + LAVD_DEPTH <= A.n_levels; j0 += LAVD_DEPTH) {
#pragma unroll
        for (int d = 0; d < LAVD_DEPTH; ++d) step(j0 + d, qx[d], qy[d], qc[d]);
    }
#pragma unroll
    for (int d = 0; d < LAVD_DEPTH - 1; ++d)
        if (j0 + d < A.n_levels) step(j0 + d, qx[d], qy[d], qc[d]);
    A.acc[i] = s_abs, A.acc[n + i] = s_sgn, A.acc[2 * n + i] = s_len;
    if (HAS_C && A.lavd) A.lavd[i] = (T)s_abs;
    if (HAS_C && A.rotation) A.rotation[i] = (T)s_sgn;
    if (A.length) A.length[i] = (T)s_len;
}

template <typename T>
void launch(lc_ctx *ctx, const lc_lavd_args *a) {
    LavdArgs<T> A;
    A.x = (const T *)a->traj_x, A.y = (const T *)a->traj_y, A.c = (const T *)a->c;
    A.acc = a->acc;
    A.lavd = (T *)a->lavd, A.rotation = (T *)a->rotation, A.length = (T *)a->length;
    A.dt = fabs(a->timestep);
    A.two_r = T(2) * (T)a->radius;
    A.n = a->n, A.n_levels = a->n_levels, A.level0 = a->level0;
    const dim3 grid((unsigned)(((long long)a->n + LAVD_THREADS - 1) / LAVD_THREADS)), block(LAVD_THREADS);
    if (a->c)
        hipLaunchKernelGGL((lavd_update_kernel<T, true>), grid, block, 0, ctx->stream, A);
    else
        hipLaunchKernelGGL((lavd_update_kernel<T, false>), grid, block, 0, ctx->stream, A);
}

}  // namespace

extern "C" int lc_lavd_update(lc_ctx *ctx, const lc_lavd_args *a) {
    const char *who = "lc_lavd_update";
    LC_REQUIRE(ctx, "%s: null context", who);
    LC_REQUIRE(a, "%s: null argument structure", who);
    LC_REQUIRE(a->struct_size == sizeof(lc_lavd_args), "%s: struct_size %zu, this library has %zu", who, (size_t)a->struct_size,
               sizeof(lc_lavd_args));
    LC_REQUIRE(a->dtype == LC_F32 || a->dtype == LC_F64, "%s: bad dtype %d", who, a->dtype);
    LC_REQUIRE(a->n >= 1, "%s: n %d (at least one parcel)", who, a->n);
    LC_REQUIRE(a->n_levels >= 2, "%s: n_levels %d (a block has at least two trajectory entries)", who, a->n_levels);
    LC_REQUIRE(a->level0 >= 0, "%s: level0 %d", who, a->level0);
    LC_REQUIRE(a->radius - a->radius == 0.0 && a->radius > 0.0, "%s: radius %g (positive and finite)", who, a->radius);
    LC_REQUIRE(a->timestep - a->timestep == 0.0 && a->timestep != 0.0, "%s: timestep %g (non-zero and finite)", who, a->timestep);
    LC_REQUIRE(a->traj_x && a->traj_y && a->acc, "%s: null pointer", who);
    LC_REQUIRE(a->c || (!a->lavd && !a->rotation), "%s: lavd and rotation need c (without it only length is produced)", who);
    LC_HIP_CHECK(hipSetDevice(ctx->device));
    if (a->dtype == LC_F32) {
        launch<float>(ctx, a);
        ctx->last_lavd_kernel = a->c ? "lavd_update_kernel<float, true>" : "lavd_update_kernel<float, false>";
    } else {
        launch<double>(ctx, a);
        ctx->last_lavd_kernel = a->c ? "lavd_update_kernel<double, true>" : "lavd_update_kernel<double, false>";
    }
    LC_HIP_CHECK(hipGetLastError());
    return LC_OK;
}

extern "C" const char *lc_ctx_last_lavd_kernel(const lc_ctx *ctx) { return ctx ? ctx->last_lavd_kernel : ""; }
