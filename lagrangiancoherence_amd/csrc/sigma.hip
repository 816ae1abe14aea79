// K3 -- flow-map gradient + largest singular value, fused.
//
// Restates, per seed:
//   LCS.flowmap_gradient, tools.derivative_spherical_coords, tools.fourth_order_derivative: the six derivatives of X,Y,Z
//                                   along the seed grid (flowmap_gradient.h, shared with strain.hip)
//   eigen step of LCS.__call__      LCS/LCS.py:152-154   ||M||_2 of the 3x3 built by a
//                                   row-major reshape of the 9 components (Q13)
// The reference materialises X,Y,Z, six derivative fields, three zero fields and a
// pandas MultiIndex; here X,Y,Z are computed once per cell (as float when fd_fp32_cast,
// Q11), differenced on chip and the 2x2 Gram eigenproblem is solved in closed form.
// HBM traffic: read x_dep,y_dep once (+halo re-reads served by L2), write sigma once.
// Three kernels, one arithmetic per type:
//   sigma_march_kernel_f32   float32, sigma only, even width (the default): a wave walks down its rows with
//                            five rows of X,Y,Z in registers, x-neighbours by wavefront shuffle
//   sigma_kernel_f32         float32, sigma only, any width: a 64 x 16 tile + halo through LDS
//   sigma_kernel<T,S>        float64 and/or the 9-plane tensor output, numba's typing of the stencil (S)
#include "flowmap_gradient.h"

namespace {

template <typename T>
struct SigmaArgs {
    const T *x_dep, *y_dep, *seed_lat;
    int in_row0, n_in_rows, nx, ny_global;
    T dlat, dlon;
    int layout;
    int out_row0, n_out_rows;
    T *sigma;   // may be null
    T *tensor;  // null, or 9 planes [n_out_rows*nx] in the reference's merge order (LCS.py:220)
};

// lc_sigma_batch: the arguments as plane blockIdx.y sees them (whole grids: [n_members][ny*nx] inputs and outputs).
template <typename T>
__device__ __forceinline__ SigmaArgs<T> sigma_member(const SigmaArgs<T> &A0, size_t plane) {
    SigmaArgs<T> A = A0;
    const size_t off = (size_t)blockIdx.y * plane;
    A.x_dep += off;
    A.y_dep += off;
    A.sigma += off;
    return A;
}

// T: arithmetic type of positions; S: type X,Y,Z are differenced in
template <typename T, typename S>
__device__ __forceinline__ void sigma_body(const SigmaArgs<T> &A) {
#pragma clang fp contract(off)
    __shared__ GradientTile<S> tile;
    int gy0, gx0;
    tile_origin(A.nx, A.out_row0, gy0, gx0);
    tile.stage(A.x_dep, A.y_dep, A.in_row0, A.n_in_rows, A.ny_global, A.nx, gy0, gx0);
    __syncthreads();

    const T dy = metric_dy(A.dlat);
    for_tile_cells(gy0, gx0, A.out_row0 + A.n_out_rows, A.nx, [&](int oy, int ox, int gy, int gx) {
        T d[6];
        tile.derivatives(oy, ox, gy, A.ny_global, metric_dx(A.seed_lat[gy - A.in_row0], A.dlon), dy, d);
        const size_t oidx = (size_t)(gy - A.out_row0) * A.nx + gx;
        if (A.tensor) {
            const size_t plane = (size_t)A.n_out_rows * A.nx;
            for (int k = 0; k < 6; ++k) A.tensor[k * plane + oidx] = d[k];
            for (int k = 6; k < 9; ++k) A.tensor[k * plane + oidx] = T(0);  // dXdr, dYdr, dZdr (LCS.py:206-208)
        }
        if (A.sigma) A.sigma[oidx] = (T)sqrt(gram_eigen(A.layout, d[0], d[1], d[2], d[3], d[4], d[5]).lam);  // NaN in -> NaN out (Q14)
    });
}
template <typename T, typename S>
__global__ void __launch_bounds__(SBLOCK) sigma_kernel(const SigmaArgs<T> A) {
    sigma_body<T, S>(A);
}
// lc_sigma_batch: plane blockIdx.y of [n_members][ny*nx] inputs and outputs, the same per-cell arithmetic (sigma only).
template <typename T, typename S>
__global__ void __launch_bounds__(SBLOCK) sigma_batch_kernel(const SigmaArgs<T> A, size_t plane) {
    sigma_body<T, S>(sigma_member(A, plane));
}

// ======================================================================================
// float fast path of K3: flowmap_gradient.h's float32 arithmetic, then the float closed form.  Tile 64 x 16 outputs per
// 256 threads (halo redundancy (68*20)/(64*16) = 1.33).  Measured on 4096^2 cells (ms): 64x64 0.201,
// 64x32 0.105, 128x16 0.112, 64x16 0.0905, 64x12 0.096, 32x32 0.094, 32x16 0.101, 128x8 0.099, 64x8 0.108 --
// occupancy (LDS per workgroup) matters more than halo redundancy.
// ======================================================================================
// largest singular value from the six derivatives (closed-form 2x2 Gram eigenvalue), float
__device__ __forceinline__ float sigma_from_derivatives_f32(int layout, float a_, float b_, float c_, float d_, float e_,
                                                            float f_) {
#pragma clang fp contract(off)
    float p, q, r;
    if (layout == LC_LAYOUT_REFERENCE) {  // LCS.py:153 (Q13)
        p = __builtin_fmaf(c_, c_, __builtin_fmaf(b_, b_, a_ * a_));
        q = __builtin_fmaf(f_, f_, __builtin_fmaf(e_, e_, d_ * d_));
        r = __builtin_fmaf(c_, f_, __builtin_fmaf(b_, e_, a_ * d_));
    } else {
        p = __builtin_fmaf(e_, e_, __builtin_fmaf(c_, c_, a_ * a_));
        q = __builtin_fmaf(f_, f_, __builtin_fmaf(d_, d_, b_ * b_));
        r = __builtin_fmaf(e_, f_, __builtin_fmaf(c_, d_, a_ * b_));
    }
    const float dpq = p - q;
    // v_sqrt_f32 (1 ulp) instead of the correctly rounded expansion: 14 fewer instructions per root
    const float disc = __builtin_amdgcn_sqrtf(__builtin_fmaf(dpq, dpq, (4.0f * r) * r));
    return __builtin_amdgcn_sqrtf(0.5f * ((p + q) + disc));
}

// general float kernel (any width, any alignment): X, Y, Z of a 64 x 16 tile + halo through LDS
__device__ __forceinline__ void sigma_f32_body(const SigmaArgs<float> &A) {
    __shared__ GradientTileF32 tile;
    const int row_end = A.out_row0 + A.n_out_rows;
    int gy0, gx0;
    tile_origin(A.nx, A.out_row0, gy0, gx0);
    tile.stage(A.x_dep, A.y_dep, A.seed_lat, A.dlon, A.in_row0, A.n_in_rows, A.ny_global, A.nx, gy0, gx0, row_end);
    __syncthreads();

    const float inv_dy = inv_dy_f32(A.dlat);
    for_tile_cells(gy0, gx0, row_end, A.nx, [&](int oy, int ox, int gy, int gx) {
        float d[6];
        tile.derivatives(oy, ox, gy, A.ny_global, inv_dy, d);
        A.sigma[(size_t)(gy - A.out_row0) * A.nx + gx] = sigma_from_derivatives_f32(A.layout, d[0], d[1], d[2], d[3], d[4], d[5]);
    });
}
__global__ void __launch_bounds__(SBLOCK) sigma_kernel_f32(const SigmaArgs<float> A) { sigma_f32_body(A); }
__global__ void __launch_bounds__(SBLOCK) sigma_batch_kernel_f32(const SigmaArgs<float> A, size_t plane) {
    sigma_f32_body(sigma_member(A, plane));
}

// ======================================================================================
// float, sigma only, even width: the marching kernel.  A WAVE owns a span of 128 columns (two per lane, one 8-byte
// load per field and row) and walks down MROWS output rows with the X, Y, Z of five rows in registers: d/dy comes
// from the registers, d/dx from the two neighbouring lanes by wavefront shuffle (`ds_bpermute_b32`: 12 per row, no
// LDS memory, no barrier).  Lanes 0 and 63 are halo lanes (124 columns written per wave), rows -2..+2 around the
// strip are loaded as halo: the sincos work per output cell is 1.03 x (1 + 4/MROWS) instead of the LDS tile's 1.33.
// Five rows of loads are in flight per wave (a register ring indexed like the window).  Same arithmetic as sigma_kernel_f32, bit for bit.
// ======================================================================================
constexpr int MARCH_ROWS = 20;  // output rows a wave walks down (the kernels' MROWS)
constexpr int MBLOCK = 256;      // threads per workgroup of the marching kernel (waves are independent)
constexpr int MCOLS = 2;                 // columns per lane
constexpr int MSPAN_OUT = 62 * MCOLS;    // columns written per wave

template <int MROWS, int LAYOUT>
__device__ __forceinline__ void sigma_march_body(const SigmaArgs<float> &A, int nspans, int nstrips) {
    static_assert(MROWS <= 64, "row metrics live one per lane");
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * (MBLOCK / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform
    const int strip = w / nspans, span = w - strip * nspans;
    if (strip >= nstrips) return;
    const int gy0 = A.out_row0 + strip * MROWS;
    const int nrows = min(MROWS, A.out_row0 + A.n_out_rows - gy0);
    const int col = span * MSPAN_OUT + (lane - 1) * MCOLS;
    const bool writes = lane >= 1 && lane <= 62 && col < A.nx;
    int c = col < 0 ? col + A.nx : col;  // cyclic column of this lane's pair (tools.py:225-228); nx is even
    if (c >= A.nx) {
        c -= A.nx;
        if (c >= A.nx) c %= A.nx;
    }
    const int from_prev = ((lane + 63) & 63) * 4, from_next = ((lane + 1) & 63) * 4;  // bpermute byte addresses
    // 1/dx of this strip's rows, one per lane, broadcast by readlane in the loop
    float my_inv_dx = 0.0f;
    if (lane < nrows) my_inv_dx = inv_dx_f32(A.seed_lat[gy0 + lane - A.in_row0], A.dlon);
    const float inv_dy = inv_dy_f32(A.dlat);

    auto row_ok = [&](int gy) {  // wave-uniform
        const int ry = gy - A.in_row0;
        return gy >= 0 && gy < A.ny_global && ry >= 0 && ry < A.n_in_rows;
    };
    auto load_row = [&](int gy, float2 &xd, float2 &yd) {  // always issued (a row outside the window reads the nearest
        const int ry = min(max(gy - A.in_row0, 0), A.n_in_rows - 1);  // one and is zeroed below): no branch around loads
        const float *px = A.x_dep + (size_t)ry * A.nx, *py = A.y_dep + (size_t)ry * A.nx;
        xd = *reinterpret_cast<const float2 *>(px + c);
        yd = *reinterpret_cast<const float2 *>(py + c);
    };
    auto shuf = [&](int addr, float v) {
        return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(addr, __builtin_bit_cast(int, v)));
    };
    float X[5][MCOLS], Y[5][MCOLS], Z[5][MCOLS];  // rows gy-2 .. gy+2; slot = (row - first row) mod 5
    float2 RX[5], RY[5];                          // the next five rows as loaded: five rows of loads in flight per wave
    const int base = gy0 - 2;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        load_row(base + j, RX[j], RY[j]);
    }
    // rows enter in slot order, so with the loop unrolled by five every register index below is static and the
    // compiler counts the loads in flight itself (vmcnt)
    for (int o = 0; o * 5 - 4 < nrows; ++o) {
#pragma unroll
        for (int S4 = 0; S4 < 5; ++S4) {         // S4: slot of the entering row
            const int i = o * 5 + S4 - 4;        // output row gy0 + i once rows up to gy0 + i + 2 are in
            if (i < nrows) {                     // wave-uniform
                const int S0 = (S4 + 1) % 5, S1 = (S4 + 2) % 5, S2 = (S4 + 3) % 5, S3 = (S4 + 4) % 5;
                const int gyn = gy0 + i + 2;     // the row entering the window
                const float2 cx = RX[S4], cy = RY[S4];
                load_row(gyn + 5, RX[S4], RY[S4]);  // its ring slot goes to the row five further down
                if (row_ok(gyn)) {
                    sphere_xyz_f32(cx.x, cy.x, X[S4][0], Y[S4][0], Z[S4][0]);
                    sphere_xyz_f32(cx.y, cy.y, X[S4][1], Y[S4][1], Z[S4][1]);
                } else {
                    X[S4][0] = X[S4][1] = Y[S4][0] = Y[S4][1] = Z[S4][0] = Z[S4][1] = 0.0f;
                }
                if (i >= 0) {
                    const int gy = gy0 + i;
                    const float inv_dx = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, my_inv_dx), i));
                    const bool edge = gy < 2 || gy >= A.ny_global - 2;  // one-sided rows (Q12): wave-uniform, rare
                    float dxs[3][MCOLS], dys[3][MCOLS];
                    auto field = [&](float (&F)[5][MCOLS], int n) {
                        const float pk0 = shuf(from_prev, F[S2][0]), pk1 = shuf(from_prev, F[S2][1]);
                        const float nk0 = shuf(from_next, F[S2][0]), nk1 = shuf(from_next, F[S2][1]);
                        dxs[n][0] = centred_f32(F[S2][1], pk1, nk0, pk0) * inv_dx;
                        dxs[n][1] = centred_f32(nk0, F[S2][0], nk1, pk1) * inv_dx;
#pragma unroll
                        for (int k = 0; k < MCOLS; ++k) {
                            float d = centred_f32(F[S3][k], F[S1][k], F[S4][k], F[S0][k]);
                            if (edge) d = ddy_f32(gy, A.ny_global, F[S0][k], F[S1][k], F[S2][k], F[S3][k], F[S4][k]);
                            dys[n][k] = d * inv_dy;
                        }
                    };
                    field(X, 0);
                    field(Y, 1);
                    field(Z, 2);
                    float sig[MCOLS];
#pragma unroll
                    for (int k = 0; k < MCOLS; ++k)
                        sig[k] = sigma_from_derivatives_f32(LAYOUT, dxs[0][k], dys[0][k], dxs[1][k], dys[1][k], dxs[2][k], dys[2][k]);
                    if (writes)
                        *reinterpret_cast<float2 *>(A.sigma + (size_t)(gy - A.out_row0) * A.nx + col) = make_float2(sig[0], sig[1]);
                }
            }
        }
    }
}
template <int MROWS, int LAYOUT>
__global__ void __launch_bounds__(MBLOCK) sigma_march_kernel_f32(const SigmaArgs<float> A, int nspans, int nstrips) {
    sigma_march_body<MROWS, LAYOUT>(A, nspans, nstrips);
}
template <int MROWS, int LAYOUT>
__global__ void __launch_bounds__(MBLOCK) sigma_march_batch_kernel_f32(const SigmaArgs<float> A, int nspans, int nstrips, size_t plane) {
    sigma_march_body<MROWS, LAYOUT>(sigma_member(A, plane), nspans, nstrips);
}

// The kernel a call takes.  The marching kernel's waves walk MROWS + 4 rows one after the other: a latency floor of ~20 us
// whatever the size, so below 2^23 cells the LDS-tile kernel (more, shorter-lived workgroups) is the faster one
// (2048^2: 27.5 vs 29.2 us; 2896^2: 50.9 vs 43.2).  sigma_march 1 forces it (tests, A/B), 2 = by size.  It needs float,
// sigma only, an even width and 8-byte aligned planes (in a batch the plane is even with nx: every member's planes keep
// the base's alignment).
enum SigmaRoute { SIGMA_MARCH, SIGMA_TILE_F32, SIGMA_TILE_TYPED };
template <typename T>
SigmaRoute sigma_route(const lc_ctx *ctx, const SigmaArgs<T> &A) {
    if (sizeof(T) != 4 || A.tensor) return SIGMA_TILE_TYPED;
    const bool march = ctx->sigma_march == 1 || (ctx->sigma_march == 2 && (long long)A.nx * A.n_out_rows >= (1ll << 23));
    const bool aligned = (((uintptr_t)A.x_dep | (uintptr_t)A.y_dep | (uintptr_t)A.sigma) & 7) == 0;
    return A.nx % MCOLS == 0 && A.nx >= 2 * MCOLS && march && aligned ? SIGMA_MARCH : SIGMA_TILE_F32;
}

// lc_sigma and lc_flowmap_gradient (n_members 0: a row window, sigma and/or the tensor) and lc_sigma_batch (n_members >= 1
// whole grids [n_members][ny*nx] in one launch, grid.y = member): one argument fill, one kernel choice, so each plane of a
// batch goes through the kernel and the arithmetic lc_sigma chooses for it alone.
template <typename T>
int sigma_impl(lc_ctx *ctx, const void *x_dep, const void *y_dep, int in_row0, int n_in_rows, int nx, int ny_global,
               const void *seed_lat, double dlat, double dlon, int fd_fp32_cast, int layout, int out_row0,
               int n_out_rows, void *sigma_out, void *tensor_out, int n_members) {
    SigmaArgs<T> A;
    A.x_dep = (const T *)x_dep;
    A.y_dep = (const T *)y_dep;
    A.seed_lat = (const T *)seed_lat;
    A.in_row0 = in_row0;
    A.n_in_rows = n_in_rows;
    A.nx = nx;
    A.ny_global = ny_global;
    A.dlat = (T)dlat;
    A.dlon = (T)dlon;
    A.layout = layout;
    A.out_row0 = out_row0;
    A.n_out_rows = n_out_rows;
    A.sigma = (T *)sigma_out;
    A.tensor = (T *)tensor_out;
    const bool batch = n_members > 0;
    const size_t plane = (size_t)n_out_rows * nx;
    // `single`, or `batched` with the member in grid.y and the plane stride as its last argument
    auto launch = [&](auto single, auto batched, int blocks, int threads, const char *name, const char *batch_name, auto... extra) {
        ctx->last_sigma_kernel = batch ? batch_name : name;
        if (batch)
            hipLaunchKernelGGL(batched, dim3(blocks, n_members), dim3(threads), 0, ctx->stream, A, extra..., plane);
        else
            hipLaunchKernelGGL(single, dim3(blocks), dim3(threads), 0, ctx->stream, A, extra...);
    };
    const int tiles = ((nx + SW - 1) / SW) * ((n_out_rows + SH - 1) / SH);
    const SigmaRoute route = sigma_route(ctx, A);
    if constexpr (sizeof(T) == 4) {
        if (route == SIGMA_MARCH) {
            constexpr int MROWS = MARCH_ROWS;
            const int nspans = (nx + MSPAN_OUT - 1) / MSPAN_OUT, nstrips = (n_out_rows + MROWS - 1) / MROWS;
            const int blocks = (nspans * nstrips + MBLOCK / 64 - 1) / (MBLOCK / 64);
            if (layout == LC_LAYOUT_REFERENCE)
                launch(sigma_march_kernel_f32<MROWS, LC_LAYOUT_REFERENCE>, sigma_march_batch_kernel_f32<MROWS, LC_LAYOUT_REFERENCE>,
                       blocks, MBLOCK, "sigma_march_kernel_f32", "sigma_march_batch_kernel_f32", nspans, nstrips);
            else
                launch(sigma_march_kernel_f32<MROWS, LC_LAYOUT_PHYSICAL>, sigma_march_batch_kernel_f32<MROWS, LC_LAYOUT_PHYSICAL>,
                       blocks, MBLOCK, "sigma_march_kernel_f32", "sigma_march_batch_kernel_f32", nspans, nstrips);
        } else if (route == SIGMA_TILE_F32) {
            launch(sigma_kernel_f32, sigma_batch_kernel_f32, tiles, SBLOCK, "sigma_kernel_f32", "sigma_batch_kernel_f32");
        } else {  // the tensor: never a batch
            ctx->last_sigma_kernel = "sigma_kernel<float, float>";
            hipLaunchKernelGGL((sigma_kernel<T, float>), dim3(tiles), dim3(SBLOCK), 0, ctx->stream, A);
        }
    } else if (fd_fp32_cast) {
        launch(sigma_kernel<T, float>, sigma_batch_kernel<T, float>, tiles, SBLOCK, "sigma_kernel<double, float>",
               "sigma_batch_kernel<double, float>");
    } else {
        launch(sigma_kernel<T, double>, sigma_batch_kernel<T, double>, tiles, SBLOCK, "sigma_kernel<double, double>",
               "sigma_batch_kernel<double, double>");
    }
    LC_HIP_CHECK(hipGetLastError());
    return LC_OK;
}

// tools.fourth_order_derivative on its own (LCS/tools.py:190-245): index-space stencil on a 2-D array, numba typing
// (flowmap_gradient.h's centred and one_sided).  dim 1: cyclic in longitude when isglobal (:220-228), else the one-sided
// difference / 2 on the two first and two last columns (:229-244), as dim 0 always does on its rows (:210-217).
template <typename S>
__global__ void index_derivative_kernel(const S *__restrict__ a, S *__restrict__ out, int ny, int nx, int dim, int isglobal) {
    const size_t n = (size_t)ny * nx;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int y = (int)(i / nx), x = (int)(i - (size_t)y * nx);
        S r;
        if (dim == 0) {
            if (y < 2)
                r = one_sided(a[i + nx], a[i]);
            else if (y >= ny - 2)
                r = one_sided(a[i], a[i - nx]);
            else
                r = centred(a[i + nx], a[i - nx], a[i + 2 * (size_t)nx], a[i - 2 * (size_t)nx]);
        } else if (isglobal) {
            const S *row = a + (size_t)y * nx;
            r = centred(row[(x + 1) % nx], row[(x - 1 + nx) % nx], row[(x + 2) % nx], row[(x - 2 + nx) % nx]);
        } else {
            if (x < 2)
                r = one_sided(a[i + 1], a[i]);
            else if (x >= nx - 2)
                r = one_sided(a[i], a[i - 1]);
            else
                r = centred(a[i + 1], a[i - 1], a[i + 2], a[i - 2]);
        }
        out[i] = r;
    }
}

}  // namespace

extern "C" int lc_fourth_order_derivative(lc_ctx *ctx, const void *in_dev, int dtype, int ny, int nx, int dim,
                                          int isglobal, void *out_dev) {
    LC_REQUIRE(ctx, "lc_fourth_order_derivative: null context");
    LC_REQUIRE(dtype == LC_F32 || dtype == LC_F64, "lc_fourth_order_derivative: bad dtype %d", dtype);
    LC_REQUIRE(in_dev && out_dev && in_dev != out_dev, "lc_fourth_order_derivative: bad pointers");
    LC_REQUIRE(ny >= 5 && nx >= 5, "lc_fourth_order_derivative: grid %dx%d too small", ny, nx);
    LC_REQUIRE(dim == 0 || dim == 1, "Dim must be either 0 or 1.");
    LC_HIP_CHECK(hipSetDevice(ctx->device));
    const size_t n = (size_t)ny * nx;
    const int blocks = (int)((n + 255) / 256 < 8192 ? (n + 255) / 256 : 8192);
    if (dtype == LC_F32)
        hipLaunchKernelGGL(index_derivative_kernel<float>, dim3(blocks), dim3(256), 0, ctx->stream,
                           (const float *)in_dev, (float *)out_dev, ny, nx, dim, isglobal != 0);
    else
        hipLaunchKernelGGL(index_derivative_kernel<double>, dim3(blocks), dim3(256), 0, ctx->stream,
                           (const double *)in_dev, (double *)out_dev, ny, nx, dim, isglobal != 0);
    LC_HIP_CHECK(hipGetLastError());
    return LC_OK;
}

extern "C" int lc_sigma(lc_ctx *ctx, const void *x_dep, const void *y_dep, int dtype, int in_row0, int n_in_rows,
                        int nx, int ny_global, const void *seed_lat_dev, double dlat, double dlon, int fd_fp32_cast,
                        int tensor_layout, int out_row0, int n_out_rows, void *sigma_out) {
    LC_REQUIRE(ctx, "lc_sigma: null context");
    LC_REQUIRE(dtype == LC_F32 || dtype == LC_F64, "lc_sigma: bad dtype %d", dtype);
    LC_REQUIRE(x_dep && y_dep && seed_lat_dev && sigma_out, "lc_sigma: null pointer");
    LC_REQUIRE(nx >= 5 && ny_global >= 5, "lc_sigma: grid %dx%d too small for the 5-point stencil", ny_global, nx);
    LC_REQUIRE(tensor_layout == LC_LAYOUT_REFERENCE || tensor_layout == LC_LAYOUT_PHYSICAL, "lc_sigma: bad layout");
    LC_REQUIRE(n_in_rows >= 1 && in_row0 >= 0 && in_row0 + n_in_rows <= ny_global, "lc_sigma: bad input window");
    LC_REQUIRE(n_out_rows >= 1 && out_row0 >= in_row0 && out_row0 + n_out_rows <= in_row0 + n_in_rows,
               "lc_sigma: output rows outside the input window");
    // every output row needs r-2..r+2 unless the global one-sided rule covers it
    const int need_lo = out_row0 < 2 ? 0 : out_row0 - 2;
    const int last = out_row0 + n_out_rows - 1;
    const int need_hi = last >= ny_global - 2 ? ny_global - 1 : last + 2;
    LC_REQUIRE(in_row0 <= need_lo && in_row0 + n_in_rows - 1 >= need_hi,
               "lc_sigma: rows [%d,%d] need halo rows [%d,%d] but the input holds [%d,%d]", out_row0, last, need_lo,
               need_hi, in_row0, in_row0 + n_in_rows - 1);
    LC_HIP_CHECK(hipSetDevice(ctx->device));
    if (dtype == LC_F32)
        return sigma_impl<float>(ctx, x_dep, y_dep, in_row0, n_in_rows, nx, ny_global, seed_lat_dev, dlat, dlon,
                                 fd_fp32_cast, tensor_layout, out_row0, n_out_rows, sigma_out, nullptr, 0);
    return sigma_impl<double>(ctx, x_dep, y_dep, in_row0, n_in_rows, nx, ny_global, seed_lat_dev, dlat, dlon,
                              fd_fp32_cast, tensor_layout, out_row0, n_out_rows, sigma_out, nullptr, 0);
}

extern "C" int lc_sigma_batch(lc_ctx *ctx, const void *x_dep, const void *y_dep, int dtype, int ny, int nx, const void *seed_lat_dev,
                              double dlat, double dlon, int fd_fp32_cast, int tensor_layout, int n_members, void *sigma_out) {
    LC_REQUIRE(ctx, "lc_sigma_batch: null context");
    LC_REQUIRE(dtype == LC_F32 || dtype == LC_F64, "lc_sigma_batch: bad dtype %d", dtype);
    LC_REQUIRE(x_dep && y_dep && seed_lat_dev && sigma_out, "lc_sigma_batch: null pointer");
    LC_REQUIRE(nx >= 5 && ny >= 5, "lc_sigma_batch: grid %dx%d too small for the 5-point stencil", ny, nx);
    LC_REQUIRE(tensor_layout == LC_LAYOUT_REFERENCE || tensor_layout == LC_LAYOUT_PHYSICAL, "lc_sigma_batch: bad layout");
    LC_REQUIRE(n_members >= 1 && n_members <= 65535, "lc_sigma_batch: bad n_members %d", n_members);
    LC_HIP_CHECK(hipSetDevice(ctx->device));
    if (dtype == LC_F32)  // every plane: the whole grid as its window
        return sigma_impl<float>(ctx, x_dep, y_dep, 0, ny, nx, ny, seed_lat_dev, dlat, dlon, fd_fp32_cast, tensor_layout, 0, ny,
                                 sigma_out, nullptr, n_members);
    return sigma_impl<double>(ctx, x_dep, y_dep, 0, ny, nx, ny, seed_lat_dev, dlat, dlon, fd_fp32_cast, tensor_layout, 0, ny,
                              sigma_out, nullptr, n_members);
}

extern "C" int lc_flowmap_gradient(lc_ctx *ctx, const void *x_dep, const void *y_dep, int dtype, int ny, int nx,
                                   const void *seed_lat_dev, double dlat, double dlon, int fd_fp32_cast,
                                   void *def_tensor_out) {
    LC_REQUIRE(ctx, "lc_flowmap_gradient: null context");
    LC_REQUIRE(dtype == LC_F32 || dtype == LC_F64, "lc_flowmap_gradient: bad dtype %d", dtype);
    LC_REQUIRE(x_dep && y_dep && seed_lat_dev && def_tensor_out, "lc_flowmap_gradient: null pointer");
    LC_REQUIRE(nx >= 5 && ny >= 5, "lc_flowmap_gradient: grid %dx%d too small for the 5-point stencil", ny, nx);
    LC_HIP_CHECK(hipSetDevice(ctx->device));
    if (dtype == LC_F32)
        return sigma_impl<float>(ctx, x_dep, y_dep, 0, ny, nx, ny, seed_lat_dev, dlat, dlon, fd_fp32_cast,
                                 LC_LAYOUT_REFERENCE, 0, ny, nullptr, def_tensor_out, 0);
    return sigma_impl<double>(ctx, x_dep, y_dep, 0, ny, nx, ny, seed_lat_dev, dlat, dlon, fd_fp32_cast,
                              LC_LAYOUT_REFERENCE, 0, ny, nullptr, def_tensor_out, 0);
}
