// Thinning and dilation of ridge masks: the device side of tools.skeletonize_ridges and tools.dilate_ridges, the two
// morphological steps of LCS/area_of_influence.py:207 and :233; pinned exactly against a numpy restatement and scipy in
// tests/test_skeleton_gpu.py.
//
// Both are iterated 3x3 neighbourhood rules on a 0/1 byte plane, n_members planes per launch:
//   intake  the float32 / float64 mask to one byte per pixel (1: != 0 and not NaN)
//   step    one workgroup per (plane, tile of MO_TH x MO_TW pixels).  It stages the tile and a halo of MO_HALO pixels as an
//           image of MO_LH rows of MO_LW bytes in LDS (columns wrap at the seam when cyclic, everything else outside the
//           plane is background) and performs up to MO_HALO whole-image sub-steps on it, ping-ponging between two LDS
//           images; every sub-step spoils one more ring of the image from its edge inwards -- the neighbours beyond the
//           edge are not there -- so after MO_HALO of them exactly the tile itself is still what the whole plane would
//           hold, and that is what it writes to the other global buffer.
//             thinning  a sub-step deletes the foreground pixels whose neighbourhood index
//                       NW + 2 N + 4 NE + 8 E + 16 SE + 32 S + 64 SW + 128 W has its bit in the table of that sub-iteration
//                       (256 bits, 8 dwords of LDS: a wave's lookups hit 8 distinct dwords in 8 banks, never a conflict);
//                       a launch starts with a first sub-iteration and does whole iterations, MO_HALO / 2 at most
//             dilation  a sub-step sets the in-plane pixels whose index has a bit of the structure
//           A thread owns one dword (4 pixels) of MO_ROWS consecutive image rows and slides a 3-row window down them:
//           3 LDS dword reads per 4 pixels, each row of 32 lanes reading 32 consecutive dwords (no bank conflict).
//   flags   every workgroup stores, with a plain store into its own slot, whether the tile it wrote differs from the tile
//           it read; one more workgroup ORs the slots into one word, which the call reads back after each launch and stops
//           when it is 0: a fixed point stays fixed, so whatever a launch does beyond it is harmless.  One synchronisation
//           per launch, i.e. per MO_HALO / 2 thinning iterations.
// The result does not depend on the tile, the halo or iterations_per_launch: they only cut the same sequence of whole-plane
// sub-iterations into launches.
// What bounds the step: LDS traffic and integer VALU work on bytes (about 30 operations per pixel and sub-step); the global
// traffic is two bytes per pixel and launch.
// No kernel waits for another workgroup: there is no look-back, no atomic and no grid synchronisation in this file -- what
// one launch needs from the one before is handed over by the end of that launch.
#include <climits>
#include <cstdint>

#include "lcs_common.h"

namespace {

constexpr int MO_THREADS = 256;
constexpr int MO_HALO = 8;                       // sub-steps one launch can do
constexpr int MO_TW = 112, MO_TH = 48;           // the tile
constexpr int MO_LW = MO_TW + 2 * MO_HALO;       // 128 bytes = 32 dwords: one row per half wave
constexpr int MO_LH = MO_TH + 2 * MO_HALO;       // 64 rows; two images: 16 KiB of LDS, the wave limit (8 workgroups) binds first
constexpr int MO_WW = MO_LW / 4;                 // dwords of an image row
constexpr int MO_ROWS = MO_LH / (MO_THREADS / MO_WW);   // image rows a thread walks: 8
static_assert(MO_LW % 4 == 0 && MO_HALO % 4 == 0 && MO_HALO % 2 == 0 && MO_THREADS % MO_WW == 0 && MO_LH % (MO_THREADS / MO_WW) == 0, "tile");

template <typename T>
__device__ __forceinline__ bool foreground(T v) {
    return v != (T)0 && v == v;   // as components.hip: NaN is background, a negative value is foreground
}

template <typename T>
__global__ __launch_bounds__(MO_THREADS) void mo_intake_kernel(const T *__restrict__ mask, uint8_t *__restrict__ out, size_t n) {
    const size_t i = (size_t)blockIdx.x * MO_THREADS + threadIdx.x;
    if (i < n) out[i] = foreground(mask[i]) ? 1 : 0;
}

struct Step {
    const uint8_t *in;    // [n_members][ny][nx], 0 / 1
    uint8_t *out;
    int *flags;           // [n_members * tiles_y * tiles_x]
    int ny, nx, tiles_y, tiles_x;
    int cyclic;
    int substeps;         // 1 .. MO_HALO; thinning: even
    unsigned structure;   // dilation: the neighbours that set a pixel, in the bits of the neighbourhood index
    uint32_t bits[2][8];  // thinning: bit i of [s] = delete at index i in sub-iteration s
};

// bytes 0..5 of the result: columns 4 cw - 1 .. 4 cw + 4 of image row r; what lies outside the image is 0 (it only reaches
// pixels the halo has given up)
__device__ __forceinline__ uint64_t strip(const uint32_t *img, int r, int cw) {
    if (r < 0 || r >= MO_LH) return 0;
    const uint32_t *row = img + r * MO_WW;
    const uint32_t l = cw > 0 ? row[cw - 1] : 0u, c = row[cw], e = cw < MO_WW - 1 ? row[cw + 1] : 0u;
    return (uint64_t)(l >> 24) | ((uint64_t)c << 8) | ((uint64_t)(e & 0xffu) << 40);
}

enum { MO_THIN = 0, MO_DILATE = 1 };

template <int OP>
__global__ __launch_bounds__(MO_THREADS) void mo_step_kernel(Step a) {
    __shared__ uint32_t s_img[2][MO_LH * MO_WW];
    __shared__ uint32_t s_bits[2][8];
    const int tid = threadIdx.x;
    const int per_plane = a.tiles_y * a.tiles_x;
    const int m = blockIdx.x / per_plane, rest = blockIdx.x - m * per_plane;
    const int ty = rest / a.tiles_x, tx = rest - ty * a.tiles_x;
    const int r0 = ty * MO_TH - MO_HALO, c0 = tx * MO_TW - MO_HALO;   // the image's first row and column in the plane
    const size_t plane = (size_t)m * (size_t)a.ny * (size_t)a.nx;
    const uint8_t *in = a.in + plane;

    if (OP == MO_THIN && tid < 16) s_bits[tid >> 3][tid & 7] = a.bits[tid >> 3][tid & 7];
    for (int w = tid; w < MO_LH * MO_WW; w += MO_THREADS) {
        const int lr = w / MO_WW, gr = r0 + lr, gc = c0 + 4 * (w - lr * MO_WW);
        uint32_t v = 0;
        if (gr >= 0 && gr < a.ny) {
            const uint8_t *row = in + (size_t)gr * a.nx;
            if (gc >= 0 && gc + 3 < a.nx && (((uintptr_t)(row + gc)) & 3) == 0) {
                v = *(const uint32_t *)(row + gc);
            } else {
                for (int b = 0; b < 4; ++b) {
                    int c = gc + b;
                    if (a.cyclic) {
                        c %= a.nx;
                        if (c < 0) c += a.nx;
                    }
                    if (c >= 0 && c < a.nx) v |= (uint32_t)row[c] << (8 * b);
                }
            }
        }
        s_img[0][w] = v;
    }
    __syncthreads();

    const int cw = tid % MO_WW, rg = (tid / MO_WW) * MO_ROWS;
    uint32_t colmask = 0;   // dilation: the bytes of this thread's dword that are columns of the plane
    if (OP == MO_DILATE)
        for (int b = 0; b < 4; ++b) {
            const int c = c0 + 4 * cw + b;
            if (a.cyclic || (c >= 0 && c < a.nx)) colmask |= 1u << (8 * b);
        }
    for (int s = 0; s < a.substeps; ++s) {
        const uint32_t *src = s_img[s & 1];
        uint32_t *dst = s_img[(s & 1) ^ 1];
        const uint32_t *bits = s_bits[s & 1];
        uint64_t up = strip(src, rg - 1, cw), mid = strip(src, rg, cw);
        for (int k = 0; k < MO_ROWS; ++k) {
            const int lr = rg + k;
            const uint64_t down = strip(src, lr + 1, cw);
            uint32_t word = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const unsigned u = (unsigned)(up >> (8 * b)), c = (unsigned)(mid >> (8 * b)), d = (unsigned)(down >> (8 * b));
                // bytes 0, 1, 2 of u / c / d: west, centre, east of the rows above, of and below the pixel
                const unsigned idx = (u & 1u) | ((u >> 7) & 2u) | ((u >> 14) & 4u) | ((c >> 13) & 8u) | ((d >> 12) & 16u) |
                                     ((d >> 3) & 32u) | ((d << 6) & 64u) | ((c << 7) & 128u);
                const unsigned centre = (c >> 8) & 1u;
                unsigned nv;
                if (OP == MO_THIN)
                    nv = centre & ~(bits[idx >> 5] >> (idx & 31u));
                else
                    nv = centre | ((idx & a.structure) != 0u ? 1u : 0u);
                word |= (nv & 1u) << (8 * b);
            }
            if (OP == MO_DILATE) {
                const int gr = r0 + lr;
                word = gr >= 0 && gr < a.ny ? word & colmask : 0u;
            }
            dst[lr * MO_WW + cw] = word;
            up = mid;
            mid = down;
        }
        __syncthreads();
    }

    const uint32_t *fin = s_img[a.substeps & 1];
    uint8_t *out = a.out + plane;
    int changed = 0;
    constexpr int TWW = MO_TW / 4;
    for (int w = tid; w < MO_TH * TWW; w += MO_THREADS) {
        const int tr = w / TWW, tw = w - tr * TWW;
        const int gr = r0 + MO_HALO + tr, gc = c0 + MO_HALO + 4 * tw;
        if (gr >= a.ny || gc >= a.nx) continue;
        const uint32_t v = fin[(tr + MO_HALO) * MO_WW + tw + MO_HALO / 4];
        const size_t p = (size_t)gr * a.nx + gc;
        if (gc + 3 < a.nx && (((uintptr_t)(out + p)) & 3) == 0 && (((uintptr_t)(in + p)) & 3) == 0) {
            changed |= *(const uint32_t *)(in + p) != v;
            *(uint32_t *)(out + p) = v;
        } else {
            for (int b = 0; b < 4 && gc + b < a.nx; ++b) {
                const uint8_t nv = (uint8_t)((v >> (8 * b)) & 1u);
                changed |= in[p + b] != nv;
                out[p + b] = nv;
            }
        }
    }
    changed = __syncthreads_or(changed);
    if (tid == 0) a.flags[blockIdx.x] = changed;
}

// one workgroup: any[0] = whether a slot of flags is set
__global__ __launch_bounds__(MO_THREADS) void mo_any_kernel(const int *__restrict__ flags, int n, int *__restrict__ any) {
    int set = 0;
    for (int i = threadIdx.x; i < n; i += MO_THREADS) set |= flags[i];
    set = __syncthreads_or(set);
    if (threadIdx.x == 0) any[0] = set != 0;
}

constexpr int MO_HEAD = 4;   // int32 in front of the flags: the word the call reads back

long long tiles_of(int ny, int nx) {
    return (((long long)ny + MO_TH - 1) / MO_TH) * (((long long)nx + MO_TW - 1) / MO_TW);
}

}  // namespace

extern "C" size_t lc_morph_work_elems(int ny, int nx, int n_members) {
    if (ny < 1 || nx < 1 || n_members < 1) return 0;
    const unsigned long long bytes = (unsigned long long)ny * (unsigned long long)nx * (unsigned long long)n_members;
    return (size_t)(MO_HEAD + (unsigned long long)tiles_of(ny, nx) * (unsigned long long)n_members + (bytes + 3) / 4);
}

extern "C" int lc_mask_morphology(lc_ctx *ctx, const lc_morph_args *a) {
    const char *who = "lc_mask_morphology";
    LC_REQUIRE(ctx, "%s: null context", who);
    LC_REQUIRE(a, "%s: null argument structure", who);
    LC_REQUIRE(a->struct_size == sizeof(lc_morph_args), "%s: struct_size %zu, this library has %zu", who, (size_t)a->struct_size,
               sizeof(lc_morph_args));
    LC_REQUIRE(a->op == LC_MORPH_THIN || a->op == LC_MORPH_DILATE, "%s: bad op %d (LC_MORPH_THIN or LC_MORPH_DILATE)", who, a->op);
    LC_REQUIRE(a->dtype == LC_F32 || a->dtype == LC_F64, "%s: bad dtype %d (LC_F32 or LC_F64)", who, a->dtype);
    LC_REQUIRE(a->ny >= 1 && a->nx >= 1 && a->n_members >= 1, "%s: bad size ny=%d nx=%d n_members=%d (each >= 1)", who, a->ny, a->nx,
               a->n_members);
    const long long npix = (long long)a->ny * a->nx;
    LC_REQUIRE(npix < (1ll << 31), "%s: plane too large: %d x %d = %lld pixels (< 2^31)", who, a->ny, a->nx, npix);
    const long long tiles = tiles_of(a->ny, a->nx) * a->n_members;
    LC_REQUIRE(tiles <= (long long)INT_MAX && (npix * a->n_members + MO_THREADS - 1) / MO_THREADS <= (long long)INT_MAX,
               "%s: too many planes: %d of %d x %d", who, a->n_members, a->ny, a->nx);
    const bool thin = a->op == LC_MORPH_THIN;
    const int per_launch_max = thin ? MO_HALO / 2 : MO_HALO;
    LC_REQUIRE(a->iterations_per_launch >= 0 && a->iterations_per_launch <= per_launch_max,
               "%s: bad iterations_per_launch %d (0: the default, or 1 .. %d for this op)", who, a->iterations_per_launch, per_launch_max);
    Step s = {};
    if (thin) {
        LC_REQUIRE(a->table, "%s: null thinning table", who);
        for (int i = 0; i < 256; ++i) {
            const unsigned code = a->table[i];
            LC_REQUIRE(code <= 3u, "%s: bad thinning table: code %u at index %d (0 .. 3)", who, code, i);
            if (code & 1u) s.bits[0][i >> 5] |= 1u << (i & 31);
            if (code & 2u) s.bits[1][i >> 5] |= 1u << (i & 31);
        }
    } else {
        LC_REQUIRE(a->structure >= 1 && a->structure <= 255, "%s: bad structure %d (bits of the eight neighbours, 1 .. 255)", who, a->structure);
        LC_REQUIRE(a->max_iterations >= 1, "%s: bad iterations %d for a dilation (>= 1)", who, a->max_iterations);
    }
    LC_REQUIRE(a->mask && a->out && a->work_dev, "%s: null pointer", who);
    LC_HIP_CHECK(hipSetDevice(ctx->device));

    const size_t total = (size_t)npix * (size_t)a->n_members;
    int *any = (int *)a->work_dev, *flags = any + MO_HEAD;
    uint8_t *buf[2] = {(uint8_t *)a->out, (uint8_t *)(flags + tiles)};
    const dim3 block(MO_THREADS), pixels((unsigned)((total + MO_THREADS - 1) / MO_THREADS));
    if (a->dtype == LC_F32)
        hipLaunchKernelGGL(mo_intake_kernel<float>, pixels, block, 0, ctx->stream, (const float *)a->mask, buf[0], total);
    else
        hipLaunchKernelGGL(mo_intake_kernel<double>, pixels, block, 0, ctx->stream, (const double *)a->mask, buf[0], total);

    s.flags = flags;
    s.ny = a->ny;
    s.nx = a->nx;
    s.tiles_y = (a->ny + MO_TH - 1) / MO_TH;
    s.tiles_x = (a->nx + MO_TW - 1) / MO_TW;
    s.cyclic = a->cyclic_x ? 1 : 0;
    s.structure = (unsigned)a->structure;
    // iterations still allowed; unbounded thinning ends at a fixed point, which no plane is further from than its pixels
    long long left = a->max_iterations >= 1 ? (long long)a->max_iterations : npix + 1;
    const int per_launch = a->iterations_per_launch ? a->iterations_per_launch : per_launch_max;
    int cur = 0, launches = 0;
    for (int set = 1; left > 0 && set; ++launches) {
        const int it = left < per_launch ? (int)left : per_launch;
        left -= it;
        s.in = buf[cur];
        s.out = buf[cur ^ 1];
        s.substeps = thin ? 2 * it : it;
        if (thin)
            hipLaunchKernelGGL(mo_step_kernel<MO_THIN>, dim3((unsigned)tiles), block, 0, ctx->stream, s);
        else
            hipLaunchKernelGGL(mo_step_kernel<MO_DILATE>, dim3((unsigned)tiles), block, 0, ctx->stream, s);
        cur ^= 1;
        if (left == 0) continue;   // the last launch: nobody asks whether it changed anything
        hipLaunchKernelGGL(mo_any_kernel, dim3(1), block, 0, ctx->stream, flags, (int)tiles, any);
        LC_HIP_CHECK(hipGetLastError());
        LC_HIP_CHECK(hipMemcpyAsync(&set, any, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        LC_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    }
    if (cur != 0) LC_HIP_CHECK(hipMemcpyAsync(buf[0], buf[1], total, hipMemcpyDeviceToDevice, ctx->stream));
    LC_HIP_CHECK(hipGetLastError());
    if (a->launches_out) *a->launches_out = launches;
    return LC_OK;
}
