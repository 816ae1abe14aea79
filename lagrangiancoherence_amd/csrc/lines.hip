// Thinned ridges as ordered lines: the device side of Engine.trace_lines / tools.ridge_lines.  Nothing in the reference computes
// it -- its chain ends at rasters (LCS/area_of_influence.py) -- so the meaning is fixed in include/lcs_hip.h and restated as a plain
// pixel walk in tests/lines.py, against which tests/test_lines_gpu.py pins every integer exactly.
//
// n_members independent planes per call, every launch for all of them, one thread per pixel (LN_TILE pixels per workgroup) or
// per state:
//   links   the foreground of a pixel's 3 x 3 neighbourhood straight from the mask -> its link byte (bit k: linked to the
//           neighbour in direction k = NW, N, NE, E, SE, S, SW, W) and the plane's counts of foreground pixels, interior pixels
//           (degree 2), nodes and links (integer atomics: no order of arrival changes them)
//   init    an interior pixel q with links a < b carries two STATES, 2 q + 0 "leaves through a" and 2 q + 1 "leaves through b"
//           (having arrived through the other).  A state holds (next, hops, n_diag, smallest dart id) and the length of what
//           it has covered, at first the one link it leaves by.  Its head is the pixel that link leads to: a node ends the
//           state at once (next = -(dart that leaves the node back along the line) - 1), an interior head h gives
//           next = the state of h that does not return.
//   round   pointer doubling, double-buffered: a state whose next is a state t takes t's values on top of its own and t's
//           next.  After r rounds a state has covered 2^r links or ended at a node.
//   rings   what has not ended once 2^r >= the largest interior count of a plane lies on a ring, and the smaller of the two
//           minima of a pixel's states is the ring's smallest dart, which leaves the ring's first pixel p0 in raster order.
//           `break` starts those states again with p0 as if it were a node; further rounds rank them as an open chain.
//   finish  per interior pixel, from the ends e0, e1 its two states reached: the line's key min(e0, e1), the canonical way
//           (state j runs it when the other one ended at the key), and the other state's hops, n_diag and length, which are the
//           pixel's position, the corner links and the distance before it.
// Convergence is found by the host side as lc_mask_morphology finds it: every launch that can leave a state unfinished ORs
// one word of its own, which the call reads back.  At most 2 ceil(log2(I)) rounds for I interior pixels.
// What bounds it, read from the code and NOT measured yet: the round is a dependent gather -- 16 bytes of the state itself,
// then 16 + 8 bytes at an address only that load reveals -- over slots of which a thinned mask fills a few per cent, so it is
// latency- and request-bound, not bandwidth-bound; hence one state per lane and 256 lanes per workgroup, with a handful of
// registers, so that every CU holds its full count of waves to hide the two round trips.  The per-pixel kernels read the plane
// once.
// No kernel waits for another workgroup: there is no look-back, no spin and no grid synchronisation in this file -- what one
// launch needs from the one before is handed over by the end of that launch.  The atomics are ordinary ones in plain C++.
#include <climits>
#include <cmath>
#include <cstdint>
#include <vector>

#include "lcs_common.h"

namespace {

constexpr int LN_THREADS = 256;
constexpr int LN_TILE = LN_THREADS;   // pixels (or states) of one workgroup
constexpr int LN_HEAD = 128;          // int32 in front of the states: the words the call reads back, one per reporting launch
constexpr int LN_INVALID = INT_MIN;   // next of a slot that is no state (the pixel is not interior)

template <typename T>
__device__ __forceinline__ bool foreground(T v) {
    return v != (T)0 && v == v;   // as components.hip: NaN is background, a negative value is foreground
}

struct Plane {
    int ny, nx, npix, cyclic;
    int blocks_per_plane;   // workgroups of LN_TILE pixels
};

// the two halves of a state: 16 bytes that travel together, and the length
struct State {
    int next;   // >= 0: a state of the same plane; < 0: ended, -(next) - 1 is the dart that leaves the end node back along the line
    int hops;   // links covered
    int diag;   // corner links among them
    int low;    // smallest dart id among them; -1 once the state is known to lie on a ring
};

__device__ __forceinline__ int row_step(int k) { return k < 3 ? -1 : (k == 3 || k == 7 ? 0 : 1); }
__device__ __forceinline__ int col_step(int k) { return (k == 0 || k >= 6) ? -1 : (k == 1 || k == 5 ? 0 : 1); }

// the pixel in direction k of (r, c), or -1 outside the plane
__device__ __forceinline__ int neighbour(const Plane &g, int r, int c, int k) {
    const int rr = r + row_step(k);
    int cc = c + col_step(k);
    if (g.cyclic) cc = cc < 0 ? cc + g.nx : (cc >= g.nx ? cc - g.nx : cc);
    if (rr < 0 || rr >= g.ny || cc < 0 || cc >= g.nx) return -1;
    return rr * g.nx + cc;
}

__device__ __forceinline__ bool pixel_of_block(const Plane &g, int *m, int *p) {
    *m = blockIdx.x / g.blocks_per_plane;
    const long long q = (long long)(blockIdx.x - *m * g.blocks_per_plane) * LN_TILE + threadIdx.x;
    *p = (int)q;
    return q < g.npix;
}

template <typename T>
__global__ __launch_bounds__(LN_THREADS) void ln_links_kernel(const T *__restrict__ mask, Plane g, uint8_t *__restrict__ links,
                                                              int *__restrict__ counts) {
    __shared__ int s_count[4];
    if (threadIdx.x < 4) s_count[threadIdx.x] = 0;
    __syncthreads();
    int m, p;
    const bool valid = pixel_of_block(g, &m, &p);
    if (valid) {
        const T *plane = mask + (size_t)m * (size_t)g.npix;
        unsigned bits = 0;
        if (foreground(plane[p])) {
            const int r = p / g.nx, c = p - r * g.nx;
            unsigned fg = 0;
            for (int k = 0; k < 8; ++k) {
                const int q = neighbour(g, r, c, k);
                if (q >= 0 && foreground(plane[q])) fg |= 1u << k;
            }
            // an edge neighbour links; a corner neighbour only if neither of the two edge neighbours beside it is foreground
            bits = fg & 0xAAu;
            for (int k = 0; k < 8; k += 2)
                if ((fg >> k & 1u) && !(fg >> ((k + 7) & 7) & 1u) && !(fg >> ((k + 1) & 7) & 1u)) bits |= 1u << k;
            const int degree = __popc(bits);
            atomicAdd(&s_count[0], 1);
            atomicAdd(&s_count[degree == 2 ? 1 : 2], 1);
            if (bits & 0x0Fu) atomicAdd(&s_count[3], __popc(bits & 0x0Fu));   // every link once: at its end whose code is NW .. E
        }
        links[(size_t)m * (size_t)g.npix + p] = (uint8_t)bits;
    }
    __syncthreads();
    if (threadIdx.x < 4 && s_count[threadIdx.x]) atomicAdd(counts + 4 * m + threadIdx.x, s_count[threadIdx.x]);
}

struct Sphere {
    const double *cl, *sl, *cx, *sx;   // all NULL: no lengths
    double diameter;
};

// great-circle length of the link between pixels p and h: lc_sphere_distance's squared chord and its arc
__device__ __forceinline__ double link_length(const Sphere &s, int nx, int p, int h) {
#pragma clang fp contract(off)
    const int rp = p / nx, cp = p - rp * nx, rh = h / nx, ch = h - rh * nx;
    const double clp = s.cl[rp], clh = s.cl[rh];
    const double dx = clp * s.cx[cp] - clh * s.cx[ch], dy = clp * s.sx[cp] - clh * s.sx[ch], dz = s.sl[rp] - s.sl[rh];
    const double cost = (dx * dx + dy * dy) + dz * dz;
    const double half = __dsqrt_rn(cost) / 2.0;
    return s.diameter * asin(half < 1.0 ? half : 1.0);
}

// where the state "q leaves through k" goes: an ended next for a node (or for `stop`, a ring's first pixel), else the state of
// the head that does not return.  links: of q's plane.
__device__ __forceinline__ int next_of(const Plane &g, const uint8_t *links, int q, int k, int stop, int *head) {
    const int r = q / g.nx, c = q - r * g.nx;
    const int h = neighbour(g, r, c, k);   // a link: inside the plane
    *head = h;
    const unsigned lh = links[h];
    const int back = (k + 4) & 7;
    if (__popc(lh) != 2 || h == stop) return -(h * 8 + back) - 1;
    const int other = __ffs(lh & ~(1u << back)) - 1;
    return 2 * h + (other > back ? 1 : 0);
}

// both buffers get the slot's validity; `a` the first values
__global__ __launch_bounds__(LN_THREADS) void ln_init_kernel(const uint8_t *__restrict__ links, Plane g, Sphere s, State *__restrict__ a,
                                                             State *__restrict__ b, double *__restrict__ len_a, int *__restrict__ head_out,
                                                             double *__restrict__ link_len_out, int *__restrict__ word) {
    int m, p, active = 0;
    if (pixel_of_block(g, &m, &p)) {
        const uint8_t *pl = links + (size_t)m * (size_t)g.npix;
        const size_t slot = 2 * ((size_t)m * (size_t)g.npix + p);
        const unsigned l = pl[p];
        if (__popc(l) != 2) {
            a[slot].next = a[slot + 1].next = b[slot].next = b[slot + 1].next = LN_INVALID;
        } else {
            const int out[2] = {__ffs(l) - 1, 31 - __clz(l)};
            for (int j = 0; j < 2; ++j) {
                const int k = out[j];
                State st;
                int head;
                st.next = next_of(g, pl, p, k, -1, &head);
                st.hops = 1;
                st.diag = (k & 1) ^ 1;
                st.low = p * 8 + k;
                a[slot + j] = st;
                b[slot + j].next = 0;   // a state: the first round writes the rest
                head_out[slot + j] = head;
                if (s.cl) {
                    const double len = link_length(s, g.nx, p, head);
                    len_a[slot + j] = len;
                    link_len_out[slot + j] = len;
                }
                active |= st.next >= 0;
            }
        }
    }
    active = __syncthreads_or(active);
    if (threadIdx.x == 0 && active) atomicOr(word, 1);
}

__global__ __launch_bounds__(LN_THREADS) void ln_round_kernel(const State *__restrict__ in, State *__restrict__ out, const double *__restrict__ len_in,
                                                              double *__restrict__ len_out, long long states_per_plane, long long total,
                                                              int *__restrict__ word) {
    const long long i = (long long)blockIdx.x * LN_TILE + threadIdx.x;
    int active = 0;
    if (i < total) {
        State st = in[i];
        if (st.next != LN_INVALID) {
            double len = len_in ? len_in[i] : 0.0;
            if (st.next >= 0) {
                const long long t = i - i % states_per_plane + st.next;   // a state of the same plane
                const State nx = in[t];
                st.next = nx.next;
                st.hops += nx.hops;
                st.diag += nx.diag;
                st.low = nx.low < st.low ? nx.low : st.low;
                if (len_in) len += len_in[t];
                active = st.next >= 0;
            }
            out[i] = st;
            if (len_in) len_out[i] = len;
        }
    }
    active = __syncthreads_or(active);
    if (threadIdx.x == 0 && active) atomicOr(word, 1);
}

// in place: only a pixel's own thread reads or writes its two slots in this launch
__global__ __launch_bounds__(LN_THREADS) void ln_break_kernel(const uint8_t *__restrict__ links, Plane g, State *__restrict__ a, double *__restrict__ len_a,
                                                              const double *__restrict__ link_len, int *__restrict__ word) {
    int m, p, active = 0;
    if (pixel_of_block(g, &m, &p)) {
        const uint8_t *pl = links + (size_t)m * (size_t)g.npix;
        const size_t slot = 2 * ((size_t)m * (size_t)g.npix + p);
        const State s0 = a[slot];
        if (s0.next >= 0) {   // on a ring, and so is the other one
            const State s1 = a[slot + 1];
            const int first = (s0.low < s1.low ? s0.low : s1.low) >> 3;   // the ring's first pixel in raster order
            const unsigned l = pl[p];
            const int out[2] = {__ffs(l) - 1, 31 - __clz(l)};
            for (int j = 0; j < 2; ++j) {
                State st;
                int head;
                st.next = next_of(g, pl, p, out[j], first, &head);
                st.hops = 1;
                st.diag = (out[j] & 1) ^ 1;
                st.low = -1;
                a[slot + j] = st;
                if (len_a) len_a[slot + j] = link_len[slot + j];
                active |= st.next >= 0;
            }
        }
    }
    active = __syncthreads_or(active);
    if (threadIdx.x == 0 && active) atomicOr(word, 1);
}

struct Out {
    int *key, *pos, *ndiag;
    uint8_t *flags;
    double *dist;   // or NULL
};

__global__ __launch_bounds__(LN_THREADS) void ln_finish_kernel(const uint8_t *__restrict__ links, Plane g, const State *__restrict__ a,
                                                               const double *__restrict__ len_a, Out o) {
    int m, p;
    if (!pixel_of_block(g, &m, &p)) return;
    const size_t slot = 2 * ((size_t)m * (size_t)g.npix + p);
    const State st[2] = {a[slot], a[slot + 1]};
    if (st[0].next == LN_INVALID) {
        o.key[slot] = o.key[slot + 1] = -1;
        o.flags[slot] = o.flags[slot + 1] = 0;
        return;
    }
    const unsigned l = links[(size_t)m * (size_t)g.npix + p];
    const int out[2] = {__ffs(l) - 1, 31 - __clz(l)};
    const int end[2] = {-(st[0].next + 1), -(st[1].next + 1)};   // both have ended
    const int key = end[0] < end[1] ? end[0] : end[1];
    const int canon = end[1] == key ? 0 : 1;   // the state that runs away from the key's node
    const bool ring = st[0].low < 0;
    const bool origin = ring && p == key >> 3;   // a ring's first pixel: its states ran all the way round
    const State &before = st[canon ^ 1];
    for (int j = 0; j < 2; ++j) {
        o.key[slot + j] = key;
        o.pos[slot + j] = origin ? 0 : before.hops;
        o.ndiag[slot + j] = origin ? 0 : before.diag;
        if (o.dist) o.dist[slot + j] = origin ? 0.0 : len_a[slot + (canon ^ 1)];
        unsigned f = j == canon ? LC_LINE_CANONICAL : 0u;
        if (st[j].hops == 1) f |= LC_LINE_HEAD_IS_END;   // it ended where it began: at a node or, once broken, at the ring's first pixel
        if (ring) f |= LC_LINE_RING;
        if (!(out[j] & 1)) f |= LC_LINE_CORNER_LINK;
        o.flags[slot + j] = (uint8_t)(f | LC_LINE_STATE);
    }
}

// the links the states do not cover (node next to node), as a list of pixel pairs of one grid
__global__ __launch_bounds__(LN_THREADS) void ln_pairs_kernel(const int *__restrict__ from, const int *__restrict__ to, long long n, int nx,
                                                              int npix, Sphere s, double *__restrict__ out) {
    const long long i = (long long)blockIdx.x * LN_TILE + threadIdx.x;
    if (i >= n) return;
    const int p = from[i], h = to[i];
    // (a pair that names no pixel of the plane reads no table)
    out[i] = p >= 0 && p < npix && h >= 0 && h < npix ? link_length(s, nx, p, h) : NAN;
}

// int32 elements of the work buffer, 0 where the sizes are bad or do not fit
size_t work_elems(int ny, int nx, int n_members) {
    if (ny < 1 || nx < 1 || n_members < 1) return 0;
    const unsigned long long npix = (unsigned long long)ny * (unsigned long long)nx;
    if (npix >= (1ull << 28)) return 0;
    // per pixel two states in two buffers: 16 bytes and a float64 each
    const unsigned long long per_plane = 24ull * npix;
    if ((unsigned long long)n_members > (SIZE_MAX / 4 - LN_HEAD) / per_plane) return 0;
    return (size_t)(LN_HEAD + per_plane * (unsigned long long)n_members);
}

}  // namespace

extern "C" size_t lc_lines_work_elems(int ny, int nx, int n_members) { return work_elems(ny, nx, n_members); }

extern "C" int lc_line_link_lengths(lc_ctx *ctx, const lc_link_lengths_args *a) {
    const char *who = "lc_line_link_lengths";
    LC_REQUIRE(ctx, "%s: null context", who);
    LC_REQUIRE(a, "%s: null argument structure", who);
    LC_REQUIRE(a->struct_size == sizeof(lc_link_lengths_args), "%s: struct_size %zu, this library has %zu", who, (size_t)a->struct_size,
               sizeof(lc_link_lengths_args));
    LC_REQUIRE(a->ny >= 1 && a->nx >= 1 && (long long)a->ny * a->nx < (1ll << 31), "%s: bad size ny=%d nx=%d (each >= 1, < 2^31 pixels)", who,
               a->ny, a->nx);
    LC_REQUIRE(a->n_pairs >= 0 && (a->n_pairs + LN_TILE - 1) / LN_TILE <= (long long)INT_MAX, "%s: bad n_pairs %lld", who, a->n_pairs);
    LC_REQUIRE(a->radius > 0.0 && std::isfinite(a->radius), "%s: bad radius %g: > 0 and finite", who, a->radius);
    if (a->n_pairs == 0) return LC_OK;
    LC_REQUIRE(a->from && a->to && a->length_out && a->cos_lat && a->sin_lat && a->cos_lon && a->sin_lon, "%s: null pointer", who);
    LC_HIP_CHECK(hipSetDevice(ctx->device));
    Sphere s = {a->cos_lat, a->sin_lat, a->cos_lon, a->sin_lon, 2.0 * a->radius};
    hipLaunchKernelGGL(ln_pairs_kernel, dim3((unsigned)((a->n_pairs + LN_TILE - 1) / LN_TILE)), dim3(LN_THREADS), 0, ctx->stream,
                       (const int *)a->from, (const int *)a->to, a->n_pairs, a->nx, a->ny * a->nx, s, (double *)a->length_out);
    LC_HIP_CHECK(hipGetLastError());
    return LC_OK;
}

extern "C" int lc_trace_lines(lc_ctx *ctx, const lc_lines_args *a) {
    const char *who = "lc_trace_lines";
    LC_REQUIRE(ctx, "%s: null context", who);
    LC_REQUIRE(a, "%s: null argument structure", who);
    LC_REQUIRE(a->struct_size == sizeof(lc_lines_args), "%s: struct_size %zu, this library has %zu", who, (size_t)a->struct_size,
               sizeof(lc_lines_args));
    LC_REQUIRE(a->dtype == LC_F32 || a->dtype == LC_F64, "%s: bad dtype %d (LC_F32 or LC_F64)", who, a->dtype);
    LC_REQUIRE(a->ny >= 1 && a->nx >= 1 && a->n_members >= 1, "%s: bad size ny=%d nx=%d n_members=%d (each >= 1)", who, a->ny, a->nx,
               a->n_members);
    const long long npix = (long long)a->ny * a->nx;
    LC_REQUIRE(npix < (1ll << 28), "%s: plane too large: %d x %d = %lld pixels, dart ids 8 p + k are int32 (< 2^28 pixels)", who, a->ny,
               a->nx, npix);
    LC_REQUIRE(!a->cyclic_x || a->nx >= 3, "%s: cyclic_x needs nx >= 3, got %d (a pixel would neighbour itself or one pixel twice)", who,
               a->nx);
    const long long blocks_per_plane = (npix + LN_TILE - 1) / LN_TILE, state_blocks = (2 * npix * a->n_members + LN_TILE - 1) / LN_TILE;
    LC_REQUIRE(state_blocks <= (long long)INT_MAX && work_elems(a->ny, a->nx, a->n_members) != 0, "%s: too many planes: %d of %d x %d", who,
               a->n_members, a->ny, a->nx);
    const bool sphere = a->cos_lat || a->sin_lat || a->cos_lon || a->sin_lon;
    if (sphere) {
        LC_REQUIRE(a->cos_lat && a->sin_lat && a->cos_lon && a->sin_lon, "%s: the four coordinate tables come together, or none", who);
        LC_REQUIRE(a->radius > 0.0 && std::isfinite(a->radius), "%s: bad radius %g: > 0 and finite", who, a->radius);
        LC_REQUIRE(a->dist_out && a->link_length_out, "%s: null pointer: dist_out and link_length_out go with the tables", who);
    }
    LC_REQUIRE(a->mask && a->links_out && a->counts_out && a->key_out && a->pos_out && a->ndiag_out && a->head_out && a->flags_out &&
                   a->work_dev,
               "%s: null pointer", who);
    LC_REQUIRE(((uintptr_t)a->work_dev & 15u) == 0, "%s: work_dev must be 16-byte aligned", who);
    LC_HIP_CHECK(hipSetDevice(ctx->device));

    Plane g;
    g.ny = a->ny;
    g.nx = a->nx;
    g.npix = (int)npix;
    g.cyclic = a->cyclic_x ? 1 : 0;
    g.blocks_per_plane = (int)blocks_per_plane;
    const size_t states = 2 * (size_t)npix * (size_t)a->n_members;
    int *words = (int *)a->work_dev;
    State *buf[2] = {(State *)(words + LN_HEAD), (State *)(words + LN_HEAD) + states};
    double *len[2] = {nullptr, nullptr};
    if (sphere) {
        len[0] = (double *)(buf[1] + states);
        len[1] = len[0] + states;
    }
    Sphere s = {a->cos_lat, a->sin_lat, a->cos_lon, a->sin_lon, 2.0 * a->radius};
    uint8_t *links = (uint8_t *)a->links_out;
    int *counts = (int *)a->counts_out;
    const dim3 block(LN_THREADS), pixels((unsigned)(blocks_per_plane * a->n_members)), slots((unsigned)state_blocks);

    LC_HIP_CHECK(hipMemsetAsync(words, 0, LN_HEAD * sizeof(int), ctx->stream));
    LC_HIP_CHECK(hipMemsetAsync(counts, 0, 4 * sizeof(int) * (size_t)a->n_members, ctx->stream));
    if (a->dtype == LC_F32)
        hipLaunchKernelGGL(ln_links_kernel<float>, pixels, block, 0, ctx->stream, (const float *)a->mask, g, links, counts);
    else
        hipLaunchKernelGGL(ln_links_kernel<double>, pixels, block, 0, ctx->stream, (const double *)a->mask, g, links, counts);
    int word = 0;   // the next launch's word; LN_HEAD of them, and at most 2 + 2 * 29 launches report
    hipLaunchKernelGGL(ln_init_kernel, pixels, block, 0, ctx->stream, (const uint8_t *)links, g, s, buf[0], buf[1], len[0], (int *)a->head_out,
                       (double *)a->link_length_out, words + word);
    LC_HIP_CHECK(hipGetLastError());
    std::vector<int> host_counts(4 * (size_t)a->n_members);
    int active = 0;
    LC_HIP_CHECK(hipMemcpyAsync(host_counts.data(), counts, host_counts.size() * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    LC_HIP_CHECK(hipMemcpyAsync(&active, words + word, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    LC_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    long long interior = 0;
    for (int m = 0; m < a->n_members; ++m) interior = host_counts[4 * m + 1] > interior ? host_counts[4 * m + 1] : interior;

    int cur = 0, rounds = 0;
    auto round = [&]() -> int {
        ++word;
        hipLaunchKernelGGL(ln_round_kernel, slots, block, 0, ctx->stream, (const State *)buf[cur], buf[cur ^ 1], (const double *)len[cur],
                           len[cur ^ 1], 2 * npix, (long long)states, words + word);
        cur ^= 1;
        ++rounds;
        LC_HIP_CHECK(hipGetLastError());
        LC_HIP_CHECK(hipMemcpyAsync(&active, words + word, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        LC_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        return LC_OK;
    };
    // open lines: a state is at most `interior` links from its node
    while (active && (1ll << rounds) < interior) {
        const int st = round();
        if (st != LC_OK) return st;
    }
    if (active) {   // rings: every state has seen its whole ring
        ++word;
        hipLaunchKernelGGL(ln_break_kernel, pixels, block, 0, ctx->stream, (const uint8_t *)links, g, buf[cur], len[cur],
                           (const double *)a->link_length_out, words + word);
        LC_HIP_CHECK(hipGetLastError());
        LC_HIP_CHECK(hipMemcpyAsync(&active, words + word, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        LC_HIP_CHECK(hipStreamSynchronize(ctx->stream));
        for (int second = 0; active; ++second) {
            if (second > 30) {   // 2^30 links: more than a plane holds
                lc_set_error("%s: the ranking of the rings did not end (internal error)", who);
                return LC_EHIP;
            }
            const int st = round();
            if (st != LC_OK) return st;
        }
    }
    Out o = {(int *)a->key_out, (int *)a->pos_out, (int *)a->ndiag_out, (uint8_t *)a->flags_out, sphere ? (double *)a->dist_out : nullptr};
    hipLaunchKernelGGL(ln_finish_kernel, pixels, block, 0, ctx->stream, (const uint8_t *)links, g, (const State *)buf[cur], (const double *)len[cur], o);
    LC_HIP_CHECK(hipGetLastError());
    if (a->rounds_out) *a->rounds_out = rounds;
    return LC_OK;
}
