// Ridges followed through time: the space-time labels of a (time, latitude, longitude) record of ridge masks and the span
// of every track, the device side of tools.track_ridges / tools.persistent_ridges.  It extends through time the filter
// LCS/area_of_influence.py:210-211 passes every plane through on its own (components.hip); the meaning is fixed in
// include/lcs_hip.h and pinned against scipy.sparse.csgraph + numpy in tests/test_tracks_gpu.py.
//
// Labelling is the union-find of components.hip over the linear voxel indices of the WHOLE record, one index space:
//   init     parent[i] = i on foreground, -1 on background
//   merge    every foreground voxel unites with its in-plane foreground neighbours of smaller index (and, with cyclic_x,
//            column 0 with column nx-1), and with every foreground voxel of the plane before it inside the reach window.
//            unite() is an atomicMin on the larger root: a parent only ever DECREASES, so every pointer leads to a smaller
//            index, every walk ends, and the root of a set is its smallest index -- its first voxel in raster order
//   flatten  parent[i] = find(i); the same pass counts the roots of each tile of TR_TILE voxels (a tile may straddle planes)
//   scan     exclusive prefix sum of the tile counts (one workgroup, any number of tiles), its total is the track count
//   rank     every tile scans its own root flags again, adds its offset: the root of rank k holds -(k + 2)
//   relabel  label = 0 on background, rank of the root + 1 elsewhere: 1..N in the order of the first voxels, which is the
//            numbering scipy.ndimage.label gives a 3-D array
// The spans are integer atomics per track (smallest and largest plane index, voxel count): no order of arrival changes them.
// No kernel waits for another workgroup: there is no flag, no look-back and no grid synchronisation anywhere in this file --
// what one stage needs from all workgroups of the stage before is handed over by the end of that launch.  The atomics are
// ordinary ones in plain C++.  find_root, unite and the block scan are restated from components.hip, which shares no header.
#include <climits>

#include "lcs_common.h"

namespace {

constexpr int TR_THREADS = 256;
constexpr int TR_ITEMS = 4;                      // consecutive voxels of one thread in the scanning stages
constexpr int TR_TILE = TR_THREADS * TR_ITEMS;   // voxels of one workgroup
constexpr int TS_ITEMS = 8;                      // consecutive voxels of one thread in the spans
constexpr int TS_TILE = TR_THREADS * TS_ITEMS;

template <typename T>
__device__ __forceinline__ bool foreground(T v) {
    return v != (T)0 && v == v;   // NaN is background, as everywhere in tools
}

// parents are read and written by many workgroups at once during merge and flatten: relaxed, device scope
__device__ __forceinline__ int load_parent(const int *a, int i) {
    return __hip_atomic_load(a + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void store_parent(int *a, int i, int v) {
    __hip_atomic_store(a + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// i is a foreground voxel.  Every step goes to a strictly smaller index >= 0.
__device__ __forceinline__ int find_root(const int *parent, int i) {
    for (;;) {
        const int p = load_parent(parent, i);
        if (p == i) return i;
        i = p;
    }
}

// a and b are foreground voxels of the record
__device__ void unite(int *parent, int a, int b) {
    for (;;) {
        a = find_root(parent, a);
        b = find_root(parent, b);
        if (a == b) return;
        if (a > b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(parent + b, a);
        if (old == b) return;   // b was still a root: it hangs under a now
        b = old;                // someone linked b first: what it was linked to and a are still to be united
    }
}

// first voxel of this workgroup's tile; n < 2^31 and the grid is ceil(n / tile_voxels), so it is < n
__device__ __forceinline__ long long tile_start(int tile_voxels) { return (long long)blockIdx.x * tile_voxels; }

// exclusive scan of one value per thread over the workgroup; *total is the sum over the workgroup
__device__ int block_exclusive_scan(int v, int *total) {
    __shared__ int s[TR_THREADS];
    const int t = threadIdx.x;
    s[t] = v;
    __syncthreads();
    for (int d = 1; d < TR_THREADS; d <<= 1) {
        const int add = t >= d ? s[t - d] : 0;
        __syncthreads();
        s[t] += add;
        __syncthreads();
    }
    const int incl = s[t];
    *total = s[TR_THREADS - 1];
    __syncthreads();   // s is written again by the next call
    return incl - v;
}

template <typename T>
__global__ __launch_bounds__(TR_THREADS) void tr_init_kernel(const T *__restrict__ mask, int *__restrict__ parent, int n) {
    const long long i0 = tile_start(TR_TILE);
    for (int k = 0; k < TR_ITEMS; ++k) {
        const long long i = i0 + k * TR_THREADS + threadIdx.x;
        if (i < n) parent[i] = foreground(mask[i]) ? (int)i : -1;
    }
}

__global__ __launch_bounds__(TR_THREADS) void tr_merge_kernel(int *__restrict__ parent, int ny, int nx, int npix, int n, int diagonals,
                                                             int cyclic, int reach) {
    const long long i0 = tile_start(TR_TILE);
    for (int k = 0; k < TR_ITEMS; ++k) {
        const long long il = i0 + k * TR_THREADS + threadIdx.x;
        if (il >= n) continue;
        const int i = (int)il;
        if (load_parent(parent, i) < 0) continue;   // background: init wrote it in the launch before, nobody writes it again
        const int t = i / npix, p = i - t * npix, base = i - p;   // base: first voxel of plane t
        const int r = p / nx, c = p - r * nx;
        // >= 0 at every moment of a foreground voxel's life; every index below lies in plane t or t - 1 of the record
        auto fg = [&](int first, int rr, int cc) { return load_parent(parent, first + rr * nx + cc) >= 0; };
        const bool up = r > 0, west = c > 0, east = c < nx - 1;
        if (!diagonals) {
            if (west && fg(base, r, c - 1)) unite(parent, i, i - 1);
            if (up && fg(base, r - 1, c)) unite(parent, i, i - nx);
        } else if (up && fg(base, r - 1, c)) {
            unite(parent, i, i - nx);   // N touches W, NW and NE itself: their own merges join them to it
        } else {
            if (west && fg(base, r, c - 1)) unite(parent, i, i - 1);
            if (up && west && fg(base, r - 1, c - 1)) unite(parent, i, i - nx - 1);
            if (up && east && fg(base, r - 1, c + 1)) unite(parent, i, i - nx + 1);
        }
        if (cyclic && c == 0) {   // the seam: column nx - 1 is the western neighbour of column 0, rows r - 1 .. r + 1 with diagonals
            const int e = nx - 1;
            if (fg(base, r, e)) unite(parent, i, base + r * nx + e);
            if (diagonals && up && fg(base, r - 1, e)) unite(parent, i, base + (r - 1) * nx + e);
            if (diagonals && r < ny - 1 && fg(base, r + 1, e)) unite(parent, i, base + (r + 1) * nx + e);
        }
        if (t == 0) continue;
        // the plane before: rows r - reach .. r + reach inside the plane, columns c - reach .. c + reach inside the plane or,
        // with cyclic, the shorter way round (a window as wide as the plane is every column once)
        const int before = base - npix;
        const int r0 = r - reach > 0 ? r - reach : 0, r1 = r + reach < ny - 1 ? r + reach : ny - 1;
        int c0 = c - reach, c1 = c + reach;
        bool wrap = cyclic != 0;
        if (wrap && 2 * reach + 1 >= nx) {
            c0 = 0;
            c1 = nx - 1;
            wrap = false;
        } else if (!wrap) {
            c0 = c0 > 0 ? c0 : 0;
            c1 = c1 < nx - 1 ? c1 : nx - 1;
        }
        for (int rr = r0; rr <= r1; ++rr)
            for (int cw = c0; cw <= c1; ++cw) {
                int cc = cw;   // wrap: 2 reach + 1 < nx, one turn brings it into the plane
                if (wrap) cc = cc < 0 ? cc + nx : (cc >= nx ? cc - nx : cc);
                if (fg(before, rr, cc)) unite(parent, i, before + rr * nx + cc);
            }
    }
}

// this thread's TR_ITEMS consecutive voxels of the tile: how many are roots (parent[i] == i); flags bit k = voxel k is one
__device__ __forceinline__ int root_flags(const int *parent, long long i0, int n, unsigned *flags) {
    int count = 0;
    *flags = 0;
    for (int k = 0; k < TR_ITEMS; ++k) {
        const long long i = i0 + k;
        if (i < n && parent[i] == (int)i) {
            *flags |= 1u << k;
            ++count;
        }
    }
    return count;
}

__global__ __launch_bounds__(TR_THREADS) void tr_flatten_kernel(int *__restrict__ parent, int n, int *__restrict__ tile_roots) {
    const long long i0 = tile_start(TR_TILE);
    int count = 0;
    for (int k = 0; k < TR_ITEMS; ++k) {
        const long long il = i0 + k * TR_THREADS + threadIdx.x;
        if (il >= n) continue;
        const int i = (int)il;
        if (load_parent(parent, i) < 0) continue;
        const int root = find_root(parent, i);   // a walk that meets an already flattened voxel ends one step later
        store_parent(parent, i, root);
        count += root == i;
    }
    int total;
    block_exclusive_scan(count, &total);
    if (threadIdx.x == 0) tile_roots[blockIdx.x] = total;
}

// one workgroup: tile_roots[0 .. tiles) becomes its own exclusive prefix sum, *count_out the total
__global__ __launch_bounds__(TR_THREADS) void tr_scan_tiles_kernel(int *__restrict__ tile_roots, int tiles, int *__restrict__ count_out) {
    int carry = 0;
    for (int t0 = 0; t0 < tiles; t0 += TR_THREADS) {   // tiles is the same for every thread: the barriers inside are met by all
        const int j = t0 + threadIdx.x;
        const int x = j < tiles ? tile_roots[j] : 0;
        int total;
        const int off = block_exclusive_scan(x, &total);
        if (j < tiles) tile_roots[j] = carry + off;
        carry += total;
    }
    if (threadIdx.x == 0) count_out[0] = carry;
}

// the root of rank k (0-based, in the order of the root indices) holds -(k + 2); -1 stays background, every other voxel keeps
// the index of its root
__global__ __launch_bounds__(TR_THREADS) void tr_rank_kernel(int *__restrict__ parent, int n, const int *__restrict__ tile_offset) {
    const long long i0 = tile_start(TR_TILE) + threadIdx.x * TR_ITEMS;
    unsigned flags;
    const int count = root_flags(parent, i0, n, &flags);
    int total;
    int rank = tile_offset[blockIdx.x] + block_exclusive_scan(count, &total);
    for (int k = 0; k < TR_ITEMS; ++k)
        if (flags >> k & 1u) parent[i0 + k] = -(rank++ + 2);
}

// A voxel reads its own cell (nobody else writes it) and, unless it is a root, the cell of its root, which may or may not
// have been rewritten by the root's own thread yet: -(k + 2) before, k + 1 after -- one label either way.
__global__ __launch_bounds__(TR_THREADS) void tr_relabel_kernel(int *__restrict__ cell, int n) {
    const long long i0 = tile_start(TR_TILE);
    for (int k = 0; k < TR_ITEMS; ++k) {
        const long long il = i0 + k * TR_THREADS + threadIdx.x;
        if (il >= n) continue;
        const int i = (int)il;
        const int v = load_parent(cell, i);
        int label = 0;
        if (v <= -2) {
            label = -v - 1;
        } else if (v >= 0) {
            const int x = load_parent(cell, v);
            label = x < 0 ? -x - 1 : x;
        }
        store_parent(cell, i, label);
    }
}

// ------------------------------------------------------------------ spans
// first is kept as an unsigned minimum: -1 (no voxel yet) is the largest unsigned value, so an entry nobody touches stays -1
__global__ void ts_init_kernel(int *__restrict__ first, int *__restrict__ last, long long *__restrict__ volume, int n_max) {
    for (long long j = blockIdx.x * (long long)blockDim.x + threadIdx.x; j < n_max; j += (long long)gridDim.x * blockDim.x) {
        first[j] = -1;
        last[j] = -1;
        volume[j] = 0;
    }
}

__global__ __launch_bounds__(TR_THREADS) void ts_spans_kernel(const int *__restrict__ labels, int npix, int n, const int *__restrict__ count,
                                                             int n_max, int *__restrict__ first, int *__restrict__ last,
                                                             long long *__restrict__ volume) {
    const int cap = count[0] < n_max ? count[0] : n_max;   // labels this call measures: 1 .. min(count, n_max)
    // a thread walks TS_ITEMS consecutive voxels and keeps the span of the label it is on: one set of atomics per change of
    // label, not per voxel (neighbours in a row share their label)
    int cur = 0, tmin = 0, tmax = 0;
    long long vol = 0;
    auto flush = [&]() {
        if (!cur) return;
        atomicMin((unsigned *)first + (cur - 1), (unsigned)tmin);
        atomicMax(last + (cur - 1), tmax);
        atomicAdd((unsigned long long *)volume + (cur - 1), (unsigned long long)vol);
    };
    const long long i0 = tile_start(TS_TILE) + (long long)threadIdx.x * TS_ITEMS;
    for (int k = 0; k < TS_ITEMS; ++k) {
        const long long il = i0 + k;
        if (il >= n) break;
        const int i = (int)il, l = labels[i];
        if (l < 1 || l > cap) continue;
        const int t = i / npix;
        if (l != cur) {
            flush();
            cur = l;
            tmin = tmax = t;
            vol = 0;
        }
        tmax = t;   // the walk goes forward in time
        ++vol;
    }
    flush();
}

}  // namespace

// What both entry points check of the record before they touch the device; *n: voxels, *tiles: workgroups at `tile_voxels` each.
static int tracks_geometry(const char *who, int ny, int nx, int n_times, int tile_voxels, int *n, int *tiles) {
    LC_REQUIRE(ny >= 1 && nx >= 1 && n_times >= 1, "%s: bad size ny=%d nx=%d n_times=%d (each >= 1)", who, ny, nx, n_times);
    const long long npix = (long long)ny * nx;                                    // < 2^62
    const long long all = npix < (1ll << 31) ? npix * n_times : (1ll << 62);     // < 2^62 either way
    LC_REQUIRE(all < (1ll << 31), "%s: record too large: %d x %d x %d voxels, labels are int32 (< 2^31)", who, n_times, ny, nx);
    *n = (int)all;
    *tiles = (int)((all + tile_voxels - 1) / tile_voxels);
    return LC_OK;
}

extern "C" size_t lc_track_work_elems(int ny, int nx, int n_times) {
    if (ny < 1 || nx < 1 || n_times < 1) return 0;
    const unsigned long long npix = (unsigned long long)ny * (unsigned long long)nx;
    if (npix >= (1ull << 31) || npix * (unsigned long long)n_times >= (1ull << 31)) return 0;
    return (size_t)((npix * (unsigned long long)n_times + TR_TILE - 1) / TR_TILE);
}

extern "C" int lc_label_tracks(lc_ctx *ctx, const void *mask, int dtype, int ny, int nx, int n_times, int connectivity, int cyclic_x,
                               int reach, void *labels_out, void *count_out, void *work_dev) {
    LC_REQUIRE(ctx, "lc_label_tracks: null context");
    LC_REQUIRE(dtype == LC_F32 || dtype == LC_F64, "lc_label_tracks: bad dtype %d (LC_F32 or LC_F64)", dtype);
    int n = 0, tiles = 0;
    const int st = tracks_geometry("lc_label_tracks", ny, nx, n_times, TR_TILE, &n, &tiles);
    if (st != LC_OK) return st;
    LC_REQUIRE(connectivity == 1 || connectivity == 2, "lc_label_tracks: bad connectivity %d (1: edges, 2: edges and corners)",
               connectivity);
    LC_REQUIRE(reach >= 0 && reach <= LC_TRACK_MAX_REACH, "lc_label_tracks: bad reach %d (0 .. %d)", reach, LC_TRACK_MAX_REACH);
    LC_REQUIRE(mask && labels_out && count_out && work_dev, "lc_label_tracks: null pointer");
    LC_HIP_CHECK(hipSetDevice(ctx->device));
    const dim3 grid((unsigned)tiles), block(TR_THREADS);
    int *parent = (int *)labels_out, *tile_roots = (int *)work_dev;
    if (dtype == LC_F32)
        hipLaunchKernelGGL(tr_init_kernel<float>, grid, block, 0, ctx->stream, (const float *)mask, parent, n);
    else
        hipLaunchKernelGGL(tr_init_kernel<double>, grid, block, 0, ctx->stream, (const double *)mask, parent, n);
    hipLaunchKernelGGL(tr_merge_kernel, grid, block, 0, ctx->stream, parent, ny, nx, ny * nx, n, connectivity == 2 ? 1 : 0,
                       cyclic_x ? 1 : 0, reach);
    hipLaunchKernelGGL(tr_flatten_kernel, grid, block, 0, ctx->stream, parent, n, tile_roots);
    hipLaunchKernelGGL(tr_scan_tiles_kernel, dim3(1), block, 0, ctx->stream, tile_roots, tiles, (int *)count_out);
    hipLaunchKernelGGL(tr_rank_kernel, grid, block, 0, ctx->stream, parent, n, (const int *)tile_roots);
    hipLaunchKernelGGL(tr_relabel_kernel, grid, block, 0, ctx->stream, parent, n);
    LC_HIP_CHECK(hipGetLastError());
    return LC_OK;
}

extern "C" int lc_track_spans(lc_ctx *ctx, const lc_track_spans_args *a) {
    LC_REQUIRE(a, "lc_track_spans: null argument structure");
    LC_REQUIRE(a->struct_size == sizeof(lc_track_spans_args), "lc_track_spans: struct_size %zu, this library has %zu",
               (size_t)a->struct_size, sizeof(lc_track_spans_args));
    LC_REQUIRE(ctx, "lc_track_spans: null context");
    int n = 0, tiles = 0;
    const int st = tracks_geometry("lc_track_spans", a->ny, a->nx, a->n_times, TS_TILE, &n, &tiles);
    if (st != LC_OK) return st;
    LC_REQUIRE(a->n_max >= 1, "lc_track_spans: bad capacity n_max=%d (>= 1)", a->n_max);
    LC_REQUIRE(a->labels && a->count && a->first_out && a->last_out && a->volume_out, "lc_track_spans: null pointer");
    LC_HIP_CHECK(hipSetDevice(ctx->device));
    const dim3 block(TR_THREADS);
    const int init_blocks = (a->n_max + TR_THREADS - 1) / TR_THREADS;
    hipLaunchKernelGGL(ts_init_kernel, dim3((unsigned)(init_blocks < 4096 ? init_blocks : 4096)), block, 0, ctx->stream,
                       (int *)a->first_out, (int *)a->last_out, (long long *)a->volume_out, a->n_max);
    hipLaunchKernelGGL(ts_spans_kernel, dim3((unsigned)tiles), block, 0, ctx->stream, (const int *)a->labels, a->ny * a->nx, n,
                       (const int *)a->count, a->n_max, (int *)a->first_out, (int *)a->last_out, (long long *)a->volume_out);
    LC_HIP_CHECK(hipGetLastError());
    return LC_OK;
}
