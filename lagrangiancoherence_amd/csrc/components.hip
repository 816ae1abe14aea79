// Connected components of a ridge mask, their per-component sums, and the filtered mask: the device side of
// tools.filter_ridges (the call LCS/area_of_influence.py:210-242 makes; the function itself comes from a package outside the
// reference, so its meaning is fixed in include/lcs_hip.h and pinned against scipy.ndimage.label + numpy in
// tests/test_components_gpu.py).
//
// Labelling is union-find over the linear pixel indices of each plane, n_members planes per launch:
//   init     parent[p] = p on foreground, -1 on background
//   merge    every foreground pixel unites with its foreground neighbours of smaller index (and, with cyclic_x, column 0 with
//            column nx-1).  unite() is an atomicMin on the larger root: a parent only ever DECREASES, so every pointer leads to
//            a smaller index, every walk ends, and the root of a set is its smallest index -- its first pixel in raster order
//   flatten  parent[p] = find(p); the same pass counts the roots of each tile of CC_TILE pixels
//   scan     exclusive prefix sum of the tile counts of each plane (one workgroup per plane, any number of tiles), its total
//            is the plane's component count
//   rank     every tile scans its own root flags again, adds its offset: the root of rank k holds -(k + 2)
//   relabel  label = 0 on background, rank of the root + 1 elsewhere: 1..N in the order of the first pixels, which is the
//            numbering scipy.ndimage.label gives
// The sums come twice: exact integer moments in index units (lc_component_sums), and float64 moments of the nodes' unit vectors
// weighted by cell area (lc_component_sphere_sums), from which one thread per label derives area, axis lengths, centroid and
// orientation on the sphere (tools.ridge_properties, filter_ridges(metric='sphere'); pinned against a numpy restatement in
// tests/test_sphere_props_gpu.py).
// No kernel waits for another workgroup: there is no flag, no look-back and no grid synchronisation anywhere in this file --
// what one stage needs from all workgroups of the stage before is handed over by the end of that launch.  The atomics are
// ordinary ones in plain C++.
#include <climits>

#include "lcs_common.h"

namespace {

constexpr int CC_THREADS = 256;
constexpr int CC_ITEMS = 4;                      // consecutive pixels of one thread in the scanning stages
constexpr int CC_TILE = CC_THREADS * CC_ITEMS;   // pixels of one workgroup
constexpr int CS_ITEMS = 8;                      // consecutive pixels of one thread in the sums
constexpr int CS_TILE = CC_THREADS * CS_ITEMS;

template <typename T>
__device__ __forceinline__ bool foreground(T v) {
    return v != (T)0 && v == v;   // NaN is background (the driver's ridges.where(~isnan(ridges), 0))
}

// parents are read and written by many workgroups at once during merge and flatten: relaxed, device scope
__device__ __forceinline__ int load_parent(const int *a, int i) {
    return __hip_atomic_load(a + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void store_parent(int *a, int i, int v) {
    __hip_atomic_store(a + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// i is a foreground pixel.  Every step goes to a strictly smaller index >= 0.
__device__ __forceinline__ int find_root(const int *parent, int i) {
    for (;;) {
        const int p = load_parent(parent, i);
        if (p == i) return i;
        i = p;
    }
}

// a and b are foreground pixels of one plane
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

// the plane and the tile of this workgroup: workgroup w of a launch of n_members * tiles
struct Tile {
    size_t base;   // first element of the plane in [n_members][npix]
    int p0;        // first pixel of the tile in the plane
};
__device__ __forceinline__ Tile tile_of_block(int tiles, int npix, int tile_pixels) {
    const int m = blockIdx.x / tiles, t = blockIdx.x - m * tiles;
    return Tile{(size_t)m * (size_t)npix, t * tile_pixels};   // t * tile_pixels < npix + tile_pixels: no overflow, see lc_label_components
}

// exclusive scan of one value per thread over the workgroup; *total is the sum over the workgroup
__device__ int block_exclusive_scan(int v, int *total) {
    __shared__ int s[CC_THREADS];
    const int t = threadIdx.x;
    s[t] = v;
    __syncthreads();
    for (int d = 1; d < CC_THREADS; d <<= 1) {
        const int add = t >= d ? s[t - d] : 0;
        __syncthreads();
        s[t] += add;
        __syncthreads();
    }
    const int incl = s[t];
    *total = s[CC_THREADS - 1];
    __syncthreads();   // s is written again by the next call
    return incl - v;
}

template <typename T>
__global__ __launch_bounds__(CC_THREADS) void cc_init_kernel(const T *__restrict__ mask, int *__restrict__ parent, int npix, int tiles) {
    const Tile w = tile_of_block(tiles, npix, CC_TILE);
    for (int k = 0; k < CC_ITEMS; ++k) {
        const long long p = (long long)w.p0 + k * CC_THREADS + threadIdx.x;
        if (p < npix) parent[w.base + p] = foreground(mask[w.base + p]) ? (int)p : -1;
    }
}

__global__ __launch_bounds__(CC_THREADS) void cc_merge_kernel(int *__restrict__ parent_all, int ny, int nx, int npix, int tiles,
                                                             int diagonals, int cyclic) {
    const Tile w = tile_of_block(tiles, npix, CC_TILE);
    int *parent = parent_all + w.base;
    for (int k = 0; k < CC_ITEMS; ++k) {
        const long long pl = (long long)w.p0 + k * CC_THREADS + threadIdx.x;
        if (pl >= npix) continue;
        const int p = (int)pl;
        if (parent[p] < 0) continue;   // background: init wrote it in the launch before, nobody writes it again
        const int r = p / nx, c = p - r * nx;
        auto fg = [&](int rr, int cc) { return parent[rr * nx + cc] >= 0; };   // >= 0 at every moment of a foreground pixel's life
        const bool up = r > 0, west = c > 0, east = c < nx - 1;
        if (!diagonals) {
            if (west && fg(r, c - 1)) unite(parent, p, p - 1);
            if (up && fg(r - 1, c)) unite(parent, p, p - nx);
        } else if (up && fg(r - 1, c)) {
            unite(parent, p, p - nx);   // N touches W, NW and NE itself: their own merges join them to it
        } else {
            if (west && fg(r, c - 1)) unite(parent, p, p - 1);
            if (up && west && fg(r - 1, c - 1)) unite(parent, p, p - nx - 1);
            if (up && east && fg(r - 1, c + 1)) unite(parent, p, p - nx + 1);
        }
        if (cyclic && c == 0) {   // the seam: column nx - 1 is the western neighbour of column 0, rows r - 1 .. r + 1 with diagonals
            const int e = nx - 1;
            if (fg(r, e)) unite(parent, p, r * nx + e);
            if (diagonals && up && fg(r - 1, e)) unite(parent, p, (r - 1) * nx + e);
            if (diagonals && r < ny - 1 && fg(r + 1, e)) unite(parent, p, (r + 1) * nx + e);
        }
    }
}

// this thread's CC_ITEMS consecutive pixels of the tile: how many are roots (parent[p] == p); flags bit k = pixel k is one
__device__ __forceinline__ int root_flags(const int *parent, long long p0, int npix, unsigned *flags) {
    int n = 0;
    *flags = 0;
    for (int k = 0; k < CC_ITEMS; ++k) {
        const long long p = p0 + k;
        if (p < npix && parent[p] == (int)p) {
            *flags |= 1u << k;
            ++n;
        }
    }
    return n;
}

__global__ __launch_bounds__(CC_THREADS) void cc_flatten_kernel(int *__restrict__ parent_all, int npix, int tiles,
                                                               int *__restrict__ tile_roots) {
    const Tile w = tile_of_block(tiles, npix, CC_TILE);
    int *parent = parent_all + w.base;
    int n = 0;
    for (int k = 0; k < CC_ITEMS; ++k) {
        const long long pl = (long long)w.p0 + k * CC_THREADS + threadIdx.x;
        if (pl >= npix) continue;
        const int p = (int)pl;
        if (load_parent(parent, p) < 0) continue;
        const int root = find_root(parent, p);   // a walk that meets an already flattened pixel ends one step later
        store_parent(parent, p, root);
        n += root == p;
    }
    int total;
    block_exclusive_scan(n, &total);
    if (threadIdx.x == 0) tile_roots[blockIdx.x] = total;
}

// one workgroup per plane: tile_roots[m][0 .. tiles) becomes its own exclusive prefix sum, counts[m] the total
__global__ __launch_bounds__(CC_THREADS) void cc_scan_tiles_kernel(int *__restrict__ tile_roots, int tiles, int *__restrict__ counts) {
    int *v = tile_roots + (size_t)blockIdx.x * tiles;
    int carry = 0;
    for (int t0 = 0; t0 < tiles; t0 += CC_THREADS) {   // tiles is the same for every thread: the barriers inside are met by all
        const int i = t0 + threadIdx.x;
        const int x = i < tiles ? v[i] : 0;
        int total;
        const int off = block_exclusive_scan(x, &total);
        if (i < tiles) v[i] = carry + off;
        carry += total;
    }
    if (threadIdx.x == 0) counts[blockIdx.x] = carry;
}

// the root of rank k (0-based, in the order of the root indices) holds -(k + 2); -1 stays background, every other pixel keeps
// the index of its root
__global__ __launch_bounds__(CC_THREADS) void cc_rank_kernel(int *__restrict__ parent_all, int npix, int tiles,
                                                            const int *__restrict__ tile_offset) {
    const Tile w = tile_of_block(tiles, npix, CC_TILE);
    int *parent = parent_all + w.base;
    const long long p0 = (long long)w.p0 + threadIdx.x * CC_ITEMS;
    unsigned flags;
    const int n = root_flags(parent, p0, npix, &flags);
    int total;
    int rank = tile_offset[blockIdx.x] + block_exclusive_scan(n, &total);
    for (int k = 0; k < CC_ITEMS; ++k)
        if (flags >> k & 1u) parent[p0 + k] = -(rank++ + 2);
}

// A pixel reads its own cell (nobody else writes it) and, unless it is a root, the cell of its root, which may or may not
// have been rewritten by the root's own thread yet: -(k + 2) before, k + 1 after -- one label either way.
__global__ __launch_bounds__(CC_THREADS) void cc_relabel_kernel(int *__restrict__ parent_all, int npix, int tiles) {
    const Tile w = tile_of_block(tiles, npix, CC_TILE);
    int *cell = parent_all + w.base;
    for (int k = 0; k < CC_ITEMS; ++k) {
        const long long pl = (long long)w.p0 + k * CC_THREADS + threadIdx.x;
        if (pl >= npix) continue;
        const int p = (int)pl;
        const int v = load_parent(cell, p);
        int label = 0;
        if (v <= -2) {
            label = -v - 1;
        } else if (v >= 0) {
            const int x = load_parent(cell, v);
            label = x < 0 ? -x - 1 : x;
        }
        store_parent(cell, p, label);
    }
}

// ------------------------------------------------------------------ per-component sums
// a double as an unsigned integer of the same order; 0 and ~0 are the keys of no number
__device__ __forceinline__ unsigned long long order_key(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double key_value(unsigned long long k) {
    if (k == 0ull || k == ~0ull) return __longlong_as_double(0x7ff8000000000000ll);   // no pixel, or a NaN among them
    const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)b);
}

struct SumsOut {
    int *root;                        // [n_members][n_max] first pixel of the component (linear index in its plane)
    long long *area;                  // [n_members][n_max]
    long long *mom;                   // [5][n_members][n_max]: sum dr, dc, dr^2, dr dc, dc^2
    double *sum;                      // [n_members][n_max], or NULL with the two below
    unsigned long long *kmax, *kmin;  // order keys while the sums run, doubles after cs_finish_kernel
};

__global__ void cs_init_kernel(SumsOut o, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        o.root[i] = INT_MAX;
        o.area[i] = 0;
        for (int k = 0; k < 5; ++k) o.mom[k * n + i] = 0;
        if (o.sum) {
            o.sum[i] = 0.0;
            o.kmax[i] = 0ull;
            o.kmin[i] = ~0ull;
        }
    }
}

// labels this plane measures: 1 .. min(counts[m], n_max)
__device__ __forceinline__ int plane_capacity(const int *counts, int m, int n_max) {
    const int c = counts[m];
    return c < n_max ? c : n_max;
}

// The first pixel of every component.  Only a pixel whose western and northern neighbours do not carry its label can be the
// first of it (either would be an earlier pixel of the same component under both connectivities): few pixels ask.
__global__ __launch_bounds__(CC_THREADS) void cs_root_kernel(const int *__restrict__ labels_all, int nx, int npix, int tiles,
                                                            const int *__restrict__ counts, int n_max, int *__restrict__ root) {
    const int m = blockIdx.x / tiles;
    const Tile w = tile_of_block(tiles, npix, CC_TILE);
    const int *labels = labels_all + w.base;
    const int cap = plane_capacity(counts, m, n_max);
    for (int k = 0; k < CC_ITEMS; ++k) {
        const long long pl = (long long)w.p0 + k * CC_THREADS + threadIdx.x;
        if (pl >= npix) continue;
        const int p = (int)pl, l = labels[p];
        if (l < 1 || l > cap) continue;
        const int c = p % nx;
        if ((c > 0 && labels[p - 1] == l) || (p >= nx && labels[p - nx] == l)) continue;
        atomicMin(root + (size_t)m * n_max + (l - 1), p);
    }
}

template <typename T>
__global__ __launch_bounds__(CC_THREADS) void cs_sums_kernel(const int *__restrict__ labels_all, const T *__restrict__ intensity_all,
                                                            int nx, int npix, int tiles, int cyclic,
                                                            const int *__restrict__ counts, int n_max, size_t n_slots, SumsOut o) {
    const int m = blockIdx.x / tiles;
    const Tile w = tile_of_block(tiles, npix, CS_TILE);
    const int *labels = labels_all + w.base;
    const T *intensity = intensity_all ? intensity_all + w.base : nullptr;
    const int cap = plane_capacity(counts, m, n_max);
    // a thread walks CS_ITEMS consecutive pixels and keeps the sums of the label it is on: one set of atomics per change of
    // label, not per pixel (neighbours in a row share their label)
    int cur = 0, rr = 0, rc = 0;
    long long area = 0, sr = 0, sc = 0, srr = 0, src = 0, scc = 0;
    double sv = 0.0;
    unsigned long long kmax = 0ull, kmin = ~0ull;
    auto flush = [&]() {
        if (!cur) return;
        const size_t i = (size_t)m * n_max + (cur - 1);
        atomicAdd((unsigned long long *)o.area + i, (unsigned long long)area);
        const long long s[5] = {sr, sc, srr, src, scc};
        for (int k = 0; k < 5; ++k)
            if (s[k]) atomicAdd((unsigned long long *)o.mom + k * n_slots + i, (unsigned long long)s[k]);   // two's complement: signed sums add up
        if (intensity) {
            atomicAdd(o.sum + i, sv);
            atomicMax(o.kmax + i, kmax);
            atomicMin(o.kmin + i, kmin);
        }
    };
    const long long p0 = (long long)w.p0 + (long long)threadIdx.x * CS_ITEMS;
    for (int k = 0; k < CS_ITEMS; ++k) {
        const long long pl = p0 + k;
        if (pl >= npix) break;
        const int p = (int)pl, l = labels[p];
        if (l < 1 || l > cap) continue;
        if (l != cur) {
            flush();
            cur = l;
            const int root = o.root[(size_t)m * n_max + (l - 1)];
            rr = root / nx;
            rc = root - rr * nx;
            area = sr = sc = srr = src = scc = 0;
            sv = 0.0;
            kmax = 0ull;
            kmin = ~0ull;
        }
        const int r = p / nx;
        long long dr = r - rr, dc = (p - r * nx) - rc;
        if (cyclic) {   // into [-(nx / 2), nx - nx / 2): the shorter way round
            if (dc >= nx - nx / 2) dc -= nx;
            else if (dc < -(nx / 2)) dc += nx;
        }
        ++area;
        sr += dr;
        sc += dc;
        srr += dr * dr;
        src += dr * dc;
        scc += dc * dc;
        if (intensity) {
            const double v = (double)intensity[p];
            sv += v;
            if (v != v) {   // a NaN is the largest and the smallest of its component
                kmax = ~0ull;
                kmin = 0ull;
            } else {
                const unsigned long long key = order_key(v);
                if (key > kmax) kmax = key;
                if (key < kmin) kmin = key;
            }
        }
    }
    flush();
}

// keys back to doubles, in place; a component that holds a NaN has a NaN sum whatever else it holds
__global__ void cs_finish_kernel(SumsOut o, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const unsigned long long kx = o.kmax[i], kn = o.kmin[i];
        ((double *)o.kmax)[i] = key_value(kx);
        ((double *)o.kmin)[i] = key_value(kn);
        if (o.root[i] == INT_MAX) o.root[i] = -1;   // no such component in this plane
    }
}

__global__ void cs_finish_roots_kernel(int *root, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        if (root[i] == INT_MAX) root[i] = -1;
}

// ------------------------------------------------------------------ area-weighted sums on the sphere
// The same walk as cs_sums_kernel with float64 sums: node (r, c) is the unit vector n = (fl(cl[r] cx[c]), fl(cl[r] sx[c]), sl[r]),
// d = fl(n - n(root)) per axis, w = fl(rw[r] cw[c]); the terms are w, fl(w d_i), fl(fl(w d_i) d_j) (i <= j) and fl(w v).  Nothing is
// contracted, so a host restatement forms the same terms bit for bit; the order of the sum is the only freedom (atomicAdd(double)).
constexpr int SP_SUMS = 11;      // W, M1 x y z, M2 xx xy xz yy yz zz, S
constexpr int SP_PROPS = 8;      // area, major, minor, centroid latitude, centroid longitude, orientation, mean, total
constexpr int SP_SWEEPS = 8;     // cyclic Jacobi sweeps of the 3 x 3 solve: it converges quadratically, 5 leave nothing to rotate

struct SphereTables {
    const double *cl, *sl, *rw;   // [ny]
    const double *cx, *sx, *cw;   // [nx]
};

struct SphereOut {
    int *root;                        // [n_members][n_max]
    double *sums;                     // [SP_SUMS][n_members][n_max]
    unsigned long long *kmax, *kmin;  // order keys while the sums run, doubles after sp_finish_kernel; NULL without an intensity
    double *props;                    // [SP_PROPS][n_members][n_max], or NULL
};

__global__ void sp_init_kernel(SphereOut o, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        o.root[i] = INT_MAX;
        for (int k = 0; k < SP_SUMS; ++k) o.sums[k * n + i] = 0.0;
        if (o.kmax) {
            o.kmax[i] = 0ull;
            o.kmin[i] = ~0ull;
        }
    }
}

template <typename T>
__global__ __launch_bounds__(CC_THREADS) void sp_sums_kernel(const int *__restrict__ labels_all, const T *__restrict__ intensity_all,
                                                            int nx, int npix, int tiles, const int *__restrict__ counts, int n_max,
                                                            size_t n_slots, SphereTables g, SphereOut o) {
#pragma clang fp contract(off)
    const int m = blockIdx.x / tiles;
    const Tile w = tile_of_block(tiles, npix, CS_TILE);
    const int *labels = labels_all + w.base;
    const T *intensity = intensity_all ? intensity_all + w.base : nullptr;
    const int cap = plane_capacity(counts, m, n_max);
    int cur = 0;
    double x0 = 0.0, y0 = 0.0, z0 = 0.0;   // the node of the root of `cur`
    double acc[SP_SUMS];
#pragma unroll
    for (int k = 0; k < SP_SUMS; ++k) acc[k] = 0.0;
    unsigned long long kmax = 0ull, kmin = ~0ull;
    auto flush = [&]() {   // atomics only: no arithmetic of the sums happens in here
        if (!cur) return;
        const size_t i = (size_t)m * n_max + (cur - 1);
        atomicAdd(o.sums + i, acc[0]);
#pragma unroll
        for (int k = 1; k < SP_SUMS - 1; ++k)
            if (acc[k] != 0.0) atomicAdd(o.sums + k * n_slots + i, acc[k]);   // a NaN is != 0; the root pixel itself adds nothing
        if (intensity) {
            atomicAdd(o.sums + (SP_SUMS - 1) * n_slots + i, acc[SP_SUMS - 1]);
            atomicMax(o.kmax + i, kmax);
            atomicMin(o.kmin + i, kmin);
        }
    };
    const long long p0 = (long long)w.p0 + (long long)threadIdx.x * CS_ITEMS;
    for (int k = 0; k < CS_ITEMS; ++k) {
        const long long pl = p0 + k;
        if (pl >= npix) break;
        const int p = (int)pl, l = labels[p];
        if (l < 1 || l > cap) continue;
        if (l != cur) {
            flush();
            cur = l;
            const int root = o.root[(size_t)m * n_max + (l - 1)];   // a pixel of the plane: cs_root_kernel saw this label
            const int rr = root / nx, rc = root - rr * nx;
            const double c = g.cl[rr];
            x0 = c * g.cx[rc];
            y0 = c * g.sx[rc];
            z0 = g.sl[rr];
#pragma unroll
            for (int j = 0; j < SP_SUMS; ++j) acc[j] = 0.0;
            kmax = 0ull;
            kmin = ~0ull;
        }
        const int r = p / nx, c = p - r * nx;
        const double clr = g.cl[r];
        const double dx = clr * g.cx[c] - x0, dy = clr * g.sx[c] - y0, dz = g.sl[r] - z0;
        const double wt = g.rw[r] * g.cw[c];
        const double wx = wt * dx, wy = wt * dy, wz = wt * dz;
        acc[0] += wt;
        acc[1] += wx;
        acc[2] += wy;
        acc[3] += wz;
        acc[4] += wx * dx;
        acc[5] += wx * dy;
        acc[6] += wx * dz;
        acc[7] += wy * dy;
        acc[8] += wy * dz;
        acc[9] += wz * dz;
        if (intensity) {
            const double v = (double)intensity[p];
            acc[10] += wt * v;
            if (v != v) {   // a NaN is the largest and the smallest of its component
                kmax = ~0ull;
                kmin = 0ull;
            } else {
                const unsigned long long key = order_key(v);
                if (key > kmax) kmax = key;
                if (key < kmin) kmin = key;
            }
        }
    }
    flush();
}

// one rotation of the cyclic Jacobi method on the symmetric 3 x 3 `a`: it zeroes a[P][Q]; R is the third index.  v collects
// the rotations: its columns become the eigenvectors.  No data-dependent loop; an element that is 0 already is left alone.
template <int P, int Q, int R>
__device__ __forceinline__ void jacobi_rotate(double (&a)[3][3], double (&v)[3][3]) {
    const double apq = a[P][Q];
    if (apq == 0.0) return;
    const double theta = (a[Q][Q] - a[P][P]) / (2.0 * apq);
    // the smaller root of t^2 + 2 theta t - 1: |t| <= 1; a theta whose square overflows gives t = 0
    const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + __dsqrt_rn(theta * theta + 1.0));
    const double c = 1.0 / __dsqrt_rn(t * t + 1.0), s = t * c;
    a[P][P] -= t * apq;
    a[Q][Q] += t * apq;
    a[P][Q] = a[Q][P] = 0.0;
    const double arp = a[R][P], arq = a[R][Q];
    a[R][P] = a[P][R] = c * arp - s * arq;
    a[R][Q] = a[Q][R] = s * arp + c * arq;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double vp = v[k][P], vq = v[k][Q];
        v[k][P] = c * vp - s * vq;
        v[k][Q] = s * vp + c * vq;
    }
}

// One thread per (plane, label): keys back to doubles, the sums into properties.
__global__ __launch_bounds__(CC_THREADS) void sp_finish_kernel(SphereOut o, size_t n, int nx, double radius, SphereTables g) {
    const double nan = __longlong_as_double(0x7ff8000000000000ll), deg = 57.29577951308232;   // 180 / pi
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        if (o.kmax) {
            const unsigned long long kx = o.kmax[i], kn = o.kmin[i];
            ((double *)o.kmax)[i] = key_value(kx);
            ((double *)o.kmin)[i] = key_value(kn);
        }
        const int root = o.root[i];
        const bool empty = root == INT_MAX;
        if (empty) o.root[i] = -1;   // no such label in this plane
        if (!o.props) continue;
        double *q = o.props + i;
        if (empty) {
            q[0] = 0.0;
            for (int k = 1; k < SP_PROPS; ++k) q[k * n] = nan;
            continue;
        }
        const double *s = o.sums + i;
        const double W = s[0];
        const double mx = s[1 * n] / W, my = s[2 * n] / W, mz = s[3 * n] / W;
        double a[3][3], v[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
        a[0][0] = s[4 * n] / W - mx * mx;
        a[0][1] = a[1][0] = s[5 * n] / W - mx * my;
        a[0][2] = a[2][0] = s[6 * n] / W - mx * mz;
        a[1][1] = s[7 * n] / W - my * my;
        a[1][2] = a[2][1] = s[8 * n] / W - my * mz;
        a[2][2] = s[9 * n] / W - mz * mz;
#pragma unroll 1
        for (int sweep = 0; sweep < SP_SWEEPS; ++sweep) {
            jacobi_rotate<0, 1, 2>(a, v);
            jacobi_rotate<0, 2, 1>(a, v);
            jacobi_rotate<1, 2, 0>(a, v);
        }
        // e1 >= e2 >= e3 and the eigenvector of e1, by selects: no indexing by a value
        const double d0 = a[0][0], d1 = a[1][1], d2 = a[2][2];
        const int i1 = (d0 >= d1 && d0 >= d2) ? 0 : (d1 >= d2 ? 1 : 2);
        const double e1 = i1 == 0 ? d0 : (i1 == 1 ? d1 : d2);
        const double ra = i1 == 0 ? d1 : d0, rb = i1 == 2 ? d1 : d2;   // the other two
        const double e2 = ra >= rb ? ra : rb;
        const double vx = i1 == 0 ? v[0][0] : (i1 == 1 ? v[0][1] : v[0][2]);
        const double vy = i1 == 0 ? v[1][0] : (i1 == 1 ? v[1][1] : v[1][2]);
        const double vz = i1 == 0 ? v[2][0] : (i1 == 1 ? v[2][1] : v[2][2]);
        const double r2 = radius * radius;
        q[0] = r2 * W;
        q[1 * n] = 4.0 * radius * __dsqrt_rn(e1 > 0.0 ? e1 : (e1 == e1 ? 0.0 : e1));
        q[2 * n] = 4.0 * radius * __dsqrt_rn(e2 > 0.0 ? e2 : (e2 == e2 ? 0.0 : e2));
        // the centroid: the root's node plus the mean offset, as a direction
        const int rr = root / nx, rc = root - rr * nx;
        const double cx = g.cl[rr] * g.cx[rc] + mx, cy = g.cl[rr] * g.sx[rc] + my, cz = g.sl[rr] + mz;
        const double h = __dsqrt_rn(cx * cx + cy * cy), rho = __dsqrt_rn(cx * cx + cy * cy + cz * cz);
        double lat = nan, lon = nan, orient = nan;
        if (rho >= 1e-6) {
            lat = atan2(cz, h);   // asin(cz / rho), in the form that keeps its accuracy at the poles
            lon = atan2(cy, cx);
            if (e1 > 0.0) {
                const double sphi = sin(lat), cphi = cos(lat), slam = sin(lon), clam = cos(lon);
                const double ve = vy * clam - vx * slam;
                const double vn = vz * cphi - sphi * (vx * clam + vy * slam);
                double t = atan2(vn, ve) * deg;   // (-180, 180]: the axis has no sign, fold into (-90, 90]
                if (t > 90.0) t -= 180.0;
                else if (t <= -90.0) t += 180.0;
                orient = t;
            }
            lat *= deg;
            lon *= deg;
        }
        q[3 * n] = lat;
        q[4 * n] = lon;
        q[5 * n] = orient;
        q[6 * n] = o.kmax ? s[10 * n] / W : nan;
        q[7 * n] = o.kmax ? r2 * s[10 * n] : nan;
    }
}

// ------------------------------------------------------------------ apply
template <typename T>
__global__ __launch_bounds__(CC_THREADS) void cc_apply_kernel(const int *__restrict__ labels, const T *__restrict__ mask,
                                                             const unsigned char *__restrict__ keep, int npix, int tiles, int n_max,
                                                             T fill, T *__restrict__ out) {
    const int m = blockIdx.x / tiles;
    const Tile w = tile_of_block(tiles, npix, CC_TILE);
    for (int k = 0; k < CC_ITEMS; ++k) {
        const long long p = (long long)w.p0 + k * CC_THREADS + threadIdx.x;
        if (p >= npix) continue;
        const int l = labels[w.base + p];
        const bool kept = l >= 1 && l <= n_max && keep[(size_t)m * n_max + (l - 1)];
        out[w.base + p] = kept ? mask[w.base + p] : fill;
    }
}

int grid_cap(size_t n) {
    const size_t b = (n + 255) / 256;
    return (int)(b < 4096 ? b : 4096);
}

}  // namespace

// What every entry point checks before it touches the device; *tiles: workgroups per plane at `tile_pixels` pixels each.
static int components_geometry(const char *who, const lc_ctx *ctx, int dtype, int ny, int nx, int n_members, int tile_pixels,
                               int *tiles) {
    LC_REQUIRE(ctx, "%s: null context", who);
    LC_REQUIRE(dtype == LC_F32 || dtype == LC_F64, "%s: bad dtype %d (LC_F32 or LC_F64)", who, dtype);
    LC_REQUIRE(ny >= 1 && nx >= 1 && n_members >= 1, "%s: bad size ny=%d nx=%d n_members=%d (each >= 1)", who, ny, nx, n_members);
    const long long npix = (long long)ny * nx;
    LC_REQUIRE(npix < (1ll << 31), "%s: plane too large: %d x %d = %lld pixels, labels are int32 (< 2^31)", who, ny, nx, npix);
    const long long t = (npix + tile_pixels - 1) / tile_pixels;
    LC_REQUIRE(t * n_members <= (long long)INT_MAX, "%s: too many planes: %d of %lld workgroups each", who, n_members, t);
    *tiles = (int)t;
    return LC_OK;
}

extern "C" size_t lc_label_work_elems(int ny, int nx, int n_members) {
    if (ny < 1 || nx < 1 || n_members < 1) return 0;
    const unsigned long long npix = (unsigned long long)ny * (unsigned long long)nx;
    return (size_t)((npix + CC_TILE - 1) / CC_TILE) * (size_t)n_members;
}

extern "C" int lc_label_components(lc_ctx *ctx, const void *mask, int dtype, int ny, int nx, int n_members, int connectivity,
                                   int cyclic_x, void *labels_out, void *counts_out, void *work_dev) {
    int tiles = 0;
    const int st = components_geometry("lc_label_components", ctx, dtype, ny, nx, n_members, CC_TILE, &tiles);
    if (st != LC_OK) return st;
    LC_REQUIRE(connectivity == 1 || connectivity == 2, "lc_label_components: bad connectivity %d (1: edges, 2: edges and corners)",
               connectivity);
    LC_REQUIRE(mask && labels_out && counts_out && work_dev, "lc_label_components: null pointer");
    LC_HIP_CHECK(hipSetDevice(ctx->device));
    const int npix = ny * nx;
    const dim3 grid((unsigned)(tiles * n_members)), block(CC_THREADS);
    int *parent = (int *)labels_out, *tile_roots = (int *)work_dev;
    if (dtype == LC_F32)
        hipLaunchKernelGGL(cc_init_kernel<float>, grid, block, 0, ctx->stream, (const float *)mask, parent, npix, tiles);
    else
        hipLaunchKernelGGL(cc_init_kernel<double>, grid, block, 0, ctx->stream, (const double *)mask, parent, npix, tiles);
    hipLaunchKernelGGL(cc_merge_kernel, grid, block, 0, ctx->stream, parent, ny, nx, npix, tiles, connectivity == 2 ? 1 : 0,
                       cyclic_x ? 1 : 0);
    hipLaunchKernelGGL(cc_flatten_kernel, grid, block, 0, ctx->stream, parent, npix, tiles, tile_roots);
    hipLaunchKernelGGL(cc_scan_tiles_kernel, dim3((unsigned)n_members), block, 0, ctx->stream, tile_roots, tiles, (int *)counts_out);
    hipLaunchKernelGGL(cc_rank_kernel, grid, block, 0, ctx->stream, parent, npix, tiles, (const int *)tile_roots);
    hipLaunchKernelGGL(cc_relabel_kernel, grid, block, 0, ctx->stream, parent, npix, tiles);
    LC_HIP_CHECK(hipGetLastError());
    return LC_OK;
}

extern "C" int lc_component_sums(lc_ctx *ctx, const lc_component_sums_args *a) {
    LC_REQUIRE(a, "lc_component_sums: null argument structure");
    LC_REQUIRE(a->struct_size == sizeof(lc_component_sums_args), "lc_component_sums: struct_size %zu, this library has %zu",
               (size_t)a->struct_size, sizeof(lc_component_sums_args));
    int tiles = 0, tiles_root = 0;
    int st = components_geometry("lc_component_sums", ctx, a->dtype, a->ny, a->nx, a->n_members, CS_TILE, &tiles);
    if (st == LC_OK) st = components_geometry("lc_component_sums", ctx, a->dtype, a->ny, a->nx, a->n_members, CC_TILE, &tiles_root);
    if (st != LC_OK) return st;
    LC_REQUIRE(a->n_max >= 1, "lc_component_sums: bad capacity n_max=%d (>= 1)", a->n_max);
    LC_REQUIRE(a->labels && a->counts && a->root_out && a->area_out && a->moments_out, "lc_component_sums: null pointer");
    LC_REQUIRE(!a->intensity || (a->sum_out && a->max_out && a->min_out),
               "lc_component_sums: null pointer (an intensity needs sum_out, max_out and min_out)");
    // the second moments are exact int64 sums: npix * max(ny, nx)^2 bounds each of them
    const double side = a->ny > a->nx ? a->ny : a->nx;
    LC_REQUIRE((double)a->ny * a->nx * side * side < 9.0e18, "lc_component_sums: plane too large: the second moments of %d x %d do not fit int64",
               a->ny, a->nx);
    LC_HIP_CHECK(hipSetDevice(ctx->device));
    const int npix = a->ny * a->nx;
    const size_t n_slots = (size_t)a->n_members * (size_t)a->n_max;
    SumsOut o;
    o.root = (int *)a->root_out;
    o.area = (long long *)a->area_out;
    o.mom = (long long *)a->moments_out;
    o.sum = a->intensity ? (double *)a->sum_out : nullptr;
    o.kmax = a->intensity ? (unsigned long long *)a->max_out : nullptr;
    o.kmin = a->intensity ? (unsigned long long *)a->min_out : nullptr;
    const dim3 block(CC_THREADS);
    hipLaunchKernelGGL(cs_init_kernel, dim3(grid_cap(n_slots)), block, 0, ctx->stream, o, n_slots);
    hipLaunchKernelGGL(cs_root_kernel, dim3((unsigned)(tiles_root * a->n_members)), block, 0, ctx->stream, (const int *)a->labels, a->nx,
                       npix, tiles_root, (const int *)a->counts, a->n_max, o.root);
    const dim3 grid((unsigned)(tiles * a->n_members));
    if (a->dtype == LC_F32)
        hipLaunchKernelGGL(cs_sums_kernel<float>, grid, block, 0, ctx->stream, (const int *)a->labels, (const float *)a->intensity, a->nx,
                           npix, tiles, a->cyclic_x ? 1 : 0, (const int *)a->counts, a->n_max, n_slots, o);
    else
        hipLaunchKernelGGL(cs_sums_kernel<double>, grid, block, 0, ctx->stream, (const int *)a->labels, (const double *)a->intensity, a->nx,
                           npix, tiles, a->cyclic_x ? 1 : 0, (const int *)a->counts, a->n_max, n_slots, o);
    if (a->intensity)
        hipLaunchKernelGGL(cs_finish_kernel, dim3(grid_cap(n_slots)), block, 0, ctx->stream, o, n_slots);
    else
        hipLaunchKernelGGL(cs_finish_roots_kernel, dim3(grid_cap(n_slots)), block, 0, ctx->stream, o.root, n_slots);
    LC_HIP_CHECK(hipGetLastError());
    return LC_OK;
}

extern "C" int lc_component_sphere_sums(lc_ctx *ctx, const lc_component_sphere_sums_args *a) {
    const char *who = "lc_component_sphere_sums";
    LC_REQUIRE(ctx, "%s: null context", who);
    LC_REQUIRE(a, "%s: null argument structure", who);
    LC_REQUIRE(a->struct_size == sizeof(lc_component_sphere_sums_args), "%s: struct_size %zu, this library has %zu", who,
               (size_t)a->struct_size, sizeof(lc_component_sphere_sums_args));
    int tiles = 0, tiles_root = 0;
    int st = components_geometry(who, ctx, a->dtype, a->ny, a->nx, a->n_members, CS_TILE, &tiles);
    if (st == LC_OK) st = components_geometry(who, ctx, a->dtype, a->ny, a->nx, a->n_members, CC_TILE, &tiles_root);
    if (st != LC_OK) return st;
    LC_REQUIRE(a->n_max >= 1, "%s: bad capacity n_max=%d (>= 1)", who, a->n_max);
    LC_REQUIRE(a->radius > 0.0 && a->radius < INFINITY, "%s: bad radius %g: > 0 and finite", who, a->radius);
    LC_REQUIRE(a->labels && a->counts && a->root_out && a->sums_out, "%s: null pointer", who);
    LC_REQUIRE(a->cos_lat && a->sin_lat && a->row_weight && a->cos_lon && a->sin_lon && a->col_weight, "%s: null pointer (six tables)", who);
    LC_REQUIRE(!a->intensity || (a->max_out && a->min_out), "%s: null pointer (an intensity needs max_out and min_out)", who);
    LC_HIP_CHECK(hipSetDevice(ctx->device));
    const int npix = a->ny * a->nx;
    const size_t n_slots = (size_t)a->n_members * (size_t)a->n_max;
    SphereOut o;
    o.root = (int *)a->root_out;
    o.sums = (double *)a->sums_out;
    o.kmax = a->intensity ? (unsigned long long *)a->max_out : nullptr;
    o.kmin = a->intensity ? (unsigned long long *)a->min_out : nullptr;
    o.props = (double *)a->props_out;
    const SphereTables g{a->cos_lat, a->sin_lat, a->row_weight, a->cos_lon, a->sin_lon, a->col_weight};
    const dim3 block(CC_THREADS);
    hipLaunchKernelGGL(sp_init_kernel, dim3(grid_cap(n_slots)), block, 0, ctx->stream, o, n_slots);
    hipLaunchKernelGGL(cs_root_kernel, dim3((unsigned)(tiles_root * a->n_members)), block, 0, ctx->stream, (const int *)a->labels, a->nx,
                       npix, tiles_root, (const int *)a->counts, a->n_max, o.root);
    const dim3 grid((unsigned)(tiles * a->n_members));
    if (a->dtype == LC_F32)
        hipLaunchKernelGGL(sp_sums_kernel<float>, grid, block, 0, ctx->stream, (const int *)a->labels, (const float *)a->intensity, a->nx,
                           npix, tiles, (const int *)a->counts, a->n_max, n_slots, g, o);
    else
        hipLaunchKernelGGL(sp_sums_kernel<double>, grid, block, 0, ctx->stream, (const int *)a->labels, (const double *)a->intensity, a->nx,
                           npix, tiles, (const int *)a->counts, a->n_max, n_slots, g, o);
    hipLaunchKernelGGL(sp_finish_kernel, dim3(grid_cap(n_slots)), block, 0, ctx->stream, o, n_slots, a->nx, a->radius, g);
    LC_HIP_CHECK(hipGetLastError());
    return LC_OK;
}

extern "C" int lc_component_apply(lc_ctx *ctx, const void *labels, const void *mask, int dtype, int ny, int nx, int n_members,
                                  const void *keep, int n_max, double fill, void *mask_out) {
    int tiles = 0;
    const int st = components_geometry("lc_component_apply", ctx, dtype, ny, nx, n_members, CC_TILE, &tiles);
    if (st != LC_OK) return st;
    LC_REQUIRE(n_max >= 1, "lc_component_apply: bad capacity n_max=%d (>= 1)", n_max);
    LC_REQUIRE(labels && mask && keep && mask_out, "lc_component_apply: null pointer");
    LC_HIP_CHECK(hipSetDevice(ctx->device));
    const int npix = ny * nx;
    const dim3 grid((unsigned)(tiles * n_members)), block(CC_THREADS);
    if (dtype == LC_F32)
        hipLaunchKernelGGL(cc_apply_kernel<float>, grid, block, 0, ctx->stream, (const int *)labels, (const float *)mask,
                           (const unsigned char *)keep, npix, tiles, n_max, (float)fill, (float *)mask_out);
    else
        hipLaunchKernelGGL(cc_apply_kernel<double>, grid, block, 0, ctx->stream, (const int *)labels, (const double *)mask,
                           (const unsigned char *)keep, npix, tiles, n_max, fill, (double *)mask_out);
    LC_HIP_CHECK(hipGetLastError());
    return LC_OK;
}
