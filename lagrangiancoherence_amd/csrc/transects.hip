// Great-circle transects across ridge lines and their per-line composites: the device side of tools.ridge_transects, the
// well-defined part of find_area (LCS/area_of_influence.py:17-87, a Python loop that paints pixels along the Hessian eigenvector
// of every ridge pixel, stepping in degrees).  Here a second field is sampled along the great circle through each point of a traced
// line (Engine.trace_lines), at right angles to the line, at the signed distances s_k = k spacing.  include/lcs_hip.h states the
// definition, tests/transects.py restates it point by point in numpy, tests/test_transects_gpu.py compares the two.
//
// The host hands over the four sphere tables of the grid (numpy's cos / sin of the coordinates, as lc_sphere_distance takes
// them), the ascending coordinates in degrees and the tables cos(s_k / radius), sin(s_k / radius): no kernel evaluates a
// trigonometric function of a coordinate or of a distance; the only library function on the device is atan2, twice per sample.
// Every kernel forbids contraction: up to atan2 the arithmetic is numpy's, operation for operation.
//   normal     one thread per point.  p = (cl cx, cl sx, sl) of the point's pixel; the chord d = p_b - p_a over the points
//              `smooth` before and after it within its line (clamped at the ends of an open line, wrapped on a ring with smooth
//              capped at (count - 1) / 2); t = (d - (d.p) p) / |d - (d.p) p|; the left normal n = p x t, flipped by `orient`;
//              east and north components of n and t against the point's own column.  NaN where a == b or |t| is not > 0.
//   sample     one thread per (point, k), k fastest: q = c_k p + s_k n, latitude = atan2(q_z, sqrt(q_x q_x + q_y q_y)), longitude
//              = atan2(q_y, q_x), both in degrees, the longitude wrapped into [lon[0], lon[0] + 360) with cyclic_x; the position is
//              formed and stored once, the cell found once by binary search from the stored position, and up to TR_FIELDS fields of
//              the point's plane are interpolated in that launch, their values held in registers (no scratch).
//   composite  one workgroup per (line, field): the line's values are one contiguous block [count][M]; thread t adds the
//              elements t, t + stride, t + 2 stride, ... (stride = the largest multiple of M within TR_CHUNK, so a thread stays in
//              one column) in ascending order, and the thread of the column's first slot adds the slots' partial sums from LDS in
//              ascending order.  With M > TR_CHUNK the columns are taken TR_CHUNK at a time.  The order is a function of the
//              sizes alone: two calls give the same bits.
// What bounds them: normal reads three pixels' tables and writes 56 bytes per point -- latency of dependent gathers, a few
// microseconds at any size met.  sample is bound by its two atan2 (some hundred float64 vector instructions each) and the two
// binary searches (log2 ny + log2 nx dependent loads from tables that stay in L1 / L2) beside four gathers per field; stores
// coalesce along k.  composite reads every value once, coalesced, and is bound by the longest line: a line is one workgroup.
// No kernel waits for another workgroup: there is no flag, no atomic, no fence and no grid synchronisation in this file.
#include <climits>
#include <cmath>
#include <cstdint>

#include "lcs_common.h"

namespace {

constexpr int TR_THREADS = 256;
constexpr int TR_CHUNK = 256;    // elements (points x offsets) of a line a composite workgroup adds per pass: one per thread
constexpr int TR_FIELDS = 4;     // fields per sample launch: 4 values and 4 weights in registers, no scratch
constexpr double TR_DEG = 57.29577951308232;   // 180 / pi rounded to float64: numpy's 180.0 / np.pi

struct Lines {
    const int *pixel;        // [n_points] linear index into the point's plane
    const int *point_line;   // [n_points]
    const int *offset, *count, *plane;   // [n_lines]
    const unsigned char *closed;         // [n_lines]
    const double *cl, *sl, *cx, *sx;     // [ny], [ny], [nx], [nx]
    int ny, nx, n_points, n_lines, n_planes;
};

// the unit vector of a pixel: one rounded product per component
__device__ __forceinline__ void unit_of(const Lines &g, int pix, double &x, double &y, double &z) {
#pragma clang fp contract(off)
    const int r = pix / g.nx, c = pix - r * g.nx;
    x = g.cl[r] * g.cx[c];
    y = g.cl[r] * g.sx[c];
    z = g.sl[r];
}

// out: [7][n_points] -- n_x, n_y, n_z, n_east, n_north, t_east, t_north
__global__ __launch_bounds__(TR_THREADS) void transect_normal_kernel(Lines g, int smooth, int orient, double *__restrict__ out) {
#pragma clang fp contract(off)
    const long long i = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
    if (i >= g.n_points) return;
    double o[7];
#pragma unroll
    for (int q = 0; q < 7; ++q) o[q] = NAN;
    const int l = g.point_line[i];
    const int pix = g.pixel[i];
    const long long npix = (long long)g.ny * g.nx;
    if (l >= 0 && l < g.n_lines && pix >= 0 && pix < npix) {
        const long long off = g.offset[l], cnt = g.count[l], j = i - off;
        if (off >= 0 && cnt >= 1 && off + cnt <= g.n_points && j >= 0 && j < cnt) {
            long long a, b;
            if (g.closed[l]) {
                const long long m = smooth < (cnt - 1) / 2 ? smooth : (cnt - 1) / 2;
                a = (j - m + cnt) % cnt;
                b = (j + m) % cnt;
            } else {
                a = j - smooth > 0 ? j - smooth : 0;
                b = j + smooth < cnt - 1 ? j + smooth : cnt - 1;
            }
            const int pa = g.pixel[off + a], pb = g.pixel[off + b];
            if (a != b && pa >= 0 && pa < npix && pb >= 0 && pb < npix) {
                double px, py, pz, ax, ay, az, bx, by, bz;
                unit_of(g, pix, px, py, pz);
                unit_of(g, pa, ax, ay, az);
                unit_of(g, pb, bx, by, bz);
                const double dx = bx - ax, dy = by - ay, dz = bz - az;
                const double dot = (dx * px + dy * py) + dz * pz;
                double tx = dx - dot * px, ty = dy - dot * py, tz = dz - dot * pz;
                const double len = __dsqrt_rn((tx * tx + ty * ty) + tz * tz);
                if (len > 0.0) {
                    tx = tx / len;
                    ty = ty / len;
                    tz = tz / len;
                    double nx = py * tz - pz * ty, ny = pz * tx - px * tz, nz = px * ty - py * tx;
                    const int r = pix / g.nx, c = pix - r * g.nx;
                    const double cl = g.cl[r], sl = g.sl[r], cx = g.cx[c], sx = g.sx[c];
                    // east = (-sx, cx, 0), north = (-sl cx, -sl sx, cl): against the longitude of the point's own column
                    const double ux = -(sl * cx), uy = -(sl * sx);
                    double ne = cx * ny - sx * nx, nn = (ux * nx + uy * ny) + cl * nz;
                    const double te = cx * ty - sx * tx, tn = (ux * tx + uy * ty) + cl * tz;
                    const bool flip = orient == LC_ORIENT_NORTH ? (nn < 0.0 || (nn == 0.0 && ne < 0.0))
                                    : orient == LC_ORIENT_EAST ? (ne < 0.0 || (ne == 0.0 && nn < 0.0))
                                                               : false;
                    if (flip) {
                        nx = -nx;
                        ny = -ny;
                        nz = -nz;
                        ne = -ne;
                        nn = -nn;
                    }
                    o[0] = nx;
                    o[1] = ny;
                    o[2] = nz;
                    o[3] = ne;
                    o[4] = nn;
                    o[5] = te;
                    o[6] = tn;
                }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 7; ++q) out[(size_t)q * (size_t)g.n_points + (size_t)i] = o[q];
}

struct Sampling {
    const double *normal;             // [7][n_points]
    const double *lat, *lon;          // degrees, ascending: [ny], [nx]
    const double *cos_off, *sin_off;  // [M]
    double *lat_out, *lon_out;        // [n_points][M], or NULL after the first launch of a call
    int M, cyclic, nearest;
};

// the largest index whose coordinate is <= v, or -1: a counted binary search over n >= 1 ascending values
__device__ __forceinline__ int last_not_above(const double *__restrict__ t, int n, double v) {
    int lo = 0, hi = n;   // the answer + 1 lies in [lo, hi]
    for (int round = 0; round < 32 && lo < hi; ++round) {
        const int mid = lo + (hi - lo) / 2;
        if (t[mid] <= v)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo - 1;
}

template <typename T, int NF>
__global__ __launch_bounds__(TR_THREADS) void transect_sample_kernel(Lines g, Sampling s, const T *__restrict__ fields,
                                                                     T *__restrict__ values, int recompute) {
#pragma clang fp contract(off)
    const long long e = (long long)blockIdx.x * TR_THREADS + threadIdx.x;
    const long long total = (long long)g.n_points * s.M;   // < 2^31
    if (e >= total) return;
    const int i = (int)(e / s.M), k = (int)(e - (long long)i * s.M);
    const size_t np = (size_t)g.n_points;
    double y = NAN, x = NAN;
    if (recompute) {
        const double nx = s.normal[i], ny = s.normal[np + i], nz = s.normal[2 * np + i];
        const int pix = g.pixel[i];
        if (nx == nx && pix >= 0 && pix < (long long)g.ny * g.nx) {
            double px, py, pz;
            unit_of(g, pix, px, py, pz);
            const double c = s.cos_off[k], sn = s.sin_off[k];
            const double qx = c * px + sn * nx, qy = c * py + sn * ny, qz = c * pz + sn * nz;
            y = atan2(qz, __dsqrt_rn(qx * qx + qy * qy)) * TR_DEG;
            x = atan2(qy, qx) * TR_DEG;
            if (s.cyclic) {
                const double x0 = s.lon[0];
                x = x - floor((x - x0) / 360.0) * 360.0;
                if (x < x0) x = x + 360.0;
                if (x >= x0 + 360.0) x = x - 360.0;
            }
        }
        s.lat_out[e] = y;
        s.lon_out[e] = x;
    } else {   // a later launch of the same call: the position this thread's predecessor stored
        y = s.lat_out[e];
        x = s.lon_out[e];
    }
    // the cell, from the stored position by exact comparisons
    bool inside = false;
    int j0 = 0, j1 = 0, i0 = 0, i1 = 0;
    double wy = 0.0, wx = 0.0;
    const int l = g.point_line[i];
    const int plane = l >= 0 && l < g.n_lines ? g.plane[l] : -1;
    if (y >= s.lat[0] && y <= s.lat[g.ny - 1] && x >= s.lon[0] && plane >= 0 && plane < g.n_planes) {   // false for a NaN
        j0 = last_not_above(s.lat, g.ny, y);   // 0 .. ny - 1
        j1 = j0 + 1 < g.ny ? j0 + 1 : j0;
        const double ya = s.lat[j0], yb = s.lat[j1];
        i0 = last_not_above(s.lon, g.nx, x);   // 0 .. nx - 1
        double xa = s.lon[i0], xb;
        if (i0 + 1 < g.nx) {
            i1 = i0 + 1;
            xb = s.lon[i1];
            inside = true;
        } else if (s.cyclic) {   // the seam cell: between lon[nx - 1] and lon[0] + 360
            i1 = 0;
            xb = s.lon[0] + 360.0;
            inside = x < xb;
        } else {
            i1 = i0;
            xb = xa;
            inside = x <= xa;    // on the last column itself
        }
        if (s.nearest) {         // the nearer node in each axis, ties to the lower index
            if (y - ya > yb - y) j0 = j1;
            if (x - xa > xb - x) i0 = i1;
        } else {
            wy = j1 != j0 ? (y - ya) / (yb - ya) : 0.0;
            wx = i1 != i0 ? (x - xa) / (xb - xa) : 0.0;
        }
    }
    const size_t npix = (size_t)g.ny * (size_t)g.nx, per_field = (size_t)g.n_planes * npix;
    const size_t base = inside ? (size_t)plane * npix : 0;
    const double w00 = (1.0 - wy) * (1.0 - wx), w01 = (1.0 - wy) * wx, w10 = wy * (1.0 - wx), w11 = wy * wx;
    T res[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        double v = NAN;
        if (inside) {
            const T *pl = fields + (size_t)f * per_field + base;
            if (s.nearest) {
                v = (double)pl[(size_t)j0 * g.nx + i0];
            } else {
                const double v00 = (double)pl[(size_t)j0 * g.nx + i0], v01 = (double)pl[(size_t)j0 * g.nx + i1];
                const double v10 = (double)pl[(size_t)j1 * g.nx + i0], v11 = (double)pl[(size_t)j1 * g.nx + i1];
                v = ((w00 * v00 + w01 * v01) + w10 * v10) + w11 * v11;   // a NaN corner makes it NaN, whatever its weight
            }
        }
        res[f] = (T)v;
    }
#pragma unroll
    for (int f = 0; f < NF; ++f) values[(size_t)f * (size_t)total + (size_t)e] = res[f];
}

// grid (n_lines, n_fields); values [n_fields][n_points][M]; mean, count [n_fields][n_lines][M]
template <typename T>
__global__ __launch_bounds__(TR_THREADS) void transect_composite_kernel(Lines g, int M, const T *__restrict__ values,
                                                                        T *__restrict__ mean, int *__restrict__ count) {
#pragma clang fp contract(off)
    __shared__ double s_sum[TR_CHUNK];
    __shared__ int s_cnt[TR_CHUNK];
    const int l = blockIdx.x, f = blockIdx.y, t = threadIdx.x;
    long long off = g.offset[l], cnt = g.count[l];
    if (off < 0 || cnt < 0 || off + cnt > g.n_points) cnt = 0;   // a list that is not trace_lines': an empty line
    const T *block = values + ((size_t)f * (size_t)g.n_points + (size_t)off) * (size_t)M;
    const long long elems = cnt * M;
    for (int k0 = 0; k0 < M; k0 += TR_CHUNK) {   // uniform
        const int cols = M - k0 < TR_CHUNK ? M - k0 : TR_CHUNK;
        const int slots = TR_CHUNK / cols;       // >= 1; threads beyond slots * cols idle
        const int slot = t / cols, col = t - slot * cols;
        double sum = 0.0;
        int n = 0;
        if (slot < slots) {
            for (long long row = slot; row < cnt; row += slots) {
                const long long at = row * M + k0 + col;   // < elems
                const double v = at < elems ? (double)block[at] : NAN;
                if (isfinite(v)) {
                    sum += v;
                    ++n;
                }
            }
        }
        s_sum[t] = sum;
        s_cnt[t] = n;
        __syncthreads();
        if (slot == 0) {
            for (int q = 1; q < slots; ++q) {
                sum += s_sum[q * cols + col];
                n += s_cnt[q * cols + col];
            }
            const size_t o = ((size_t)f * (size_t)g.n_lines + (size_t)l) * (size_t)M + (size_t)(k0 + col);
            mean[o] = n > 0 ? (T)(sum / (double)n) : (T)NAN;
            count[o] = n;
        }
        __syncthreads();   // the partial sums are overwritten in the next round
    }
}

template <typename T>
void launch(lc_ctx *ctx, const lc_transects_args *a, const Lines &g, Sampling s) {
    const long long total = (long long)a->n_points * a->n_offsets;
    const dim3 block(TR_THREADS), grid((unsigned)((total + TR_THREADS - 1) / TR_THREADS));
    const size_t per_field = (size_t)a->n_planes * (size_t)a->ny * (size_t)a->nx;
    for (int f0 = 0; f0 < a->n_fields; f0 += TR_FIELDS) {
        const int nf = a->n_fields - f0 < TR_FIELDS ? a->n_fields - f0 : TR_FIELDS;
        const T *fields = (const T *)a->fields + (size_t)f0 * per_field;
        T *values = (T *)a->values_out + (size_t)f0 * (size_t)total;
        const int first = f0 == 0;
        switch (nf) {
            case 1: hipLaunchKernelGGL((transect_sample_kernel<T, 1>), grid, block, 0, ctx->stream, g, s, fields, values, first); break;
            case 2: hipLaunchKernelGGL((transect_sample_kernel<T, 2>), grid, block, 0, ctx->stream, g, s, fields, values, first); break;
            case 3: hipLaunchKernelGGL((transect_sample_kernel<T, 3>), grid, block, 0, ctx->stream, g, s, fields, values, first); break;
            default: hipLaunchKernelGGL((transect_sample_kernel<T, 4>), grid, block, 0, ctx->stream, g, s, fields, values, first); break;
        }
    }
    hipLaunchKernelGGL(transect_composite_kernel<T>, dim3((unsigned)a->n_lines, (unsigned)a->n_fields), block, 0, ctx->stream, g,
                       a->n_offsets, (const T *)a->values_out, (T *)a->mean_out, (int *)a->count_out);
}

}  // namespace

extern "C" const char *lc_ctx_last_transects_kernel(const lc_ctx *ctx) { return ctx ? ctx->last_transects_kernel : ""; }

extern "C" int lc_ridge_transects(lc_ctx *ctx, const lc_transects_args *a) {
    const char *who = "lc_ridge_transects";
    LC_REQUIRE(ctx, "%s: null context", who);
    LC_REQUIRE(a, "%s: null argument structure", who);
    LC_REQUIRE(a->struct_size == sizeof(lc_transects_args), "%s: struct_size %zu, this library has %zu", who,
               (size_t)a->struct_size, sizeof(lc_transects_args));
    LC_REQUIRE(a->dtype == LC_F32 || a->dtype == LC_F64, "%s: bad dtype %d (LC_F32 or LC_F64)", who, a->dtype);
    LC_REQUIRE(a->ny >= 2 && a->nx >= 2 && a->n_planes >= 1 && a->n_points >= 1 && a->n_lines >= 1 && a->n_fields >= 1,
               "%s: bad size ny=%d nx=%d n_planes=%d n_points=%d n_lines=%d n_fields=%d (ny, nx >= 2, the others >= 1)", who, a->ny,
               a->nx, a->n_planes, a->n_points, a->n_lines, a->n_fields);
    LC_REQUIRE(a->n_offsets >= 1 && a->n_offsets % 2 == 1, "%s: bad n_offsets %d: 2 K + 1 with K >= 0", who, a->n_offsets);
    LC_REQUIRE(a->smooth >= 1, "%s: bad smooth %d: >= 1", who, a->smooth);
    LC_REQUIRE(a->orient == LC_ORIENT_LEFT || a->orient == LC_ORIENT_NORTH || a->orient == LC_ORIENT_EAST,
               "%s: bad orient %d (LC_ORIENT_LEFT, LC_ORIENT_NORTH or LC_ORIENT_EAST)", who, a->orient);
    LC_REQUIRE(a->method == LC_TRANSECT_LINEAR || a->method == LC_TRANSECT_NEAREST,
               "%s: bad method %d (LC_TRANSECT_LINEAR or LC_TRANSECT_NEAREST)", who, a->method);
    LC_REQUIRE(!a->cyclic_x || a->nx >= 3, "%s: cyclic_x needs at least 3 columns, got %d", who, a->nx);
    if ((long long)a->ny * a->nx >= (1ll << 31) || (long long)a->n_points * a->n_offsets >= (1ll << 31) ||
        (long long)a->n_lines * a->n_offsets >= (1ll << 31) || a->n_fields > 65535) {
        lc_set_error("%s: too large: a plane of %d x %d, %d points, %d lines or %d fields with %d offsets (ny nx, n_points n_offsets and "
                     "n_lines n_offsets below 2^31, at most 65535 fields)", who, a->ny, a->nx, a->n_points, a->n_lines, a->n_fields,
                     a->n_offsets);
        return LC_EUNSUPPORTED;
    }
    LC_REQUIRE(a->pixel && a->point_line && a->line_offset && a->line_count && a->line_plane && a->line_closed && a->cos_lat &&
                   a->sin_lat && a->cos_lon && a->sin_lon && a->lat_deg && a->lon_deg && a->cos_off && a->sin_off && a->fields &&
                   a->normal_out && a->lat_out && a->lon_out && a->values_out && a->mean_out && a->count_out,
               "%s: null pointer", who);
    LC_HIP_CHECK(hipSetDevice(ctx->device));

    Lines g;
    g.pixel = a->pixel;
    g.point_line = a->point_line;
    g.offset = a->line_offset;
    g.count = a->line_count;
    g.plane = a->line_plane;
    g.closed = a->line_closed;
    g.cl = a->cos_lat;
    g.sl = a->sin_lat;
    g.cx = a->cos_lon;
    g.sx = a->sin_lon;
    g.ny = a->ny;
    g.nx = a->nx;
    g.n_points = a->n_points;
    g.n_lines = a->n_lines;
    g.n_planes = a->n_planes;
    Sampling s;
    s.normal = a->normal_out;
    s.lat = a->lat_deg;
    s.lon = a->lon_deg;
    s.cos_off = a->cos_off;
    s.sin_off = a->sin_off;
    s.lat_out = a->lat_out;
    s.lon_out = a->lon_out;
    s.M = a->n_offsets;
    s.cyclic = a->cyclic_x != 0;
    s.nearest = a->method == LC_TRANSECT_NEAREST;
    hipLaunchKernelGGL(transect_normal_kernel, dim3((unsigned)((a->n_points + TR_THREADS - 1) / TR_THREADS)), dim3(TR_THREADS), 0,
                       ctx->stream, g, a->smooth, a->orient, a->normal_out);
    if (a->dtype == LC_F32)
        launch<float>(ctx, a, g, s);
    else
        launch<double>(ctx, a, g, s);
    LC_HIP_CHECK(hipGetLastError());
    ctx->last_transects_kernel = "transect_normal_kernel+transect_sample_kernel+transect_composite_kernel";
    return LC_OK;
}
