// The host orchestration of lc_advect_series_dirs (csrc/advect.hip) against tests/c/fake_hip.c, under AddressSanitizer + UBSan
// (tests/test_bidir_host.py builds and runs it):
//   * n_dirs = 2: every level chunk makes one fused launch per direction, twice lc_advect_series's launches for the same
//     windows; n_dirs = 1 is lc_advect_series;
//   * the outer clamp per plane (plane 2w + d): one flag per plane, read back once per chunk; the two directions of a window
//     firing in different chunks (or one never) enter the sub-step phase at their own chunk, all planes in ONE launch per
//     sub-step;
//   * the refusals before any HIP call: n_dirs, row blocks, trajectories, the level range (counted in windows);
//   * an allocation failure injected at EVERY allocation, and a copy failure at every copy: an error status (or LC_OK where
//     a scratch buffer has a fallback), nothing left allocated, and the context still usable afterwards.
// The stand-in runtime launches nothing, so the flags the fused kernel would raise are raised here: the link wraps
// hipMemcpyAsync (-Wl,--wrap=hipMemcpyAsync) and the wrapper sets plane p's flag in the read-back of chunk fire_at[p] on.
// Prints "OK <n checks>" on success.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/lcs_hip.h"

extern "C" {
int fake_hip_live(void);
int fake_hip_mallocs(void);
int fake_hip_copies(void);
int fake_hip_launches(void);
int fake_hip_bad_frees(void);
void fake_hip_fail_malloc_at(int n);
void fake_hip_fail_memcpy_at(int n);
void fake_hip_reset_counts(void);
int hipMalloc(void **p, size_t bytes);
int hipFree(void *p);
int __real_hipMemcpyAsync(void *dst, const void *src, size_t n, int kind, void *stream);
int __wrap_hipMemcpyAsync(void *dst, const void *src, size_t n, int kind, void *stream);
}

static int g_checks = 0;
#define CHECK(cond)                                                                                         \
    do {                                                                                                    \
        ++g_checks;                                                                                         \
        if (!(cond)) {                                                                                      \
            fprintf(stderr, "%s:%d: CHECK failed: %s   [%s]\n", __FILE__, __LINE__, #cond, lc_last_error()); \
            exit(1);                                                                                        \
        }                                                                                                   \
    } while (0)

// the fire schedule: plane p's flag reads 1 from read-back number fire_at[p] (0-based) on; -1 never
static std::vector<int> g_fire_at;
static int g_readbacks = 0;
static const int kDeviceToHost = 2;  // hipMemcpyDeviceToHost

int __wrap_hipMemcpyAsync(void *dst, const void *src, size_t n, int kind, void *stream) {
    const int rc = __real_hipMemcpyAsync(dst, src, n, kind, stream);
    if (rc == 0 && kind == kDeviceToHost && !g_fire_at.empty() && n == g_fire_at.size() * sizeof(unsigned)) {
        unsigned *f = (unsigned *)dst;
        for (size_t m = 0; m < g_fire_at.size(); ++m)
            if (g_fire_at[m] >= 0 && g_readbacks >= g_fire_at[m]) f[m] = 1u;
        ++g_readbacks;
    }
    return rc;
}

struct Dev {
    void *p = nullptr;
    explicit Dev(size_t bytes) { CHECK(hipMalloc(&p, bytes) == 0); std::memset(p, 0, bytes); }
    ~Dev() { hipFree(p); }
};

template <typename F>
static void sweep_failures(const char *what, F route) {
    const int live0 = fake_hip_live();
    fake_hip_reset_counts();
    CHECK(route() == LC_OK);
    const int n_malloc = fake_hip_mallocs(), n_copy = fake_hip_copies();
    CHECK(fake_hip_live() == live0 && n_malloc > 0 && fake_hip_launches() > 0);
    for (int k = 1; k <= n_malloc; ++k) {
        fake_hip_fail_malloc_at(k);
        const int rc = route();
        fake_hip_fail_malloc_at(0);
        if (!(rc == LC_ENOMEM || rc == LC_EHIP || rc == LC_OK) || fake_hip_live() != live0) {
            fprintf(stderr, "%s: allocation %d of %d failing gave status %d, %d buffers live (%d before) [%s]\n", what, k, n_malloc,
                    rc, fake_hip_live(), live0, lc_last_error());
            exit(1);
        }
        ++g_checks;
    }
    for (int k = 1; k <= n_copy; ++k) {
        fake_hip_fail_memcpy_at(k);
        const int rc = route();
        fake_hip_fail_memcpy_at(0);
        if (rc == LC_OK || fake_hip_live() != live0) {
            fprintf(stderr, "%s: copy %d of %d failing gave status %d, %d buffers live (%d before) [%s]\n", what, k, n_copy, rc,
                    fake_hip_live(), live0, lc_last_error());
            exit(1);
        }
        ++g_checks;
    }
    CHECK(route() == LC_OK && fake_hip_live() == live0);   // the context is still usable
}

int main() {
    lc_ctx *ctx = nullptr;
    CHECK(lc_ctx_create(0, &ctx) == LC_OK && ctx != nullptr);
    const int nt = 50, ny_f = 24, nx_f = 40, ny = 20, nx = 33, nw = 3, K = 1, nsteps = 40, stride = 2;
    const int base = fake_hip_live();
    {
        Dev lin(lc_packed_elems(nt, ny_f, nx_f) * sizeof(float));
        Dev slat(ny * sizeof(float)), slon(nx * sizeof(float));
        Dev x((size_t)2 * nw * ny * nx * sizeof(float)), y((size_t)2 * nw * ny * nx * sizeof(float));
        Dev tx((size_t)(nsteps + 1) * ny * nx * sizeof(float)), ty((size_t)(nsteps + 1) * ny * nx * sizeof(float));
        {
            float *la = (float *)slat.p, *lo = (float *)slon.p;
            for (int i = 0; i < ny; ++i) la[i] = -60.0f + 120.0f * i / (ny - 1);
            for (int i = 0; i < nx; ++i) lo[i] = -170.0f + 340.0f * i / (nx - 1);
        }
        const int live1 = fake_hip_live();
        auto args = [&](int cyclic) {
            lc_advect_args a = {};
            a.struct_size = sizeof(a);
            a.packed_lin = lin.p;
            a.dtype = LC_F32;
            a.nt = nt;
            a.ny_f = ny_f;
            a.nx_f = nx_f;
            a.lat_min = -80.0;
            a.lat_max = 80.0;
            a.lon_min = -180.0;
            a.lon_max = 180.0;
            a.seed_lat_dev = slat.p;
            a.ny = ny;
            a.seed_lon_dev = slon.p;
            a.nx = nx;
            a.ny_global = ny;
            a.timestep = -900.0;
            a.settls_order = K;
            a.interp_order = 1;
            a.cyclic_x = cyclic;
            a.t0 = 0;
            a.nsteps = nsteps;
            a.n_members = nw;
            a.t0_stride = stride;
            a.x_out = x.p;
            a.y_out = y.p;
            return a;
        };
        auto run = [&](int cyclic, std::vector<int> fire, int n_dirs = 2) {
            g_fire_at = fire;
            g_readbacks = 0;
            const lc_advect_args a = args(cyclic);
            const int rc = lc_advect_series_dirs(ctx, &a, n_dirs);
            g_fire_at.clear();
            return rc;
        };
        const int n_chunks = (nsteps + 15) / 16;   // lcplan::OUTER_CHUNK levels per fused launch
        // cyclic and per-point boundaries: twice lc_advect_series's launches (one per direction)
        for (int mode : {LC_X_CYCLIC, LC_X_CLAMP_POINT}) {
            fake_hip_reset_counts();
            const lc_advect_args a = args(mode);
            CHECK(lc_advect_series(ctx, &a) == LC_OK);
            const int one = fake_hip_launches();
            fake_hip_reset_counts();
            CHECK(run(mode, {}) == LC_OK && fake_hip_live() == live1 && fake_hip_launches() == 2 * one);
            CHECK(lc_ctx_last_advect_launches(ctx) == 2 * one);
            fake_hip_reset_counts();
            CHECK(run(mode, {}, 1) == LC_OK && fake_hip_launches() == one);   // n_dirs = 1: lc_advect_series
        }
        // the outer clamp, no plane leaving the box: the fused launches only (two per chunk), every flag read back once per chunk
        fake_hip_reset_counts();
        CHECK(run(LC_X_CLAMP_REFERENCE_OUTER, {-1, -1, -1, -1, -1, -1}) == LC_OK && fake_hip_live() == live1);
        CHECK(fake_hip_launches() == 2 * n_chunks && g_readbacks == n_chunks);
        CHECK(strcmp(lc_ctx_last_advect_kernel(ctx), "outer_substep_batch_kernel") != 0);
        // the two directions of each window apart: window 0 only backward in the first chunk, window 1 only forward in the
        // last, window 2 backward in the second and forward in the first
        fake_hip_reset_counts();
        CHECK(run(LC_X_CLAMP_REFERENCE_OUTER, {0, -1, -1, 2, 1, 0}) == LC_OK && fake_hip_live() == live1);
        CHECK(strcmp(lc_ctx_last_advect_kernel(ctx), "outer_substep_batch_kernel") == 0);
        CHECK(fake_hip_launches() == 2 * n_chunks + 2 * nsteps * (K + 1) + 2);
        // every plane fires in the first chunk: no further fused launch
        fake_hip_reset_counts();
        CHECK(run(LC_X_CLAMP_REFERENCE_OUTER, {0, 0, 0, 0, 0, 0}) == LC_OK && fake_hip_launches() == 2 + 2 * nsteps * (K + 1) + 2);
        // one direction only, from the second chunk on: the sub-step phase starts at step 16
        fake_hip_reset_counts();
        CHECK(run(LC_X_CLAMP_REFERENCE_OUTER, {-1, 1, -1, 2, -1, 1}) == LC_OK &&
              fake_hip_launches() == 2 * n_chunks + 2 * (nsteps - 16) * (K + 1) + 2);
        // one window in both directions
        {
            g_fire_at = {-1, 1};
            g_readbacks = 0;
            lc_advect_args a = args(LC_X_CLAMP_REFERENCE_OUTER);
            a.n_members = 1;
            fake_hip_reset_counts();
            CHECK(lc_advect_series_dirs(ctx, &a, 2) == LC_OK && fake_hip_launches() == 2 * n_chunks + 2 * (nsteps - 16) * (K + 1) + 2);
            g_fire_at.clear();
        }

        // refusals: nothing may stay allocated
        {
            fake_hip_reset_counts();
            lc_advect_args a = args(LC_X_CLAMP_REFERENCE_OUTER);
            for (int bad : {0, 3, -2}) CHECK(lc_advect_series_dirs(ctx, &a, bad) == LC_EINVAL && strstr(lc_last_error(), "n_dirs"));
            a.row0 = 2;
            a.ny = ny - 2;
            CHECK(lc_advect_series_dirs(ctx, &a, 2) == LC_EUNSUPPORTED && strstr(lc_last_error(), "whole seed grids"));
            a = args(LC_X_CYCLIC);
            a.ny_global = ny + 4;
            CHECK(lc_advect_series_dirs(ctx, &a, 2) == LC_EUNSUPPORTED);
            a = args(LC_X_CLAMP_REFERENCE_OUTER);
            a.traj_x = tx.p;
            a.traj_y = ty.p;
            CHECK(lc_advect_series_dirs(ctx, &a, 2) == LC_EINVAL && strstr(lc_last_error(), "traj_x"));
            a = args(LC_X_CYCLIC);
            a.nsteps = nt - (nw - 1) * stride;             // one level beyond the series (the range counts windows, not planes)
            CHECK(lc_advect_series_dirs(ctx, &a, 2) == LC_EINVAL);
            a.nsteps = nt - 1 - (nw - 1) * stride;         // the last level: accepted
            CHECK(lc_advect_series_dirs(ctx, &a, 2) == LC_OK);
            a = args(LC_X_CYCLIC);
            a.n_members = 40000;                           // 80000 planes: more than a launch's grid.y
            CHECK(lc_advect_series_dirs(ctx, &a, 2) == LC_EINVAL);
            a = args(LC_X_CLAMP_REFERENCE_OUTER);
            a.struct_size = sizeof(a) - 8;
            CHECK(lc_advect_series_dirs(ctx, &a, 2) == LC_EINVAL && lc_advect_series_dirs(ctx, nullptr, 2) == LC_EINVAL);
            a = args(LC_X_CLAMP_REFERENCE_OUTER);
            CHECK(lc_advect_series_dirs(nullptr, &a, 2) == LC_EINVAL);
            CHECK(fake_hip_live() == live1);
        }

        // every allocation and every copy failing in turn
        sweep_failures("lc_advect_series_dirs outer, directions apart", [&] { return run(LC_X_CLAMP_REFERENCE_OUTER, {0, -1, -1, 2, 1, 0}); });
        sweep_failures("lc_advect_series_dirs outer, all late", [&] { return run(LC_X_CLAMP_REFERENCE_OUTER, {2, 1, 1, 2, 1, 2}); });
        sweep_failures("lc_advect_series_dirs outer, none leaving", [&] { return run(LC_X_CLAMP_REFERENCE_OUTER, {-1, -1, -1, -1, -1, -1}); });
        CHECK(fake_hip_bad_frees() == 0);
    }
    CHECK(fake_hip_live() == base);
    CHECK(lc_ctx_destroy(ctx) == LC_OK);
    CHECK(fake_hip_bad_frees() == 0);
    printf("OK %d\n", g_checks);
    return 0;
}
