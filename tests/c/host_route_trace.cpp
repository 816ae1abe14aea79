// The runtime-call trace of the one-call host routes and of the positional advect entry points, against tests/c/fake_hip.c
// with its trace switched on: for every call of the table below, "== <label>" and then what the call asked of the HIP runtime
// -- launches by kernel name, copies, memsets, event records, waits, synchronisations, and the sizes it allocated (fake_hip.c
// says how pointers are written).  The shapes are tests/c/host_orchestration.cpp's.  Built, run and compared with the record
// of the commit before the routes shared one core by tests/test_host_route_trace.py.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/lcs_hip.h"

extern "C" {
void fake_hip_trace_host(const char *name, const void *base, size_t bytes);
void fake_hip_trace_begin(FILE *out);
void fake_hip_trace_end(void);
}

#define MUST(expr)                                                                             \
    do {                                                                                       \
        if ((expr) != LC_OK) {                                                                 \
            fprintf(stderr, "%s:%d: %s failed [%s]\n", __FILE__, __LINE__, #expr, lc_last_error()); \
            exit(1);                                                                           \
        }                                                                                      \
    } while (0)

// one traced call: the context's kept buffers let go first (every call allocates everything anew), the status last
template <typename F>
static void traced(lc_ctx *ctx, const std::string &label, F call) {
    MUST(lc_ctx_trim(ctx));
    printf("== %s\n", label.c_str());
    fake_hip_trace_begin(stdout);
    const int rc = call();
    fake_hip_trace_end();
    printf("status %d\n", rc);
}

template <typename T>
struct Case {   // (host_orchestration.cpp's)
    int nt, ny_f, nx_f, ny, nx;
    std::vector<T> u, v, lat, lon, slat, slon, sigma, x, y, tx, ty;
    Case(int nt_, int nyf, int nxf, int ny_, int nx_) : nt(nt_), ny_f(nyf), nx_f(nxf), ny(ny_), nx(nx_) {
        u.assign((size_t)nt * ny_f * nx_f, T(3));
        v.assign(u.size(), T(-1));
        for (size_t i = 0; i < u.size(); ++i) u[i] += T(0.01) * T(i % 97), v[i] += T(0.02) * T(i % 53);
        lat.resize(ny_f), lon.resize(nx_f), slat.resize(ny), slon.resize(nx);
        for (int i = 0; i < ny_f; ++i) lat[i] = T(-80.0 + 160.0 * i / (ny_f - 1));
        for (int i = 0; i < nx_f; ++i) lon[i] = T(-180.0 + 360.0 * i / nx_f);
        for (int i = 0; i < ny; ++i) slat[i] = T(-80.0 + 160.0 * i / (ny - 1));
        for (int i = 0; i < nx; ++i) slon[i] = T(-180.0 + 359.0 * i / (nx - 1));
        sigma.resize((size_t)ny * nx), x.resize(sigma.size()), y.resize(sigma.size());
        tx.resize((size_t)nt * ny * nx), ty.resize(tx.size());
    }
    void name_arrays() const {
        const struct { const char *name; const std::vector<T> *a; } all[] = {{"u", &u}, {"v", &v}, {"lat", &lat}, {"lon", &lon}, {"slat", &slat},
            {"slon", &slon}, {"sigma", &sigma}, {"x", &x}, {"y", &y}, {"tx", &tx}, {"ty", &ty}};
        for (auto &h : all) fake_hip_trace_host(h.name, h.a->data(), h.a->size() * sizeof(T));
    }
    void run(lc_ctx *ctx, const std::string &label, int dtype, int K, int order, int cyclic, double gauss, bool traj, int t0, int nsteps) {
        name_arrays();
        traced(ctx, label, [&] {
            return lc_lcs_host(ctx, u.data(), v.data(), dtype, nt, ny_f, nx_f, lat.data(), lon.data(), slat.data(), ny, slon.data(), nx, -900.0, K,
                               order, cyclic, t0, nsteps, gauss, 1, LC_LAYOUT_REFERENCE, sigma.data(), x.data(), y.data(),
                               traj ? tx.data() : nullptr, traj ? ty.data() : nullptr);
        });
    }
};

static std::string fmt(const char *f, ...) {
    char buf[256];
    va_list ap;
    va_start(ap, f);
    vsnprintf(buf, sizeof buf, f, ap);
    va_end(ap);
    return buf;
}

template <typename T>
static void host_table(lc_ctx *ctx, int dtype, const char *dname, const char *fid) {
    Case<T> c(5, 24, 40, 33, 47), p(41, 24, 40, 33, 47);
    for (int order = 1; order <= 3; ++order)
        for (int cyclic = 0; cyclic <= 2; ++cyclic)   // LC_X_CLAMP_POINT, LC_X_CYCLIC, LC_X_CLAMP_REFERENCE_OUTER
            for (int K = 0; K <= 4; K += 4)
                for (int traj = 0; traj <= 1; ++traj)
                    for (int g = 0; g <= 1; ++g)
                        for (int pipe = 0; pipe <= 1; ++pipe) {
                            MUST(lc_ctx_set_host_pipeline(ctx, pipe));
                            c.run(ctx, fmt("lcs_host nt=5 %s fid=%s order=%d cyclic=%d K=%d traj=%d gauss=%s pipe=%d", dname, fid, order, cyclic, K, traj,
                                           g ? "1.5" : "0", pipe), dtype, K, order, cyclic, g ? 1.5 : 0.0, traj != 0, 0, 4);
                        }
    MUST(lc_ctx_set_host_pipeline(ctx, 1));
    // the pipelined form (float32 at order 1, float64 fast at order 3) and the sub-ranges: levels 3 .. 38 of 41, and a short one
    const bool f32 = dtype == LC_F32;
    if (f32 || std::string(fid) == "fast") {
        const int order = f32 ? 1 : 3;
        const int ranges[3][2] = {{0, 40}, {3, 35}, {5, 7}};
        for (auto &r : ranges)
            p.run(ctx, fmt("lcs_host nt=41 %s fid=%s order=%d cyclic=1 K=4 traj=0 gauss=0 pipe=1 t0=%d nsteps=%d", dname, fid, order, r[0], r[1]), dtype, 4,
                  order, 1, 0.0, false, r[0], r[1]);
    }
}

int main() {
    lc_ctx *ctx = nullptr;
    MUST(lc_ctx_create(0, &ctx));
    {   // the staging ring comes into being with the first call: outside every trace
        Case<float> w(5, 24, 40, 33, 47);
        MUST(lc_lcs_host(ctx, w.u.data(), w.v.data(), LC_F32, w.nt, w.ny_f, w.nx_f, w.lat.data(), w.lon.data(), w.slat.data(), w.ny, w.slon.data(), w.nx,
                         -900.0, 4, 1, 1, 0, 4, 0.0, 1, LC_LAYOUT_REFERENCE, w.sigma.data(), w.x.data(), w.y.data(), nullptr, nullptr));
    }
    host_table<float>(ctx, LC_F32, "f32", "-");
    MUST(lc_ctx_set_f64_fidelity(ctx, LC_F64_EXACT_ORDER));
    host_table<double>(ctx, LC_F64, "f64", "exact");
    MUST(lc_ctx_set_f64_fidelity(ctx, LC_F64_FAST));
    host_table<double>(ctx, LC_F64, "f64", "fast");
    MUST(lc_ctx_set_f64_fidelity(ctx, LC_F64_AUTO));
    {   // the reference's default global call form on a 45 x 90 grid (poles included)
        int gy = 0, gx = 0;
        MUST(lc_common_grid(&gy, &gx, nullptr, nullptr));
        const int nt = 3, ny_f = 45, nx_f = 90;
        std::vector<double> u((size_t)nt * ny_f * nx_f, 5.0), v(u.size(), 1.0), lat(ny_f), lon(nx_f);
        for (size_t i = 0; i < u.size(); ++i) u[i] += 0.1 * std::sin(0.01 * (double)i);
        for (int i = 0; i < ny_f; ++i) lat[i] = -90.0 + 180.0 * i / (ny_f - 1);
        for (int i = 0; i < nx_f; ++i) lon[i] = -180.0 + 360.0 * i / nx_f;
        std::vector<double> sg((size_t)gy * gx), x(sg.size()), y(sg.size());
        const int forms[3][2] = {{0, 10}, {0, -1}, {1, 20}};
        for (auto &f : forms) {
            fake_hip_trace_host("u", u.data(), u.size() * 8);
            fake_hip_trace_host("v", v.data(), v.size() * 8);
            fake_hip_trace_host("sigma", sg.data(), sg.size() * 8);
            fake_hip_trace_host("x", x.data(), x.size() * 8);
            fake_hip_trace_host("y", y.data(), y.size() * 8);
            traced(ctx, fmt("lcs_global_host f64 common=%d truncation=%d", f[0], f[1]), [&] {
                return lc_lcs_global_host(ctx, u.data(), v.data(), LC_F64, nt, ny_f, nx_f, lat.data(), lon.data(), f[0], f[1], -21600.0, 4, 3, 0.0, 1,
                                          LC_LAYOUT_REFERENCE, sg.data(), x.data(), y.data());
            });
        }
    }
    {   // the positional advect entry points on device buffers: float32 at order 1 with both images
        const int nt = 5, ny_f = 24, nx_f = 40, ny = 33, nx = 47, nsteps = 2;
        const size_t plane = (size_t)ny * nx * 4;
        void *u, *v, *lin, *ext, *slat, *slon, *x, *y, *xs, *ys, *tx, *ty;
        MUST(lc_malloc(ctx, (size_t)nt * ny_f * nx_f * 4, &u));
        MUST(lc_malloc(ctx, (size_t)nt * ny_f * nx_f * 4, &v));
        MUST(lc_malloc(ctx, lc_packed_elems(nt, ny_f, nx_f) * 4, &lin));
        MUST(lc_malloc(ctx, lc_packed_elems(nt - 1, ny_f, nx_f) * 4, &ext));
        MUST(lc_malloc(ctx, ny * 4, &slat));
        MUST(lc_malloc(ctx, nx * 4, &slon));
        for (void **b : {&x, &y}) MUST(lc_malloc(ctx, 3 * plane, b));
        for (void **b : {&xs, &ys}) MUST(lc_malloc(ctx, plane, b));
        for (void **b : {&tx, &ty}) MUST(lc_malloc(ctx, (nsteps + 1) * plane, b));
        MUST(lc_field_pack(ctx, u, v, LC_F32, nt, ny_f, nx_f, 1, lin, ext));
        traced(ctx, "lc_advect f32 order=1 K=4 cyclic=1 traj=1", [&] {
            return lc_advect(ctx, lin, nullptr, ext, LC_F32, nt, ny_f, nx_f, -80.0, 80.0, -180.0, 171.0, slat, ny, slon, nx, 0, ny, -900.0, 4, 1, 1, 1,
                             nsteps, x, y, tx, ty);
        });
        traced(ctx, "lc_advect_from f32 order=1 K=4 cyclic=1", [&] {
            return lc_advect_from(ctx, lin, nullptr, ext, LC_F32, nt, ny_f, nx_f, -80.0, 80.0, -180.0, 171.0, slat, ny, slon, nx, 0, ny, xs, ys, -900.0, 4,
                                  1, 1, 1, nsteps, x, y, nullptr, nullptr);
        });
        traced(ctx, "lc_advect_batch f32 order=1 K=4 cyclic=1 n_members=3 t0_stride=1", [&] {
            return lc_advect_batch(ctx, lin, nullptr, ext, LC_F32, nt, ny_f, nx_f, -80.0, 80.0, -180.0, 171.0, slat, ny, slon, nx, 0, ny, nullptr, nullptr,
                                   -900.0, 4, 1, 1, 0, nsteps, 3, 1, x, y, nullptr, nullptr);
        });
        for (void *b : {u, v, lin, ext, slat, slon, x, y, xs, ys, tx, ty}) MUST(lc_free(ctx, b));
    }
    MUST(lc_ctx_destroy(ctx));
    return 0;
}
