// The runtime-call trace of the advect dispatcher (csrc/advect.hip: advect_ex_checked -> advect_impl, tracer_impl, sample_impl)
// against tests/c/fake_hip.c with its trace switched on, over the inputs and context settings that choose a kernel: for every
// case "== <group> | <case>" and then what the call asked of the HIP runtime -- launches by kernel symbol with grid and block,
// copies, memsets, synchronisations, the sizes it allocated -- and "status <rc> <reported name> launches=<n>": what
// lc_ctx_last_advect_kernel / lc_ctx_last_tracer_kernel say ran, beside the symbol that was launched.  A call the intake
// refuses is a case too: its status alone.  The shapes are tests/kernel_routes.py's (FLOW, SEEDS, T0, NSTEPS, MEMBERS), at
// which the GPU route test reaches every kernel.  Built, run and compared with the record of the commit before the launch
// ladders shared one helper by tests/test_advect_route_trace.py.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../../include/lcs_hip.h"

extern "C" {
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

static std::string fmt(const char *f, ...) {
    char buf[256];
    va_list ap;
    va_start(ap, f);
    vsnprintf(buf, sizeof buf, f, ap);
    va_end(ap);
    return buf;
}

// kernel_routes.FLOW, SEEDS, T0, NSTEPS, MEMBERS
constexpr int NT = 14, NY_F = 36, NX_F = 72, NY = 45, NX = 76, T0 = 1, NSTEPS = 10, MEMBERS = 3;
constexpr size_t PLANE = (size_t)NY * NX, FIELD = (size_t)NT * NY_F * NX_F;

// every buffer at its float64 size: the same ones serve all four dtype codes (nothing reads them: the kernels are stubs)
struct Buffers {
    void *u, *v, *lin, *cub, *ext, *slat, *slon, *x, *y, *tx, *ty, *c1, *c2, *sum1, *sum2, *m1, *m2;
    explicit Buffers(lc_ctx *ctx) {
        const size_t sizes[] = {FIELD, FIELD, lc_packed_elems(NT, NY_F, NX_F), lc_packed_elems(NT, NY_F, NX_F), lc_packed_elems(NT - 1, NY_F, NX_F),
                                NY, NX, 2 * MEMBERS * PLANE, 2 * MEMBERS * PLANE, (NSTEPS + 1) * PLANE, (NSTEPS + 1) * PLANE,
                                (NSTEPS + 1) * PLANE, (NSTEPS + 1) * PLANE, PLANE, PLANE, PLANE, PLANE};
        void **all[] = {&u, &v, &lin, &cub, &ext, &slat, &slon, &x, &y, &tx, &ty, &c1, &c2, &sum1, &sum2, &m1, &m2};
        for (size_t i = 0; i < sizeof(all) / sizeof(all[0]); ++i) MUST(lc_malloc(ctx, sizes[i] * 8, all[i]));
    }
    void release(lc_ctx *ctx) {
        for (void *b : {u, v, lin, cub, ext, slat, slon, x, y, tx, ty, c1, c2, sum1, sum2, m1, m2}) MUST(lc_free(ctx, b));
    }
};

// which of packed_lin, packed_ext, u_raw / v_raw and fuse_levels_raw a call is given (packed_cub: whenever interp_order > 1)
struct Source {
    const char *name;
    bool lin, ext, raw, fuse;
};
static const Source SOURCES[] = {{"lin", true, false, false, false},     {"lin+ext", true, true, false, false}, {"raw", false, false, true, false},
                                 {"raw+ext", false, true, true, false},  {"raw+fuse", false, false, true, true}, {"lin+fuse", true, false, false, true}};
static const char *const DTYPES[] = {"f32", "f64", "f64_wind_f32", "f64_wind_f32_lin32"};   // LC_F32 .. LC_F64_WIND_F32_LIN32

template <typename F>
static void traced(const std::string &label, F call, const char *(*reported)(const lc_ctx *), lc_ctx *ctx) {
    printf("== %s\n", label.c_str());
    fake_hip_trace_begin(stdout);
    const int rc = call();
    fake_hip_trace_end();
    if (rc == LC_OK && reported)
        printf("status %d %s launches=%d\n", rc, reported(ctx), reported == lc_ctx_last_advect_kernel ? lc_ctx_last_advect_launches(ctx) : 1);
    else
        printf("status %d\n", rc);
}

struct Setting {
    int lds, verify, chunk;   // lc_ctx_set_lds_tiles (-1: what creation set), lc_ctx_set_verify, lc_ctx_set_level_chunk (-1: by size)
};

enum CallKind { EX1, EX3, SERIES, DIRS };
static const char *const CALLS[] = {"ex1", "ex3", "series", "dirs"};

static void advect_table(lc_ctx *ctx, const Buffers &b, const char *env, const Setting &s) {
    const std::string set = fmt("lds=%d verify=%d chunk=%d", s.lds, s.verify, s.chunk);
    for (int kind = EX1; kind <= DIRS; ++kind)
        for (int dtype = LC_F32; dtype <= LC_F64_WIND_F32_LIN32; ++dtype)
            for (int cyclic = LC_X_CLAMP_POINT; cyclic <= LC_X_CLAMP_REFERENCE_OUTER; ++cyclic)
                for (int order = 1; order <= 5; ++order)
                    for (int K = 0; K <= 5; ++K)
                        for (int traj = 0; traj <= (kind == EX1 ? 1 : 0); ++traj)   // (with members: refused, once in refusals())
                            for (const Source &src : SOURCES) {
                                lc_advect_args a = {};
                                a.struct_size = sizeof a;
                                a.packed_lin = src.lin ? b.lin : nullptr;
                                a.packed_cub = order > 1 ? b.cub : nullptr;
                                a.packed_ext = src.ext ? b.ext : nullptr;
                                a.u_raw = src.raw ? b.u : nullptr;
                                a.v_raw = src.raw ? b.v : nullptr;
                                a.fuse_levels_raw = src.fuse;
                                a.dtype = dtype, a.nt = NT, a.ny_f = NY_F, a.nx_f = NX_F;
                                a.lat_min = -87.5, a.lat_max = 87.5, a.lon_min = -180.0, a.lon_max = 175.0;
                                a.seed_lat_dev = b.slat, a.ny = NY, a.seed_lon_dev = b.slon, a.nx = NX, a.row0 = 0, a.ny_global = NY;
                                a.timestep = -1800.0, a.settls_order = K, a.interp_order = order, a.cyclic_x = cyclic;
                                a.t0 = T0, a.nsteps = NSTEPS, a.n_members = kind == EX1 ? 1 : MEMBERS, a.t0_stride = 1;
                                a.x_out = b.x, a.y_out = b.y, a.traj_x = traj ? b.tx : nullptr, a.traj_y = traj ? b.ty : nullptr;
                                traced(fmt("env=%s call=%s dtype=%s cyclic=%d | %s order=%d K=%d traj=%d src=%s", env, CALLS[kind], DTYPES[dtype], cyclic,
                                           set.c_str(), order, K, traj, src.name),
                                       [&] {
                                           return kind == SERIES ? lc_advect_series(ctx, &a) : kind == DIRS ? lc_advect_series_dirs(ctx, &a, 2) : lc_advect_ex(ctx, &a);
                                       },
                                       lc_ctx_last_advect_kernel, ctx);
                            }
}

// lc_tracer_sample and lc_sample_raw: both dtypes, orders 1 to 5, the order-1 source as an image, as planes, as both
static void sample_table(lc_ctx *ctx, const Buffers &b) {
    for (int dtype = LC_F32; dtype <= LC_F64; ++dtype)
        for (int order = 1; order <= 5; ++order)
            for (int src = 0; src < 3; ++src) {
                const void *lin = src != 1 ? b.lin : nullptr, *cub = order > 1 ? b.cub : nullptr, *ru = src ? b.u : nullptr, *rv = src ? b.v : nullptr;
                const char *sname = src == 0 ? "lin" : src == 1 ? "raw" : "lin+raw";
                lc_tracer_args t = {};
                t.struct_size = sizeof t;
                t.tracer_lin = lin, t.tracer_cub = cub, t.c1_raw = ru, t.c2_raw = rv;
                t.dtype = dtype, t.nt = NT, t.ny_f = NY_F, t.nx_f = NX_F;
                t.lat_min = -87.5, t.lat_max = 87.5, t.lon_min = -180.0, t.lon_max = 175.0;
                t.ny = NY, t.nx = NX, t.row0 = 0, t.ny_global = NY, t.interp_order = order;
                t.traj_x = b.tx, t.traj_y = b.ty, t.level0 = T0, t.n_levels = NSTEPS + 1;
                t.c1_out = b.c1, t.c2_out = b.c2, t.sum1 = (double *)b.sum1, t.sum2 = (double *)b.sum2, t.mean1_out = b.m1, t.mean2_out = b.m2;
                t.mean_count = NSTEPS + 1;
                traced(fmt("env=none call=tracer dtype=%s cyclic=- | order=%d src=%s", DTYPES[dtype], order, sname), [&] { return lc_tracer_sample(ctx, &t); },
                       lc_ctx_last_tracer_kernel, ctx);
                traced(fmt("env=none call=sample dtype=%s cyclic=- | order=%d src=%s", DTYPES[dtype], order, sname),
                       [&] {
                           return lc_sample_raw(ctx, lin, cub, ru, rv, dtype, NT, NY_F, NX_F, -87.5, 87.5, -180.0, 175.0, T0, b.tx, b.ty, NY, NX, 0, NY, order,
                                                b.c1, b.c2);
                       },
                       nullptr, ctx);
            }
}

// what the intake and the setters refuse beyond the table's own refusals
static void refusals(lc_ctx *ctx, const Buffers &b) {
    lc_advect_args a = {};
    a.struct_size = sizeof a;
    a.packed_lin = b.lin, a.packed_ext = b.ext;
    a.dtype = LC_F32, a.nt = NT, a.ny_f = NY_F, a.nx_f = NX_F;
    a.lat_min = -87.5, a.lat_max = 87.5, a.lon_min = -180.0, a.lon_max = 175.0;
    a.seed_lat_dev = b.slat, a.ny = NY, a.seed_lon_dev = b.slon, a.nx = NX, a.row0 = 0, a.ny_global = NY;
    a.timestep = -1800.0, a.settls_order = 4, a.interp_order = 1, a.cyclic_x = LC_X_CYCLIC;
    a.t0 = T0, a.nsteps = NSTEPS, a.n_members = MEMBERS, a.t0_stride = 1;
    a.x_out = b.x, a.y_out = b.y, a.traj_x = b.tx, a.traj_y = b.ty;
    const char *group = "env=none call=refusals dtype=f32 cyclic=- | ";
    traced(std::string(group) + "ex3 traj=1", [&] { return lc_advect_ex(ctx, &a); }, lc_ctx_last_advect_kernel, ctx);
    traced(std::string(group) + "series traj=1", [&] { return lc_advect_series(ctx, &a); }, lc_ctx_last_advect_kernel, ctx);
    traced(std::string(group) + "dirs traj=1", [&] { return lc_advect_series_dirs(ctx, &a, 2); }, lc_ctx_last_advect_kernel, ctx);
    a.traj_x = a.traj_y = nullptr;
    traced(std::string(group) + "dirs n_dirs=3", [&] { return lc_advect_series_dirs(ctx, &a, 3); }, lc_ctx_last_advect_kernel, ctx);
    a.cyclic_x = LC_X_CLAMP_REFERENCE_OUTER;
    traced(std::string(group) + "ex3 outer", [&] { return lc_advect_ex(ctx, &a); }, lc_ctx_last_advect_kernel, ctx);
    a.cyclic_x = LC_X_CYCLIC, a.interp_order = 6;
    traced(std::string(group) + "ex3 order=6", [&] { return lc_advect_ex(ctx, &a); }, lc_ctx_last_advect_kernel, ctx);
    a.interp_order = 1, a.nsteps = NT - T0;
    traced(std::string(group) + "ex3 steps past the last level", [&] { return lc_advect_ex(ctx, &a); }, lc_ctx_last_advect_kernel, ctx);
    traced(std::string(group) + "set_lds_tiles(3)", [&] { return lc_ctx_set_lds_tiles(ctx, 3); }, nullptr, ctx);
}

int main() {
    // lds 3 is outside the setter's range (-1 .. 2): refused (refusals()), the context keeps what creation set
    static const Setting full[] = {{-1, 0, -1}, {0, 0, -1}, {1, 0, -1}, {2, 0, -1}, {3, 0, -1}, {-1, 1, -1}, {2, 1, -1},
                                   {-1, 0, 4},  {0, 0, 4},  {1, 0, 4},  {2, 0, 4},  {2, 1, 4}};
    // the environments of kernel_routes' routes choose among the two-seed (lds 1) and the float64 tile kernels (default)
    static const Setting knob[] = {{-1, 0, -1}, {1, 0, -1}, {1, 0, 4}};
    static const struct { const char *name, *var, *value; const Setting *settings; int n; } envs[] = {
        {"none", nullptr, nullptr, full, 12}, {"LCS_PATCH_MODE=1", "LCS_PATCH_MODE", "1", knob, 3},
        {"LCS_PATCH_MODE=2", "LCS_PATCH_MODE", "2", knob, 3}, {"LCS_F64_WG_TILE=1", "LCS_F64_WG_TILE", "1", knob, 3}};
    for (auto &e : envs) {
        unsetenv("LCS_PATCH_MODE");
        unsetenv("LCS_F64_WG_TILE");
        if (e.var) setenv(e.var, e.value, 1);   // (read once, in lc_ctx_create)
        lc_ctx *ctx = nullptr;
        MUST(lc_ctx_create(0, &ctx));
        Buffers b(ctx);
        for (int i = 0; i < e.n; ++i) {
            const Setting &s = e.settings[i];
            MUST(lc_ctx_set_lds_tiles(ctx, -1));
            (void)lc_ctx_set_lds_tiles(ctx, s.lds);
            MUST(lc_ctx_set_verify(ctx, s.verify));
            MUST(lc_ctx_set_level_chunk(ctx, s.chunk));
            advect_table(ctx, b, e.name, s);
        }
        MUST(lc_ctx_set_verify(ctx, 0));
        if (!e.var) {
            sample_table(ctx, b);
            refusals(ctx, b);
        }
        b.release(ctx);
        MUST(lc_ctx_destroy(ctx));
    }
    return 0;
}
