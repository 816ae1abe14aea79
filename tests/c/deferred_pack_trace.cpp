// The runtime-call trace of lc_advect_ex behind a deferred pack (lc_field_pack_deferred; csrc/pack.hip, advect_impl), against
// tests/c/fake_hip.c with its trace switched on.  Every call is traced three times: "today" after a plain lc_field_pack, "off"
// after lc_field_pack_deferred in a context with deferring switched off, "deferred" after lc_field_pack_deferred with a pack
// pending -- "== <call> | <setting>", what the call asked of the runtime, and "status <rc> <kernel> launches=<n> pending=<level>".
// The packs themselves are traced as "pack | <setting>".  Shapes: the GPU test's (48 x 96-node float32 field, 512 x 512 seeds,
// two seeds per lane forced), so that the call runs in level chunks with a non-zero grading zone.  Compared by
// tests/test_deferred_pack_trace.py.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../../include/lcs_hip.h"

extern "C" {
void fake_hip_trace_begin(FILE *out);
void fake_hip_trace_end(void);
}

#define MUST(expr)                                                                                  \
    do {                                                                                            \
        if ((expr) != LC_OK) {                                                                      \
            fprintf(stderr, "%s:%d: %s failed [%s]\n", __FILE__, __LINE__, #expr, lc_last_error()); \
            exit(1);                                                                                \
        }                                                                                           \
    } while (0)

constexpr int NY_F = 48, NX_F = 96, NY = 512, NX = 512, NT_MAX = 72;

struct Buffers {
    void *u, *v, *lin, *ext, *lin2, *ext2, *cub, *slat, *slon, *x, *y, *tx, *ty;
    explicit Buffers(lc_ctx *ctx) {
        const size_t img = lc_packed_elems(NT_MAX, NY_F, NX_F), plane = (size_t)NY * NX;
        const size_t sizes[] = {(size_t)NT_MAX * NY_F * NX_F, (size_t)NT_MAX * NY_F * NX_F, img, img, img, img, img, NY, NX, 2 * plane, 2 * plane, NT_MAX * plane, NT_MAX * plane};
        void **all[] = {&u, &v, &lin, &ext, &lin2, &ext2, &cub, &slat, &slon, &x, &y, &tx, &ty};
        for (size_t i = 0; i < sizeof(all) / sizeof(all[0]); ++i) MUST(lc_malloc(ctx, sizes[i] * 4, all[i]));
    }
    void release(lc_ctx *ctx) {
        for (void *b : {u, v, lin, ext, lin2, ext2, cub, slat, slon, x, y, tx, ty}) MUST(lc_free(ctx, b));
    }
};

struct Case {
    const char *name;
    int nt, K, order, traj, members, cyclic, t0, other_images, chunk;   // chunk: lc_ctx_set_level_chunk (-1: by size, graded)
};
static const Case CASES[] = {
    {"eligible nt=72", 72, 4, 1, 0, 1, LC_X_CYCLIC, 0, 0, -1},
    {"eligible nt=72 per-point", 72, 4, 1, 0, 1, LC_X_CLAMP_POINT, 0, 0, -1},
    {"eligible nt=72 K=2 chunk=16", 72, 2, 1, 0, 1, LC_X_CYCLIC, 0, 0, 16},
    {"eligible nt=72 uniform chunk=32", 72, 4, 1, 0, 1, LC_X_CYCLIC, 0, 0, 32},
    {"eligible nt=72 uniform chunk=8 t0=5", 72, 4, 1, 0, 1, LC_X_CYCLIC, 5, 0, 8},
    {"ineligible nt=41: the first launch reaches past the packed levels", 41, 4, 1, 0, 1, LC_X_CYCLIC, 0, 0, -1},
    {"ineligible K=0", 72, 0, 1, 0, 1, LC_X_CYCLIC, 0, 0, -1},
    {"ineligible order=3", 72, 4, 3, 0, 1, LC_X_CYCLIC, 0, 0, -1},
    {"ineligible traj_x", 72, 4, 1, 1, 1, LC_X_CYCLIC, 0, 0, -1},
    {"ineligible two members", 72, 4, 1, 0, 2, LC_X_CYCLIC, 0, 0, -1},
    {"ineligible outer clamp", 72, 4, 1, 0, 1, LC_X_CLAMP_REFERENCE_OUTER, 0, 0, -1},
    {"ineligible t0=10", 72, 4, 1, 0, 1, LC_X_CYCLIC, 10, 0, -1},
    {"ineligible other images", 72, 4, 1, 0, 1, LC_X_CYCLIC, 0, 1, -1},
    {"ineligible one launch", 72, 4, 1, 0, 1, LC_X_CYCLIC, 0, 0, 0},
};

template <typename F>
static void traced(const std::string &label, lc_ctx *ctx, bool advect, F call) {
    printf("== %s\n", label.c_str());
    fake_hip_trace_begin(stdout);
    const int rc = call();
    fake_hip_trace_end();
    if (rc == LC_OK && advect)
        printf("status %d %s launches=%d pending=%d\n", rc, lc_ctx_last_advect_kernel(ctx), lc_ctx_last_advect_launches(ctx), lc_ctx_pack_pending(ctx));
    else
        printf("status %d pending=%d\n", rc, lc_ctx_pack_pending(ctx));
}

static int advect(lc_ctx *ctx, const Buffers &b, const Case &c) {
    lc_advect_args a = {};
    a.struct_size = sizeof a;
    a.packed_lin = c.other_images ? b.lin2 : b.lin;
    a.packed_cub = c.order > 1 ? b.cub : nullptr;
    a.packed_ext = c.order > 1 ? nullptr : (c.other_images ? b.ext2 : b.ext);
    a.dtype = LC_F32, a.nt = c.nt, a.ny_f = NY_F, a.nx_f = NX_F;
    a.lat_min = -88.0, a.lat_max = 88.0, a.lon_min = -180.0, a.lon_max = 176.0;
    a.seed_lat_dev = b.slat, a.ny = NY, a.seed_lon_dev = b.slon, a.nx = NX, a.row0 = 0, a.ny_global = NY;
    a.timestep = -900.0, a.settls_order = c.K, a.interp_order = c.order, a.cyclic_x = c.cyclic;
    a.t0 = c.t0, a.nsteps = (c.traj ? 40 : c.nt - 1) - c.t0 - (c.members - 1), a.n_members = c.members, a.t0_stride = 1;
    a.x_out = b.x, a.y_out = b.y, a.traj_x = c.traj ? b.tx : nullptr, a.traj_y = c.traj ? b.ty : nullptr;
    return lc_advect_ex(ctx, &a);
}

int main() {
    lc_ctx *ctx = nullptr;
    unsetenv("LCS_DEFER_PACK");
    MUST(lc_ctx_create(0, &ctx));
    Buffers b(ctx);
    MUST(lc_ctx_set_lds_tiles(ctx, 1));
    for (const Case &c : CASES) {
        MUST(lc_ctx_set_level_chunk(ctx, c.chunk));
        for (int setting = 0; setting < 3; ++setting) {
            const char *sname = setting == 0 ? "today" : setting == 1 ? "off" : "deferred";
            MUST(lc_ctx_set_deferred_pack(ctx, setting == 2));
            traced(std::string("pack ") + c.name + " | " + sname, ctx, false, [&] {
                return setting == 0 ? lc_field_pack(ctx, b.u, b.v, LC_F32, c.nt, NY_F, NX_F, 1, b.lin, b.ext)
                                    : lc_field_pack_deferred(ctx, b.u, b.v, c.nt, NY_F, NX_F, 0, b.lin, b.ext);
            });
            traced(std::string(c.name) + " | " + sname, ctx, true, [&] { return advect(ctx, b, c); });
            traced(std::string("flush ") + c.name + " | " + sname, ctx, false, [&] { return lc_ctx_flush_pack(ctx); });
        }
    }
    // a second deferred pack completes the first; so do a change of stream (the new stream waits for it), lc_sync, lc_sample,
    // lc_tracer_sample and lc_ctx_destroy
    MUST(lc_ctx_set_deferred_pack(ctx, 1));
    traced("pack first | twice", ctx, false, [&] { return lc_field_pack_deferred(ctx, b.u, b.v, 72, NY_F, NX_F, 0, b.lin, b.ext); });
    traced("pack second | twice", ctx, false, [&] { return lc_field_pack_deferred(ctx, b.u, b.v, 72, NY_F, NX_F, 0, b.lin2, b.ext2); });
    traced("set_stream | twice", ctx, false, [&] { return lc_ctx_set_stream(ctx, nullptr); });
    traced("pack third | twice", ctx, false, [&] { return lc_field_pack_deferred(ctx, b.u, b.v, 72, NY_F, NX_F, 0, b.lin, b.ext); });
    traced("sync | twice", ctx, false, [&] { return lc_sync(ctx); });
    MUST(lc_ctx_use_own_stream(ctx));
    traced("pack fourth | twice", ctx, false, [&] { return lc_field_pack_deferred(ctx, b.u, b.v, 72, NY_F, NX_F, 0, b.lin, b.ext); });
    traced("sample | twice", ctx, false, [&] {
        return lc_sample(ctx, b.lin, nullptr, LC_F32, 72, NY_F, NX_F, -88.0, 88.0, -180.0, 176.0, 3, b.x, b.y, NY, NX, 0, NY, 1, b.tx, b.ty);
    });
    traced("pack fifth | twice", ctx, false, [&] { return lc_field_pack_deferred(ctx, b.u, b.v, 72, NY_F, NX_F, 0, b.lin, b.ext); });
    traced("tracer | twice", ctx, false, [&] {   // an order-1 tracer sample: other images altogether, the pack is completed all the same
        lc_tracer_args t = {};
        t.struct_size = sizeof t;
        t.tracer_lin = b.lin2, t.dtype = LC_F32, t.nt = 72, t.ny_f = NY_F, t.nx_f = NX_F;
        t.lat_min = -88.0, t.lat_max = 88.0, t.lon_min = -180.0, t.lon_max = 176.0;
        t.ny = NY, t.nx = NX, t.row0 = 0, t.ny_global = NY, t.interp_order = 1;
        t.traj_x = b.tx, t.traj_y = b.ty, t.level0 = 40, t.n_levels = 4;
        t.c1_out = b.x, t.c2_out = b.y;
        return lc_tracer_sample(ctx, &t);
    });
    traced("pack sixth | twice", ctx, false, [&] { return lc_field_pack_deferred(ctx, b.u, b.v, 72, NY_F, NX_F, 0, b.lin, b.ext); });
    traced("copy_to_host | twice", ctx, false, [&] {   // a download of the image itself
        static float host[64];
        return lc_copy_to_host(ctx, host, (const char *)b.lin + lc_packed_elems(60, NY_F, NX_F) * sizeof(float), sizeof host);
    });
    lc_ctx *other = nullptr;
    MUST(lc_ctx_create(0, &other));
    MUST(lc_field_pack_deferred(other, b.u, b.v, 72, NY_F, NX_F, 0, b.lin2, b.ext2));
    printf("== destroy | twice\n");
    fake_hip_trace_begin(stdout);
    const int rc = lc_ctx_destroy(other);
    fake_hip_trace_end();
    printf("status %d pending=0\n", rc);
    b.release(ctx);
    MUST(lc_ctx_destroy(ctx));
    return 0;
}
