// Internal header shared by the HIP translation units of liblcs_hip.so.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>

#include "../../include/lcs_hip.h"

struct lc_trunc_cache;                       // preprocess.hip: spectral-truncation operators of the last (nlat, nlon, T)
void lc_trunc_cache_free(lc_trunc_cache *c);

// The rest of a deferred pack (lc_field_pack_deferred; float32, order 1, both images): lin[0, next) and ext[0, next - 1) are
// complete, the levels from there to the series' end are packed by the eligible advect call's own launches or by lc_pack_flush.
struct lc_pending_pack {
    const float *u, *v;
    float *lin, *ext;
    int nt, ny_f, nx_f;
    int next;            // first level of lin not packed yet; 0: nothing pending
    hipStream_t stream;  // the stream the first levels were packed on: where a flush completes the rest
};

// EVERY entry point that takes image pointers, packs, copies device memory or changes the context's stream begins with
// LC_FLUSH_PACK(ctx) (below) -- lc_advect_ex alone decides for itself (advect_impl) --: a pending pack (`pend`) is otherwise read
// half written.  A new entry point of that kind must do the same.
struct lc_ctx {
    int device;
    int n_cus;           // compute units of the device (the fused prefilter sizes its last round by it)
    hipStream_t own_stream;
    hipStream_t stream;  // the one work is enqueued on (own or borrowed)
    int lds_tiles;       // lc_advect float32 kernel choice: 3 LDS tiles, seeds per lane by size (default); 1 two seeds, 2 one seed per lane; 0 direct gathers (LCS_LDS_TILES at creation)
    int lds_tiles_init, sigma_march_init;  // what lc_ctx_create set (environment or built-in default): what -1 restores
    int sigma_march;     // lc_sigma float32 kernel choice: 2 by size (default: marching kernel from 2^23 cells), 1 marching kernel with wavefront shuffles, 0 LDS tiles (LCS_SIGMA_MARCH at creation)
    int xcd_split;       // lc_advect tile order: > 0 = a chunk is 1 / xcd_split of xcd_chunk_rows tile rows; -1 (default) = 8 when whole chunks would leave the XCDs > 15 % apart, else 0 (LCS_XCD_SPLIT at creation)
    int xcd_chunk_rows;  // lc_advect tile order: tile rows per chunk dealt to the XCDs cyclically; default 1; 0 = one contiguous band per XCD (LCS_XCD_CHUNK_ROWS at creation)
    int fir_prefilter;   // float32 order-3 pack: 1 one-pass truncated-convolution prefilter (default), 0 the recursive sweeps (LCS_FIR_PREFILTER at creation)
    int fused_prefilter; // float64 order-3 pack: 1 both sweeps in one pass (prefilter_fused_stream_kernel, default), 0 the two streaming sweeps (LCS_FUSED_PREFILTER at creation)
    int tile_order;      // lc_advect tile-row order: -1 per kernel (default), 0 as stored, 1 last row first, 2 poles inwards (LCS_TILE_ORDER at creation)
    int pole_blocks;     // lc_advect: 1 leading workgroups take the global pole rows (default), 0 the tiles do (LCS_POLE_BLOCKS at creation)
    int level_chunk;     // lc_advect: time levels per launch (-1 by size, the default: 32 from 2^18 seeds per call; 0 = the whole series in one launch); LCS_LEVEL_CHUNK at creation / lc_ctx_set_level_chunk
    int f64_fidelity;    // one-call host routes, float64: enum lc_f64_fidelity (LCS_F64_FIDELITY at creation / lc_ctx_set_f64_fidelity)
    int patch_mode;      // two-seed advect kernel, seeds of a wave / form of the trajectory stores: -1 by call (default: whole-line stores through LDS with trajectories, tall patches without, groups of members for lc_advect_batch), 0 tall, 1 wide, 2 lines, 3 two ensemble members per lane (LCS_PATCH_MODE at creation; advect.hip enum Patch)
    lc_flag_allreduce_fn flag_reduce;  // NULL, or the caller's max-all-reduce over the ranks of a row-sharded grid (lc_ctx_set_flag_allreduce)
    void *flag_reduce_user;
    int last_advect_launches;  // kernel launches the last lc_advect made (level chunks)
    const char *last_advect_kernel;
    const char *last_sigma_kernel;
    const char *last_pack_kernel;   // what the last lc_field_pack launched for the prefilter / interleave stage (lc_ctx_last_pack_kernel)
    const char *last_tracer_kernel; // what the last lc_tracer_sample launched (lc_ctx_last_tracer_kernel)
    unsigned *verify_dev;  // NULL, or 16 uint32 wave-state counters in device memory (lc_ctx_set_verify)
    lc_trunc_cache *trunc;
    struct lc_host_xfer *xfer;  // NULL until a one-call host route first needs it: the pinned staging ring + its threads (hostxfer.h)
    void *host_ws;              // lc_lcs_host's device buffers of the last call, kept for the next one (api.hip: HostWorkspace; lc_ctx_trim frees them)
    int host_cache;             // 1 (default): keep them; 0: hipMalloc / hipFree per call (LCS_HOST_CACHE at creation)
    double host_marks[4];       // the last lc_lcs_host call, ms since its entry: buffers allocated, uploads + launches issued, kernels done, results in the caller's buffers (lc_ctx_last_host_marks)
    int host_timing;            // lc_lcs_host: 1 = one line of wall-clock marks per call on stderr (LCS_HOST_TIMING at creation)
    int f64_wg_tile;            // float64 order 1, fused levels: 1 = one LDS tile per workgroup (advect_wg64_kernel; LCS_F64_WG_TILE at creation; measured, off)
    int host_threads;           // staging ring: worker threads beside the caller (-1: by the host's core count; LCS_HOST_THREADS at creation)
    int host_piece_mb;          // staging ring: piece size in MB (0: 32; LCS_HOST_PIECE_MB at creation)
    int host_pipeline;          // lc_lcs_host: 1 (default) staged transfers, upload cut into level chunks and overlapped with pack + advect; 0 the serial round-5 form (LCS_HOST_PIPELINE at creation)
    const char *last_strain_kernel;  // what the last lc_strain launched (lc_ctx_last_strain_kernel)
    // lc_advect, graded level counts (launch_plan.h; lc_ctx_set_level_grading): levels per launch where the grading applies
    // (0: the by-size chunk), dispatch positions at a launch's end that are cut short, levels the last one loses (-1: the
    // built-in defaults; depth 0: off).  Only with level_chunk = -1: an explicit level chunk is uniform chunks.
    int grade_chunk, grade_zone, grade_depth;
    const char *last_ridges_kernel;  // what the last lc_ridges_batch launched (lc_ctx_last_ridges_kernel)
    const char *last_threshold_kernel;  // what the last lc_local_threshold launched (lc_ctx_last_threshold_kernel)
    const char *last_idw_kernel;  // what the last lc_idw_interp launched (lc_ctx_last_idw_kernel)
    const char *last_transects_kernel;  // what the last lc_ridge_transects launched (lc_ctx_last_transects_kernel)
    const char *last_aux_kernel;  // what the last lc_aux_gradient launched (lc_ctx_last_aux_kernel)
    const char *last_fsle_kernel;  // what the last lc_fsle_update launched (lc_ctx_last_fsle_kernel)
    const char *last_vorticity_kernel;  // what the last lc_vorticity launched (lc_ctx_last_vorticity_kernel)
    const char *last_lavd_kernel;  // what the last lc_lavd_update launched (lc_ctx_last_lavd_kernel)
    const char *last_footprint_kernel;  // what the last lc_footprint_update launched (lc_ctx_last_footprint_kernel)
    int footprint_form;         // lc_footprint_update's kernel form: -1 auto (default), 0 direct, 1 tiled, 2 tiled with the window census (lc_ctx_set_footprint_form)
    lc_pending_pack pend;       // the context's one pending pack (pack.hip)
    int defer_pack;             // lc_field_pack_deferred defers (1, default) or packs the whole series at once as lc_field_pack does (0; LCS_DEFER_PACK at creation / lc_ctx_set_deferred_pack)
    int pack_share, pack_period_shift, pack_item_levels;  // a launch that carries a pack: pack workgroups (8 / 16 / 24) in every 2^shift blocks (32 .. 16384; shift 0, the default: by the pack's size), levels per item of theirs (2 / 4 / 8): lc_ctx_set_deferred_pack_mix
#ifdef LCS_TIMELINE  // diagnostic build only: start / end stamps of the two-seed order-1 kernel's workgroups (lc_debug_read_timeline)
    unsigned long long *timeline_dev;
    size_t timeline_cap;  // records allocated
    int timeline_launches, timeline_grid;  // of the last call that wrote it
#endif
};

void lc_set_error(const char *fmt, ...);

// (a failed runtime call also leaves its code in the thread's sticky "last error", which the NEXT lc_* call's
//  hipGetLastError() after its kernel launches would report as its own: consumed here, with the failure it belongs to --
//  found by tests/test_host_orchestration_asan.py's injected failures)
#define LC_HIP_CHECK(expr)                                                              \
    do {                                                                                \
        hipError_t _e = (expr);                                                         \
        if (_e != hipSuccess) {                                                         \
            lc_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, \
                         __LINE__);                                                     \
            (void)hipGetLastError();                                                    \
            return LC_EHIP;                                                             \
        }                                                                               \
    } while (0)

#define LC_REQUIRE(cond, ...)          \
    do {                               \
        if (!(cond)) {                 \
            lc_set_error(__VA_ARGS__); \
            return LC_EINVAL;          \
        }                              \
    } while (0)

// Padded gather image geometry (see lc_field_pack in lcs_hip.h).
constexpr int LC_PAD_LO = 1;
constexpr int LC_PAD_HI = 2;
constexpr int LC_PAD = LC_PAD_LO + LC_PAD_HI;

static inline size_t lc_level_elems(int ny_f, int nx_f) {
    return (size_t)(ny_f + LC_PAD) * (size_t)(nx_f + LC_PAD) * 2;
}

// A wind on the device, a seed grid on the device, the packed images of the wind (NULL where there is none) and the path's
// options: what a whole-grid advect call is described by.  The coordinate extremes are rounded to the wind's dtype; dlat / dlon
// are the seed spacings as numpy evaluates lat[1] - lat[0] in the coordinate dtype (lc_sigma's; lc_advect does not read them).
struct lc_dev_wind {
    const void *u, *v;  // the raw planes [nt][ny_f][nx_f], or NULL
    int dtype, nt, ny_f, nx_f;
    double lat_min, lat_max, lon_min, lon_max;
};
struct lc_dev_seeds {
    const void *lat, *lon;
    int ny, nx;
    double dlat, dlon;
};
struct lc_dev_images {
    const void *lin, *cub, *ext;
};
struct lc_path_options {
    double timestep;
    int settls_order, interp_order, cyclic_x;
};

// lc_advect_args of one member over the whole seed grid from level 0, zero steps, no outputs: a caller sets what its call
// differs in (t0, nsteps, x_start / y_start, n_members, t0_stride, a row block, the outputs and trajectories).  The one fill
// of the structure in the library (lc_advect_batch, the one-call host routes): a new field is given its value here.
static inline lc_advect_args lc_whole_grid_args(const lc_dev_wind &w, const lc_dev_images &img, const lc_dev_seeds &s,
                                                const lc_path_options &o) {
    lc_advect_args a = {};
    a.struct_size = sizeof(a);
    a.packed_lin = img.lin;
    a.packed_cub = img.cub;
    a.packed_ext = img.ext;
    a.u_raw = w.u;
    a.v_raw = w.v;
    a.dtype = w.dtype;
    a.nt = w.nt;
    a.ny_f = w.ny_f;
    a.nx_f = w.nx_f;
    a.lat_min = w.lat_min;
    a.lat_max = w.lat_max;
    a.lon_min = w.lon_min;
    a.lon_max = w.lon_max;
    a.seed_lat_dev = s.lat;
    a.ny = s.ny;
    a.seed_lon_dev = s.lon;
    a.nx = s.nx;
    a.ny_global = s.ny;
    a.timestep = o.timestep;
    a.settls_order = o.settls_order;
    a.interp_order = o.interp_order;
    a.cyclic_x = o.cyclic_x;
    a.n_members = 1;
    return a;
}

// kernel launchers implemented in the .hip files
int lc_launch_pack(lc_ctx *ctx, const void *u, const void *v, int dtype, int nt, int ny_f, int nx_f,
                   int order, void *packed, void *ext);
int lc_launch_extrapolate(lc_ctx *ctx, const void *img, int dtype, int nt, int ny_f, int nx_f, void *ext);
int lc_pack_flush(lc_ctx *ctx);  // completes the context's pending pack, if any, with the stand-alone kernel on its stream
// ... and makes `next`, the stream the context is about to work on, wait for it: the pack was begun on another stream, whose
// order the caller's own waits (recorded before this moment) do not cover
int lc_pack_flush_before(lc_ctx *ctx, hipStream_t next);
#define LC_FLUSH_PACK(ctx)                  \
    do {                                    \
        const int _rc = lc_pack_flush(ctx); \
        if (_rc != LC_OK) return _rc;       \
    } while (0)
