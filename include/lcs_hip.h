/*
 * lcs_hip.h -- C ABI of the MI355X-native FTLE engine (liblcs_hip.so).
 *
 * Drop-in boundary for the parcel-advection -> flow-map-gradient -> sigma_max
 * hot path of gabrielmpp/LagrangianCoherence.  The reference is pure Python
 * (no FFI of its own), so every entry point below names the reference Python
 * function it replaces (file:line relative to the reference checkout).  The
 * reference-side binding a maintainer would add is a ctypes stub; it is shown
 * in INTEGRATION.md.
 *
 * Conventions
 *   - plain C: pointers, sizes, doubles.  No torch / C++ types.
 *   - every function returns an lc_status (0 = ok, <0 = error) and records a
 *     message retrievable with lc_last_error() (thread-local).
 *   - "dev" pointers are HIP device pointers valid on the context's device;
 *     "host" pointers are ordinary process memory.  The library never keeps a
 *     caller pointer after the call returns and never hands out memory it
 *     owns, except through lc_malloc (freed with lc_free).
 *   - arrays are C-contiguous; fields are (time, latitude, longitude) with
 *     latitude and longitude ASCENDING (what the reference reaches after its
 *     sortby calls, LCS/trajectory.py:49-52, LCS/LCS.py:101-104).
 *   - dtype selects the arithmetic type of fields AND positions:
 *     LC_F32 (all float) or LC_F64 (all double).
 *   - device work is enqueued on the context's stream and is asynchronous
 *     unless stated; lc_sync() waits for it.
 */
#ifndef LCS_HIP_H
#define LCS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 101: lc_spectral_truncate gained `gridtype`, lc_fourth_order_derivative gained `isglobal` (arguments inserted: a
 * client built against 100 must be rebuilt), lc_ctx_get_level_chunk, lc_ctx_set/get_f64_fidelity, lc_advect_ex and
 * lc_sample_raw added, lc_field_pack accepts packed_dev == NULL at order 1 (fused-level image only).  lc_version() returns the value the LIBRARY
 * was built with: compare it with this macro before any other call (tests/c/abi_smoke.c, _capi.load do). */
#define LC_VERSION 104 /* 0.1.4: + lc_vorticity, lc_vorticity_work_elems, lc_ctx_last_vorticity_kernel, lc_lavd_update, lc_ctx_last_lavd_kernel (added without a bump), + lc_fsle_update, lc_ctx_last_fsle_kernel (added without a bump), + lc_aux_gradient, lc_ctx_last_aux_kernel (added without a bump), + lc_mask_morphology, lc_morph_work_elems (added without a bump), + lc_label_components, lc_label_work_elems, lc_component_sums, lc_component_apply, + lc_strain, lc_ctx_last_strain_kernel, + lc_advect_series_dirs, + lc_advect_series, lc_sigma_batch, + lc_tracer_sample, lc_ctx_last_tracer_kernel (additive: no argument list changed), + lc_ctx_set_host_pipeline, lc_copy_to_device, lc_copy_to_host, lc_ctx_set_host_cache, lc_ctx_trim, lc_ctx_last_host_marks, lc_ctx_set_xcd_split (0.1.3: + lc_ctx_last_pack_kernel; 0.1.2: + lc_ctx_set_verify, lc_ctx_read_verify, LC_F64_WIND_F32_LIN32) */

typedef struct lc_ctx lc_ctx;

enum lc_dtype {
    LC_F32 = 0,
    LC_F64 = 1,
    /* lc_advect only: float64 positions and images whose wind values are float32-valued; the
     * arithmetic follows numpy's promotion for that mix in the reference (samples rounded to float,
     * latitude increments formed in float; LCS/trajectory.py:86-87,110-112 with SURVEY Q10). */
    LC_F64_WIND_F32 = 2,
    /* lc_advect_ex only, interp_order 1 or 3, cyclic or per-point boundaries: the same arithmetic with the wind KEPT float32
     * wherever scipy keeps it; positions, seeds and outputs are float64; results equal LC_F64_WIND_F32's bit for bit.
     *   interp_order 1: packed_lin is the order-1 image lc_field_pack builds for LC_F32 (half the bytes, no float64 copy of
     *                   the wind: a node is widened as it is read), every other image pointer NULL; per-wave LDS tiles of
     *                   levels t and t + 1.
     *   interp_order 3: packed_cub is the FLOAT64 coefficient image of the float32 planes -- lc_field_pack(LC_F64_WIND_F32,
     *                   order 3): scipy's spline_filter(output=float64) inside map_coordinates -- and u_raw / v_raw are the
     *                   float32 planes themselves (the order-1 source of the pole rows); packed_lin NULL.
     * (lc_field_pack accepts LC_F64_WIND_F32 for interp_order 2..5 without ext_dev: float32 planes in, float64 image out.) */
    LC_F64_WIND_F32_LIN32 = 3
};

enum lc_status {
    LC_OK = 0,
    LC_EINVAL = -1,       /* bad argument (null pointer, bad size, bad enum) */
    LC_EUNSUPPORTED = -2, /* e.g. interp_order outside 1..5                  */
    LC_EHIP = -3,         /* a HIP runtime call failed                       */
    LC_ENOMEM = -4,
    LC_ERCCL = -5         /* RCCL missing or an RCCL call failed             */
};

/* lc_advect's cyclic_x argument: what happens to a longitude that leaves [lon_min, lon_max]
 * (LCS/trajectory.py:92-97, 118-123). */
enum lc_xboundary {
    LC_X_CLAMP_POINT = 0, /* cyclic_xboundary=False, each parcel clamped on its own (NOT the reference when a parcel
                             leaves the box: see LC_X_CLAMP_REFERENCE_OUTER) */
    LC_X_CYCLIC = 1,      /* cyclic_xboundary=True: wrap hard-coded to +-180 with Python's floor-mod (Q7)          */
    /* cyclic_xboundary=False exactly as the reference computes it: `positions_x[np.where(x < x_min)] = x_min` on a
     * DataArray is orthogonal indexing, so every (row, col) in the cross product of offending rows and offending
     * columns is set (trajectory.py:96-97, 122-123).  lc_advect runs the fused kernel in chunks of 16 time
     * levels, reads a "clamp fired" flag back after each (the call is SYNCHRONOUS in this mode: one stream
     * synchronisation per chunk) and, from the chunk in which a parcel first left the box, continues sub-step by
     * sub-step with that rule (2 (K+1) launches per time level, positions in global memory) from the positions saved
     * before that chunk; if no parcel ever leaves, the fused result stands.
     * The rule couples every seed row through the offending COLUMNS: a call on a row block (row0 != 0 or
     * ny != ny_global) needs lc_ctx_set_flag_allreduce, through which the ranks of a row-sharded grid OR their
     * column flags after every sub-step; without it such a call is refused. */
    LC_X_CLAMP_REFERENCE_OUTER = 2
};

enum lc_tensor_layout {
    LC_LAYOUT_REFERENCE = 0, /* 9 comps reshaped row-major to 3x3 (LCS/LCS.py:152-153) */
    LC_LAYOUT_PHYSICAL = 1   /* Jacobian d(X,Y,Z)/d(x,y); NOT reference behaviour      */
};

/* ---- library / context ------------------------------------------------- */
int lc_version(void);
const char *lc_last_error(void);
/* What this binary was built from: the hash of the kernel sources + this header (comments and white space stripped;
 * lagrangiancoherence_amd/build.py csrc_hash), followed by "+<flags>" when it is an experiment build with extra -D
 * flags; "unstamped" for a build that bypassed build.py.  A benchmark replays committed profiler counters only for
 * the binary they were measured on. */
const char *lc_build_id(void);

/* One context per device; distinct contexts may be used from distinct host
 * threads.  The context owns one HIP stream unless lc_ctx_set_stream lends it
 * an external one (e.g. the stream a host framework is already using). */
int lc_ctx_create(int device, lc_ctx **out);
int lc_ctx_destroy(lc_ctx *ctx);
int lc_ctx_set_stream(lc_ctx *ctx, void *hip_stream /* hipStream_t; NULL = the device's default stream */);
int lc_ctx_use_own_stream(lc_ctx *ctx); /* back to the context's private stream */
int lc_sync(lc_ctx *ctx);

/* Kernel choice of lc_advect: -1 = what lc_ctx_create set (LCS_LDS_TILES, else the default): per-wave LDS tiles -- float32
 * orders 1 and 3 with two seeds per lane from 2^23 seeds per call upwards and one seed per lane below (smaller launches
 * want the waves), float64 order 1 with packed_ext one seed per lane; 1 = LDS tiles, two seeds per lane whatever the
 * size; 2 = LDS tiles, one seed per lane; 0 = direct gathers (float32 and float64).  SETTLS_order = 0 stages no tile at
 * order 1: direct gathers, two seeds per lane from 2^23 seeds per call upwards (the two-seed kernel compiled without its tile
 * and iteration blocks), one per lane below; the LDS kernels at order 3.  The environment variable LCS_LDS_TILES (0/1/2) sets the initial
 * value, read ONCE in lc_ctx_create (profiling A/B; results are bit-identical either way).  No reference counterpart. */
int lc_ctx_set_lds_tiles(lc_ctx *ctx, int mode);
/* Kernel choice of lc_sigma for float32 sigma-only calls on grids of even width: 1 = marching kernel (a wave walks
 * down its rows with five rows of X, Y, Z in registers and takes the x-neighbours by wavefront shuffle), 0 = the
 * LDS-tile kernel that also serves odd widths, -1 = what lc_ctx_create set (LCS_SIGMA_MARCH, else the default): the marching kernel from 2^23 cells per call upwards
 * (its waves walk 24 rows one after the other: smaller grids finish sooner as many short-lived tiles).
 * LCS_SIGMA_MARCH (0/1) sets the initial value, read ONCE in lc_ctx_create.  Results are bit-identical either way.
 * No reference counterpart. */
int lc_ctx_set_sigma_march(lc_ctx *ctx, int on);
/* Row-sharded grids with LC_X_CLAMP_REFERENCE_OUTER: `fn(user, flags_dev, count)` must replace the `count` uint32
 * flags at `flags_dev` (device memory of this context) by their element-wise MAXIMUM over all ranks that hold row
 * blocks of the same seed grid, ordered after the work already enqueued on the context's stream and before
 * anything enqueued on it afterwards (an all-reduce on that stream, or one that synchronises with it); it returns
 * 0 on success.  Every rank's lc_advect calls it the same number of times: once for "did any parcel leave the box
 * anywhere", then -- only if one did -- twice per sub-step for the offending-column flags (nx of them) of the
 * reference's two assignments (LCS/trajectory.py:96-97, 122-123).  NULL (the default) = single process.
 * lc_comm_flag_allreduce (below) is such a function for an lc_comm. */
typedef int (*lc_flag_allreduce_fn)(void *user, void *flags_dev, size_t count);
int lc_ctx_set_flag_allreduce(lc_ctx *ctx, lc_flag_allreduce_fn fn, void *user);
/* lc_advect / lc_advect_from run a series of nsteps time levels as consecutive launches of at most `levels` levels,
 * each continuing from the positions the previous one stored (0 = one launch; -1 = by size, the default: from 2^18
 * seeds per call upwards 32 levels per launch for SETTLS_order >= 3, 64 for 2, one launch below).  Results are bit-identical whatever the value; it shapes the launches
 * only (workgroups of one launch stay within `levels` levels of each other, so their tiles of the wind images meet in
 * L2 / the Infinity Cache, and the launch's tail is one chunk long: long series and sparse seed grids gain 7-17 %).
 * The environment variable LCS_LEVEL_CHUNK sets the initial value, read ONCE in lc_ctx_create.  No reference
 * counterpart (the reference's loop over time levels is LCS/trajectory.py:80-126). */
int lc_ctx_set_level_chunk(lc_ctx *ctx, int levels);
/* The value in force (what lc_ctx_set_level_chunk was last given, or what LCS_LEVEL_CHUNK set at creation): a caller
 * that changes it for one call restores THIS, not a guess. */
int lc_ctx_get_level_chunk(const lc_ctx *ctx, int *levels_out);
/* Graded level counts (additive: LC_VERSION stays 104).  With the by-size level chunk (lc_ctx_set_level_chunk(-1), the
 * default) the float32 order-1 two-seed kernel -- one member, no trajectories, cyclic or per-point boundaries -- may give
 * the workgroups at the END of a launch's dispatch order fewer levels than `chunk`, so that a launch ends at once instead
 * of draining through one workgroup lifetime; they make the levels up in the next launch, which starts them early.
 *   chunk  levels per launch where the grading applies (0 = the by-size chunk; > 0 also on grids the by-size rule runs in
 *          one launch: tests);
 *   zone   workgroups at a launch's end that are cut short (-1 = the default for the device; rounded down to a multiple
 *          of 8 and to what the launch count allows);
 *   depth  levels the last workgroup loses, linearly less before it (-1 = the default; 0 = off: uniform chunks).
 * Results are bit-identical whatever the values: positions at a level's end are the kernel's whole state.  Every other
 * kernel, and any explicit lc_ctx_set_level_chunk(n >= 0), runs uniform chunks.  lc_ctx_last_advect_launches counts the
 * launches as before.  No environment variable; no reference counterpart (LCS/trajectory.py:80-126 is one loop). */
int lc_ctx_set_level_grading(lc_ctx *ctx, int chunk, int zone, int depth);
int lc_ctx_get_level_grading(const lc_ctx *ctx, int *chunk_out, int *zone_out, int *depth_out);
/* float64 on the ONE-CALL host routes (lc_lcs_host, lc_lcs_global_host -- what a reference-side binding calls, where a
 * user expects the reference's numbers): which form of the SETTLS iteration they take.
 *   LC_F64_EXACT_ORDER  numpy / scipy's operation order (two samples per iteration, true divisions, scipy's tap sums;
 *                       LCS/trajectory.py:86-87,110-112): ~1e-13 degrees from the reference's float64 result;
 *   LC_F64_FAST         one sample of the fused-level image 2F[t]-F[t+1] per iteration, multiplied index map, fused
 *                       lerps: the same mathematics with different ROUNDING, 1.4-2x faster at BASELINE config 2's size;
 *                       distance from the reference <= 1e-9 degrees, or the flow's own amplification of a 1e-12 degree
 *                       seed shift if that is larger (ill-conditioned flows; INTEGRATION.md "Behavioural notes");
 *   LC_F64_AUTO         (default) exact order up to LC_EXACT_ORDER_MAX_SEEDS seeds per call -- there the time is launch
 *                       latency, not arithmetic: the reference's example (89 x 180) and the 360 x 721 common grid of
 *                       isglobal=True are on this side -- and the fast form above.
 * float32 always takes the fused form (it cannot be bit-comparable with scipy's float64 interpolation anyway).
 * lc_advect itself is explicit: packed_ext == NULL is the exact order.  LCS_F64_FIDELITY (auto / exact / fast) sets the
 * initial value, read ONCE in lc_ctx_create. */
enum lc_f64_fidelity { LC_F64_AUTO = 0, LC_F64_EXACT_ORDER = 1, LC_F64_FAST = 2 };
#define LC_EXACT_ORDER_MAX_SEEDS (1 << 18)
int lc_ctx_set_f64_fidelity(lc_ctx *ctx, int mode);
int lc_ctx_get_f64_fidelity(const lc_ctx *ctx, int *mode_out);
/* How the one-call host routes move their host buffers (no reference counterpart: LCS/LCS.py:129-157 runs on host arrays).
 *   1 (default)  through a ring of four 32 MB pinned staging buffers filled / emptied by a few host threads (ONE ring per device
 *                and process, shared by its contexts -- a process's second copy stream runs 25 % slower --, taken by a context's
 *                first staged transfer, released by lc_ctx_destroy, freed with the last context that holds it; transfers of
 *                different contexts take turns): pageable caller memory
 *                then travels at the bus rate whatever state its pages are in (hipMemcpy from pages the runtime has not pinned
 *                before runs at a quarter of it), the upload is cut at time-level boundaries and the pack + advect kernels of level
 *                chunk c run while chunk c + 1 is on the bus (cyclic_x = LC_X_CYCLIC, fused levels, no trajectories, 32 steps or
 *                more; lc_advect_from continuation: bit-identical to the serial form), only the levels [t0, t0 + nsteps] travel,
 *                and the caller's output pages are populated by background threads meanwhile.  A host with no pinned memory to
 *                give falls back to 0 by itself.
 *   0            plain hipMemcpyAsync of the whole series on the context's stream, then pack, advect, sigma, copies back.
 * LCS_HOST_PIPELINE (0 / 1) sets the initial value, read ONCE in lc_ctx_create. */
int lc_ctx_set_host_pipeline(lc_ctx *ctx, int on);
/* Copies between a caller's ordinary (pageable) host array and device memory through the context's staging ring (see
 * lc_ctx_set_host_pipeline; plain hipMemcpy with it switched off), ordered with the context's stream: work enqueued on the
 * stream after lc_copy_to_device sees the data (the source may be reused as soon as the call returns); lc_copy_to_host sees
 * everything enqueued before it and returns when the bytes are in `host`.  What the Python host moves large arrays with
 * (numpy -> device tensor, results -> numpy): a first-touch hipMemcpy of pageable memory runs at 12-14 GB/s, these at the bus's 55. */
int lc_copy_to_device(lc_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);
int lc_copy_to_host(lc_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);
/* lc_lcs_host keeps the device buffers of its last call on the context (1, the default) and hands them to the next call that
 * fits them: hipMalloc + hipFree of BASELINE configs[2]'s 2.6 GB are 1.6 ms of a 21 ms call.  lc_ctx_trim frees what is kept
 * (device memory returns to the system; the next call allocates again), lc_ctx_destroy does too; 0 = allocate and free per call.
 * LCS_HOST_CACHE (0 / 1) sets the initial value, read ONCE in lc_ctx_create. */
int lc_ctx_set_host_cache(lc_ctx *ctx, int on);
int lc_ctx_trim(lc_ctx *ctx);
/* Wall-clock marks of the context's last lc_lcs_host call, milliseconds since its entry: [0] device buffers allocated, [1] the
 * last upload piece handed to the DMA engine and the last kernel launched, [2] kernels finished (0 with plain copies), [3]
 * results in the caller's buffers.  (A benchmark reports the upload / compute tail / download split with them.) */
int lc_ctx_last_host_marks(const lc_ctx *ctx, double *ms4_out);
/* How lc_advect deals the workgroups of a launch to the 8 XCDs: -1 (default) by the launch's shape -- whole workgroup rows
 * cyclically, eighths of a row when the row count would leave the XCDs more than 15 % apart; 0 whole rows always; n > 0 a
 * 1 / n part of a row per chunk.  (A seed block whose rows do not cost alike -- the polar rows of a global grid take several
 * times longer -- ends on the XCD that drew them; 8 spreads every row over all XCDs at ~4-15 % on launches that were even.)
 * LCS_XCD_SPLIT sets the initial value, read ONCE in lc_ctx_create. */
int lc_ctx_set_xcd_split(lc_ctx *ctx, int split);
/* Name of the kernel the context's last lc_advect call launched (static string, "" before the first call);
 * what a profiler shows, so a benchmark labels its numbers with the kernel that actually ran. */
const char *lc_ctx_last_advect_kernel(const lc_ctx *ctx);
/* Kernel launches that call made (level chunks: lc_ctx_set_level_chunk); a benchmark divides its event time by it to
 * quote the duration of ONE launch, the figure a profiler's per-kernel average shows. */
int lc_ctx_last_advect_launches(const lc_ctx *ctx);
/* The same for the context's last lc_sigma / lc_flowmap_gradient call. */
const char *lc_ctx_last_sigma_kernel(const lc_ctx *ctx);
/* The kernel the last lc_field_pack launched for its first stage (interleave / spline prefilter; "" before any): e.g.
 * "pack_fused_kernel", "prefilter_fir_kernel", "prefilter_fused_stream_kernel<double>" (float64 order 3, both axes of 64
 * nodes or more: both prefilter sweeps in one pass), "prefilter_cols_stream_kernel + prefilter_rows_stream_kernel".  Every
 * path names the kernels it launched: the split sweeps as "<latitude kernel> + <longitude kernel>" (prefilter_cols_kernel /
 * prefilter_cols_stream_kernel, then prefilter_rows_kernel / prefilter_rows_lds_kernel -- lines of 64 nodes or more outside
 * the streaming form -- / prefilter_rows_stream_kernel), LCS_FIR_PREFILTER=2 with ext_dev as "prefilter_fir_kernel (img + ext)"
 * (the fused-level image as a second filtered image), orders 2, 4, 5 as "pack_interior_kernel + prefilter_general_kernel".  The pads
 * / fused-level pass that follows is not named.  Same lifetime as lc_ctx_last_advect_kernel's string. */
const char *lc_ctx_last_pack_kernel(const lc_ctx *ctx);
/* The kernel the context's last lc_tracer_sample launched ("" before any): "tracer_kernel<float | double, interp_order>".
 * Same lifetime as lc_ctx_last_advect_kernel's string. */
const char *lc_ctx_last_tracer_kernel(const lc_ctx *ctx);
/* Wave-state audit (diagnostic; no reference counterpart).  mode 1: float32 lc_advect calls that dispatch to the one-seed
 * LDS-tile kernels (orders 1 and 3 below 2^23 seeds per call, SETTLS_order > 0, no whole-line trajectory stores) run their "verify" instances:
 * after the iterations of every time level each wave reads back the tile of the wind image it staged in LDS for that
 * level and compares it, 16 bytes per lane, with the registers it staged it from, and compares HW_REG_HW_ID /
 * HW_REG_XCC_ID with the values it read when it started.  A wave's tile and registers are written by that wave only,
 * so a non-zero count means the wave's state was changed from OUTSIDE the kernel: its context saved and restored by
 * the driver (several processes time-sharing one GPU) with something lost on the way, or a hardware fault.  Results
 * are bit-identical to the plain instances (a few percent slower).  mode 2 additionally overwrites one tile entry once
 * (tile 5, wave 1, second level) so that a test can see the audit fire; mode 0 frees the counters.
 * lc_ctx_read_verify synchronises the context's stream and copies the LC_VERIFY_WORDS counters:
 *   [0] wave-levels whose tile differed, [1] 16-byte entries that differed, [2] wave-levels at which the wave sat in
 *   another hardware slot than one level earlier (a context switch; harmless by itself), [3] wave-levels audited,
 *   [4..11] the first event: workgroup, tile, wave, time level, HW_ID before / after, lane mask low / high word.
 * `reset` != 0 zeroes them afterwards. */
#define LC_VERIFY_WORDS 16
int lc_ctx_set_verify(lc_ctx *ctx, int mode);
int lc_ctx_read_verify(lc_ctx *ctx, unsigned *out16, int reset);

/* ---- device memory (so a ctypes-only host needs nothing else) ---------- */
int lc_malloc(lc_ctx *ctx, size_t bytes, void **dev_out);
int lc_free(lc_ctx *ctx, void *dev);
int lc_memcpy_h2d(lc_ctx *ctx, void *dev_dst, const void *host_src, size_t bytes); /* synchronous */
int lc_memcpy_d2h(lc_ctx *ctx, void *host_dst, const void *dev_src, size_t bytes); /* synchronous */

/* ---- field preparation --------------------------------------------------
 * Replaces the per-call work of tools.xr_map_coordinates that does not depend
 * on the seeds (LCS/tools.py:12-14 copies; for order 3 the whole-field spline
 * prefilter scipy redoes inside every map_coordinates call, LCS/tools.py:26).
 *
 * Builds the gather-ready image of a wind time series: per time level a
 * (ny_f+3) x (nx_f+3) array of interleaved (u,v) nodes -- 1 mirrored node in
 * front and 2 behind on each axis, so the 2x2 / 4x4 tap windows never need
 * index logic.  order 1: raw values.  orders 2..5: B-spline coefficients of that order
 * (mirror-boundary prefilter with scipy's pole lists, exact-sum initialisation ==
 * scipy.ndimage.spline_filter(order, mode='mirror'); orders 4, 5 agree with scipy to 1e-12: the pole
 * constants differ in the last bit).
 *
 * lc_packed_elems() = number of dtype elements the image needs.
 * interp_order 1 with packed_dev == NULL and ext_dev != NULL builds ONLY the fused-level image: what a float64
 * caller needs who hands lc_advect_ex the raw planes as the order-1 source (half the bytes written).          */
size_t lc_packed_elems(int nt, int ny_f, int nx_f);
int lc_field_pack(lc_ctx *ctx, const void *u_dev, const void *v_dev, int dtype,
                  int nt, int ny_f, int nx_f, int interp_order, void *packed_dev,
                  void *ext_dev /* NULL, or lc_packed_elems(nt-1,..): also build the
                                   lc_field_extrapolate image of this order in the same call */);

/* Deferred pack (additive: LC_VERSION stays 104).  lc_field_pack(LC_F32, order 1) with both images, of which only the levels
 * the first launch of a fused lc_advect call reads are packed now -- packed_dev[0 .. first_levels] and ext_dev[0 .. first_levels - 1];
 * first_levels <= 0: the default level chunk, 32 -- while the rest stays PENDING in the context: an lc_advect_ex call on exactly
 * these images that runs the tall-patch two-seed kernel in more than one launch (one member, settls_order > 0, no
 * trajectories, no outer clamp, t0 + its first launch's levels below the packed ones) packs them inside its own launches, in
 * extra workgroups placed among the advecting ones: the pack streams memory that the advect kernel leaves idle.  EVERY other
 * entry point that takes image pointers or packs completes the pending pack first with the stand-alone kernel, as do a
 * second deferred pack (one pending pack per context), a change of the context's stream, lc_sync, lc_free, lc_memcpy_d2h,
 * lc_copy_to_host, lc_copy_to_device and
 * lc_ctx_destroy: nothing called through this interface reads an incomplete image.  The images are the same bits as
 * lc_field_pack's.  u_dev and v_dev must stay alive and unchanged until the pack is complete (lc_ctx_pack_pending() == 0).  A
 * caller that reads the images by other means (its own kernels, copies not made through this library) calls
 * lc_ctx_flush_pack first.  A series that the first levels cover anyway (nt - 1 <= first_levels), and every call while
 * deferring is switched off (lc_ctx_set_deferred_pack(ctx, 0), or LCS_DEFER_PACK=0 in the environment when the context is
 * created), is packed at once, exactly as lc_field_pack does.
 * lc_ctx_pack_pending: the first level of packed_dev not packed yet, 0 when nothing is pending.
 * lc_ctx_set_deferred_pack_mix: of every `period` consecutive workgroups of a launch that carries a pack (a power of two, 32
 * to 16384; 0, the default: chosen per launch so that a pack workgroup has 7 items or a few more) the last pack_blocks (8, 16 or 24; default 8) are pack workgroups; item_levels (2, 4 or 8; default 8):
 * the time levels per item of theirs.  Measurement knobs: results do not depend on them.  No environment variables.
 * A change of the context's stream completes the pack on the stream it began on and makes the new stream wait for it. */
int lc_field_pack_deferred(lc_ctx *ctx, const void *u_dev, const void *v_dev, int nt, int ny_f, int nx_f, int first_levels,
                           void *packed_dev, void *ext_dev);
int lc_ctx_flush_pack(lc_ctx *ctx);
int lc_ctx_pack_pending(const lc_ctx *ctx);
int lc_ctx_set_deferred_pack(lc_ctx *ctx, int on);
int lc_ctx_set_deferred_pack_mix(lc_ctx *ctx, int pack_blocks, int period, int item_levels); /* UNSTABLE: for measurements only, may change or go without a version bump */

/* Optional third image for the SETTLS iterations: ext[t] = 2*packed[t] - packed[t+1],
 * t = 0..nt-2 (same layout, nt-1 levels).  Interpolation is linear in the field, so
 * one sample of ext[t] equals 2*interp(F[t]) - interp(F[t+1]) of trajectory.py:110-112
 * up to rounding, and halves the gathers of every SETTLS iteration.  Build it from
 * the image that matches interp_order (raw for 1, coefficients for 3). */
int lc_field_extrapolate(lc_ctx *ctx, const void *packed_dev, int dtype,
                         int nt, int ny_f, int nx_f, void *ext_dev);

/* ---- global pre-processing of LCS.__call__(isglobal=True) -----------------
 * lc_regrid_common_grid replaces LCS/LCS.py:107-114: `u.interp(latitude=lats, longitude=lons, method='linear')`
 * with the holes (targets outside the source range, NaN results) filled from `u.reindex(method='nearest')`.
 * One fused kernel: latitude lerp, longitude lerp (scipy.interpolate.interp1d's operation order), nearest
 * fill.  src [nt][ny_s][nx_s] in `dtype` on the device, coordinates ascending, as host doubles; out
 * [nt][ny_d][nx_d] float64 on the device (xarray's interp result is float64).  The reference's target grid is
 * lats = linspace(-89.75, 89.75, 360), lons = linspace(-180, 179.5, 721). */
int lc_regrid_common_grid(lc_ctx *ctx, const void *src_dev, int dtype, int nt, int ny_s, int nx_s,
                          const double *src_lat_host, const double *src_lon_host,
                          const double *dst_lat_host, int ny_d, const double *dst_lon_host, int nx_d,
                          double *out_dev);

/* lc_spectral_truncate replaces LCS/LCS.py:115-118: windspharm `VectorWind(u, v).truncate(f, truncation=T)`
 * = spherical-harmonic analysis, triangular truncation n <= T, synthesis.  gridtype is what windspharm's grid
 * inspection finds: LC_GRID_REGULAR = SPHEREPACK's equally spaced grid (theta_i = i pi / (nlat-1); shaes/shses),
 * LC_GRID_GAUSSIAN = Gauss-Legendre latitudes (shags/shsgs: Gaussian quadrature).  f, out: [nbatch][nlat][nlon] in
 * `dtype`, latitude ASCENDING; computed in float64.  Operators are built on the host once per (nlat, nlon, T,
 * gridtype) and cached on the context.  Any T <= min(nlat-1, (nlon-1)/2).  Restates the published algorithm
 * (Swarztrauber 1979); not pinned against pyspharm. */
enum lc_gridtype { LC_GRID_REGULAR = 0, LC_GRID_GAUSSIAN = 1 };
/* windspharm's latitude inspection (what VectorWind does with the grid it is handed, LCS/LCS.py:116): equally spaced
 * global latitudes -> LC_GRID_REGULAR, Gaussian latitudes -> LC_GRID_GAUSSIAN (both to 5e-4 degrees), anything else
 * LC_EINVAL with windspharm's message.  lat_ascending: host doubles.  No device work. */
int lc_inspect_gridtype(const double *lat_ascending, int nlat, int *gridtype_out);
int lc_spectral_truncate(lc_ctx *ctx, const void *f_dev, int dtype, int nbatch, int nlat, int nlon,
                         int truncation, int gridtype, void *out_dev);

/* ---- K1: parcel advection ------------------------------------------------
 * Replaces trajectory.parcel_propagation (LCS/trajectory.py:8-144) together
 * with every tools.xr_map_coordinates call it makes (LCS/tools.py:11-41):
 * Euler + settls_order accumulate-"SETTLS" sub-steps per time level, latitude
 * clamp, cyclic (+-180) or clamped longitude, all nsteps fused in one launch.
 *
 *   packed_lin   image from lc_field_pack(order=1)   (always required: the
 *                first/last interp_order seed rows use order 1 + 'constant')
 *   packed_cub   image from lc_field_pack(order=interp_order), or NULL when interp_order==1.  interp_order may be
 *                any of scipy's spline orders 1..5 (LCS/trajectory.py:16, LCS/tools.py:26-30 hand it to
 *                map_coordinates); 1 and 3 have the fused / LDS-tile kernels, 2, 4 and 5 a generic direct one
 *                (no packed_ext).  0 fails in the reference itself (empty interior slice).
 *   packed_ext   image from lc_field_extrapolate, or NULL.  NULL = two samples per
 *                SETTLS iteration in the reference's operation order (the float64
 *                default, results identical to numpy/scipy's); non-NULL = one sample
 *                of the combined field 2F[t]-F[t+1] (the float32 default; opt-in for
 *                LC_F64, where it moves results by rounding only, ~1e-13 degrees)
 *   lat_min..lon_max   extremes of the FIELD coordinates (index scale, tools.py:21-22,
 *                and the clamp bounds, trajectory.py:63-66)
 *   seed_lat[ny], seed_lon[nx]   seed coordinates (dtype elements, device).  The
 *                reference seeds at the field nodes (trajectory.py:68-70): pass the
 *                field coordinates for that.
 *   row0, ny_global   this call advects seed rows [row0, row0+ny) of a grid of
 *                ny_global rows (row sharding across GPUs); the pole-row rule
 *                applies to the global row index.  Single GPU: 0, ny.
 *   timestep     seconds, sign = direction; fields are always consumed in stored
 *                order t0, t0+1, ... (trajectory.py:58-60,80)
 *   cyclic_x     enum lc_xboundary
 *   t0, nsteps   first time level and number of steps (t0+nsteps <= nt-1);
 *                the reference is t0=0, nsteps=nt-1
 *   x_out,y_out  [ny*nx] departure longitude / latitude, degrees
 *   traj_x,traj_y  NULL, or [(nsteps+1)*ny*nx]: positions after every step,
 *                entry 0 = seed grid (return_traj=True, trajectory.py:125-139)
 */
int lc_advect(lc_ctx *ctx, const void *packed_lin, const void *packed_cub,
              const void *packed_ext, int dtype,
              int nt, int ny_f, int nx_f,
              double lat_min, double lat_max, double lon_min, double lon_max,
              const void *seed_lat_dev, int ny, const void *seed_lon_dev, int nx,
              int row0, int ny_global,
              double timestep, int settls_order, int interp_order, int cyclic_x,
              int t0, int nsteps,
              void *x_out, void *y_out, void *traj_x, void *traj_y);

/* lc_advect continuing from given positions instead of the seed grid: x_start, y_start [ny*nx] (dtype elements,
 * device; both NULL = lc_advect).  The seed coordinates are still needed -- conversion_x is a function of the SEED
 * latitude for the whole integration (LCS/trajectory.py:56-57, Q5) and the pole-row rule of the seed row index
 * (LCS/tools.py:24-39, Q3).  Running levels [t0, t0+a) with lc_advect and [t0+a, t0+a+b) with lc_advect_from on the
 * first call's outputs gives, bit for bit, what one call over a+b levels gives: the loop body of
 * LCS/trajectory.py:80-126 carries no state from one time level to the next except the positions.  x_start / y_start
 * may alias x_out / y_out (in place).  traj entry 0 = the start positions.  Not with LC_X_CLAMP_REFERENCE_OUTER. */
int lc_advect_from(lc_ctx *ctx, const void *packed_lin, const void *packed_cub,
                   const void *packed_ext, int dtype,
                   int nt, int ny_f, int nx_f,
                   double lat_min, double lat_max, double lon_min, double lon_max,
                   const void *seed_lat_dev, int ny, const void *seed_lon_dev, int nx,
                   int row0, int ny_global,
                   const void *x_start, const void *y_start,
                   double timestep, int settls_order, int interp_order, int cyclic_x,
                   int t0, int nsteps,
                   void *x_out, void *y_out, void *traj_x, void *traj_y);

/* lc_advect_from for an ENSEMBLE of n_members start times over one seed grid and one wind series, in one launch per
 * level chunk: member m integrates nsteps steps from time level t0 + m * t0_stride (BASELINE config 5: stride 1) and
 * keeps its positions in the m-th [ny*nx] plane of x_start / x_out ([n_members][ny*nx]; x_start NULL = every member
 * starts on the seed grid; in place allowed).  With lc_ctx_set_level_chunk(c) the members advance together c levels
 * at a time (level-major order), so the launches of a chunk share all but a few of their time levels in the caches
 * and a launch is n_members times deeper than a member's own (no tail of idle compute units between members).  In
 * float32 at order 1 with SETTLS_order > 0, from 2^23 seeds per call, consecutive members share a LANE (members 2p and
 * 2p + 1 at the same grid point: at field level l one takes its step l, the other its step l - t0_stride, from one staged
 * tile of the wind), and the launches walk the pair's level window instead of a step range.  Each
 * member's result is, bit for bit, what lc_advect(t0 + m * t0_stride) gives.  traj_x / traj_y must be NULL and
 * cyclic_x must not be LC_X_CLAMP_REFERENCE_OUTER when n_members > 1.  No reference counterpart: there the caller
 * loops over start times (LCS/trajectory.py:80 consumes one series). */
int lc_advect_batch(lc_ctx *ctx, const void *packed_lin, const void *packed_cub,
                    const void *packed_ext, int dtype,
                    int nt, int ny_f, int nx_f,
                    double lat_min, double lat_max, double lon_min, double lon_max,
                    const void *seed_lat_dev, int ny, const void *seed_lon_dev, int nx,
                    int row0, int ny_global,
                    const void *x_start, const void *y_start,
                    double timestep, int settls_order, int interp_order, int cyclic_x,
                    int t0, int nsteps, int n_members, int t0_stride,
                    void *x_out, void *y_out, void *traj_x, void *traj_y);

/* lc_advect_batch with its arguments in one structure (same names, same meaning), plus the RAW wind planes as the
 * order-1 source in place of the packed_lin image:
 *   u_raw, v_raw   NULL, or the [nt][ny_f][nx_f] arrays lc_field_pack was given (dtype elements, device, still alive and
 *                  unchanged).  With them packed_lin may be NULL when interp_order != 1 (the first / last interp_order
 *                  seed rows gather their order-1 / 'constant' samples, LCS/tools.py:31-39, straight from the planes) and
 *                  in LC_F64 / LC_F64_WIND_F32 at interp_order 1 (the Euler sample, LCS/trajectory.py:82-84, too): the
 *                  order-1 image is then never built, written or read -- one third of the pack's traffic at order 1 and a
 *                  fifth at order 3 -- and the results are bit-identical to the packed_lin form (same node values, same
 *                  arithmetic).  LC_F32 at interp_order 1 keeps packed_lin (its kernels read 16-byte {u, v} node pairs)
 *                  and ignores the planes.
 *   struct_size    sizeof(lc_advect_args) as the caller compiled it: a library built for another layout refuses.
 * lc_advect / lc_advect_from / lc_advect_batch are this call with u_raw = v_raw = NULL. */
typedef struct lc_advect_args {
    size_t struct_size;
    const void *packed_lin, *packed_cub, *packed_ext;
    const void *u_raw, *v_raw;
    int dtype, nt, ny_f, nx_f;
    double lat_min, lat_max, lon_min, lon_max;
    const void *seed_lat_dev;
    int ny;
    const void *seed_lon_dev;
    int nx;
    int row0, ny_global;
    const void *x_start, *y_start;
    double timestep;
    int settls_order, interp_order, cyclic_x;
    int t0, nsteps, n_members, t0_stride;
    void *x_out, *y_out, *traj_x, *traj_y;
    /* LC_F64 at interp_order 1 with u_raw / v_raw and packed_ext == NULL: 1 = take the fused-level form all the same -- the
     * value packed_ext would hold, 2 F[t] - F[t+1], is formed from the raw planes node by node inside the kernels (the
     * same expression, one rounding: results equal those with packed_ext bit for bit).  No packed image exists then:
     * lc_field_pack is not called at all for such a field.
     * LC_F64 at interp_order 3 with packed_cub and packed_ext == NULL: 1 = the same for the spline coefficients -- the
     * kernels form 2 c[t] - c[t+1] from packed_cub node by node (lc_field_pack's own expression: bit-identical to a call
     * with packed_ext), so lc_field_pack(order 3, ext_dev = NULL) is the whole pack: it neither reads the coefficients back
     * nor writes a second image, and the advect kernel streams one image series from memory instead of two.
     * 0 (and every other dtype / order): packed_ext == NULL means the reference's two-sample operation order, as in
     * lc_advect. */
    int fuse_levels_raw;
} lc_advect_args;
int lc_advect_ex(lc_ctx *ctx, const lc_advect_args *args);

/* A sliding-window series of lc_advect_ex calls in one: lc_advect_ex's arguments and semantics for n_members >= 1 (member m
 * integrates nsteps steps from time level t0 + m * t0_stride, its positions in the m-th [ny*nx] plane of x_out / y_out),
 * whole seed grids only (row0 == 0, ny == ny_global), traj_x / traj_y NULL.  LC_X_CYCLIC and LC_X_CLAMP_POINT run as
 * lc_advect_batch does.  LC_X_CLAMP_REFERENCE_OUTER (which lc_advect_batch refuses) runs lc_advect's rule for every member
 * at once: the fused ensemble launch in chunks of 16 levels with one clamp flag PER MEMBER (all read back once per chunk),
 * each member's positions saved before its current chunk; a member whose flag never fires keeps its fused result, the
 * others re-run from the start of the chunk in which their own flag fired, sub-step by sub-step, all of them in one launch
 * per sub-step (lc_ctx_last_advect_kernel: "outer_substep_batch_kernel").  Each member's result is, bit for bit, what
 * lc_advect_ex(t0 + m * t0_stride, n_members = 1) gives.  No flag all-reduce is made (lc_ctx_set_flag_allreduce is for
 * row blocks). */
int lc_advect_series(lc_ctx *ctx, const lc_advect_args *args);

/* lc_advect_series in both directions of time at once: the reference example's pair of calls
 * LCS(timestep=+dt)(ds) and LCS(timestep=-dt)(ds) (examples/ideal_vortex.py:280-288) on one packed record.  Quirk Q6: the
 * reference reads the levels in stored order whatever the sign of timestep (LCS/trajectory.py:58-60,80-84,105-108), so both
 * directions read the same levels.
 * n_dirs = 1 is lc_advect_series.  n_dirs = 2: x_out / y_out hold 2 * n_members planes [2 * n_members][ny*nx]; plane
 * 2w + d is window w (nsteps steps from level t0 + w * t0_stride), with args->timestep for d = 0 and -args->timestep for
 * d = 1, and equals lc_advect_ex(t0 + w * t0_stride, +-timestep, n_members = 1) bit for bit (T(-x) == -T(x): each plane's
 * kernel sees the four step constants that call forms).  The outer clamp
 * (LC_X_CLAMP_REFERENCE_OUTER) is decided per plane, as lc_advect_series decides it per window.  Each level chunk makes
 * one fused launch per direction, the launches lc_advect_series makes for the same windows (lc_ctx_last_advect_kernel
 * names the same kernel).  Refused before any HIP call: what lc_advect_series refuses (row blocks, traj_x / traj_y), and
 * n_dirs other than 1 or 2 (LC_EINVAL).  The level range is checked in windows. */
int lc_advect_series_dirs(lc_ctx *ctx, const lc_advect_args *args, int n_dirs);

/* One interpolation pass on its own: tools.xr_map_coordinates (LCS/tools.py:11-41) for the
 * u and v fields of time level `level` at the given positions (degrees), same index
 * scale, row classes and boundary modes as inside lc_advect.  pos_x/pos_y/out_u/out_v
 * are [ny*nx] dtype elements on the device.
 * Positions that are not finite (every interp_order, both dtypes; the finite positions of the same call are not affected):
 *   - on a 'wrap' row (interior seed rows) a NaN or infinite coordinate gives NaN: scipy's wrap of an infinite
 *     coordinate is inf - inf;
 *   - on a 'constant' row (the first / last interp_order global seed rows) an infinite coordinate is outside the field:
 *     the sample is exactly 0, as for any coordinate outside [0, n-1], whatever the other coordinate is; a NaN
 *     coordinate gives NaN unless the other coordinate is outside.
 * This departs from scipy on purpose: scipy.ndimage.map_coordinates casts such a coordinate to an integer, which is
 * undefined (scipy 1.15 on x86-64 answers 0 for a NaN or -inf coordinate on a 'wrap' row). */
int lc_sample(lc_ctx *ctx, const void *packed_lin, const void *packed_cub, int dtype,
              int nt, int ny_f, int nx_f,
              double lat_min, double lat_max, double lon_min, double lon_max, int level,
              const void *pos_x_dev, const void *pos_y_dev, int ny, int nx,
              int row0, int ny_global, int interp_order, void *out_u, void *out_v);

/* lc_sample with the raw planes as the order-1 source (see lc_advect_ex): packed_lin may then be NULL (interp_order != 1:
 * only the pole rows sample order 1; LC_F64 at interp_order 1: every row does). */
int lc_sample_raw(lc_ctx *ctx, const void *packed_lin, const void *packed_cub, const void *u_raw, const void *v_raw, int dtype,
                  int nt, int ny_f, int nx_f,
                  double lat_min, double lat_max, double lon_min, double lon_max, int level,
                  const void *pos_x_dev, const void *pos_y_dev, int ny, int nx,
                  int row0, int ny_global, int interp_order, void *out_u, void *out_v);

/* ---- scalar tracers along trajectories --------------------------------------
 * The C= argument the reference's research driver hands parcel_propagation (LCS/area_of_influence.py:314-321; the
 * dead flag tracer_account of LCS/trajectory.py:45): a tracer C [nt][ny_f][nx_f] on the wind's grid and time levels,
 * sampled at the parcel positions.  Trajectory entry j is sampled at field level level0 + j with lc_sample's rule
 * (tools.xr_map_coordinates at interp_order: Q2 index scale, 'wrap' on interior rows, order 1 + 'constant' on the first /
 * last interp_order GLOBAL seed rows, row0 / ny_global as in lc_advect).
 *   tracer_lin, tracer_cub, c1_raw, c2_raw   the (C1, C2) tracer images / planes, exactly as lc_sample_raw takes the (u, v)
 *                ones: lc_field_pack(C1, C2) with the tracers in the (u, v) slots; one tracer is packed as (C, C) with
 *                c2_out / sum2 / mean2_out NULL.  Order 1 needs tracer_lin (LC_F32) or the raw planes (LC_F64); orders
 *                2..5 need tracer_cub of that order and an order-1 source for the pole rows (tracer_lin or the planes).
 *   traj_x, traj_y   [n_levels][ny*nx] positions in degrees (dtype elements, device): lc_advect's traj_x / traj_y, or a
 *                range of entries of them.
 *   c1_out, c2_out   NULL or [n_levels][ny*nx] dtype: the sampled values.
 *   sum1, sum2   NULL or [ny*nx] float64, device: the entries' values are ADDED in level order (float64 for both dtypes),
 *                so a series sampled in consecutive ranges carries its sums from call to call.
 *   mean1_out, mean2_out   NULL or [ny*nx] dtype: (dtype)(sum / mean_count) after this range, sum including what sum1 /
 *                sum2 held on entry -- the reference driver's cs.mean('time') over entries 0..nsteps is mean_count =
 *                nsteps + 1 (equal up to summation order).
 * NaN in the tracer is not specified: the sampled value is whatever the interpolation makes of it.  A NaN or infinite
 * POSITION is specified: lc_sample's rule for positions that are not finite, entry by entry (a NaN value enters the sums). */
typedef struct lc_tracer_args {
    size_t struct_size;                                       /* sizeof(lc_tracer_args) as the caller compiled it */
    const void *tracer_lin, *tracer_cub, *c1_raw, *c2_raw;
    int dtype, nt, ny_f, nx_f;                                /* dtype: LC_F32 or LC_F64 (tracer, positions, outputs) */
    double lat_min, lat_max, lon_min, lon_max;
    int ny, nx, row0, ny_global, interp_order;
    const void *traj_x, *traj_y;
    int level0, n_levels;                                     /* entry j is sampled at field level level0 + j (< nt) */
    void *c1_out, *c2_out;
    double *sum1, *sum2;
    void *mean1_out, *mean2_out;
    int mean_count;
} lc_tracer_args;
int lc_tracer_sample(lc_ctx *ctx, const lc_tracer_args *args);

/* ---- K3: flow-map gradient + largest singular value ------------------------
 * Replaces LCS.flowmap_gradient (LCS/LCS.py:171-225), tools.derivative_spherical_coords
 * + tools.fourth_order_derivative (LCS/tools.py:248-267, 190-228) and the eigen
 * step of LCS.__call__ (LCS/LCS.py:145-157) in one fused kernel.
 *
 *   x_dep,y_dep  [n_in_rows*nx] departure points for global seed rows
 *                [in_row0, in_row0+n_in_rows)
 *   out_row0, n_out_rows   rows to produce; each needs rows r-2..r+2 inside the
 *                input window unless it is one of the 2 first / 2 last GLOBAL rows
 *                (one-sided rule, tools.py:210-217)
 *   seed_lat     [n_in_rows] latitude of the input rows (dtype elements, device)
 *   dlat, dlon   seed spacing in degrees (lat[1]-lat[0], lon[1]-lon[0]; tools.py:255-256)
 *   fd_fp32_cast 1 = round X,Y,Z to float before differencing (reference, tools.py:258)
 *   sigma_out    [n_out_rows*nx]
 */
int lc_sigma(lc_ctx *ctx, const void *x_dep, const void *y_dep, int dtype,
             int in_row0, int n_in_rows, int nx, int ny_global,
             const void *seed_lat_dev, double dlat, double dlon,
             int fd_fp32_cast, int tensor_layout,
             int out_row0, int n_out_rows, void *sigma_out);

/* lc_sigma for n_members whole grids at once (in_row0 = out_row0 = 0, n_in_rows = n_out_rows = ny_global = ny): x_dep, y_dep
 * and sigma_out are [n_members][ny*nx], seed_lat_dev [ny]; one launch covers every member, and every plane equals lc_sigma
 * on that plane bit for bit (the same kernel choice per plane, under a batch name in lc_ctx_last_sigma_kernel:
 * "sigma_march_batch_kernel_f32", "sigma_batch_kernel_f32", "sigma_batch_kernel<double, float|double>"). */
int lc_sigma_batch(lc_ctx *ctx, const void *x_dep, const void *y_dep, int dtype, int ny, int nx,
                   const void *seed_lat_dev, double dlat, double dlon, int fd_fp32_cast, int tensor_layout,
                   int n_members, void *sigma_out);

/* Both singular values of the 3x2 flow-map Jacobian F = [[dXdx, dXdy], [dYdx, dYdy], [dZdx, dZdy]] (LC_LAYOUT_PHYSICAL; NOT the
 * reference's 3x3 reshape, LCS/LCS.py:153) and its leading right singular vector, for n_members whole grids in one launch.  No
 * reference counterpart: the reference keeps the largest singular value only (LCS/LCS.py:154).  Geometry, stencil and
 * fd_fp32_cast as lc_sigma; inputs and outputs [n_members][ny*nx] dtype elements, seed_lat_dev [ny].
 *   s1_out      largest singular value; in LC_F64 equal to lc_sigma(LC_LAYOUT_PHYSICAL) bit for bit
 *   s2_out      smallest singular value, as |col1 x col2| / s1 (0 where s1 == 0): s1 * s2 is the area change of the flow map
 *   e_lon_out, e_lat_out   unit eigenvector of F^T F for s1^2 in local (east, north) components at the seed, the direction
 *               that is stretched by s1; sign: e_lon > 0, or e_lon == 0 and e_lat > 0; (1, 0) where F^T F is a multiple of
 *               the identity
 * s2_out, e_lon_out, e_lat_out may each be NULL (that plane is not written).  A NaN departure point gives NaN in every output
 * of every cell whose stencil touches it.  lc_ctx_last_strain_kernel: the kernel the context's last lc_strain launched (""
 * before any): "strain_kernel_f32", "strain_kernel<double, float>" (fd_fp32_cast) or "strain_kernel<double, double>". */
int lc_strain(lc_ctx *ctx, const void *x_dep, const void *y_dep, int dtype, int ny, int nx,
              const void *seed_lat_dev, double dlat, double dlon, int fd_fp32_cast, int n_members,
              void *s1_out, void *s2_out, void *e_lon_out, void *e_lat_out);
const char *lc_ctx_last_strain_kernel(const lc_ctx *ctx);

/* The flow-map gradient from an AUXILIARY GRID, reduced in one launch: for callers who advect four extra parcels per output
 * point, seeded at (lat[r], lon[c] +- d_lon) and (lat[r] +- d_lat, lon[c]), and hand their departure points in.  Replaces
 * LCS.flowmap_gradient (LCS/LCS.py:171-225) + tools.derivative_spherical_coords (LCS/tools.py:248-267) + the singular value
 * (LCS/LCS.py:152-154) where the caller asks for it, and differs from them on purpose:
 *   - the six derivatives are centred differences of the four auxiliary parcels of the SAME output point, not a 5-point index
 *     stencil over neighbouring output points: no cyclic longitude wrap, no one-sided / 2 rows, ny and nx may be 1;
 *   - the chords P_e - P_w and P_n - P_s on the reference's sphere (LCS/LCS.py:195-199) are formed from half-sums and
 *     half-differences of the angles (no cancellation), in the dtype; X, Y, Z are never rounded to float32 (Q11);
 *   - dXdx = dX_ew / (k sep_lon[c] R cos(k seed_lat[r])), dXdy = dX_ns / (k sep_lat[r] R), k = pi / 180, likewise Y and Z;
 *   - a NaN in any of a cell's eight inputs, or in its sep_lat / sep_lon, gives NaN in every output of that cell and in no
 *     other cell (the caller marks invalid rows / columns with a NaN separation).
 *   x_e .. y_s     departure points of the east, west, north and south parcels, [n_members][ny*nx] dtype elements
 *   seed_lat_dev   [ny] latitudes of the output rows (the centre grid)
 *   sep_lat_dev    [ny] lat_n[r] - lat_s[r], sep_lon_dev [nx] lon_e[c] - lon_w[c], in degrees, from the coordinates as rounded
 *   tensor_layout  for sigma_out only: LC_LAYOUT_REFERENCE is lc_sigma's value of these derivatives, LC_LAYOUT_PHYSICAL equals s1
 *   sigma_out, s1_out, s2_out, e_lon_out, e_lat_out   [n_members][ny*nx]; s1, s2 and the direction as lc_strain defines them
 *                  (same sign and isotropy rules); each may be NULL (not written), at least one is not
 * dtype LC_F32 or LC_F64.  Refused with LC_EINVAL before any HIP call: a null context or argument structure, a wrong
 * struct_size, a bad dtype or tensor_layout, ny or nx < 1, a plane of 2^31 cells or more, n_members outside 1..65535, a null
 * input, no output.  lc_ctx_last_aux_kernel: what the context's last lc_aux_gradient launched ("" before any, or for a null
 * context): "aux_gradient_kernel_f32" or "aux_gradient_kernel<double>". */
typedef struct lc_aux_gradient_args {
    size_t struct_size; /* sizeof(lc_aux_gradient_args): checked before any other field */
    const void *x_e, *y_e, *x_w, *y_w, *x_n, *y_n, *x_s, *y_s;
    int dtype, ny, nx, n_members;
    const void *seed_lat_dev, *sep_lat_dev, *sep_lon_dev;
    int tensor_layout;
    void *sigma_out, *s1_out, *s2_out, *e_lon_out, *e_lat_out;
} lc_aux_gradient_args;
int lc_aux_gradient(lc_ctx *ctx, const lc_aux_gradient_args *args);
const char *lc_ctx_last_aux_kernel(const lc_ctx *ctx);

/* ---- finite-size Lyapunov exponents (LCS.fsle, Engine.fsle) ----
 * No counterpart in the reference.  A record of trajectory planes (lc_advect_ex's traj_x / traj_y) is reduced, block of levels by
 * block of levels, to the time tau that the neighbour pairs of every cell take to separate to a threshold, and to the exponent.
 * Positions are degrees, k = pi / 180, the grid has ny x nx seeds.
 *   pairs       every horizontally or vertically adjacent couple of seeds; with cyclic_x column nx-1 pairs with column 0.  A cell
 *               owns up to four pairs, in the order E, W, N, S; the E pair of (r, c) is the W pair of (r, c+1): same parcels,
 *               same numbers
 *   separation  of pair p at level j, the great-circle distance on a sphere of `radius` in half-angle form:
 *               h = sin^2(k dphi / 2) + cos(k phi1) cos(k phi2) sin^2(k dlambda / 2),  d = 2 radius asin(min(1, sqrt h));
 *               dlambda is the raw difference (the form is periodic: the seam needs no wrap).  d_p(0) is formed from seed_lat /
 *               seed_lon, which is trajectory entry 0 (entry 0 of the block with level0 == 0 is not read)
 *   threshold   q of pair p: mode LC_FSLE_RATIO T = thresholds[q] d_p(0); LC_FSLE_DISTANCE T = thresholds[q] metres.  A pair
 *               is eligible for q when d_p(0) is finite, > 0 and < T
 *   crossing    an eligible pair upcrosses at the first level j >= 1 where both separations are finite and d_p(j-1) < T <=
 *               d_p(j); its time is t_p = (j-1 + (T - d_p(j-1)) / (d_p(j) - d_p(j-1))) |timestep|.  A level where either
 *               separation is not finite contributes nothing
 *   cell        tau[q][r][c] = the minimum of t_p over the cell's pairs, ties to the first pair in E, W, N, S order;
 *               fsle[q][r][c] = ln(T / d_p*(0)) / tau for the pair p* that gave it (ratio mode: ln(thresholds[q]) / tau); both
 *               NaN where no pair of the cell ever upcrosses.  tau is a positive duration whatever the sign of timestep: as
 *               with FTLE, a backward record gives the attracting field
 *   streaming   tau and fsle are the only state carried from one block of levels to the next: the test needs levels j-1 and j
 *               only, entry 0 of a continued block is the last entry of the block before, and a cell whose tau[q] is finite is
 *               final for q.  Any split of the levels into blocks gives, bit for bit, what one block gives.  (A block walks its
 *               levels in order and closes a cell at the first level where a pair of it upcrosses.  Where rounding makes a
 *               later level's time equal to an earlier level's, the earlier level's pair keeps the cell.)
 *   traj_x, traj_y   [n_levels][ny*nx] dtype elements: positions after level0, level0 + 1, ... steps
 *   level0      steps already consumed by earlier blocks; 0: the call writes NaN into tau and fsle itself before it starts
 *   tau, fsle   [n_thr][ny*nx], in and out
 *   thresholds  n_thr of them, passed by value and rounded to the dtype; the checks below apply to the rounded values
 * dtype LC_F32 or LC_F64.  Refused with LC_EINVAL before any HIP call: a null context or argument structure, a wrong
 * struct_size, a bad dtype or mode, ny or nx < 1 or ny * nx == 1, n_levels < 2, level0 < 0, n_thr outside 1..8, a threshold
 * that is not finite or is <= 1 in ratio mode or <= 0 in distance mode, a radius or |timestep| that is not positive and finite,
 * a plane of 2^31 cells or more (or a grid that needs more workgroups than one launch takes), a null pointer.
 * lc_ctx_last_fsle_kernel: what the context's last lc_fsle_update launched ("" before any, or for a null context):
 * "fsle_update_kernel<float, 8>" or "fsle_update_kernel<double, 8>". */
enum lc_fsle_mode { LC_FSLE_RATIO = 0, LC_FSLE_DISTANCE = 1 };
typedef struct lc_fsle_args {
    size_t struct_size; /* sizeof(lc_fsle_args): checked before any other field */
    const void *traj_x, *traj_y;
    int dtype, ny, nx, n_levels, level0;
    const void *seed_lat_dev, *seed_lon_dev;
    int mode, n_thr; /* enum lc_fsle_mode */
    double thresholds[8];
    double radius, timestep;
    int cyclic_x; /* non-zero: column nx-1 pairs with column 0 */
    void *tau, *fsle;
} lc_fsle_args;
int lc_fsle_update(lc_ctx *ctx, const lc_fsle_args *args);
const char *lc_ctx_last_fsle_kernel(const lc_ctx *ctx);

/* ---- relative vorticity of a wind record (Engine.vorticity, tools.relative_vorticity, LCS.lavd) ----
 * No counterpart in the reference.  u, v: [nt][ny_f][nx_f] dtype elements on a uniform ascending grid, as the samplers assume;
 * k = pi / 180 (the float64 pi), row r lies at lat_r = lat_min + r dlat degrees, dlat = (lat_max - lat_min) / (ny_f - 1), both in
 * float64; dphi = k dlat and dlambda = k (lon_max - lon_min) / (nx_f - 1), formed in float64 and rounded to the dtype T together
 * with the factor 2 of the stencils; cos phi_r = cos(k lat_r) in float64, rounded to T where it multiplies a T.
 *   omega       = (dv/dlambda - d(u cos phi)/dphi) / (radius cos phi), every operation in T; the product u cos phi is formed in
 *               T before it is differenced
 *   latitude    interior rows: (f[r+1] - f[r-1]) / 2dphi.  First row: ((-3 f[0] + 4 f[1]) - f[2]) / 2dphi; last row its mirror
 *               ((3 f[n-1] - 4 f[n-2]) + f[n-3]) / 2dphi: second order (first-order edges are wrong by 23 % for solid-body
 *               rotation on a 5 degree grid at +-80 degrees, these by 1.3 %)
 *   longitude   centred; with cyclic_x centred across the seam (column -1 is column nx_f - 1, at spacing dlambda: the samplers'
 *               wrap mode makes the same assumption); without it the one-sided forms above on the first and last column
 *   pole rows   a first or last row with 90 - |lat_r| <= 1e-6 degrees (cos(pi/2) is 6e-17 in float64, not 0: dividing by it
 *               gives garbage, not NaN).  There omega is, at every column, the mean -- summed in float64, rounded to T -- over
 *               the finite nodes of the adjacent row's omega, NaN where that row has none: the limit a smooth flow has there.
 *               A pole row's weight in the domain mean is exactly 0
 *   NaN         a u or v that is not finite anywhere in a node's stencil gives NaN at that node, and only there
 *   level_mean  [nt] float64, written in every mode: sum w omega / sum w over the finite nodes of level t off the pole rows,
 *               w = cos phi_r, sums and products in float64 whatever T is; NaN when no node is finite
 *   deviation   LC_VORT_DEVIATION_DOMAIN: omega = (T)((double)omega - level_mean[t]) at every node, pole rows included;
 *               LC_VORT_DEVIATION_NONE: omega stays (regional domains, where the box's mean means little);
 *               LC_VORT_DEVIATION_GIVEN: the same with given_dev[t] (nt float64, device) in place of level_mean[t]
 *   work_dev    lc_vorticity_work_elems(nt, ny_f, nx_f) float64 elements of device scratch (0: sizes the call refuses): one
 *               partial (sum w omega, sum w) per workgroup, each formed in a fixed tree; a second launch adds a level's partials
 *               in index order.  No floating-point atomics: two runs give the same bits
 * Refused with LC_EINVAL before any HIP call: a null context or argument structure, a wrong struct_size, a bad dtype or mode,
 * nt < 1, ny_f < 4 or nx_f < 4 (the samplers' own minimum), a plane of 2^31 nodes or more or a record that needs more workgroups
 * than one launch takes, latitudes or longitudes that are not finite and ascending or lie outside -90 .. 90, a radius that is
 * not positive and finite, a null pointer (given_dev only in its mode).
 * lc_ctx_last_vorticity_kernel: what the context's last lc_vorticity launched ("" before any, or for a null context):
 * "vorticity_kernel<T>+vorticity_finish_kernel<T>" and, but for LC_VORT_DEVIATION_NONE, "+vorticity_subtract_kernel<T>",
 * T float or double. */
enum lc_vort_deviation { LC_VORT_DEVIATION_DOMAIN = 0, LC_VORT_DEVIATION_NONE = 1, LC_VORT_DEVIATION_GIVEN = 2 };
typedef struct lc_vorticity_args {
    size_t struct_size; /* sizeof(lc_vorticity_args): checked before any other field */
    const void *u, *v;
    int dtype, nt, ny_f, nx_f;
    double lat_min, lat_max, lon_min, lon_max;
    int cyclic_x, deviation; /* enum lc_vort_deviation */
    double radius;
    const double *given_dev;
    void *omega;
    double *level_mean;
    void *work_dev;
} lc_vorticity_args;
size_t lc_vorticity_work_elems(int nt, int ny_f, int nx_f);
int lc_vorticity(lc_ctx *ctx, const lc_vorticity_args *args);
const char *lc_ctx_last_vorticity_kernel(const lc_ctx *ctx);

/* ---- vorticity deviation, rotation and path length along trajectories (Engine.lavd_update, Engine.lavd, LCS.lavd) ----
 * No counterpart in the reference.  LAVD(x0) = integral of |omega(x(t), t) - mean(t)| dt along the trajectory from x0 (Haller,
 * Hadjighasem, Farazmand and Huhn 2016); the signed integral is the rotation; the great-circle length of the trajectory is the
 * arc-length Lagrangian descriptor M of Mancho et al.  One block of trajectory levels is folded into the three running
 * integrals of every parcel; nothing is shared between parcels.
 *   traj_x, traj_y   [n_levels][n] dtype elements, degrees: positions after level0, level0 + 1, ... steps
 *   c           [n_levels][n] dtype elements or NULL: omega - mean sampled at the same entries (lc_tracer_sample's c1_out)
 *   per interval j = 1 .. n_levels - 1, in level order, in float64 without contraction (T widened first):
 *               acc[0] += (0.5 (|c[j-1]| + |c[j]|)) |timestep|
 *               acc[1] += (0.5 ( c[j-1]  +  c[j] )) |timestep|
 *               acc[2] += d(j-1, j), the great-circle distance of lc_fsle_update's separation formed in T:
 *               h = sin^2(k dphi / 2) + cos(k phi1) cos(k phi2) sin^2(k dlambda / 2),  d = 2 radius asin(min(1, sqrt h)),
 *               dlambda the raw difference (periodic: a step across the seam is the short way round)
 *   acc         [3][n] float64, the carried state: read unless level0 == 0 (then the sums start at 0), always written.  Entry 0
 *               of a continued block is the last entry of the block before; each sum is float64 added in level order, so any
 *               split of a record into blocks gives, bit for bit, what one block gives
 *   lavd, rotation, length   [n] dtype elements, each NULL or written as (T)acc[0], (T)acc[1], (T)acc[2] (metres)
 *   NaN         a NaN position makes that parcel's length, a NaN value that parcel's lavd and rotation, NaN from that level on,
 *               and no other parcel's; a NaN in c does not touch length
 *   c == NULL   only length is produced: acc[0] and acc[1] are carried unchanged (0 from level0 == 0), lavd and rotation must
 *               be NULL
 * Refused with LC_EINVAL before any HIP call: a null context or argument structure, a wrong struct_size, a bad dtype, n < 1,
 * n_levels < 2, level0 < 0, a radius or |timestep| that is not positive and finite, a null traj_x, traj_y or acc, lavd or
 * rotation without c.
 * lc_ctx_last_lavd_kernel: "lavd_update_kernel<float | double, true | false>" (false: c == NULL); "" before any call. */
typedef struct lc_lavd_args {
    size_t struct_size; /* sizeof(lc_lavd_args): checked before any other field */
    const void *traj_x, *traj_y, *c;
    int dtype, n, n_levels, level0;
    double timestep, radius;
    double *acc;
    void *lavd, *rotation, *length;
} lc_lavd_args;
int lc_lavd_update(lc_ctx *ctx, const lc_lavd_args *args);
const char *lc_ctx_last_lavd_kernel(const lc_ctx *ctx);

/* ---- footprints: trajectory entries binned into residence-time maps (Engine.footprint_update, Engine.footprint,
 * LCS.footprint, tools.trajectory_density) ----
 * No counterpart in the reference.  Where the other folds write one value per parcel back on the seed grid, this one scatters
 * every (parcel, level) entry of a block of trajectory levels into the cell of a target grid it lies in.  Every output is a sum
 * of 64-bit integers, so the result does not depend on launch shape, kernel form, the split into blocks or the run.
 *   traj_x, traj_y   [n_levels][n] dtype elements, degrees, n = ny nx: the layout lc_lavd_update takes
 *   c           the same shape or NULL: the value sampled at the same entries (lc_tracer_sample's c1_out)
 *   q           int32 [n] or NULL (all 1): the parcel's integer weight, 0 <= q <= 2^20 (the caller's guarantee, with
 *               n levels 2^21 < 2^63 over a record).  A parcel with q == 0 contributes nothing anywhere, stats included: the
 *               receptor mask
 *   ny, nx      the seed grid's shape (a workgroup owns a patch of neighbouring seeds); ny = 1 for an unstructured list
 *   entries     entry 0 of a continued block (level0 > 0) is the last entry of the block before and is skipped.  An entry's
 *               half-weight h is 1 for the record's first entry (entry 0 of a block with level0 == 0) and for its last (the
 *               last entry of a block with final), 2 otherwise: hits |timestep| / 2 is the trapezoid rule in time, in integers
 *   cell        in float64 without contraction, the position widened first whatever the dtype:
 *               fy = ((double)y - lat0) inv_dy + 0.5 with inv_dy = (ny_t - 1) / (lat1 - lat0) formed once on the host in
 *               double, fx likewise; lat0, lat1, lon0, lon1 are the centres of the first and last target cell.  The row is
 *               floor(fy), valid when 0 <= fy < ny_t; the column floor(fx), valid when 0 <= fx < nx_t, or with cyclic_x
 *               floor(fx) reduced by floored modulo nx_t, valid when |fx| < 2^31.  Every comparison is made on the doubles
 *               before any conversion: NaN, +-inf and 1e30 are simply not valid.  A position exactly on a cell edge goes to
 *               the upper cell
 *   sums        for a valid entry of a parcel with q > 0: hits[cell] += h, mass[cell] += h q and, with c, v = rint((double)c
 *               c_scale) (ties to even): csum[cell] += h v and chits[cell] += h when v is finite and |v| <= 2^31, else
 *               stats[1] += h.  For an invalid entry stats[0] += h.  stats[2] and stats[3] are written as 0 with zero_first
 *               and otherwise left alone (but see the census form below).  Over a whole record
 *               sum(hits) + stats[0] == 2 (levels - 1) #{q > 0}
 *   zero_first  hits, mass, csum, chits (those given) and stats are cleared on the context's stream before the launch
 *   outputs     hits, mass, csum, chits: each int64 [ny_t nx_t] or NULL, at least one non-NULL; csum and chits both or neither,
 *               and only with c.  stats: int64 [4], required
 * Refused with LC_EINVAL before any HIP call: a null context or argument structure, a wrong struct_size, a bad dtype, n < 1,
 * ny nx != n, n_levels < 2, level0 < 0, a target grid with fewer than 2 cells a side or with ends that are not finite and
 * ascending, c without a positive finite c_scale, csum or chits without c or only one of the two, no output at all, a null
 * traj_x, traj_y or stats.
 * Two kernel forms give the same integers.  "footprint_direct_kernel<T, HAS_C>": one thread per parcel, one 64-bit global
 * atomic per sum and entry.  "footprint_tile_kernel<T, HAS_C>": a workgroup owns a patch of 8 x 64 neighbouring seeds, sums
 * into a window of 32 x 64 target cells held in LDS -- anchored anew every 4 levels at the cell of the counted parcel nearest
 * the patch's centre -- and flushes the window's non-zero cells with one global atomic each; an entry outside the window goes
 * straight to global atomics, so the window never decides a result.  lc_ctx_set_footprint_form: -1 auto (the default: the rule
 * is in footprint.hip, from the measurements in DESIGN.md), 0 direct, 1 tiled, 2 tiled with a census -- stats[2] += h for every
 * valid entry that left the window, a measuring aid outside the contract above; any other mode is refused.
 * lc_ctx_last_footprint_kernel: the kernel the context's last lc_footprint_update launched, T float or double, HAS_C true or
 * false; "" before any call or for a null context. */
typedef struct lc_footprint_args {
    size_t struct_size; /* sizeof(lc_footprint_args): checked before any other field */
    const void *traj_x, *traj_y, *c;
    const int32_t *q;
    int dtype, ny, nx, n, n_levels, level0, final;
    int ny_t, nx_t;
    double lat0, lat1, lon0, lon1;
    int cyclic_x;
    double c_scale;
    int zero_first;
    int64_t *hits, *mass, *csum, *chits;
    int64_t *stats;
} lc_footprint_args;
int lc_footprint_update(lc_ctx *ctx, const lc_footprint_args *args);
const char *lc_ctx_last_footprint_kernel(const lc_ctx *ctx);
int lc_ctx_set_footprint_form(lc_ctx *ctx, int mode);

/* The 9-component "def_tensor" itself, for callers of LCS.flowmap_gradient
 * (LCS/LCS.py:171-225): planes dXdx,dXdy,dYdx,dYdy,dZdx,dZdy,dXdr,dYdr,dZdr (the last
 * three all zero, LCS.py:206-208), each [ny*nx], whole grid on one device. */
int lc_flowmap_gradient(lc_ctx *ctx, const void *x_dep, const void *y_dep, int dtype,
                        int ny, int nx, const void *seed_lat_dev, double dlat, double dlon,
                        int fd_fp32_cast, void *def_tensor_out);

/* tools.fourth_order_derivative (LCS/tools.py:190-245): 5-point index-space difference of a [ny*nx] array along
 * dim 0 (latitude; one-sided/2 on the 2 first/last rows, :210-217) or dim 1 (longitude: cyclic when isglobal != 0,
 * :220-228, else one-sided/2 on the 2 first/last columns, :229-244; the reference ignores isglobal for dim 0 and so
 * does this); result in the input dtype. */
int lc_fourth_order_derivative(lc_ctx *ctx, const void *in_dev, int dtype, int ny, int nx,
                               int dim, int isglobal, void *out_dev);

/* ---- optional smoothing of the departure fields ----------------------------
 * Replaces scipy.ndimage.gaussian_filter(x, sigma) at LCS/LCS.py:187-190
 * (truncate=4.0, mode='reflect', separable).  In place is not allowed. */
int lc_gaussian_filter(lc_ctx *ctx, const void *in_dev, int dtype, int ny, int nx,
                       double sigma, void *tmp_dev, void *out_dev);

/* ---- ridge classification (consumer of the sigma / FTLE field) ---------------------
 * Replaces the per-point Python loop of tools.find_ridges_spherical_hessian
 * (LCS/tools.py:99-138): numpy.linalg.eig of the symmetric 2x2 Hessian
 * [[hxx,hxy],[hxy,hyy]] (inf/NaN entries zeroed), the reference's row-indexed
 * eigenvector dotted with the gradient, the eigenvalue of largest magnitude, and the
 * mask (|dot| <= tolerance and that eigenvalue negative).  All arrays [n] doubles on the
 * device; dt_out (the raw dot product, tools.py:115) and eigvec_out ([2][n]: the two
 * components of that row-indexed eigenvector, tools.py:107, unmasked -- the
 * return_eigvectors=True outputs of tools.py:123-150 are built from it) may be NULL. */
int lc_ridge_classify(lc_ctx *ctx, const void *hxx, const void *hxy, const void *hyy,
                      const void *gx, const void *gy, size_t n, double tolerance,
                      void *mask_out, void *eigmin_out, void *dt_out, void *eigvec_out);

/* ---- ridges of a stack of planes (find_ridges_spherical_hessian on a series) -----------
 * tools.find_ridges_spherical_hessian (LCS/tools.py:52-155) from the smoothing on, for n_members independent planes
 * [n_members][ny*nx] of float64 (latitude and longitude ascending, tools.py:70-71) in two kernels instead of about thirty
 * launches per plane.  Both entry points and the getter were added at LC_VERSION 104 without a bump: nothing that existed
 * changed.  A plane never reads another plane; plane m of every output equals what lc_gaussian_filter,
 * lc_fourth_order_derivative and lc_ridge_classify give for plane m alone, bit for bit.
 *   tools.py:74-75    sigma > 0: scipy.ndimage.gaussian_filter per plane (truncate 4, reflect; never across planes: the
 *                     reference's call on a 3-D array would smooth across time and then fail at its reshape, :87-90).
 *                     sigma <= 0 or NaN: no smoothing, work_dev is not read.  A radius int(4 sigma + 0.5) above 256 is
 *                     refused with LC_EUNSUPPORTED, as lc_gaussian_filter refuses it.
 *   tools.py:77-78    ddadx, ddady = derivative_spherical_coords(da, 1 / 0): the float32 cast (:258), the 5-point index stencil
 *                     (:202-244: one-sided / 2 on the two first and last rows; in longitude cyclic when isglobal != 0, else
 *                     one-sided / 2 on the two first and last columns), widened to float64 and divided by dx_dev[row]
 *                     (:255, :264) or multiplied by 1 / dy rounded once (:256, :262: what the per-plane route's division by
 *                     the scalar dy does on the device).  grad_out [n_members][2][ny*nx]: these two, float64.
 *   tools.py:79-81    d2dadx2, d2dady2, d2dadxdy the same way from the float32 casts of ddadx, ddady.
 *   tools.py:87-93    the Hessian per point, inf / NaN entries zeroed.
 *   tools.py:99-118   numpy.linalg.eig of it, the row-indexed eigenvector (:107), its product with the gradient (:115) and
 *                     the eigenvalue of largest magnitude (:118), as lc_ridge_classify: dt_out [n_members][ny*nx] the raw
 *                     product, eigmin_out that eigenvalue, eigvec_out [n_members][2][ny*nx] the vector, unmasked.
 *   tools.py:123-133  the angle and the eigmin < 0 masking of the vector are left to the caller (two element-wise expressions).
 *   tools.py:136-138  mask_out: 1 where |product| <= tolerance (or the product is NaN) and that eigenvalue is negative, else 0.
 * Every output may be NULL.  work_dev: float64 [lc_ridges_work_elems(ny, nx, n_members)] scratch (0 elements for bad sizes).
 * A null context, a wrong struct_size, ny < 5 or nx < 5 (lc_fourth_order_derivative's limit), a plane of 2^31 points or
 * more, a radius above 256, and any overlap between f / dx_dev, work_dev and the outputs are refused before any HIP call.
 * lc_ctx_last_ridges_kernel: what the context's last lc_ridges_batch launched, "gauss_planes_kernel+hessian_ridge_kernel"
 * or "hessian_ridge_kernel" ("" before the first).  No kernel of this call waits for another workgroup. */
size_t lc_ridges_work_elems(int ny, int nx, int n_members);
typedef struct lc_ridges_args {
    size_t struct_size; /* sizeof(lc_ridges_args): checked before any other field */
    const void *f;      /* float64 [n_members][ny*nx] */
    int ny, nx, n_members;
    const void *dx_dev; /* float64 [ny]: metres per longitude step of every row (tools.py:255) */
    double dy;          /* metres per latitude step (tools.py:256) */
    double sigma;       /* <= 0 or NaN: no smoothing */
    double tolerance;
    int isglobal;
    void *work_dev;
    void *mask_out, *eigmin_out, *dt_out; /* float64 [n_members][ny*nx], or NULL */
    void *eigvec_out, *grad_out;          /* float64 [n_members][2][ny*nx], or NULL */
} lc_ridges_args;
int lc_ridges_batch(lc_ctx *ctx, const lc_ridges_args *args);
const char *lc_ctx_last_ridges_kernel(const lc_ctx *ctx);

/* ---- connected components of a ridge mask (filter_ridges) ----------------------------
 * What the driver does with the raw mask before it uses it (LCS/area_of_influence.py:210-242): label its connected
 * components, measure each, keep those that pass a threshold.  The function the driver imports for it comes from a package
 * outside the reference, so the meaning is fixed here; scipy.ndimage.label and numpy are what it is tested against.
 * n_members independent planes [n_members][ny*nx] per call, every stage one launch for all of them.
 *
 * Foreground: a pixel whose value is != 0 and not NaN (negative values are foreground).  mask: `dtype` elements, LC_F32 or
 * LC_F64.  A plane of 2^31 pixels or more is refused.
 *
 * lc_label_components
 *   connectivity  1: pixels that share an edge; 2: an edge or a corner (scipy's generate_binary_structure(2, connectivity))
 *   cyclic_x      != 0: column nx-1 is the western neighbour of column 0 (rows r-1 .. r+1 at connectivity 2)
 *   labels_out    int32 [n_members][ny*nx]: 0 on background, else 1 .. N, the components of each plane numbered in the order of
 *                 their first pixel in raster order -- the numbering of scipy.ndimage.label
 *   counts_out    int32 [n_members]: N of each plane
 *   work_dev      int32 [lc_label_work_elems(ny, nx, n_members)] scratch (0 elements for bad sizes)
 * No kernel of these calls waits for another workgroup. */
size_t lc_label_work_elems(int ny, int nx, int n_members);
int lc_label_components(lc_ctx *ctx, const void *mask, int dtype, int ny, int nx, int n_members,
                        int connectivity, int cyclic_x, void *labels_out, void *counts_out, void *work_dev);

/* Sums over the pixels of every component, per compact label: entry [m][l-1] belongs to label l of plane m; labels above
 * min(counts[m], n_max) are not measured, entries without a component hold area 0, root -1 and NaN extrema.
 *   root_out     int32: the component's first pixel in raster order, as a linear index into its plane
 *   area_out     int64: pixels
 *   moments_out  int64 [5][n_members][n_max]: sums of dr, dc, dr^2, dr*dc, dc^2 with dr = row - row of the root, dc = column -
 *                column of the root; with cyclic_x dc is first wrapped into [-(nx/2), nx - nx/2).  Exact.
 *   sum_out      float64: sum of the intensity (order of summation not fixed: last bits may differ from run to run)
 *   max_out, min_out  float64: extrema of the intensity, exact; NaN if the component holds a NaN (its sum is NaN too)
 * intensity: `dtype` elements [n_members][ny*nx], or NULL: sum_out, max_out and min_out are then not written and may be NULL. */
typedef struct lc_component_sums_args {
    size_t struct_size; /* sizeof(lc_component_sums_args): checked first */
    const void *labels; /* int32 [n_members][ny*nx], as lc_label_components wrote them */
    const void *counts; /* int32 [n_members] */
    const void *intensity;
    int dtype, ny, nx, n_members;
    int cyclic_x;
    int n_max; /* capacity per plane of every output */
    void *root_out, *area_out, *moments_out, *sum_out, *max_out, *min_out;
} lc_component_sums_args;
int lc_component_sums(lc_ctx *ctx, const lc_component_sums_args *args);

/* The same per label ON THE SPHERE: area-weighted moment sums and the properties that follow from them, so that a filter or a
 * table measures a ridge in square metres and metres, not in pixels whose size shrinks with cos(latitude).  Added at
 * LC_VERSION 104 without a bump: nothing that existed changed.
 *   labels       int32 [n_members][ny*nx]; any label map with values in 0 .. counts[m] (it need not be connected: the owner map
 *                of a distance transform and track ids are valid); 0, negative values and labels above min(counts[m], n_max) are
 *                not measured
 *   tables       float64 on the device: cos_lat, sin_lat, row_weight [ny]; cos_lon, sin_lon, col_weight [nx].  Node (r, c) is the
 *                unit vector n = (fl(cos_lat[r] cos_lon[c]), fl(cos_lat[r] sin_lon[c]), sin_lat[r]) as in lc_sphere_distance, its
 *                cell has the area w = fl(row_weight[r] col_weight[c]) in steradians; no kernel evaluates a trigonometric
 *                function of a coordinate.
 *   root_out     int32: the label's first pixel in raster order (-1: no pixel of that label in the plane), as lc_component_sums
 *   sums_out     float64 [11][n_members][n_max]: with d = fl(n - n(root)) per axis, the sums over the label's pixels of
 *                w | w dx, w dy, w dz | w dx dx, w dx dy, w dx dz, w dy dy, w dy dz, w dz dz | w v -- every term formed as
 *                fl(fl(w d_i) d_j), every operation rounded once to float64 and nothing fused, so a host restatement forms the
 *                same terms bit for bit.  The ORDER of the sum is not fixed (float64 atomic adds): last bits may differ from
 *                run to run.  The eleventh plane (w v) is 0 without an intensity.  Offsets about the root: nothing large is
 *                subtracted from anything large.
 *   max_out, min_out  float64: extrema of the intensity, exact; NaN if the label holds a NaN (its w v sum is NaN too); NULL
 *                allowed without an intensity
 *   props_out    float64 [8][n_members][n_max], or NULL.  With W, M1, M2, S the sums above, m = M1 / W, C = M2 / W - m m^T and
 *                e1 >= e2 >= e3 the eigenvalues of C (cyclic Jacobi, a fixed number of sweeps), v the eigenvector of e1:
 *                  0 area               radius^2 W
 *                  1 major_axis_length  4 radius sqrt(max(e1, 0))   the regionprops formula on chords: it saturates for
 *                  2 minor_axis_length  4 radius sqrt(max(e2, 0))   labels that are not small against the sphere
 *                  3 centroid_latitude  degrees, of the direction c = n(root) + m: asin(c_z / |c|), evaluated as
 *                                       atan2(c_z, hypot(c_x, c_y)) so that it keeps its accuracy at the poles
 *                  4 centroid_longitude degrees(atan2(c_y, c_x)); both NaN when |c| < 1e-6
 *                  5 orientation        degrees(atan2(v . north, v . east)) at the centroid, folded into (-90, 90]: 0 zonal, 90
 *                                       meridional, positive from SW to NE; NaN unless e1 > 0 (one pixel) and where the
 *                                       centroid is NaN
 *                  6 mean_intensity     S / W (area-weighted)        7 total_intensity  radius^2 S      (NaN without an intensity)
 *                Entries past a plane's count and labels without a pixel in the plane: area 0, everything else NaN.
 * A null context or argument structure, a wrong struct_size, ny, nx, n_members or n_max below 1, a dtype other than LC_F32 /
 * LC_F64 (of the intensity; not read without one, but still checked) and a radius that is not positive and finite are refused
 * with LC_EINVAL before any HIP call.  No kernel of this call waits for another workgroup. */
typedef struct lc_component_sphere_sums_args {
    size_t struct_size; /* sizeof(lc_component_sphere_sums_args): checked before any other field */
    const void *labels; /* int32 [n_members][ny*nx] */
    const void *counts; /* int32 [n_members] */
    const void *intensity; /* `dtype` elements [n_members][ny*nx], or NULL */
    int dtype, ny, nx, n_members;
    int n_max; /* capacity per plane of every output */
    const double *cos_lat, *sin_lat, *row_weight; /* device, [ny] */
    const double *cos_lon, *sin_lon, *col_weight; /* device, [nx] */
    double radius;                                /* > 0, finite */
    void *root_out, *sums_out, *max_out, *min_out, *props_out;
} lc_component_sphere_sums_args;
int lc_component_sphere_sums(lc_ctx *ctx, const lc_component_sphere_sums_args *args);

/* mask_out[p] = mask[p] where keep[m][label[p]-1] != 0, else fill (on background pixels and on labels above n_max too).
 * keep: uint8 [n_members][n_max]; mask, mask_out: `dtype` elements, two distinct buffers. */
int lc_component_apply(lc_ctx *ctx, const void *labels, const void *mask, int dtype, int ny, int nx, int n_members,
                       const void *keep, int n_max, double fill, void *mask_out);

/* ---- ridges followed through time (track_ridges, persistent_ridges) -------------------
 * The filter above (LCS/area_of_influence.py:210-211) extended through time: its components end at the plane, so it cannot
 * measure how long a ridge lasts.  Added at LC_VERSION 104 without a bump: nothing that existed changed.
 *
 * A record is n_times planes [n_times][ny*nx] in the order given; consecutive means adjacent index, nothing is sorted along
 * time.  Foreground: as above, a voxel whose value is != 0 and not NaN.  Two foreground voxels are LINKED when
 *   - they lie in the same plane and are neighbours under `connectivity` (1: edges; 2: edges and corners), with cyclic_x across
 *     the longitude seam too: exactly what lc_label_components joins; or
 *   - they lie in adjacent planes and are at most `reach` pixels apart in both row and column (Chebyshev distance), with
 *     cyclic_x the column offset taken the shorter way round.  reach 0: the same pixel.  reach 1 with connectivity 2 is
 *     scipy's generate_binary_structure(3, 3); reach 0 with connectivity 1 is generate_binary_structure(3, 1).
 * A TRACK is a connected component of that relation.  Ridges that merge or split therefore belong to ONE track: a track is
 * not cut where two ridges meet, and everything that ever touched it through time carries its label.
 * Tracks are numbered 1 .. N in the order of their first voxel in raster order (time, latitude, longitude) -- the numbering
 * of scipy.ndimage.label on the 3-D array; background is 0.  A track's first / last are the smallest / largest plane index it
 * occupies, its duration last - first + 1, its volume its voxel count.
 * reach is an integer in 0 .. LC_TRACK_MAX_REACH: a stated condition, not a tuned value -- every foreground voxel reads a
 * window of (2 reach + 1)^2 voxels of the plane before it, and ridge masks are sparse.  A record of 2^31 voxels or more is
 * refused ("record too large").
 *
 * lc_label_tracks
 *   labels_out    int32 [n_times][ny*nx]
 *   count_out     int32 [1]: N
 *   work_dev      int32 [lc_track_work_elems(ny, nx, n_times)] scratch (0 elements for a bad or oversized geometry)
 * lc_track_spans: entry [l-1] belongs to track l; labels above min(count, n_max) are not measured; entries past the count hold
 * first = last = -1 and volume = 0.  All integer: the result does not depend on the order the voxels arrive in.
 * To apply a keep table, call lc_component_apply on the record viewed as ONE plane of n_times*ny rows.
 * No kernel of these calls waits for another workgroup: each stage hands over at the end of its launch. */
#define LC_TRACK_MAX_REACH 16
size_t lc_track_work_elems(int ny, int nx, int n_times);
int lc_label_tracks(lc_ctx *ctx, const void *mask, int dtype, int ny, int nx, int n_times, int connectivity, int cyclic_x,
                    int reach, void *labels_out, void *count_out, void *work_dev);
typedef struct lc_track_spans_args {
    size_t struct_size; /* sizeof(lc_track_spans_args): checked first */
    const void *labels; /* int32 [n_times][ny*nx], as lc_label_tracks wrote them */
    const void *count;  /* int32 [1] */
    int ny, nx, n_times;
    int n_max; /* capacity of every output */
    void *first_out, *last_out; /* int32 [n_max] */
    void *volume_out;           /* int64 [n_max] */
} lc_track_spans_args;
int lc_track_spans(lc_ctx *ctx, const lc_track_spans_args *args);

/* ---- distance to the nearest ridge pixel (exact Euclidean distance transform) ----------
 * The driver's next step after the filter (LCS/area_of_influence.py:231): scipy.ndimage.distance_transform_edt(~ridges_bool),
 * of which it keeps `dist < 12` as the swath a ridge influences.  n_members independent planes [n_members][ny*nx] per call.
 *
 * Foreground: as above, a pixel whose value is != 0 and not NaN; mask: `dtype` elements, LC_F32 or LC_F64.
 *   dist_out     float64 [n_members][ny*nx]: 0 on foreground, elsewhere sqrt of the smallest
 *                cost = (dr * sampling_y)^2 + (dc * sampling_x)^2 over the foreground pixels, every product, the sum and the
 *                root rounded once to float64 and nothing fused -- scipy's expression, and equal to its result bit for bit.
 *                With cyclic_x the column offset is min(|dc|, nx - |dc|).
 *   nearest_out  int32 [n_members][ny*nx], or NULL: the linear index into its plane of the foreground pixel that cost belongs
 *                to (a pixel's own index on foreground).  Tie rule: among pixels of equal cost the smallest linear index.
 *                (Inside a column the two candidates at equal |dr| go to the smaller row; the rule holds as long as different
 *                |dr| of one column never round to one cost, i.e. (ny sy)^2 + (nx sx)^2 < 2^52 sy^2: any plane a user has.)
 *   empty plane  a plane without a foreground pixel is +inf everywhere, nearest -1: our definition, scipy's answer there
 *                has no meaning.
 *   max_distance > 0: the result equals the unbounded one where that is <= max_distance and is +inf, nearest -1, elsewhere;
 *                the search of every pixel ends at that radius.  <= 0: unbounded.
 *   work_dev     int32 [lc_distance_work_elems(ny, nx, n_members)] scratch (0 elements for bad sizes)
 * Width limit: nx <= 16384 (a row of int32 offsets is staged in LDS: 64 KiB, two workgroups per CU); a wider plane is refused
 * with LC_EUNSUPPORTED, a plane of 2^31 pixels or more with LC_EINVAL, both before any HIP call.
 * No kernel of this call waits for another workgroup. */
size_t lc_distance_work_elems(int ny, int nx, int n_members);
typedef struct lc_distance_args {
    size_t struct_size; /* sizeof(lc_distance_args): checked before any other field */
    const void *mask;
    int dtype, ny, nx, n_members;
    int cyclic_x;
    double sampling_y, sampling_x; /* > 0 and finite */
    double max_distance;           /* <= 0: unbounded */
    void *dist_out;                /* float64 [n_members][ny*nx] */
    void *nearest_out;             /* int32, or NULL */
    void *work_dev;
} lc_distance_args;
int lc_distance_transform(lc_ctx *ctx, const lc_distance_args *args);

/* ---- great-circle distance to the nearest ridge pixel ----------------------------------
 * Replaces nothing in the reference: it is the latitude-dependent metric that the index-unit transform above, the driver's
 * LCS/area_of_influence.py:231, cannot give on a latitude-longitude grid (wrong by 1 / cos(latitude) along longitude, blind
 * across the poles and, without cyclic_x, across the seam).  Added at LC_VERSION 104 without a bump: nothing that existed
 * changed.  n_members independent planes [n_members][ny*nx] per call, all on the same grid.
 *
 * Foreground: as above, a pixel whose value is != 0 and not NaN; mask: `dtype` elements, LC_F32 or LC_F64.
 * Coordinates: the caller hands over, float64 on the device, cos_lat / sin_lat [ny] and cos_lon / sin_lon [nx] of its
 * latitudes and longitudes (any grid: not uniform, not global, not sorted); no kernel evaluates a trigonometric function of a
 * coordinate.  Node (r, c) is the unit vector X = fl(cos_lat[r] cos_lon[c]), Y = fl(cos_lat[r] sin_lon[c]), Z = sin_lat[r].
 *   cost_out     float64 [n_members][ny*nx], or NULL: the smallest, over the foreground pixels q of the plane, squared chord
 *                cost = fl(fl(fl(dX dX) + fl(dY dY)) + fl(dZ dZ)) with dX = fl(Xp - Xq), ...: every operation rounded once to
 *                float64 and nothing fused.  0 on foreground.
 *   nearest_out  int32 [n_members][ny*nx], or NULL: the linear index into its plane of the foreground pixel that cost belongs
 *                to.  Tie rule: among pixels of equal cost the smallest linear index.
 *   dist_out     float64 [n_members][ny*nx], or NULL: 2 radius asin(min(1, sqrt(cost) / 2)), exactly 0 on foreground.
 *                (At least one of the three outputs is given.)
 *   empty plane  a plane without a foreground pixel is +inf everywhere, nearest -1.
 *   max_chord2 > 0: (2 sin(max_distance / (2 radius)))^2, squared by the caller in float64; a pixel keeps its result where
 *                cost <= max_chord2 and is +inf, nearest -1, elsewhere -- exactly the unbounded result under that mask.  A
 *                query row is searched against the rows whose same-meridian chord to it is within the bound only (plus a
 *                margin far above every rounding: no culling changes a result).  <= 0: unbounded.
 *   max_distance the same bound in the unit of radius: > 0 beside a max_chord2 > 0, not read otherwise.
 *   work_dev     int32 [lc_sphere_distance_work_elems(ny, nx, n_members)] scratch, 8-byte aligned (0 elements for bad sizes,
 *                a plane of 2^31 pixels or more among them)
 * A plane of 2^31 pixels or more and non-positive sizes are refused with LC_EINVAL before any HIP call.  Every query pixel is
 * compared with every foreground pixel of its band: the cost of a call is their product.
 * No kernel of this call waits for another workgroup. */
size_t lc_sphere_distance_work_elems(int ny, int nx, int n_members);
typedef struct lc_sphere_distance_args {
    size_t struct_size; /* sizeof(lc_sphere_distance_args): checked before any other field */
    const void *mask;
    int dtype, ny, nx, n_members;
    const double *cos_lat, *sin_lat; /* device, [ny] */
    const double *cos_lon, *sin_lon; /* device, [nx] */
    double radius;                   /* > 0, finite */
    double max_chord2;               /* <= 0: unbounded */
    double max_distance;             /* > 0 where max_chord2 > 0 */
    void *dist_out;                  /* float64, or NULL */
    void *nearest_out;               /* int32, or NULL */
    void *cost_out;                  /* float64, or NULL */
    void *work_dev;
} lc_sphere_distance_args;
int lc_sphere_distance(lc_ctx *ctx, const lc_sphere_distance_args *args);

/* ---- thinning and dilating a ridge mask (skeletonize_ridges, dilate_ridges) -------------
 * The two morphological steps of the driver's chain: skeletonize(ridges.values) between the Hessian mask and the filter
 * (LCS/area_of_influence.py:207) and binary_dilation(ridges.values) at its end (:233).  Both entry points were added at
 * LC_VERSION 104 without a bump: nothing that existed changed.  n_members independent planes [n_members][ny*nx] per call,
 * every launch for all of them; pixels outside a plane are background; cyclic_x != 0: column nx-1 is the western neighbour
 * of column 0 (rows r-1 .. r+1).
 *
 * Foreground: as above, a pixel whose value is != 0 and not NaN; mask: `dtype` elements, LC_F32 or LC_F64.
 *   out          uint8 [n_members][ny*nx]: 1 on the pixels of the result, else 0
 *   LC_MORPH_THIN    a parallel two-sub-iteration thinning driven by a table.  The neighbourhood index of a pixel is
 *                NW + 2 N + 4 NE + 8 E + 16 SE + 32 S + 64 SW + 128 W (north: row r-1); table[index] is a 2-bit code, bit 0
 *                "delete in the first sub-iteration", bit 1 "in the second".  A sub-iteration reads the whole plane as the
 *                one before left it and deletes every foreground pixel whose code has its bit; an iteration is the first
 *                followed by the second; thinning ends when an iteration deletes nothing, or after max_iterations (<= 0:
 *                unbounded).  table: HOST pointer to 256 bytes, read before the call returns; a code above 3 is refused.
 *   LC_MORPH_DILATE  a background pixel becomes foreground when a neighbour named in `structure` (bits of the same index:
 *                170 = N, E, S, W; 255 = all eight) is foreground; max_iterations (>= 1) times.
 *   iterations_per_launch  0: the library's default (4 thinning iterations = 8 sub-steps, 8 dilations); 1 .. that many: fewer
 *                per launch.  The result does not depend on it.
 *   launches_out HOST int, or NULL: the step launches the call made
 *   work_dev     int32 [lc_morph_work_elems(ny, nx, n_members)] scratch (0 elements for bad sizes)
 * Convergence is found by the host side of the call: after each launch but the last it reads back one word (the OR of one
 * flag per tile) and stops when nothing changed.  That is one stream synchronisation per launch, i.e. per 4 thinning
 * iterations; the call returns with at most one copy still enqueued.
 * A null context, a wrong struct_size, a bad op, a plane of 2^31 pixels or more and a table code above 3 are refused with
 * LC_EINVAL before any HIP call.
 * No kernel of this call waits for another workgroup. */
enum lc_morph_op { LC_MORPH_THIN = 0, LC_MORPH_DILATE = 1 };
size_t lc_morph_work_elems(int ny, int nx, int n_members);
typedef struct lc_morph_args {
    size_t struct_size; /* sizeof(lc_morph_args): checked before any other field */
    const void *mask;
    int dtype, ny, nx, n_members;
    int op;                      /* enum lc_morph_op */
    int cyclic_x;
    const uint8_t *table;        /* LC_MORPH_THIN: host, 256 codes 0 .. 3 */
    int structure;               /* LC_MORPH_DILATE: 1 .. 255 */
    int max_iterations;
    int iterations_per_launch;   /* 0: the library's default */
    void *out;                   /* uint8 [n_members][ny*nx] */
    int *launches_out;           /* host, or NULL */
    void *work_dev;
} lc_morph_args;
int lc_mask_morphology(lc_ctx *ctx, const lc_morph_args *args);

/* ---- thinned ridges as ordered lines (trace_lines, ridge_lines) --------------------------
 * The vector form of a one-pixel-wide mask: which pixels make up each ridge line and in which order, where lines end and branch,
 * and how long they are on the sphere.  Nothing in the reference computes it (its chain, LCS/area_of_influence.py, ends at
 * rasters), so the meaning is fixed here; tests/lines.py restates it as a plain pixel walk.  Added at LC_VERSION 104 without a
 * bump: nothing that existed changed.  n_members independent planes [n_members][ny*nx] per call.
 *
 * Foreground: as above, a pixel whose value is != 0 and not NaN; mask: `dtype` elements, LC_F32 or LC_F64.  cyclic_x != 0: column
 * nx-1 is the western neighbour of column 0; it needs nx >= 3 (a pixel would otherwise neighbour itself or one pixel twice).
 *   direction codes  k = 0 .. 7: NW, N, NE, E, SE, S, SW, W with north at row r-1 -- the bit order of lc_morph_args; the opposite
 *                of k is (k + 4) % 8.
 *   links        a foreground pixel is linked to each foreground edge neighbour (N, E, S, W), and to a foreground corner neighbour
 *                only if neither of the two pixels edge-adjacent to both is foreground: a staircase is a path, not a chain of
 *                triangles.  links_out[p]: bit k set per link; the degree is its popcount (at most 4).
 *   nodes        a pixel of degree 2 is INTERIOR; every other foreground pixel is a NODE: degree 0 isolated, 1 a free end, >= 3 a
 *                junction.
 *   darts        a link with a direction: id = p * 8 + k, p the linear index in the plane, k the code it leaves p by.
 *   lines        two links belong to the same line when they meet in an interior pixel, so every link lies in exactly one line.
 *                An open line is a path from node to node (both may be the same junction: its first and last point coincide and
 *                it is still open); a ring consists of interior pixels only; a pixel of degree 0 is a line of one point.
 *   key          the line's canonical first dart: of an open line the smaller id of the two darts that leave its end nodes along
 *                it; of a ring the smallest id of all its darts (it leaves the ring's first pixel in raster order by its lower
 *                code); of an isolated pixel p * 8.  The points of a line are the pixels met from that dart on, both end nodes
 *                included; a ring does not repeat its first pixel.  Lines of a plane are numbered in the order of their keys.
 *   measures     n_diag: corner links; position: links before a point; length of a link (with the tables): 2 radius
 *                asin(min(1, sqrt(cost) / 2)) with lc_sphere_distance's node vectors and squared chord cost, from the same tables.
 *
 * The call ranks the STATES of the interior pixels: pixel q with links a < b has the states s = 2 q + 0, which leaves q through a,
 * and 2 q + 1, which leaves through b; the HEAD of a state is the pixel its link leads to.  Per state, [n_members][2 * ny*nx]:
 *   key_out      int32: the key of the line q lies on; -1 in the slots of pixels that are not interior, where flags_out is 0 and
 *                nothing else is written
 *   pos_out      int32: the position of q along its line (the same in both states)
 *   ndiag_out    int32: corner links before q
 *   dist_out     float64: sum of the link lengths before q (order of summation not fixed by this text; the call itself is
 *                deterministic).  With the tables only.
 *   head_out     int32: the head, as a linear index into the plane
 *   link_length_out  float64: length of the link the state leaves by.  With the tables only.
 *   flags_out    uint8: LC_LINE_STATE on every state; LC_LINE_CANONICAL: the state runs away from the line's first point;
 *                LC_LINE_HEAD_IS_END: the head is an end node of the line or, on a ring, the ring's first pixel;
 *                LC_LINE_RING; LC_LINE_CORNER_LINK: the link it leaves by is a corner link.
 * So the points of a line that interior pixels do not give are the heads of the states flagged LC_LINE_HEAD_IS_END (position 0 from
 * a state that is not canonical, position + 1 from a canonical one), and lines without an interior pixel -- node next to node,
 * isolated pixels -- follow from links_out alone.
 *   counts_out   int32 [n_members][4]: foreground pixels, interior pixels, nodes, links
 *   rounds_out   HOST int, or NULL: the doubling rounds the call ran, at most 2 ceil(log2(I)) for I the largest interior count
 *   tables       cos_lat, sin_lat [ny], cos_lon, sin_lon [nx]: float64 on the device, as for lc_sphere_distance; all four NULL:
 *                no lengths, dist_out and link_length_out are not written
 *   work_dev     int32 [lc_lines_work_elems(ny, nx, n_members)] scratch, 16-byte aligned: 96 bytes per pixel (two states, each
 *                16 bytes and a float64, in two buffers) and 512 bytes (0 elements for bad sizes)
 * Ranking is pointer doubling, one launch per round, double-buffered: a state carries its successor, the links covered, the corner
 * links among them, their length and the smallest dart id seen, and ends at the first node.  What has not ended once 2^rounds is at
 * least the largest interior count of a plane lies on a ring; the minimum it carries is then the ring's, the ring is broken at that
 * dart and ranked again as an open chain.  Convergence is found as lc_mask_morphology finds it: one word read back per launch.
 * A null context or argument structure, a wrong struct_size, a bad dtype, non-positive sizes, a plane of 2^28 pixels or more
 * (dart ids are int32), cyclic_x with nx < 3, tables given in part and a radius that is not positive and finite beside them are
 * refused with LC_EINVAL before any HIP call.
 * No kernel of this call waits for another workgroup. */
enum lc_line_flags {
    LC_LINE_STATE = 1, LC_LINE_CANONICAL = 2, LC_LINE_HEAD_IS_END = 4, LC_LINE_RING = 8, LC_LINE_CORNER_LINK = 16
};
size_t lc_lines_work_elems(int ny, int nx, int n_members);
typedef struct lc_lines_args {
    size_t struct_size; /* sizeof(lc_lines_args): checked before any other field */
    const void *mask;
    int dtype, ny, nx, n_members;
    int cyclic_x;
    const double *cos_lat, *sin_lat; /* device, [ny]; or all four NULL */
    const double *cos_lon, *sin_lon; /* device, [nx] */
    double radius;                   /* > 0, finite (with the tables) */
    void *links_out;                 /* uint8 [n_members][ny*nx] */
    void *counts_out;                /* int32 [n_members][4] */
    void *key_out, *pos_out, *ndiag_out, *head_out; /* int32 [n_members][2 * ny*nx] */
    void *flags_out;                 /* uint8 [n_members][2 * ny*nx] */
    void *dist_out, *link_length_out; /* float64 [n_members][2 * ny*nx]; with the tables */
    int *rounds_out;                 /* host, or NULL */
    void *work_dev;
} lc_lines_args;
int lc_trace_lines(lc_ctx *ctx, const lc_lines_args *args);

/* The length of the links no state leaves by -- a node next to a node --, or of any list of pixel pairs of one grid:
 * length_out[i] = 2 radius asin(min(1, sqrt(cost) / 2)) between pixels from[i] and to[i] (linear indices into a plane of ny x nx),
 * the expression of lc_trace_lines' link_length_out; NaN for a pair that names no pixel of the plane.  n_pairs 0 is no work.  A
 * null context, a wrong struct_size, bad sizes and a radius that is not positive and finite are refused with LC_EINVAL before any
 * HIP call.  One kernel, which waits for no other workgroup. */
typedef struct lc_link_lengths_args {
    size_t struct_size;   /* sizeof(lc_link_lengths_args): checked before any other field */
    const void *from, *to; /* int32 [n_pairs], device */
    long long n_pairs;
    int ny, nx;
    const double *cos_lat, *sin_lat; /* device, [ny] */
    const double *cos_lon, *sin_lon; /* device, [nx] */
    double radius;
    void *length_out;     /* float64 [n_pairs] */
} lc_link_lengths_args;
int lc_line_link_lengths(lc_ctx *ctx, const lc_link_lengths_args *args);

/* ---- adaptive local threshold (threshold_local, above_local_threshold) ------------------
 * The other half of the driver's result, its "local strain" area (LCS/area_of_influence.py:194-199):
 *   local_thresh = threshold_local(ftle_local.values, block_size=301, offset=-.8);  binary_local = ftle_local > local_thresh
 * skimage.filters.threshold_local with its defaults is scipy.ndimage.gaussian_filter(f, sigma, mode='reflect') - offset with
 * sigma = (block_size - 1) / 6 and scipy's radius int(4 sigma + 0.5): block 301 is sigma 50, radius 200.  Both entry points
 * were added at LC_VERSION 104 without a bump: nothing that existed changed.  n_members independent planes [n_members][ny*nx]
 * per call, every launch for all of them; a plane is smoothed on its own.
 *
 *   f              `dtype` elements, LC_F32 or LC_F64; float32 is widened to float64 where it is read: the results are those of
 *                  the widened field bit for bit
 *   sigma_y, sigma_x  the Gaussian's width along latitude / longitude in grid steps.  An axis with sigma <= 1e-15 is not
 *                  filtered, as scipy skips it (both: threshold = f - offset).  Weights, radius, accumulation in double and
 *                  the summation order are lc_gaussian_filter's (centre first, then the pairs from the outermost inwards):
 *                  with offset 0, equal sigmas and float64 the threshold equals its result bit for bit.
 *   cyclic         != 0: longitude is periodic (scipy mode 'wrap' on that axis) instead of reflected; latitude is always
 *                  reflected.  Either rule holds at any distance: a radius many times the plane is legal.
 *   threshold_out  float64 [n_members][ny*nx] or NULL: smooth - offset, one rounding
 *   mask_out       uint8 [n_members][ny*nx] or NULL: 1 where f > threshold, else 0; a NaN on either side gives 0.  With only
 *                  the mask wanted no threshold plane is written.
 *   work           float64 [lc_local_threshold_work_elems(ny, nx, n_members)] scratch (0 elements for bad sizes): the planes
 *                  between the two passes; may be NULL when at most one axis is filtered
 * Refused with LC_EINVAL before any HIP call: a null context or argument structure, a wrong struct_size, a bad dtype or size, a
 * plane of 2^31 points or more, a NaN sigma, an offset that is not finite, both outputs NULL, any overlap among f, work and the
 * outputs; with LC_EUNSUPPORTED, as lc_gaussian_filter: a radius above 256.
 * lc_ctx_last_threshold_kernel: the kernels of the last call joined by '+' ("" before the first call or for a null context).
 * No kernel of this call waits for another workgroup. */
size_t lc_local_threshold_work_elems(int ny, int nx, int n_members);
typedef struct lc_local_threshold_args {
    size_t struct_size; /* sizeof(lc_local_threshold_args): checked before any other field */
    const void *f;
    int dtype, ny, nx, n_members;
    double sigma_y, sigma_x;
    double offset;      /* finite */
    int cyclic;
    void *work;          /* float64 */
    void *threshold_out; /* float64, or NULL */
    void *mask_out;      /* uint8, or NULL */
} lc_local_threshold_args;
int lc_local_threshold(lc_ctx *ctx, const lc_local_threshold_args *args);
const char *lc_ctx_last_threshold_kernel(const lc_ctx *ctx);

/* ---- inverse-distance weighting of scattered values on the sphere (Inverse_weighted_interpolation, xr_idx_interp) ----
 * LCS/tools.py:285-333: values known at scattered longitude / latitude points, gridded with weights 1 / d^power of the
 * great-circle distance d.  Two departures from the reference: its distance calls arctan(sqrt(a), sqrt(1 - a)) where it means
 * arctan2 (the second argument is numpy's out=), and a source that coincides with a target gives inf / inf = NaN there.  Here
 * the distance is the project's own (lc_sphere_distance's chord form) and a coincident source is the limit of the weighting.
 * All three entry points were added at LC_VERSION 104 without a bump: nothing that existed changed.
 *
 * Points: the caller hands over, float64 on the device, the unit vectors of its sources and targets,
 *   X = fl(cos lat cos lon), Y = fl(cos lat sin lon), Z = sin lat   (for a grid: from the row / column tables, one rounded
 * product, as lc_sphere_distance's nodes); no kernel evaluates a trigonometric function of a coordinate.  A source or a target
 * that is to be left out (a coordinate that is not finite, |lat| > 90) is given NaN components.
 *   cost   = fl(fl(fl(dX dX) + fl(dY dY)) + fl(dZ dZ)), dX = fl(Xt - Xs), ...: float64, every operation rounded once, nothing
 *            fused.  A source is within reach of a target where cost <= max_chord2 (unbounded: where cost is not NaN).
 *   d      = 2 radius asin(min(1, sqrt(cost) / 2));  w = 1 / d^power, as 1 / (d d) for power 2, 1 / d for power 1, 1 / pow(d,
 *            power) otherwise.
 *   values `dtype` elements (LC_F32 or LC_F64) [n_planes][n_src] on shared positions; the geometry of a pair is evaluated once
 *            for up to 4 planes.  A NaN value leaves its source out of that plane, in every sum below.
 *   out    `dtype` [n_planes][n_tgt]: sum(w z) / sum(w) over the contributing sources, accumulated in float64 (w z + sum is
 *            one fused operation) and rounded to `dtype` once.  Where one or more contributing sources have cost == 0: the mean
 *            of their values.  Without a contributing source: NaN.
 *   weight_out  float64 [n_planes][n_tgt], or NULL: sum(w); +inf on an exact hit, 0 without a contributing source.
 *   count_out   int32 [n_tgt], or NULL: the sources within reach, whatever their values are.
 *   max_chord2 > 0: (2 sin(max_distance / (2 radius)))^2, squared by the caller in float64.  Each workgroup of 256 targets then
 *            walks only the smallest contiguous range of sources that holds every source whose same-meridian chord to the
 *            latitudes of its targets is within the bound plus a margin far above every rounding: no culling changes a result.
 *            The range is short where the sources are sorted by Z; they need not be.  <= 0: unbounded.
 *   max_distance  the same bound in the unit of radius: > 0 beside a max_chord2 > 0, not read otherwise.
 *   work_dev  float64 [lc_idw_work_elems(n_src, n_tgt, n_planes)] scratch (0 elements for bad sizes).
 * The order of summation is not part of the contract; it is a function of the sizes alone -- with fewer than 256 workgroups of
 * targets the sources of each are split over several workgroups, whose partial sums a second kernel adds in ascending order --
 * so two calls on the same arguments give the same bits.  There is no atomic operation.
 * Refused with LC_EINVAL before any HIP call: a null context, argument structure or pointer (weight_out and count_out may be
 * NULL), a wrong struct_size, a dtype other than LC_F32 / LC_F64, a size <= 0 or one that cannot be sized, a power outside
 * (0, 16], a radius that is not positive and finite, a NaN max_chord2, a max_chord2 > 0 without a max_distance > 0.
 * lc_ctx_last_idw_kernel: the kernels of the last call joined by '+' ("" before the first call or for a null context).
 * No kernel of this call waits for another workgroup. */
size_t lc_idw_work_elems(int n_src, int n_tgt, int n_planes);
typedef struct lc_idw_args {
    size_t struct_size; /* sizeof(lc_idw_args): checked before any other field */
    const double *src_x, *src_y, *src_z; /* device, [n_src] */
    const void *values;                  /* dtype [n_planes][n_src] */
    const double *tgt_x, *tgt_y, *tgt_z; /* device, [n_tgt] */
    int dtype, n_src, n_tgt, n_planes;
    double power;        /* in (0, 16] */
    double radius;       /* > 0, finite */
    double max_chord2;   /* <= 0: unbounded */
    double max_distance; /* > 0 where max_chord2 > 0 */
    void *out;           /* dtype [n_planes][n_tgt] */
    void *weight_out;    /* float64 [n_planes][n_tgt], or NULL */
    void *count_out;     /* int32 [n_tgt], or NULL */
    void *work_dev;
} lc_idw_args;
int lc_idw_interp(lc_ctx *ctx, const lc_idw_args *args);
const char *lc_ctx_last_idw_kernel(const lc_ctx *ctx);

/* ---- great-circle transects across ridge lines and their composites (tools.ridge_transects) ----
 * Replaces LCS/area_of_influence.py:17-87 (find_area), as far as that function is well defined: it paints pixels along the
 * Hessian eigenvector of every ridge pixel in a Python loop, steps in degrees with argmin lookups (wrong away from the equator)
 * and gives the sign of the normal no meaning; its painted mask is not reproduced.  Here a second field is sampled along the
 * great circle through every point of a traced line (lc_trace_lines; Engine.trace_lines orders the points), at right angles to
 * the line, at signed distances s_k = k spacing, k = -K .. K, and the samples of a line are averaged offset by offset.
 * tests/transects.py restates what follows point by point in numpy.  Both entry points were added at LC_VERSION 104 without a
 * bump: nothing that existed changed.
 *
 * Lines: pixel int32 [n_points] (the linear index of a point in its plane), point_line int32 [n_points], and per line
 *   line_offset, line_count, line_plane int32 [n_lines], line_closed uint8 [n_lines]: the points of line l are offset ..
 *   offset + count, ordered along it; a ring's first point is not repeated.
 * Grid: cos_lat, sin_lat [ny], cos_lon, sin_lon [nx] float64 as for lc_sphere_distance (the caller's cos / sin of the
 *   coordinates), and the coordinates themselves in degrees, lat_deg [ny], lon_deg [nx], strictly ascending, |lat| <= 90; with
 *   cyclic_x lon_deg[nx - 1] - lon_deg[0] < 360.  The latitudes need not be uniform.
 * Offsets: cos_off[k] = cos(s_k / radius), sin_off[k] = sin(s_k / radius), float64 [n_offsets], n_offsets = 2 K + 1, formed by
 *   the caller with |s_k| / radius < pi / 2.  No kernel evaluates a trigonometric function of a coordinate or of a distance.
 * Every operation below is float64, rounded once, nothing fused, in the order written:
 *   point    p_i = (cl cx, cl sx, sl) of the point's row and column.
 *   tangent  with m = smooth: a = max(i - m, 0), b = min(i + m, count - 1) within an open line; on a ring m is capped at
 *            (count - 1) / 2 and a = (i - m) mod count, b = (i + m) mod count.  d = p_b - p_a, dot = (d_x p_x + d_y p_y) + d_z p_z,
 *            u = d - dot p, len = sqrt((u_x u_x + u_y u_y) + u_z u_z), t = u / len.  Where a == b or len is not > 0 the point has
 *            no tangent: its normal, its components and all its samples are NaN (lone pixels, lines of one point).
 *   normal   the left normal n = p x t = (p_y t_z - p_z t_y, p_z t_x - p_x t_z, p_x t_y - p_y t_x).  Components against the point's
 *            own column (so they are defined at a pole): east (-sx, cx, 0), north (-(sl cx), -(sl sx), cl);
 *            n_east = cx n_y - sx n_x, n_north = (north_x n_x + north_y n_y) + cl n_z, likewise t_east, t_north.
 *            LC_ORIENT_LEFT keeps n; LC_ORIENT_NORTH negates it where n_north < 0, or n_north == 0 and n_east < 0;
 *            LC_ORIENT_EAST the same with the roles exchanged.
 *   sample   q = cos_off[k] p + sin_off[k] n; latitude = atan2(q_z, sqrt(q_x q_x + q_y q_y)) (180 / pi), longitude = atan2(q_y,
 *            q_x) (180 / pi) -- the hypotenuse as a rounded square root of the rounded sum: |q| is about 1, nothing overflows --;
 *            with cyclic_x the longitude x becomes x - floor((x - lon[0]) / 360) 360, then + 360 if below lon[0], then - 360 if
 *            not below lon[0] + 360.  lat_out / lon_out hold these positions.
 *   cell     from the stored position by exact comparisons: j0 the last row with lat[j0] <= y, j1 = min(j0 + 1, ny - 1), the
 *            columns likewise; with cyclic_x the cell after the last column ends at lon[0] + 360 in column 0.  A position
 *            outside [lat[0], lat[ny - 1]], or without cyclic_x outside [lon[0], lon[nx - 1]], is NaN.
 *   value    LC_TRANSECT_LINEAR: w_y = (y - lat[j0]) / (lat[j1] - lat[j0]) (0 where j1 == j0), w_x likewise,
 *            ((w00 v00 + w01 v01) + w10 v10) + w11 v11 with w00 = (1 - w_y)(1 - w_x), w01 = (1 - w_y) w_x, w10 = w_y (1 - w_x),
 *            w11 = w_y w_x, the corners widened to float64, the sum rounded to `dtype` once; NaN when a corner is NaN.
 *            LC_TRANSECT_NEAREST: row j1 where y - lat[j0] > lat[j1] - y, else j0 (ties to the lower index), columns likewise.
 *   fields   `dtype` [n_fields][n_planes][ny][nx]; the points of a line of plane m read plane m of every field.
 * Outputs: normal_out float64 [7][n_points]: n_x, n_y, n_z, n_east, n_north, t_east, t_north; lat_out, lon_out float64
 *   [n_points][n_offsets]; values_out `dtype` [n_fields][n_points][n_offsets]; mean_out `dtype` and count_out int32
 *   [n_fields][n_lines][n_offsets]: the mean of the finite values of the line's points at that offset, accumulated in float64,
 *   and how many there were; NaN where there were none.  The order of summation depends on the sizes alone: two calls agree
 *   bit for bit.  There is no atomic operation and no kernel waits for another workgroup.
 * Refused with LC_EINVAL before any HIP call: a null context, argument structure or pointer, a wrong struct_size, a dtype other
 * than LC_F32 / LC_F64, ny or nx < 2, another size < 1, an even n_offsets, smooth < 1, an unknown orient or method, cyclic_x with
 * fewer than 3 columns; with LC_EUNSUPPORTED: ny nx, n_points n_offsets or n_lines n_offsets of 2^31 or more, more than 65535
 * fields.  lc_ctx_last_transects_kernel: the kernels of the last call joined by '+' ("" before the first call or for a null
 * context); it replaces nothing of LCS/area_of_influence.py:17-87 but names what ran in its place. */
enum { LC_ORIENT_LEFT = 0, LC_ORIENT_NORTH = 1, LC_ORIENT_EAST = 2 };
enum { LC_TRANSECT_LINEAR = 0, LC_TRANSECT_NEAREST = 1 };
typedef struct lc_transects_args {
    size_t struct_size; /* sizeof(lc_transects_args): checked before any other field */
    const int *pixel, *point_line;                      /* device, int32 [n_points] */
    const int *line_offset, *line_count, *line_plane;   /* device, int32 [n_lines] */
    const unsigned char *line_closed;                   /* device, [n_lines] */
    const double *cos_lat, *sin_lat, *cos_lon, *sin_lon; /* device */
    const double *lat_deg, *lon_deg;                    /* device, ascending degrees */
    const double *cos_off, *sin_off;                    /* device, [n_offsets] */
    const void *fields;                                 /* dtype [n_fields][n_planes][ny][nx] */
    int dtype, ny, nx, n_planes, n_points, n_lines, n_offsets, n_fields;
    int smooth, orient, method, cyclic_x;
    double *normal_out;        /* [7][n_points] */
    double *lat_out, *lon_out; /* [n_points][n_offsets] */
    void *values_out;          /* dtype [n_fields][n_points][n_offsets] */
    void *mean_out;            /* dtype [n_fields][n_lines][n_offsets] */
    int *count_out;            /* [n_fields][n_lines][n_offsets] */
} lc_transects_args;
int lc_ridge_transects(lc_ctx *ctx, const lc_transects_args *args);
const char *lc_ctx_last_transects_kernel(const lc_ctx *ctx);

/* ---- multi-GPU: halo exchange on RCCL ----------------------------------------
 * New (the reference is single-process).  One process per GPU,
 * seed rows block-partitioned, wind replicated; lc_advect needs no communication
 * (row0 / ny_global).  Between lc_advect and lc_sigma every rank needs the 2 boundary
 * rows of (x_dep, y_dep) of the previous and the next rank (4th-order stencil,
 * LCS/tools.py:202-207): lc_halo_exchange does that in place, point-to-point over
 * RCCL (xGMI), on the context's stream, non-periodic in rank, no collective.
 *
 *   lc_comm_unique_id   rank 0 makes the 128-byte id; the caller hands it to every rank
 *                       (MPI, a file, torch.distributed ...)
 *   lc_comm_create      collective over the nranks processes; ctx fixes the device
 *   lc_halo_exchange    x_ext, y_ext: [n_rows][nx] device buffers whose middle
 *                       n_rows - n_lo - n_hi rows hold this rank's departure points
 *                       (write them there with lc_advect on a sub-view); the first n_lo /
 *                       last n_hi rows receive the neighbours' boundary rows.  n_lo must be
 *                       2 except on rank 0 (0), n_hi 2 except on the last rank (0).
 * RCCL is loaded at run time (dlopen), shared with the host process if it already
 * carries one; without it these calls return LC_ERCCL and everything else works. */
typedef struct lc_comm lc_comm;
int lc_comm_unique_id(void *id_out, size_t id_bytes /* >= 128 */);
int lc_comm_create(lc_ctx *ctx, int nranks, int rank, const void *id, size_t id_bytes, lc_comm **out);
int lc_comm_destroy(lc_comm *comm);
/* ncclCommCount / ncclCommUserRank of the communicator: the ranks RCCL itself spans (a benchmark reports it). */
int lc_comm_count(const lc_comm *comm, int *nranks_out, int *rank_out);
int lc_halo_exchange(lc_ctx *ctx, lc_comm *comm, void *x_ext, void *y_ext, int dtype,
                     int n_rows, int nx, int n_lo, int n_hi);
/* An lc_flag_allreduce_fn on RCCL: ncclAllReduce(max, uint32) in place over the communicator, on the stream of the
 * context the communicator was created with.  Use: lc_ctx_set_flag_allreduce(ctx, lc_comm_flag_allreduce, comm). */
int lc_comm_flag_allreduce(void *comm /* lc_comm* */, void *flags_dev, size_t count);

/* ---- one-call host entry point ----------------------------------------------
 * What a reference-side binding would call from LCS.__call__ (LCS/LCS.py:129-157):
 * host arrays in, host arrays out; upload, pack, advect, sigma, download, sync -- with the upload overlapped with the
 * kernels level chunk by level chunk and every transfer staged through pinned memory (lc_ctx_set_host_pipeline, the
 * default); keep the context across calls: it owns the staging ring.  The output buffers may be written (zeros) before the
 * results arrive.  Any of sigma_out / x_out / y_out / traj_x / traj_y may be NULL. */
int lc_lcs_host(lc_ctx *ctx, const void *u_host, const void *v_host, int dtype,
                int nt, int ny_f, int nx_f,
                const void *lat_f_host, const void *lon_f_host,
                const void *seed_lat_host, int ny, const void *seed_lon_host, int nx,
                double timestep, int settls_order, int interp_order, int cyclic_x,
                int t0, int nsteps, double gauss_sigma /* <=0: none */,
                int fd_fp32_cast, int tensor_layout,
                void *sigma_out, void *x_out, void *y_out, void *traj_x, void *traj_y);

/* ---- the reference's default global call form in one call, torch-free -------
 * LCS(...)(ds, isglobal=True) (LCS/LCS.py:105-157, examples/ideal_vortex.py:280-287) on host arrays:
 * [interp_to_common_grid: lc_regrid_common_grid of u and v onto lc_common_grid's grid, float64]
 * -> [truncation >= 0: lc_spectral_truncate at that wavenumber on the grid type lc_inspect_gridtype finds (equally
 * spaced global or Gaussian latitudes; anything else is refused as windspharm refuses it)] -> lc_field_pack -> lc_advect (cyclic, seeds = grid nodes, all nt-1 steps)
 * -> [gauss_sigma > 0: lc_gaussian_filter] -> lc_sigma.
 * Outputs [ny_o * nx_o] on the host, any may be NULL: ny_o x nx_o = 360 x 721 and float64 when
 * interp_to_common_grid, else ny_f x nx_f in `dtype`.  Synchronous. */
int lc_common_grid(int *ny_out, int *nx_out, double *lats_out /* NULL or [360] */, double *lons_out /* NULL or [721] */);
int lc_lcs_global_host(lc_ctx *ctx, const void *u_host, const void *v_host, int dtype,
                       int nt, int ny_f, int nx_f, const double *lat_f_host, const double *lon_f_host,
                       int interp_to_common_grid, int truncation /* < 0: none */,
                       double timestep, int settls_order, int interp_order,
                       double gauss_sigma /* <= 0: none */, int fd_fp32_cast, int tensor_layout,
                       void *sigma_out, void *x_out, void *y_out);

#ifdef __cplusplus
}
#endif
#endif /* LCS_HIP_H */
