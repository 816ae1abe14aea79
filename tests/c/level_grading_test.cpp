// CPU unit test of the graded level counts in lagrangiancoherence_amd/csrc/launch_plan.h (lcplan::grading, graded_slot,
// graded_range): every tile's ranges over the launches of a call tile [0, total) in order, the longest range is bounded,
// the per-launch map of dispatch positions to slots is a bijection that keeps the XCD, and degenerate parameters are the
// uniform chunks.  Then every plan tests/test_gpu_level_grading_matrix.py runs, by name (launch shape from xcd_chunk_tiles /
// xcd_grid / pole_rows, normalised n / zone / depth, the kinds of ranges its tiles get), and the composition the kernel runs,
// tile_of_block(graded_slot(...)), over every tile map that file sets.  Built by tests/test_level_grading.py with
// g++ -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../lagrangiancoherence_amd/csrc/launch_plan.h"

static long g_fail = 0;
#define CHECK(cond, ...)                                                    \
    do {                                                                    \
        if (!(cond)) {                                                      \
            if (++g_fail <= 20) {                                           \
                std::printf("FAIL %s:%d  %s  ", __FILE__, __LINE__, #cond); \
                std::printf(__VA_ARGS__);                                   \
                std::printf("\n");                                          \
            }                                                               \
        }                                                                   \
    } while (0)

using namespace lcplan;

struct Seen {
    long cases = 0, graded = 0, empty = 0, one = 0, longer = 0;
};

// One plan: total levels, `launches` asked for (the chunk that gives them), zone / depth as a caller would set them.
static void check_plan(int total, int chunk, int zone, int depth, int blocks, Seen &seen) {
    const Grading g = grading(total, chunk, zone, depth, blocks);
    ++seen.cases;
    CHECK(g.n == n_chunks(total, chunk) && g.total == total && g.chunk == chunk && g.blocks == blocks, "plan echoes its arguments");
    CHECK(g.zone >= 0 && g.zone % XCDS == 0 && g.zone <= (zone > 0 ? zone : 0), "zone %d of %d", g.zone, zone);
    CHECK(g.zone == 0 || g.zone * (g.n + 2) <= blocks, "zone %d x (%d + 2) launches > %d blocks", g.zone, g.n, blocks);
    CHECK(g.depth >= 0 && g.depth <= chunk && g.depth <= (depth > 0 ? depth : 0), "depth %d of %d (chunk %d)", g.depth, depth, chunk);
    CHECK((g.zone == 0) == (g.depth == 0), "zone %d and depth %d vanish together", g.zone, g.depth);
    if (g.zone > 0) ++seen.graded;
    // the normalised plan is a fixed point
    const Grading g2 = grading(total, chunk, g.zone, g.depth, blocks);
    CHECK(g2.zone == g.zone && g2.depth == g.depth, "normalising twice changes the plan");
    std::vector<int> end(blocks, 0), hits(blocks);
    for (int launch = 0; launch < g.n; ++launch) {
        hits.assign(blocks, 0);
        for (int d = 0; d < blocks; ++d) {
            const int slot = graded_slot(g, launch, d);
            CHECK(slot >= 0 && slot < blocks, "slot %d of position %d", slot, d);
            if (slot < 0 || slot >= blocks) continue;
            ++hits[slot];
            // (a grid is a multiple of 8 blocks: xcd_grid)
            if (blocks % XCDS == 0) CHECK(slot % XCDS == d % XCDS, "position %d (XCD %d) runs slot %d (XCD %d)", d, d % XCDS, slot, slot % XCDS);
            CHECK(graded_position(g, launch, slot) == d, "graded_position is not the inverse at launch %d, position %d", launch, d);
            const Range r = graded_range(g, launch, d);
            CHECK(r.a == end[slot], "launch %d slot %d starts at %d, the previous launch ended at %d (total %d chunk %d zone %d depth %d blocks %d)",
                  launch, slot, r.a, end[slot], total, chunk, g.zone, g.depth, blocks);
            CHECK(r.b >= r.a && r.b <= total, "range [%d, %d) of %d levels", r.a, r.b, total);
            CHECK(r.b - r.a <= graded_longest(g), "range of %d levels, bound %d", r.b - r.a, graded_longest(g));
            if (g.zone == 0)  // degenerate: today's uniform chunks, exactly
                CHECK(r.a == chunk_first(launch, chunk) && r.b - r.a == chunk_levels(launch, total, chunk), "uniform launch %d: [%d, %d)", launch, r.a, r.b);
            else {
                seen.empty += r.b == r.a;
                seen.one += r.b - r.a == 1;
                seen.longer += r.b - r.a > chunk;
                // only the zone at the end of the dispatch order is cut short (the last launch: whatever is left)
                if (launch < g.n - 1 && d < blocks - g.zone) CHECK(r.b - r.a >= chunk_levels(launch, total, chunk), "position %d before the zone is short: %d levels", d, r.b - r.a);
                // the last position of every launch but a short last one loses the full depth
                if (d == blocks - 1 && launch < g.n - 1) CHECK(r.b - r.a <= chunk - g.depth, "the last position keeps %d of %d levels, depth %d", r.b - r.a, chunk, g.depth);
            }
            end[slot] = r.b;
        }
        for (int s = 0; s < blocks; ++s) CHECK(hits[s] == 1, "launch %d: slot %d taken %d times", launch, s, hits[s]);
    }
    for (int s = 0; s < blocks; ++s) CHECK(end[s] == total, "slot %d ends at level %d of %d", s, end[s], total);
}

// ---- the plans of tests/test_gpu_level_grading_matrix.py --------------------------------------------------------------------
// Seeds of that file: 136 columns, tall patches of 8 x 64 seeds (advect.hip: TILE_W = 8, TILE_H * SPL = 64, workgroups of 256),
// order 1.  The tile map and the grid come from the header's own functions, as advect.hip's two_seed_patch_grid takes them.
constexpr int M_NX = 136, M_TILE_W = 8, M_TILE_ROWS = 64, M_BLOCK = 256, M_ORDER = 1;
struct Launch {
    int ntx, ntiles, xcd_chunk, blocks, pole_blocks;
};
static Launch matrix_launch(int ny, int row0, int ny_global, int xcd_rows, int xcd_split, bool pole_blocks_on = true) {
    Launch L;
    L.ntx = (M_NX + M_TILE_W - 1) / M_TILE_W;
    const int nty = (ny + M_TILE_ROWS - 1) / M_TILE_ROWS;
    L.ntiles = L.ntx * nty;
    L.xcd_chunk = xcd_chunk_tiles(L.ntx, nty, xcd_rows, xcd_split);
    L.blocks = xcd_grid(L.ntiles, L.xcd_chunk);
    L.pole_blocks = pole_rows(M_ORDER, row0, ny, ny_global, M_NX, pole_blocks_on, M_BLOCK).blocks;
    return L;
}

// What the kernel runs: tile_of_block(graded_slot(g, launch, d), ...) at dispatch position d, levels graded_range(g, launch, d).
// Every tile has exactly one workgroup per launch, and its ranges over the launches are [0, total) in order.  Returns
// the ranges seen among the workgroups that hold a tile.
struct RangesSeen {
    int empty = 0, one = 0, longer = 0;
};
static RangesSeen check_composition(const Grading &g, const Launch &L, int tile_order, const char *what) {
    RangesSeen rs;
    const int launches = g.zone > 0 ? g.n : 1;  // (a zeroed plan: the dispatcher makes one launch, tile_of_block of the block itself)
    std::vector<int> end(L.ntiles, 0), hits(L.ntiles);
    for (int launch = 0; launch < launches; ++launch) {
        hits.assign(L.ntiles, 0);
        for (int d = 0; d < L.blocks; ++d) {
            const int tile = tile_of_block(g.zone > 0 ? graded_slot(g, launch, d) : d, L.ntiles, L.ntx, L.xcd_chunk, tile_order);
            CHECK(tile >= 0, "%s: tile %d at position %d", what, tile, d);
            if (tile < 0 || tile >= L.ntiles) continue;
            ++hits[tile];
            Range r{0, g.total};
            if (g.zone > 0) r = graded_range(g, launch, d);
            CHECK(r.a == end[tile], "composition, %s order %d: launch %d tile %d starts at level %d, it was left at %d", what, tile_order, launch, tile, r.a, end[tile]);
            CHECK(r.b >= r.a && r.b <= g.total, "%s: range [%d, %d)", what, r.a, r.b);
            rs.empty += r.b == r.a;
            rs.one += r.b - r.a == 1;
            rs.longer += g.zone > 0 && r.b - r.a > g.chunk;
            end[tile] = r.b;
        }
        for (int t = 0; t < L.ntiles; ++t)
            CHECK(hits[t] == 1, "composition, %s order %d xcd_chunk %d: launch %d runs tile %d %d times", what, tile_order, L.xcd_chunk, launch, t, hits[t]);
    }
    for (int t = 0; t < L.ntiles; ++t) CHECK(end[t] == g.total, "%s order %d: tile %d ends at level %d of %d", what, tile_order, t, end[t], g.total);
    return rs;
}

// One plan of the GPU file by name: the launch's shape, what grading() makes of the wish, and the ranges its tiles get.
// `all_kinds`: the plan must hold empty, one-level and longer-than-a-chunk ranges among the workgroups with a tile (a plan
// whose depth is the whole chunk does; depth 1 moves one level of one workgroup and can hold neither an empty nor, in
// chunks of 14, a one-level range; in the grids of 80 and 136 blocks the last eight positions of a launch hold no tile -- the
// grid is rounded up to whole XCD chunks -- so with three launches only the tiles that make levels up show, and it takes the
// fourth launch's rotation to bring tiles into a zone).
struct Plan {
    const char *what;
    int ny, row0, ny_global, xcd_rows, xcd_split;     // the seeds' rows and the context's tile map
    int total, chunk, zone, depth;                    // the call's levels and lc_ctx_set_level_grading's arguments
    int tiles, blocks, pole_blocks, xcd_chunk;        // expected launch
    int n, nzone, ndepth;                             // expected normalised plan
    bool all_kinds;
};
static void check_named_plan(const Plan &p, Seen &seen) {
    const Launch L = matrix_launch(p.ny, p.row0, p.ny_global, p.xcd_rows, p.xcd_split);
    CHECK(L.ntiles == p.tiles && L.blocks == p.blocks && L.pole_blocks == p.pole_blocks && L.xcd_chunk == p.xcd_chunk,
          "%s: %d tiles, %d blocks, %d pole blocks, xcd_chunk %d", p.what, L.ntiles, L.blocks, L.pole_blocks, L.xcd_chunk);
    const Grading g = grading(p.total, p.chunk, p.zone, p.depth, L.blocks);
    CHECK(g.n == p.n && g.zone == p.nzone && g.depth == p.ndepth, "%s: n %d zone %d depth %d", p.what, g.n, g.zone, g.depth);
    check_plan(p.total, p.chunk, p.zone, p.depth, L.blocks, seen);
    RangesSeen rs;
    for (int order = 0; order <= 3; ++order) rs = check_composition(g, L, order, p.what);  // (which blocks hold a tile does not depend on the order)
    if (p.all_kinds) CHECK(rs.empty > 0 && rs.one > 0 && rs.longer > 0, "%s: %d empty, %d one-level, %d longer ranges", p.what, rs.empty, rs.one, rs.longer);
    if (g.zone > 0) CHECK(rs.longer > 0, "%s: no tile makes levels up", p.what);
    if (g.zone == 0) CHECK(rs.empty == 0 && rs.one == 0, "%s: a zeroed plan grades nothing", p.what);  // (every tile: [0, total) at once)
    std::printf("plan %-46s %3d tiles %3d + %d blocks xcd_chunk %2d: %d launches zone %2d depth %2d; tiles' ranges: %d empty, %d one-level, %d longer\n",
                p.what, L.ntiles, L.blocks, L.pole_blocks, L.xcd_chunk, g.zone > 0 ? g.n : 1, g.zone, g.depth, rs.empty, rs.one, rs.longer);
}

int main() {
    Seen seen;
    // exhaustive over small cases: every total, every launch count (through the chunk that gives it), every block count --
    // the multiples of 8 a grid is rounded up to among them -- and depths from none to more than a chunk
    for (int total = 1; total <= 70; ++total)
        for (int launches = 1; launches <= 5; ++launches) {
            const int chunk = (total + launches - 1) / launches;
            for (int blocks = 1; blocks <= 40; ++blocks)
                for (int zone : {0, 8, 16, 1000})
                    for (int depth : {0, 1, 2, chunk / 2, chunk - 1, chunk, chunk + 3}) check_plan(total, chunk, zone, depth, blocks, seen);
        }
    // grids of more blocks: zones of several eights, every launch count up to 5 graded
    for (int total : {1, 2, 5, 41, 64, 70, 96})
        for (int launches = 1; launches <= 5; ++launches) {
            const int chunk = (total + launches - 1) / launches;
            for (int blocks : {48, 56, 64, 72, 96, 136, 200, 512})
                for (int zone : {8, 16, 24, 64, 1000})
                    for (int depth : {1, chunk / 2, chunk - 1, chunk}) check_plan(total, chunk, zone, depth, blocks, seen);
        }
    CHECK(seen.graded > 1000 && seen.empty > 0 && seen.one > 0 && seen.longer > 0, "graded %ld empty %ld one-level %ld longer %ld", seen.graded,
          seen.empty, seen.one, seen.longer);
    // the plan of the GPU test (tests/test_gpu_level_grading.py): 41 levels in 3 launches of 14, 72 blocks, zone 8, depth 14 --
    // some ranges empty, some one level long
    {
        const Grading g = grading(41, 14, 8, 14, 72);
        CHECK(g.n == 3 && g.zone == 8 && g.depth == 14, "the GPU test's plan: n %d zone %d depth %d", g.n, g.zone, g.depth);
        int empty = 0, one = 0;
        for (int launch = 0; launch < g.n; ++launch)
            for (int d = 0; d < 72; ++d) {
                const Range r = graded_range(g, launch, d);
                empty += r.b == r.a;
                one += r.b - r.a == 1;
            }
        CHECK(empty > 0 && one > 0, "the GPU test's plan: %d empty ranges, %d of one level", empty, one);
    }
    // the plans of tests/test_gpu_level_grading_matrix.py, each by name: 41 levels (34 for the continuation), windows of a
    // 328-row global grid and the first 200 rows as a grid of their own, the default tile map (one tile row per chunk, split by
    // shape) and LCS_XCD_CHUNK_ROWS = 0 / 2, LCS_XCD_SPLIT = 0
    {
        const Plan plans[] = {
            //                                              ny row0  nyg rows split  total chunk zone depth  tiles blocks pole xcd   n zone depth
            {"200 rows (14, 8, 14)",                       200,   0, 200, 1, -1,      41, 14,    8, 14,      68,  72, 8,  3,     3,  8, 14, true},
            {"rows [0, 128) of 328 (14, 8, 14)",           128,   0, 328, 1, -1,      41, 14,    8, 14,      34,  48, 8,  3,     3,  8, 14, true},
            {"rows [64, 264) of 328 (14, 8, 14)",          200,  64, 328, 1, -1,      41, 14,    8, 14,      68,  72, 0,  3,     3,  8, 14, true},
            {"rows [100, 300) of 328 (14, 8, 14)",         200, 100, 328, 1, -1,      41, 14,    8, 14,      68,  72, 0,  3,     3,  8, 14, true},
            {"rows [128, 328) of 328 (14, 8, 14)",         200, 128, 328, 1, -1,      41, 14,    8, 14,      68,  72, 8,  3,     3,  8, 14, true},
            {"328 rows (14, 24, 14): three eights",        328,   0, 328, 1, -1,      41, 14,   24, 14,     102, 120, 8,  3,     3, 24, 14, true},
            {"200 rows (12, 8, 12): 4 launches",           200,   0, 200, 1, -1,      41, 12,    8, 12,      68,  72, 8,  3,     4,  8, 12, true},
            {"200 rows (9, 8, 9): 5 launches",             200,   0, 200, 1, -1,      41,  9,    8,  9,      68,  72, 8,  3,     5,  8,  9, true},
            {"200 rows (14, 8, 1)",                        200,   0, 200, 1, -1,      41, 14,    8,  1,      68,  72, 8,  3,     3,  8,  1, false},
            {"200 rows (14, 8, 20): depth capped",         200,   0, 200, 1, -1,      41, 14,    8, 20,      68,  72, 8,  3,     3,  8, 14, true},
            {"200 rows (14, 1000, 14): zone capped",       200,   0, 200, 1, -1,      41, 14, 1000, 14,      68,  72, 8,  3,     3,  8, 14, true},
            {"rows [0, 128) (9, 8, 9): zeroed",            128,   0, 328, 1, -1,      41,  9,    8,  9,      34,  48, 8,  3,     5,  0,  0, false},
            {"rows [100, 300) 34 levels (12, 8, 12)",      200, 100, 328, 1, -1,      34, 12,    8, 12,      68,  72, 0,  3,     3,  8, 12, true},
            {"contiguous bands (14, 8, 14)",               200, 100, 328, 0, -1,      41, 14,    8, 14,      68,  72, 0,  0,     3,  8, 14, true},
            {"contiguous bands (12, 8, 12)",               200,   0, 200, 0, -1,      41, 12,    8, 12,      68,  72, 8,  0,     4,  8, 12, true},
            {"two tile rows per chunk (14, 8, 14)",        200, 100, 328, 2, -1,      41, 14,    8, 14,      68,  80, 0,  5,     3,  8, 14, false},
            {"two tile rows per chunk (12, 8, 12)",        200,   0, 200, 2, -1,      41, 12,    8, 12,      68,  80, 8,  5,     4,  8, 12, true},
            {"whole tile rows (14, 8, 14)",                200, 100, 328, 1,  0,      41, 14,    8, 14,      68, 136, 0, 17,     3,  8, 14, false},
            {"whole tile rows (12, 8, 12)",                200,   0, 200, 1,  0,      41, 12,    8, 12,      68, 136, 8, 17,     4,  8, 12, true},
        };
        for (const Plan &p : plans) check_named_plan(p, seen);
        // LCS_POLE_BLOCKS = 0: no leading pole blocks whatever the rows (a grid that holds pole rows is then not graded: the dispatcher)
        CHECK(matrix_launch(200, 0, 200, 1, -1, false).pole_blocks == 0 && matrix_launch(200, 100, 328, 1, -1, false).pole_blocks == 0, "pole blocks off");
    }
    // the composition over every tile map the GPU file sets: xcd_chunk 0 (bands), 3 (default), 5 (two tile rows, split), 17
    // (whole rows), tile orders 0-3, 34 / 68 / 102 tiles in 17 tile columns, 3 / 4 / 5 launches with zones of one and three eights
    {
        bool chunk_seen[18] = {};
        long maps = 0;
        for (int ny : {128, 200, 328})
            for (int rs : {0, 1, 2, 3})  // (xcd_rows, xcd_split): bands; the default; two rows; whole rows
            {
                const Launch L = matrix_launch(ny, 0, ny, rs == 0 ? 0 : (rs == 2 ? 2 : 1), rs == 3 ? 0 : -1);
                CHECK(L.ntx == 17 && L.ntiles == 17 * ((ny + 63) / 64) && L.xcd_chunk >= 0 && L.xcd_chunk <= 17, "tile map of %d rows", ny);
                if (L.xcd_chunk >= 0 && L.xcd_chunk <= 17) chunk_seen[L.xcd_chunk] = true;
                for (int chunk : {14, 12, 9})
                    for (int zone : {8, 24, 1000})
                        for (int depth : {1, chunk / 2, chunk})
                            for (int order = 0; order <= 3; ++order) {
                                check_composition(grading(41, chunk, zone, depth, L.blocks), L, order, "tile-map sweep");
                                ++maps;
                            }
            }
        int n_chunks_seen = 0;
        for (bool b : chunk_seen) n_chunks_seen += b;
        CHECK(chunk_seen[0] && chunk_seen[3] && chunk_seen[5] && chunk_seen[17] && n_chunks_seen == 4, "xcd_chunk values of the sweep");
        std::printf("composition tile_of_block(graded_slot): %ld (plan, tile map, tile order) cases, xcd_chunk 0 / 3 / 5 / 17\n", maps);
    }
    // the headline call: 96 levels in chunks of 32, 32768 tiles
    {
        const Grading g = grading(96, 32, 3584, 32, 32768);
        CHECK(g.n == 3 && g.zone == 3584 && g.depth == 32 && graded_longest(g) == 64, "headline plan");
        check_plan(96, 32, 3584, 32, 32768, seen);
    }
    if (g_fail) {
        std::printf("%ld checks FAILED\n", g_fail);
        return 1;
    }
    std::printf("all checks passed (%ld plans, %ld graded)\n", seen.cases, seen.graded);
    return 0;
}
