// CPU unit test of the graded level counts in lagrangiancoherence_amd/csrc/launch_plan.h (lcplan::grading, graded_slot,
// graded_range): every tile's ranges over the launches of a call tile [0, total) in order, the longest range is bounded,
// the per-launch map of dispatch positions to slots is a bijection that keeps the XCD, and degenerate parameters are the
// uniform chunks.  Built by tests/test_level_grading.py with g++ -fsanitize=address,undefined.
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
