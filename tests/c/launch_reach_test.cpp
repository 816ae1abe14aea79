// CPU unit test of what the deferred pack takes from lagrangiancoherence_amd/csrc/launch_plan.h:
//   lcplan::launch_reach    exhaustively over small (total, chunk, zone, depth, blocks): no slot's range in launch i ends above
//                           launch_reach(i), and some slot attains it; uniform chunks are min(total, (i + 1) chunk);
//   lcplan::pack_mix / pack_mix_block    the blocks of a launch that carries pack workgroups: every advect position d appears
//                           exactly once with d % 8 == block % 8, every pack workgroup index exactly once, the pack
//                           workgroups come in groups of 8 consecutive blocks, no block is left over;
//   lcplan::pack_items      workgroup p of P taking the items p, p + P, ... covers every (x chunk, padded row, level group)
//                           exactly once, for item counts that are no multiple of P; the level groups cover the levels.
// Built by tests/test_launch_reach.py with g++ -fsanitize=address,undefined.
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

static long g_plans = 0, g_graded = 0, g_outwards = 0;

static void check_reach(int total, int chunk, int zone, int depth, int blocks) {
    const Grading g = grading(total, chunk, zone, depth, blocks);
    ++g_plans;
    g_graded += g.zone > 0;
    int before = 0;
    for (int i = 0; i < g.n; ++i) {
        const int reach = launch_reach(total, chunk, g, i);
        int top = -1;
        for (int d = 0; d < blocks; ++d) {
            const Range r = graded_range(g, i, d);
            if (r.b > top) top = r.b;
            CHECK(r.b <= reach, "launch %d position %d ends at level %d, reach %d (total %d chunk %d zone %d depth %d blocks %d)", i, d, r.b, reach, total,
                  chunk, g.zone, g.depth, blocks);
        }
        CHECK(top == reach, "launch %d: no slot attains the reach %d (highest end %d; total %d chunk %d zone %d depth %d blocks %d)", i, reach, top, total, chunk,
              g.zone, g.depth, blocks);
        CHECK(reach >= before && reach <= total, "reach %d after %d of %d levels", reach, before, total);
        // the pole workgroups go by the launch's uniform range: inside the reach too
        CHECK(imin(total, (i + 1) * chunk) <= reach, "launch %d: the uniform chunk ends above the reach %d", i, reach);
        if (g.zone == 0) CHECK(reach == imin(total, (i + 1) * chunk), "uniform launch %d reaches %d", i, reach);
        g_outwards += reach > (i + 1) * chunk;
        before = reach;
    }
    CHECK(launch_reach(total, chunk, g, g.n - 1) == total, "the last launch reaches %d of %d", launch_reach(total, chunk, g, g.n - 1), total);
}

static void check_mix(int adv_blocks, int pack_per_period, int shift) {
    const PackMix m = pack_mix(adv_blocks, pack_per_period, shift);
    CHECK(m.na == (1 << shift) - pack_per_period && m.shift == shift && m.na % XCDS == 0 && m.na > 0, "na %d", m.na);
    CHECK(m.grid == adv_blocks + m.pack_blocks && m.pack_blocks % XCDS == 0, "grid %d = %d + %d", m.grid, adv_blocks, m.pack_blocks);
    std::vector<int> adv(adv_blocks, 0), pack(m.pack_blocks, 0);
    int run = 0;   // consecutive pack blocks so far
    for (int b = 0; b < m.grid; ++b) {
        int idx = -1;
        const bool is_pack = pack_mix_block(b, m.na, m.shift, idx);
        if (is_pack) {
            CHECK(idx >= 0 && idx < m.pack_blocks, "block %d: pack index %d of %d", b, idx, m.pack_blocks);
            if (idx >= 0 && idx < m.pack_blocks) ++pack[idx];
            ++run;
        } else {
            CHECK(idx >= 0 && idx < adv_blocks, "block %d: position %d of %d", b, idx, adv_blocks);
            if (idx >= 0 && idx < adv_blocks) ++adv[idx];
            CHECK(idx % XCDS == b % XCDS, "block %d (XCD %d) runs position %d (XCD %d)", b, b % XCDS, idx, idx % XCDS);
            CHECK(run % XCDS == 0, "a run of %d pack blocks ends at block %d", run, b);
            run = 0;
        }
    }
    CHECK(run == 0 || adv_blocks % m.na == 0, "the launch ends on %d pack blocks after a partial period", run);
    for (int d = 0; d < adv_blocks; ++d) CHECK(adv[d] == 1, "position %d taken %d times (%d blocks, %d pack per period)", d, adv[d], adv_blocks, pack_per_period);
    for (int p = 0; p < m.pack_blocks; ++p) CHECK(pack[p] == 1, "pack workgroup %d taken %d times", p, pack[p]);
}

static void check_items(int ny_f, int nx_f, int levels, int item_levels, int P) {
    const PackItems it = pack_items(ny_f, nx_f, 3, levels, item_levels);
    CHECK(it.xchunks * 256 >= nx_f + 3 && (it.xchunks - 1) * 256 < nx_f + 3 && it.rows == ny_f + 3, "%d x chunks, %d rows", it.xchunks, it.rows);
    CHECK(it.groups * item_levels >= levels && (it.groups - 1) * item_levels < levels, "%d groups of %d for %d levels", it.groups, item_levels, levels);
    CHECK(it.n == it.xchunks * it.rows * it.groups, "%d items", it.n);
    std::vector<int> seen(it.n, 0);
    for (int p = 0; p < P; ++p)
        for (int item = p; item < it.n; item += P) {
            // the kernel's decomposition (advect.hip: pack_items_run)
            const int rest = item / it.xchunks, xc = item - rest * it.xchunks, g = rest / it.rows, py = rest - g * it.rows;
            CHECK(xc >= 0 && xc < it.xchunks && py >= 0 && py < it.rows && g >= 0 && g < it.groups, "item %d -> (%d, %d, %d)", item, xc, py, g);
            const int key = (g * it.rows + py) * it.xchunks + xc;
            if (key >= 0 && key < it.n) ++seen[key];
        }
    for (int k = 0; k < it.n; ++k) CHECK(seen[k] == 1, "item %d covered %d times (P = %d)", k, seen[k], P);
}

int main() {
    for (int total = 1; total <= 40; ++total)
        for (int chunk = 1; chunk <= 14; ++chunk)
            for (int blocks : {8, 40, 64, 96, 200})
                for (int zone : {0, 8, 16, 24, 1000})
                    for (int depth : {0, 1, 3, chunk / 2, chunk, chunk + 5}) check_reach(total, chunk, zone, depth, blocks);
    // the headline call (97 levels in chunks of 32, 32768 workgroups, the default zone of 21 per compute unit) and the GPU test's
    check_reach(96, 32, 21 * 256, 32, 32768);
    check_reach(71, 32, 21 * 256, 32, 512);
    check_reach(40, 32, 21 * 256, 32, 512);
    {
        const Grading g = grading(96, 32, 21 * 256, 32, 32768);
        CHECK(launch_reach(96, 32, g, 0) == 32 && launch_reach(96, 32, g, 1) == 96 && launch_reach(96, 32, g, 2) == 96, "the headline call's reaches");
        const Grading h = grading(40, 32, 21 * 256, 32, 512);
        CHECK(h.zone > 0 && launch_reach(40, 32, h, 0) == 40, "two launches: the first reaches past its chunk (%d)", launch_reach(40, 32, h, 0));
    }
    std::printf("launch_reach: %ld plans, %ld graded, %ld launches that reach past their chunk\n", g_plans, g_graded, g_outwards);
    CHECK(g_graded > 1000 && g_outwards > 1000, "the sweep does not reach the graded cases");

    for (int shift = PACK_SHIFT_MIN; shift <= PACK_SHIFT_MAX; ++shift)
        for (int pack = 8; pack <= 24; pack += 8)
            for (int adv = 0; adv <= 2560; adv += (adv < 520 ? 8 : 136)) check_mix(adv, pack, shift);
    check_mix(32768, 8, 5);
    check_mix(32768, 8, 7);
    check_mix(131072, 8, 14);
    // the period by the pack's size: the headline call (64 levels in items of 8: 6 x 723 x 8 items) takes a period of 64, a launch of
    // 8192^2 seeds that carries 32 levels one of 512; never more pack workgroups than items / 7 unless the shortest period has fewer
    {
        const PackMix c3 = pack_mix_for_items(32768, 8, 6 * 723 * 8), c4 = pack_mix_for_items(131072, 8, 6 * 723 * 4);
        CHECK(c3.shift == 6 && c3.pack_blocks == 4680, "the headline call: period %d, %d pack workgroups", 1 << c3.shift, c3.pack_blocks);
        CHECK(c4.shift == 9 && c4.pack_blocks == 2080, "8192^2 seeds, 32 levels: period %d, %d pack workgroups", 1 << c4.shift, c4.pack_blocks);
        for (int adv = 24; adv <= 4096; adv += 8)
            for (int items : {1, 64, 255, 1000, 40000}) {
                const PackMix m = pack_mix_for_items(adv, 8, items);
                CHECK(m.pack_blocks > 0 && m.shift >= PACK_SHIFT_MIN && m.shift <= PACK_SHIFT_MAX, "%d blocks, %d items: %d pack workgroups", adv, items, m.pack_blocks);
                CHECK(m.pack_blocks <= imax(items / PACK_ITEMS_PER_WG, 8) || pack_mix(adv, 8, m.shift + 1).pack_blocks <= 0 || m.shift == PACK_SHIFT_MAX,
                      "%d blocks, %d items: %d pack workgroups at period %d", adv, items, m.pack_blocks, 1 << m.shift);
            }
    }
    std::printf("pack_mix: every advect position and every pack workgroup once, XCD kept\n");

    for (int P : {8, 16, 56, 136})
        for (int item_levels : {2, 4, 8})
            for (int levels : {1, 2, 7, 39, 64}) {
                check_items(48, 96, levels, item_levels, P);
                check_items(5, 300, levels, item_levels, P);     // two x chunks
                check_items(36, 72, levels, item_levels, P);
            }
    std::printf("pack_items: every item once\n");
    if (g_fail) {
        std::printf("%ld checks FAILED\n", g_fail);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
