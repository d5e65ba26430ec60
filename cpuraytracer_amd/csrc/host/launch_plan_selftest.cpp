// launch_plan_selftest.cpp -- the launch plan (rt_launch_plan.h) in a program of its own: no device, no Python, no files, no library.
// 200,000 generated launches; for every plan that is not refused it checks what the kernels rely on when they carve the dynamic LDS
// image (rt_kernels.h) and take their work from the queue:
//   * the image is a multiple of 16 bytes and at most a workgroup's 160 KiB; with a hit stash or a path cache it also stays within
//     the block's share of the CU (160 KiB / blocks per CU), and that region ends exactly where the image ends;
//   * outside the cell-grid and materials-through-L2 variants the parts the RT_VERBOSE line prints add up to the image;
//   * a hit-stash kernel gets 16..63 records and processes no more than it holds; materials go through L2 only under a stash;
//   * the chosen variant (and the unit kernels' scan) is in the list of instantiated ones (rt_trace_variants.h), has the launch's
//     workgroup size, and carries exactly in Mode::Carry;
//   * the grid is 1 .. CUs x blocks per CU, the static part of the queue ends within the launch's paths and the shards cover the rest.
// Exit status 0 only when all hold.  `make launch_plan_selftest_san` builds the same program under AddressSanitizer + UBSan.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "rt_launch_plan.h"

namespace {

uint64_t g_state = 0x9E3779B97F4A7C15ull;
uint32_t Next() {  // xorshift64*
    g_state ^= g_state >> 12;
    g_state ^= g_state << 25;
    g_state ^= g_state >> 27;
    return (uint32_t)((g_state * 0x2545F4914F6CDD1Dull) >> 32);
}
uint32_t Below(uint32_t n) { return Next() % n; }
bool Chance(uint32_t percent) { return Below(100) < percent; }
template <typename T, size_t N>
T Pick(const T (&a)[N]) {
    return a[Below((uint32_t)N)];
}

int g_failures = 0;
void Check(bool ok, const char* what, uint32_t caseNo) {
    if (ok) return;
    if (++g_failures <= 20) std::printf("FAIL case %u: %s\n", caseNo, what);
}

}  // namespace

int main() {
    using namespace rtplan;
    static const uint32_t kSmall[] = {4, 8, 64, 256, 400, 484, 680, 681, 682, 683, 684};
    static const uint32_t kAny[] = {4, 1000, 2044, 2047, 2048, 2049, 2052, 4096, 10004, 30000, 65532, 65535, 65536};
    static const uint32_t kTop[] = {1, 32, 33, 128};
    static const uint32_t kCells[][2] = {{1, 1}, {64, 64}, {240, 250}, {16, 16}};
    static const uint32_t kShadow[][4] = {{0, 0, 0, 0}, {16, 16, 500, 3}, {64, 64, 8000, 10}, {128, 128, 60000, 64}};
    static const uint32_t kThreads[] = {256, 512, 1024, 1024};
    static const uint32_t kBlocks[] = {1, 1, 2, 4};
    static const uint32_t kCap[] = {63, 63, 16, 15, 8};
    static const uint32_t kPaths[] = {0, 1, 64, 65, 1000000, 0xffffffffu};
    static const uint32_t kDepth[] = {6, 65535, 65536};
    static const uint32_t kQueue[] = {0, 0, 64, 200};
    const uint32_t nCases = 200000;
    uint32_t refused = 0, reached[kTraceVariantCount][2] = {};
    for (uint32_t c = 0; c < nCases; ++c) {
        SceneShape S;
        const bool small = Chance(50);
        S.n_padded = small ? Pick(kSmall) : (Chance(50) ? Pick(kAny) : 4 * (1 + Below(16384)));
        S.n_levels = small ? 1 : 1 + Below(3);
        // one level: the groups are the top level; more: the preparation builds levels until the top has at most 128 nodes
        S.top_cnt = (S.n_levels == 1 && Chance(30)) ? (S.n_padded / 4 > 1 ? S.n_padded / 4 - 1 : 1) : Pick(kTop);
        S.top_off = S.n_levels == 1 ? 0 : Below(12000);
        S.grid = Chance(small ? 25 : 40);
        if (S.grid) {
            const uint32_t* g = kCells[Below(4)];
            S.grid_nu = g[0], S.grid_nv = g[1];
        }
        S.grid_quant = Chance(75);
        const uint32_t* sg = kShadow[Below(4)];
        S.sg_enabled = sg[0] != 0;
        S.sg_nx = sg[0], S.sg_ny = sg[1], S.sg_nentries = sg[2], S.sg_nglobal = sg[3];
        S.mats16 = Chance(50);
        S.n_lights = Chance(50) ? 1 : (Chance(50) ? 0 : 3);
        Settings C;
        C.cuCount = Chance(50) ? 256 : 8;
        C.blocksPerCu = Pick(kBlocks);
        C.blockThreads = Pick(kThreads);
        C.useMfma = Chance(80), C.matsInLds = Chance(70), C.useRayCache = Chance(70), C.useStash = Chance(60), C.treeInLds = Chance(70);
        C.forceGlobal = Chance(15);
        Knobs K;
        K.mats16 = Below(3), K.matsL2 = Chance(70), K.stashCap = Pick(kCap), K.stashProcess = Chance(60) ? 63 : Below(64);
        K.gridQuant = Below(2), K.gridSgLds = Chance(30), K.queueBlock = Pick(kQueue), K.queueStatic = Chance(60) ? 1 : Below(3);
        Ask A;
        A.total_paths = Pick(kPaths), A.max_depth = Pick(kDepth);
        A.mode = Chance(small && !S.grid ? 30 : 5) ? Mode::Carry : Mode::Ordinary;

        const ScanOnlyPlan U = PlanScanOnly(S, C);
        Check(FindScanVariant(U.kernel) >= 0, "the unit kernels' scan is not instantiated", c);
        Check(U.tree_in_lds == 0 || U.kernel.kScan == 2, "tree_in_lds without the hierarchy scan (unit kernels)", c);
        const TracePlan P = PlanTrace(S, C, K, A);
        {
            // the launcher's account (rt_unit_last_trace_launch): the case it packs reads back as itself -- PlanPacked on those words
            // answers with the words of this very plan, refusals included
            uint32_t in[kCaseWords], viaCase[kPlanWords], direct[kPlanWords];
            PackCase(S, C, K, A, in);
            PackPlan(P, U, direct);
            Check(PlanPacked(in, viaCase) == 0 && std::memcmp(viaCase, direct, sizeof(direct)) == 0, "PlanPacked(PackCase(...)) is not PackPlan(PlanTrace(...))", c);
            Check(P.status != 0 || direct[25] == KernelWord(P.kernel), "word [25] is not the plan's kernel", c);
        }
        if (P.status != 0) {
            Check(P.refusal != Refusal::None && P.message != nullptr, "a refusal without its text", c);
            Check(P.refusal != Refusal::MatsL2NoStash, "materials through L2 were decided without the stash they are decided with", c);
            ++refused;
            continue;
        }
        const TraceKernelId& k = P.kernel;
        const uint32_t waves = C.blockThreads / 64;
        const size_t budget = kLdsPerCu / C.blocksPerCu;
        const size_t region = (size_t)waves * P.ray_cache_stride16 * 16;
        Check(P.ldsBytes % 16 == 0, "the image is not a multiple of 16 bytes", c);
        Check(P.ldsBytes <= kLdsPerCu, "the image exceeds 160 KiB", c);
        if (P.ray_cache_off16 != 0) {
            Check(P.ldsBytes <= budget, "an image with a stash or cache exceeds the block's share of the CU", c);
            Check((size_t)P.ray_cache_off16 * 16 + region == P.ldsBytes, "the stash or cache does not end where the image ends", c);
        } else {
            Check(P.ray_cache_stride16 == 0 && P.stash_cap == 0, "a stash or cache without a place", c);
        }
        if (!P.grid && !k.kMatsL2) {
            const size_t parts = P.candBytes + P.tablesBytes + P.leafBytes + P.opsBytes + P.sgBytes + P.treeBytes;
            Check((parts + 15) / 16 * 16 + (P.ray_cache_off16 ? region : 0) == P.ldsBytes, "the printed parts do not add up to the image", c);
        }
        if (k.kStash) {
            Check(P.stash_cap >= 16 && P.stash_cap <= 63, "a stash kernel with fewer than 16 or more than 63 records", c);
            Check(P.stash_process <= P.stash_cap, "more hits left unprocessed than the stash holds", c);
            Check(P.ray_cache_stride16 * 16 >= P.stash_cap * 19 * 4, "a wave's region is smaller than its stash", c);
        }
        Check(!k.kMatsL2 || k.kStash, "materials through L2 without the stash", c);
        const int row = FindTraceVariant(k);
        Check(row >= 0, "the chosen variant is not instantiated", c);
        Check(k.kThreads == (int)C.blockThreads, "the variant's workgroup size is not the launch's", c);
        Check(k.kCarry == (A.mode == Mode::Carry) && P.pipelines == k.kCarry, "carrying variant and mode disagree", c);
        Check(k.lights == (S.n_lights != 1), "the _lights twin and the number of lights disagree", c);
        Check(!k.kCache || P.ray_cache_off16 != 0, "a caching variant without a cache", c);
        Check(P.lastTraceSky == (k.kStash && k.kScan == 1 && !k.kCarry), "lastTraceSky is not kStash && kScan == 1 && !kCarry", c);
        const uint32_t maxBlocks = C.cuCount * C.blocksPerCu;
        Check(P.blocks >= 1 && P.blocks <= maxBlocks, "the grid is not 1 .. CUs x blocks per CU", c);
        if (A.mode == Mode::Ordinary) {
            const QueueCut& q = P.queue;
            Check(q.queue_block >= 64 && q.queue_block % 64 == 0, "queue blocks are not whole waves' worth of paths", c);
            Check(q.dyn_begin <= A.total_paths, "the static part of the queue ends beyond the paths", c);
            Check((uint64_t)q.dyn_begin + (uint64_t)q.dyn_blocks * q.queue_block >= A.total_paths, "the shards do not cover the paths", c);
        }
        if (row >= 0) ++reached[row][k.lights ? 1 : 0];
    }
    uint32_t nReached = 0;
    for (int r = 0; r < kTraceVariantCount; ++r) nReached += (reached[r][0] != 0) + (reached[r][1] != 0);
    std::printf("%u cases, %u refused, %u of %d kernel functions chosen\n", nCases, refused, nReached, 2 * kTraceVariantCount);
    Check(nReached == 2u * kTraceVariantCount, "not every instantiated function was chosen", nCases);
    if (g_failures) {
        std::printf("launch_plan_selftest: %d checks failed\n", g_failures);
        return 1;
    }
    std::printf("launch_plan_selftest: ok\n");
    return 0;
}
