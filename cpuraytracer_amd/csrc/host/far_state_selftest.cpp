// far_state_selftest.cpp -- the far-hit-state rule of the launch plan (rt_launch_plan.h FarStateLean) in a program of its own: no
// device, no Python, no files, no library.  Directed cases first -- the stock scenes' shapes take their row's lean kernel; a disabled
// index, a path list, per-path traversal counts and RT_FAR_STATE=1 keep the far-hit state -- then 100,000 generated launches, on which
// the rule must be exactly: ordinary launch, light 0 has an index, no path list, no traversal counts, knob at rest, and the planned
// kernel is of the flat LDS hit-stash family; a lean launch never changes the plan, and every lean function is chosen.
// Exit status 0 only when all hold.  `make far_state_selftest_san` builds the same program under AddressSanitizer + UBSan.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "rt_launch_plan.h"

namespace {

uint64_t g_state = 0xD1B54A32D192ED03ull;
uint32_t Next() {  // xorshift64*
    g_state ^= g_state >> 12;
    g_state ^= g_state << 25;
    g_state ^= g_state >> 27;
    return (uint32_t)((g_state * 0x2545F4914F6CDD1Dull) >> 32);
}
uint32_t Below(uint32_t n) { return Next() % n; }
bool Chance(uint32_t percent) { return Below(100) < percent; }

int g_failures = 0;
void Check(bool ok, const char* what, uint32_t caseNo) {
    if (ok) return;
    if (++g_failures <= 20) std::printf("FAIL case %u: %s\n", caseNo, what);
}

// the cover scene as rt_scene_upload shapes it (488 spheres: 128 groups, a 36 x 59 index of 2,036 entries with the floor in its global
// list) under rt_create's defaults on a 256-CU device, at the benchmark's size
rtplan::SceneShape Cover() {
    rtplan::SceneShape S;
    S.n_padded = 516, S.n_levels = 1, S.top_cnt = 128, S.top_off = 0;
    S.sg_enabled = true, S.sg_nx = 36, S.sg_ny = 59, S.sg_nentries = 2036, S.sg_nglobal = 1;
    S.n_lights = 1;
    return S;
}
// grid10k (10,004 spheres: 2,504 groups in 102 x 102 cells, a 78 x 133 index of 40,038 entries): the cell-grid scan, tables in global memory
rtplan::SceneShape Grid10k() {
    rtplan::SceneShape S;
    S.n_padded = 10020, S.n_levels = 1, S.top_cnt = 2504, S.top_off = 0;
    S.grid = true, S.grid_nu = 102, S.grid_nv = 102, S.grid_quant = true;
    S.sg_enabled = true, S.sg_nx = 78, S.sg_ny = 133, S.sg_nentries = 40038, S.sg_nglobal = 1;
    S.n_lights = 1;
    return S;
}
rtplan::Settings Defaults() {
    rtplan::Settings C;
    C.cuCount = 256, C.blocksPerCu = 1, C.blockThreads = 1024;
    return C;
}

}  // namespace

int main() {
    using namespace rtplan;
    const Knobs K;
    const Ask picture{1200u * 800u * 128u, 50u, Mode::Ordinary};
    const FarStateAsk rest;
    uint32_t c = 0;
    // ---- directed: the stock scenes
    {
        const SceneShape S = Cover();
        const TracePlan P = PlanTrace(S, Defaults(), K, picture);
        Check(P.status == 0 && P.kernel.kLds && P.kernel.kScan == 1 && P.kernel.kStash && P.kernel.kMatsL2 && !P.kernel.lights, "cover does not plan the headline row", c);
        Check(FarStateLean(S, picture, P, rest), "cover, picture launch: not lean", c);
        for (uint32_t lights : {0u, 2u, 3u}) {  // the _lights twin: lean too (light 0's index exists whenever the list is not empty)
            SceneShape L = S;
            L.n_lights = lights;
            L.sg_enabled = lights != 0u;  // (an empty list has no light to index: rt_scene_prep.cpp PrepareScene)
            const TracePlan PL = PlanTrace(L, Defaults(), K, picture);
            Check(PL.status == 0 && PL.kernel.lights && FindLeanVariant(PL.kernel) >= 0, "cover with a light list: not a lean row's twin", c);
            Check(FarStateLean(L, picture, PL, rest) == (lights != 0u), "cover with a light list: lean exactly when light 0 has an index", c);
        }
        ++c;
        FarStateAsk f = rest;
        f.forceFull = true;
        Check(!FarStateLean(S, picture, P, f), "RT_FAR_STATE=1 does not force the far-hit state", c);
        ++c;
        f = rest, f.pathList = true;
        Check(!FarStateLean(S, picture, P, f), "a path list takes the lean kernel", c);
        ++c;
        f = rest, f.travOut = true;
        Check(!FarStateLean(S, picture, P, f), "a launch with trav_out takes the lean kernel", c);
        ++c;
        f = rest, f.shadowGrid = false;
        Check(!FarStateLean(S, picture, P, f), "RT_SHADOW_GRID=0 takes the lean kernel", c);
        ++c;
        SceneShape off = S;  // a disabled index: a light that is no direction, a scene the builder gives up on
        off.sg_enabled = false, off.sg_nx = off.sg_ny = off.sg_nentries = off.sg_nglobal = 0;
        const TracePlan Poff = PlanTrace(off, Defaults(), K, picture);
        Check(Poff.status == 0 && FindLeanVariant(Poff.kernel) >= 0 && !FarStateLean(off, picture, Poff, rest), "a scene without an index takes the lean kernel", c);
        ++c;
        const Ask carry{1200u * 800u, 50u, Mode::Carry};  // frame pipelining: the carrying kernel keeps its state
        const TracePlan Pc = PlanTrace(S, Defaults(), K, carry);
        Check(Pc.status == 0 && Pc.kernel.kCarry && !FarStateLean(S, carry, Pc, rest), "the frame-pipelining launch takes a lean kernel", c);
        ++c;
        Settings noStash = Defaults();
        noStash.useStash = false;
        const TracePlan Pn = PlanTrace(S, noStash, K, picture);
        Check(Pn.status == 0 && !Pn.kernel.kStash && !FarStateLean(S, picture, Pn, rest), "RT_STASH=0 takes a lean kernel", c);
        ++c;
        Knobs noL2 = K;  // the other two rows of the family
        noL2.matsL2 = 0;
        const TracePlan P17 = PlanTrace(S, Defaults(), noL2, picture);
        Check(P17.status == 0 && P17.kernel.kStash && !P17.kernel.kMatsL2 && P17.kernel.kHitLds && FarStateLean(S, picture, P17, rest), "RT_MATS_L2=0: not lean", c);
        Settings noMats = Defaults();
        noMats.matsInLds = false;
        const TracePlan P18 = PlanTrace(S, noMats, K, picture);
        Check(P18.status == 0 && P18.kernel.kStash && !P18.kernel.kHitLds && FarStateLean(S, picture, P18, rest), "RT_MATS_LDS=0: not lean", c);
        ++c;
    }
    {
        const SceneShape S = Grid10k();
        const TracePlan P = PlanTrace(S, Defaults(), K, picture);
        Check(P.status == 0 && P.kernel.kScan == 3 && !FarStateLean(S, picture, P, rest), "grid10k (cell-grid scan) takes a lean kernel", c);
        ++c;
        SceneShape T = S;
        T.grid = false, T.n_levels = 3, T.top_cnt = 40, T.top_off = 3128;  // laid out as a three-level hierarchy (RT_GRID=0)
        const TracePlan Pt = PlanTrace(T, Defaults(), K, picture);
        Check(Pt.status == 0 && Pt.kernel.kScan == 2 && !FarStateLean(T, picture, Pt, rest), "the hierarchy scan takes a lean kernel", c);
        ++c;
    }
    // ---- generated: the rule is exactly its statement, and it changes nothing of the plan
    static const uint32_t kSmall[] = {4, 8, 64, 256, 400, 484, 680, 681, 682, 683, 684, 2048, 10004};
    static const uint32_t kShadow[][4] = {{0, 0, 0, 0}, {16, 16, 500, 3}, {64, 64, 8000, 10}, {128, 128, 60000, 64}};
    static const uint32_t kThreads[] = {256, 512, 1024, 1024};
    uint32_t lean[kTraceLeanVariantCount][2] = {}, nLean = 0;
    const uint32_t nCases = 100000;
    for (uint32_t g = 0; g < nCases; ++g, ++c) {
        SceneShape S;
        S.n_padded = kSmall[Below(13)];
        S.n_levels = S.n_padded > 2048 ? 3 : 1;
        S.top_cnt = S.n_levels == 1 ? (S.n_padded / 4 > 1 ? S.n_padded / 4 - 1 : 1) : 40;
        if (S.top_cnt > 128 && S.n_levels == 1) S.top_cnt = 128;
        S.top_off = S.n_levels == 1 ? 0 : 3000;
        S.grid = Chance(20);
        if (S.grid) S.grid_nu = S.grid_nv = 64;
        const uint32_t* sg = kShadow[Below(4)];
        S.sg_enabled = sg[0] != 0;
        S.sg_nx = sg[0], S.sg_ny = sg[1], S.sg_nentries = sg[2], S.sg_nglobal = sg[3];
        S.n_lights = Chance(50) ? 1 : (Chance(50) ? 0 : 3);
        Settings C;
        C.cuCount = 256, C.blocksPerCu = Chance(70) ? 1 : 2, C.blockThreads = kThreads[Below(4)];
        C.useMfma = Chance(85), C.matsInLds = Chance(70), C.useRayCache = Chance(70), C.useStash = Chance(75), C.forceGlobal = Chance(10);
        Knobs Kn;
        Kn.matsL2 = Chance(70);
        Ask A;
        A.total_paths = Chance(80) ? 1000000u : Below(200), A.max_depth = Chance(90) ? 50 : 65536;
        A.mode = Chance(10) ? Mode::Carry : Mode::Ordinary;
        FarStateAsk F;
        F.pathList = Chance(15), F.travOut = F.pathList && Chance(80), F.shadowGrid = Chance(90), F.forceFull = Chance(15);
        const TracePlan P = PlanTrace(S, C, Kn, A);
        const bool isLean = FarStateLean(S, A, P, F);
        if (P.status != 0) {
            Check(!isLean, "a refused launch is lean", c);
            continue;
        }
        const TraceKernelId& k = P.kernel;
        const bool family = k.kLds && k.kScan == 1 && k.kStash && !k.kCarry;
        Check(family == (FindLeanVariant(k) >= 0), "the lean list is not the flat LDS hit-stash family", c);
        const bool want = A.mode == Mode::Ordinary && family && S.sg_enabled && F.shadowGrid && !F.pathList && !F.travOut && !F.forceFull;
        Check(isLean == want, "FarStateLean is not its statement", c);
        Check(!isLean || (k.kThreads == 1024 && P.stash_cap >= 16 && P.lastTraceSky), "a lean launch without the stash kernel's plan", c);
        {
            // the packed form (rt_unit_far_state_plan) agrees, and the plan's words know nothing of the choice
            uint32_t in[kCaseWords], a[kPlanWords], b[kPlanWords];
            PackCase(S, C, Kn, A, in);
            Check(FarStateLeanPacked(in, F) == isLean, "FarStateLeanPacked(PackCase(...)) is not FarStateLean(...)", c);
            PackPlan(P, PlanScanOnly(S, C), a);
            Check(PlanPacked(in, b) == 0 && std::memcmp(a, b, sizeof(a)) == 0, "the plan's words changed", c);
        }
        if (isLean) {
            ++lean[FindLeanVariant(k)][k.lights ? 1 : 0];
            ++nLean;
        }
    }
    uint32_t nReached = 0;
    for (int r = 0; r < kTraceLeanVariantCount; ++r) nReached += (lean[r][0] != 0) + (lean[r][1] != 0);
    std::printf("%u generated cases, %u lean, %u of %d lean kernel functions chosen\n", nCases, nLean, nReached, 2 * kTraceLeanVariantCount);
    Check(nReached == 2u * kTraceLeanVariantCount, "not every lean function was chosen", c);
    if (g_failures) {
        std::printf("far_state_selftest: %d checks failed\n", g_failures);
        return 1;
    }
    std::printf("far_state_selftest: ok\n");
    return 0;
}
