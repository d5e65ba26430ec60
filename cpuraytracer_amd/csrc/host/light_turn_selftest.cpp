// light_turn_selftest.cpp -- the host piece of rt_turn_lights in a program of its own: no device, no Python.
//   rt_turn_lights rebuilds the shadow indices with rtprep::PrepareShadows over the part of the layout it kept from the upload
//   (rtprep::ShadowLayoutOf).  For random scenes of every layout kind (flat, hierarchy, cell grid; negative radii included), 0 to 3
//   lights and three consecutive turns each: PrepareShadows over the layout kept from PrepareScene(spheres, lights A) equals the shadow
//   members of a fresh PrepareScene(spheres, lights B) -- shadow, extraShadow, shadowFar, sgSph -- byte for byte, and every table of an
//   enabled index stays inside the bounds the upload reserves (rt_scene_prep.h kShadow...).  The staging plan of every turn, and of the
//   scene's material tables, lies inside the slot sized from the upload alone (rt_scene_edit.h StageBytesMax), every table inside its
//   room and on a 16-byte boundary; the largest plan / slot ratio is printed and must not be zero.
//   The builder's branches are counted (rtprep::ShadowBuildCounts) and the program fails where one that a scene can reach stayed at
//   zero.  "Only huge spheres" is counted, reported and must stay at ZERO: the median radius is the radius of some sphere, and that
//   sphere is not huge (r <= 4 median), so the branch cannot be reached by any scene; the directed scenes below try.
// Exit status 0 and a summary, or the first failed condition and status 1.  Also built with AddressSanitizer and UBSan
// (make light_turn_selftest_san).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../../include/rt_api.h"
#include "rt_scene_edit.h"
#include "rt_scene_prep.h"

using namespace rtprep;

namespace {

struct Rng {  // splitmix64
    uint64_t s;
    uint64_t next() {
        uint64_t z = (s += 0x9e3779b97f4a7c15ull);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        return z ^ (z >> 31);
    }
    uint32_t below(uint32_t n) { return (uint32_t)(next() % n); }
    float uni(float lo, float hi) { return lo + (hi - lo) * (float)((next() >> 40) * (1.0 / 16777216.0)); }
};

uint32_t g_case = 0;
#define CHECK(cond)                                                                          \
    do {                                                                                     \
        if (!(cond)) {                                                                       \
            std::printf("FAILED case %u: %s (%s:%d)\n", g_case, #cond, __FILE__, __LINE__); \
            std::exit(1);                                                                    \
        }                                                                                    \
    } while (0)

// kind 0: scattered, few enough for the flat scan; 1: scattered, more groups than treeTop takes (the hierarchy); 2: a uniform layer of
// small spheres under a few big ones (the cell grid); 3: 16,500 spheres of two sizes on a 256 x 256 patch, whose footprints at 256
// cells per axis make 65,535 entries and more (the halving rule); 4: a cluster among 70 far larger spheres, all of which spill (the
// give-up rule: a global list beyond 64); 5: sizes chosen to come as close to "only huge spheres" as a scene can
std::vector<rt_sphere> MakeSpheres(uint32_t kind, Rng& rng, PrepOptions& opt) {
    std::vector<rt_sphere> sp;
    auto sign = [&]() { return rng.below(4) == 0 ? -1.f : 1.f; };
    if (kind == 0) {
        const uint32_t n = 1 + rng.below(rng.below(4) == 0 ? 200 : 24);
        for (uint32_t k = 0; k < n; ++k) sp.push_back({rng.uni(-9.f, 9.f), rng.uni(-9.f, 9.f), rng.uni(-9.f, 9.f), sign() * rng.uni(0.1f, 1.2f)});
        if (n > 2 && rng.below(3) == 0) sp[rng.below(n)].r = -30.f;
    } else if (kind == 1) {
        opt.treeTop = 4u + rng.below(5);  // 4 .. 8 groups of four at the top: 40 spheres and more need levels below it
        opt.grid = false;
        const uint32_t n = 40 + rng.below(80);
        for (uint32_t k = 0; k < n; ++k) sp.push_back({rng.uni(-12.f, 12.f), rng.uni(-12.f, 12.f), rng.uni(-12.f, 12.f), sign() * rng.uni(0.1f, 0.6f)});
        if (rng.below(2) == 0) sp[rng.below(n)].r = -50.f;
    } else if (kind == 2) {
        opt.treeTop = 16u;
        sp.push_back({0.f, -1000.f, 0.f, 1000.f});
        sp.push_back({-4.f, 1.f, 0.f, -1.f});
        const int half = 8 + (int)rng.below(3);  // 256 small spheres, the fewest the grid takes, to 400
        for (int a = -half; a < half; ++a)
            for (int b = -half; b < half; ++b) sp.push_back({(float)a + rng.uni(0.f, 0.9f), 0.2f, (float)b + rng.uni(0.f, 0.9f), 0.2f * sign()});
    } else if (kind == 3) {
        // (more than 4,096 groups: the layout skips its pairwise refinement, which would cost seconds here; the index stays in global
        // memory, 256 cells per axis allowed, and an entry count of 65,535 and more at 256 and at 128 cells halves the limit twice)
        for (uint32_t k = 0; k < 16500; ++k) sp.push_back({rng.uni(-128.f, 128.f), rng.uni(0.f, 1.f), rng.uni(-128.f, 128.f), (k & 1u) ? 1.6f : 0.4f});
        sp[1].r = 0.4f;  // (the small ones are the majority: the median is theirs)
    } else if (kind == 4) {
        for (uint32_t k = 0; k < 200; ++k) sp.push_back({rng.uni(-2.f, 2.f), rng.uni(-2.f, 2.f), rng.uni(-2.f, 2.f), 0.1f});
        for (uint32_t k = 0; k < 70; ++k) sp.push_back({rng.uni(-40.f, 40.f), rng.uni(-40.f, 40.f), rng.uni(-40.f, 40.f), sign() * 1.f});
    } else {
        const uint32_t n = 1 + rng.below(9), tiny = rng.below(n + 1);
        for (uint32_t k = 0; k < n; ++k) sp.push_back({rng.uni(-5.f, 5.f), rng.uni(-5.f, 5.f), rng.uni(-5.f, 5.f), k < tiny ? (rng.below(2) ? 0.f : 1e-6f) : sign() * rng.uni(50.f, 500.f)});
    }
    return sp;
}

// A light record of one of the classes of direction a caller can hand over
enum DirClass { kRandomUnit, kXDominates, kStraightDown, kGrazing, kUnnormalised, kNoDirection, kDirClasses };
rt_light MakeLight(uint32_t cls, Rng& rng) {
    rt_light l{};
    float d[3] = {rng.uni(-1.f, 1.f), rng.uni(-1.f, 1.f), rng.uni(-1.f, 1.f)};
    float len = 1.f;
    if (cls == kXDominates) d[0] = rng.below(2) ? 3.f : -3.f;
    if (cls == kStraightDown) d[0] = 0.f, d[1] = 1.f, d[2] = 0.f;
    if (cls == kGrazing) d[0] = 1.f, d[1] = 0.05f, d[2] = rng.below(2) ? 0.f : rng.uni(-0.2f, 0.2f);
    if (cls == kUnnormalised) len = rng.uni(0.55f, 1.9f);
    if (cls == kNoDirection) len = rng.below(3) == 0 ? 0.f : (rng.below(2) ? 3.f : 0.2f);
    const float n = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    for (int c = 0; c < 3; ++c) {
        l.direction[c] = n > 0.f ? d[c] / n * len : (c == 1 ? len : 0.f);
        l.color[c] = rng.uni(0.f, 1.f);
    }
    l.luminance = rng.uni(0.f, 10.f);
    return l;
}

template <typename T>
bool SameBytes(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}
bool SameGrid(const ShadowGrid& a, const ShadowGrid& b) {
    return SameBytes(a.cellStart, b.cellStart) && SameBytes(a.entries, b.entries) && SameBytes(a.global, b.global) && a.nx == b.nx && a.ny == b.ny &&
           std::memcmp(a.e1, b.e1, sizeof a.e1) == 0 && std::memcmp(a.e2, b.e2, sizeof a.e2) == 0 && std::memcmp(&a.u0, &b.u0, 4) == 0 &&
           std::memcmp(&a.v0, &b.v0, 4) == 0 && std::memcmp(&a.invCell, &b.invCell, 4) == 0 && std::memcmp(&a.p0sq, &b.p0sq, 4) == 0 && a.enabled == b.enabled;
}
// an enabled index inside what the upload reserves for an index of `maxCells` cells per axis
void CheckBounds(const ShadowGrid& G, uint32_t maxCells) {
    if (!G.enabled) return;  // (a disabled index is not copied anywhere)
    CHECK(G.nx >= 1 && G.ny >= 1 && G.nx <= maxCells && G.ny <= maxCells);
    CHECK(G.cellStart.size() == (size_t)G.nx * G.ny + 1 && G.cellStart.size() <= ShadowCellWordsMax(maxCells));
    CHECK(G.entries.size() < kShadowEntriesEnd && G.global.size() <= kShadowGlobalMax);
    CHECK(G.cellStart.back() == G.entries.size());
}

// ... and the same through the staging plan (rt_scene_edit.h): every table inside the room reserved for an index of `maxCells` cells per
// axis, on a 16-byte boundary of the slot, and the whole plan inside the slot as the upload sized it
rtscene::IndexDest RoomAt(uint32_t maxCells) {
    const rtscene::ShadowRoom r = rtscene::ShadowRoomOf(maxCells);
    return {{nullptr, r.cellWords * sizeof(uint16_t)}, {nullptr, r.entries * sizeof(uint16_t)}, {nullptr, r.global * sizeof(uint16_t)}};
}
uint32_t g_plans = 0, g_emptyPlans = 0;
void CheckPlan(const rtscene::StagePlan& plan, size_t slotBytes, double& largestRatio) {
    CHECK(plan.status == RT_OK);
    size_t at = 0;
    for (const rtscene::StageItem& it : plan.items) {
        CHECK(it.bytes <= it.dst.room && it.offset % 16 == 0 && it.offset >= at);
        at = it.offset + it.bytes;
    }
    CHECK(at <= plan.total && plan.total <= slotBytes);
    ++g_plans, g_emptyPlans += plan.total == 0;
    const double ratio = (double)plan.total / (double)slotBytes;
    largestRatio = ratio > largestRatio ? ratio : largestRatio;
}

}  // namespace

int main() {
    Rng rng{20261021};
    const uint32_t kCases = 800;  // x 3 turns: 2,400 scene x direction comparisons, each against a fresh PrepareScene
    uint32_t kinds[3] = {0, 0, 0}, lightCounts[4] = {0, 0, 0, 0}, tier2On = 0, tier2Off = 0, offOnOff = 0, onOffOn = 0, sgSphTables = 0, oneByOne = 0, turns = 0;
    uint32_t shapeChanged = 0, grew = 0;
    double turnRatio = 0.0, materialRatio = 0.0;  // largest staging plan / slot
    ShadowBuildCounts counts;
    for (g_case = 0; g_case < kCases; ++g_case) {
        uint32_t want = g_case % 10 < 6 ? 0u : (g_case % 10 < 8 ? 1u : 2u);
        if (g_case % 400 == 7) want = 3u;
        if (g_case % 50 == 13) want = 4u;
        if (g_case % 20 == 5) want = 5u;
        PrepOptions opt;
        const std::vector<rt_sphere> sp = MakeSpheres(want, rng, opt);
        const uint32_t n = (uint32_t)sp.size();
        opt.sgSph = rng.below(4) == 0;
        if (rng.below(8) == 0) opt.shadowCellsGlobal = 32u << rng.below(3);  // 32, 64, 128 in place of 256
        CHECK(AllFinite(sp.data(), n, nullptr));
        const std::vector<rt_material> mats(n, rt_material{});
        const uint32_t nl = want == 3u ? 1u : rng.below(4);
        ++lightCounts[nl];
        auto lights = [&](bool mayBeNoDirection) {
            std::vector<rt_light> ls(nl);
            for (rt_light& l : ls) {
                uint32_t cls = rng.below(kDirClasses);
                if (cls == kNoDirection && !mayBeNoDirection) cls = kRandomUnit;
                l = MakeLight(cls, rng);
            }
            return ls;
        };
        const std::vector<rt_light> A = lights(true);
        const PreparedScene PA = PrepareScene(sp.data(), mats.data(), n, A.data(), nl, opt);
        const SceneLayout& L = PA.layout;
        CHECK(L.scan.size() < 65536 && L.orig.size() == L.scan.size());
        ++kinds[L.gridOn ? 2u : (L.nLevels > 1 ? 1u : 0u)];
        const SceneLayout kept = ShadowLayoutOf(L, opt);  // what the context keeps, and nothing else of the layout
        CHECK(kept.scan.empty() || (opt.sgSph && L.InGlobalMemory()));
        CHECK(kept.leaf.empty() && kept.tree.empty() && kept.gridCellStart.empty() && kept.InGlobalMemory() == L.InGlobalMemory());
        const uint32_t cells0 = L.InGlobalMemory() ? opt.shadowCellsGlobal : opt.shadowCellsLds;
        // the slot, from the upload alone; the material tables of the scene fit it too
        rtscene::StageShape shape;
        shape.nPad = L.scan.size(), shape.n = n, shape.nIdx = opt.shadowGrid ? nl : 0u, shape.inGlobalMemory = L.InGlobalMemory();
        const size_t slotBytes = rtscene::StageBytesMax(shape, opt);
        const std::vector<rtscene::IndexDest> extraRoom(nl, RoomAt(opt.shadowCellsGlobal));
        const rtscene::TableDest sgSphRoom{nullptr, opt.sgSph && L.InGlobalMemory() ? kShadowSphRecordsMax * sizeof(F4) : 0};
        const PreparedMaterials M = PrepareMaterials(mats.data(), n, L.orig.data(), L.orig.size());
        CheckPlan(rtscene::PlanMaterialStage(M, {nullptr, L.orig.size() * sizeof(rt_material)}, {nullptr, L.orig.size() * sizeof(U4)}, {nullptr, n * sizeof(uint32_t)}),
                  slotBytes, materialRatio);
        bool was[4] = {PA.shadow.enabled, false, false, false};
        ShadowGrid before = PA.shadow;
        for (uint32_t t = 1; t <= 3; ++t, ++turns) {
            // the middle turn of every third scene has no direction for light 0: on -> off -> on across consecutive turns
            std::vector<rt_light> B = lights(true);
            if (nl != 0 && g_case % 3 == 0) B[0] = MakeLight(t == 2 ? (uint32_t)kNoDirection : (uint32_t)kRandomUnit, rng);
            const PreparedShadows S = PrepareShadows(sp.data(), kept, B.data(), nl, opt, &counts);
            const PreparedScene PB = PrepareScene(sp.data(), mats.data(), n, B.data(), nl, opt);
            CHECK(SameBytes(PB.layout.orig, L.orig));  // the layout does not look at the lights
            CHECK(SameGrid(S.shadow, PB.shadow));
            CHECK(S.extraShadow.size() == PB.extraShadow.size() && S.extraShadow.size() == (nl > 1 ? nl - 1 : 0));
            for (size_t k = 0; k < S.extraShadow.size(); ++k) CHECK(SameGrid(S.extraShadow[k], PB.extraShadow[k]));
            CHECK(SameGrid(S.shadowFar, PB.shadowFar));
            CHECK(SameBytes(S.sgSph, PB.sgSph));
            // ... and inside the reservation
            CheckBounds(S.shadow, cells0);
            for (const ShadowGrid& G : S.extraShadow) CheckBounds(G, opt.shadowCellsGlobal);
            CheckBounds(S.shadowFar, opt.shadowCellsGlobal);
            CHECK(S.sgSph.size() <= kShadowSphRecordsMax && (S.sgSph.empty() || (S.shadow.enabled && S.sgSph.size() == S.shadow.entries.size() + 1)));
            CHECK(!S.shadowFar.enabled || S.shadow.enabled);  // the far tier exists only with light 0's first index
            CheckPlan(rtscene::PlanShadowStage(S, RoomAt(cells0), extraRoom.data(), RoomAt(opt.shadowCellsGlobal), sgSphRoom), slotBytes, turnRatio);
            sgSphTables += !S.sgSph.empty();
            tier2On += S.shadowFar.enabled;
            tier2Off += S.shadow.enabled && !S.shadowFar.enabled;
            oneByOne += S.shadow.enabled && S.shadow.nx == 1 && S.shadow.ny == 1;
            if (S.shadow.enabled && before.enabled) {
                shapeChanged += S.shadow.nx != before.nx || S.shadow.ny != before.ny;
                grew += S.shadow.entries.size() > before.entries.size() || S.shadow.cellStart.size() > before.cellStart.size();
            }
            was[t] = S.shadow.enabled;
            before = S.shadow;
        }
        for (int t = 0; t < 2; ++t) {
            onOffOn += was[t] && !was[t + 1] && was[t + 2];
            offOnOff += !was[t] && was[t + 1] && !was[t + 2];
        }
    }
    g_case = kCases;
    std::printf("light turns: %u scenes (flat %u, hierarchy %u, cell grid %u; 0/1/2/3 lights %u/%u/%u/%u), %u turns, %llu indices built\n", kCases, kinds[0],
                kinds[1], kinds[2], lightCounts[0], lightCounts[1], lightCounts[2], lightCounts[3], turns, (unsigned long long)counts.built);
    std::printf("branches: basis switch %llu, spilled %llu, wide %llu, only huge %llu, tier 2 on %u, tier 2 off %u (by its radius %llu), no direction %llu, "
                "on-off-on %u, off-on-off %u, enabled %llu\n",
                (unsigned long long)counts.basisSwitch, (unsigned long long)counts.spilled, (unsigned long long)counts.wide, (unsigned long long)counts.onlyHuge,
                tier2On, tier2Off, (unsigned long long)counts.noTier2, (unsigned long long)counts.notADirection, onOffOn, offOnOff,
                (unsigned long long)counts.enabled);
    std::printf("rules: halved %llu, gave up %llu; 1 x 1 grids %u, sgSph tables %u, turns that changed nx or ny %u, turns that grew a table %u\n",
                (unsigned long long)counts.halved, (unsigned long long)counts.gaveUp, oneByOne, sgSphTables, shapeChanged, grew);
    CHECK(kinds[0] > 0 && kinds[1] > 0 && kinds[2] > 0);
    CHECK(lightCounts[0] > 0 && lightCounts[1] > 0 && lightCounts[2] > 0 && lightCounts[3] > 0);
    CHECK(counts.basisSwitch > 0 && counts.spilled > 0 && counts.wide > 0);
    CHECK(tier2On > 0 && tier2Off > 0 && counts.noTier2 > 0);
    CHECK(counts.notADirection > 0 && onOffOn > 0);
    CHECK(counts.halved > 0 && counts.gaveUp > 0);  // (both reached by directed scenes, kinds 3 and 4 above)
    CHECK(oneByOne > 0 && sgSphTables > 0 && shapeChanged > 0 && grew > 0);
    std::printf("staging: %u plans (%u with nothing to stage), largest plan / slot: turns %.6f, material tables %.6f\n", g_plans, g_emptyPlans, turnRatio,
                materialRatio);
    CHECK(turnRatio > 0.0 && turnRatio <= 1.0 && materialRatio > 0.0 && materialRatio <= 1.0 && g_emptyPlans > 0);
    CHECK(counts.onlyHuge == 0);  // unreachable (the head of this file): if a scene ever gets here, the reasoning is wrong and this says so
    std::printf("light_turn_selftest ok\n");
    return 0;
}
