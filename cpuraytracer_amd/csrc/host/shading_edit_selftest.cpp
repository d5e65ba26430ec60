// shading_edit_selftest.cpp -- the host pieces of the shading edits in a program of its own: no device, no Python.
//   1. rt_set_materials rebuilds the three material tables with rtprep::PrepareMaterials over the orig table it kept from the upload.
//      For random scenes of every layout kind (flat, hierarchy, cell grid; negative radii included) and random material tables A and
//      B: PrepareScene(spheres, B)'s mats, mats16, mats16Ok and matType equal PrepareMaterials(B) over the orig table of
//      PrepareScene(spheres, A), byte for byte -- B unpackable over a packable A and the reverse among them.
//   2. rt_unit_temporal_forget_host (the membership rule of ../rt_forget.h over PlanForget's set, as the kernel) against a naive double
//      loop: random id sets of both forms (up to 16 ids inline, more as a table), the sky id, ids out of range, empty sets; and its
//      refusals.
// Exit status 0 and a summary line, or the first failed condition and status 1.  Also built with AddressSanitizer and UBSan
// (make shading_edit_selftest_san).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../../include/rt_api.h"
#include "rt_edit_launch.h"
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

// A table inside the material domain.  packable: every colour on the byte grid; else about one record in eight has one off it.
std::vector<rt_material> MakeMaterials(uint32_t n, bool packable, Rng& rng) {
    std::vector<rt_material> m(n);
    std::memset(m.data(), 0, n * sizeof(rt_material));
    bool off = false;
    for (uint32_t k = 0; k < n; ++k) {
        m[k].type = rng.below(4);
        m[k].tex_type = rng.below(2);
        m[k].smoothness = rng.uni(0.f, 1.f);
        m[k].ior = rng.uni(1.1f, 2.f);
        m[k].tiling = rng.uni(-8.f, 8.f);
        m[k].luminance = rng.uni(0.f, 20.f);
        for (int c = 0; c < 3; ++c) {
            m[k].rgb0[c] = (float)rng.below(256) * (1.0f / 255.0f);
            m[k].rgb1[c] = (float)rng.below(256) * (1.0f / 255.0f);
        }
        if (!packable && m[k].type != RT_MAT_DIELECTRIC_TRANSPARENT && (rng.below(8) == 0 || (k + 1 == n && !off))) {
            m[k].rgb0[rng.below(3)] = 0.123456f;  // read by types 0, 1, 3 and not byte * (1 / 255)
            off = true;
        }
    }
    if (!packable && !off) {  // (every record was glass: make the last one opaque and off the grid)
        m[n - 1].type = RT_MAT_DIELECTRIC_OPAQUE;
        m[n - 1].rgb0[0] = 0.123456f;
    }
    return m;
}

// kind 0: scattered, few enough for the flat scan; 1: scattered, more groups than treeTop takes (the hierarchy); 2: a uniform layer
// of small spheres under a few big ones (the cell grid)
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
    } else {
        opt.treeTop = 16u;
        sp.push_back({0.f, -1000.f, 0.f, 1000.f});
        sp.push_back({-4.f, 1.f, 0.f, -1.f});
        const int half = 8 + (int)rng.below(3);  // 256 small spheres, the fewest the grid takes, to 400
        for (int a = -half; a < half; ++a)
            for (int b = -half; b < half; ++b) sp.push_back({(float)a + rng.uni(0.f, 0.9f), 0.2f, (float)b + rng.uni(0.f, 0.9f), 0.2f * sign()});
    }
    return sp;
}

template <typename T>
bool SameBytes(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

void MaterialTables() {
    Rng rng{20261021};
    uint32_t kinds[3] = {0, 0, 0}, flips[2][2] = {{0, 0}, {0, 0}};
    double largestRatio = 0.0;
    for (g_case = 0; g_case < 2000; ++g_case) {
        const uint32_t want = g_case % 10 < 7 ? 0u : (g_case % 10 < 9 ? 1u : 2u);
        PrepOptions opt;
        const std::vector<rt_sphere> sp = MakeSpheres(want, rng, opt);
        const uint32_t n = (uint32_t)sp.size();
        const bool packA = rng.below(2) == 0, packB = rng.below(2) == 0;
        const std::vector<rt_material> A = MakeMaterials(n, packA, rng), B = MakeMaterials(n, packB, rng);
        CHECK(AllFinite(sp.data(), n, nullptr));
        CHECK(MaterialsInDomain(A.data(), n, nullptr, nullptr) && MaterialsInDomain(B.data(), n, nullptr, nullptr));
        const PreparedScene PA = PrepareScene(sp.data(), A.data(), n, nullptr, 0, opt);
        const PreparedScene PB = PrepareScene(sp.data(), B.data(), n, nullptr, 0, opt);
        const SceneLayout& L = PA.layout;
        CHECK(L.scan.size() < 65536 && L.orig.size() == L.scan.size());
        const uint32_t kind = L.gridOn ? 2u : (L.nLevels > 1 ? 1u : 0u);
        ++kinds[kind];  // (counted as built, whatever was aimed at; each kind must occur, below)
        CHECK(SameBytes(L.orig, PB.layout.orig));  // the layout does not look at the materials
        CHECK(PA.mats16Ok == packA && PB.mats16Ok == packB);
        ++flips[packA][packB];
        const PreparedMaterials M = PrepareMaterials(B.data(), n, L.orig.data(), L.orig.size());
        CHECK(SameBytes(M.mats, PB.mats));
        CHECK(SameBytes(M.mats16, PB.mats16));
        CHECK(M.mats16Ok == PB.mats16Ok);
        CHECK(SameBytes(M.matType, PB.matType));
        CHECK(M.mats.size() == L.orig.size() && M.mats16.size() == L.orig.size() && M.matType.size() == n);  // the sizes an edit copies
        // ... through the staging plan (rt_scene_edit.h): inside the slot as the upload sizes it -- a scene without lights reserves no
        // index, so the slot is the material tables' or the forget table's -- every table inside its room, on a 16-byte boundary
        rtscene::StageShape shape;
        shape.nPad = L.orig.size(), shape.n = n, shape.inGlobalMemory = L.InGlobalMemory();
        const size_t slotBytes = rtscene::StageBytesMax(shape, opt);
        const rtscene::StagePlan plan =
            rtscene::PlanMaterialStage(M, {nullptr, L.orig.size() * sizeof(rt_material)}, {nullptr, L.orig.size() * sizeof(U4)}, {nullptr, n * sizeof(uint32_t)});
        CHECK(plan.status == RT_OK && plan.items.size() == 3 && plan.total > 0 && plan.total <= slotBytes);
        for (const rtscene::StageItem& it : plan.items) CHECK(it.bytes <= it.dst.room && it.offset % 16 == 0 && it.offset + it.bytes <= plan.total);
        const double ratio = (double)plan.total / (double)slotBytes;
        largestRatio = ratio > largestRatio ? ratio : largestRatio;
        // ... and the radii, which PrepareScene still writes itself, do not depend on the table
        CHECK(SameBytes(PA.radius, PB.radius));
    }
    CHECK(kinds[0] > 0 && kinds[1] > 0 && kinds[2] > 0);
    CHECK(flips[0][0] > 0 && flips[0][1] > 0 && flips[1][0] > 0 && flips[1][1] > 0);
    std::printf("material tables: 2000 scenes (flat %u, hierarchy %u, cell grid %u); packable A->B: no->no %u, no->yes %u, yes->no %u, yes->yes %u\n", kinds[0],
                kinds[1], kinds[2], flips[0][0], flips[0][1], flips[1][0], flips[1][1]);
    std::printf("staging: largest plan / slot %.6f\n", largestRatio);
    CHECK(largestRatio > 0.0 && largestRatio <= 1.0);
}

void Forget() {
    Rng rng{77};
    uint32_t inlineForms = 0, tableForms = 0, empties = 0, withSky = 0, outOfRange = 0;
    for (g_case = 0; g_case < 3000; ++g_case) {
        const uint32_t nSpheres = 1 + rng.below(rng.below(2) ? 40 : 3000);
        const uint32_t npix = rng.below(700);
        std::vector<uint32_t> ids(npix), len(npix);
        for (uint32_t p = 0; p < npix; ++p) {
            ids[p] = rng.below(5) == 0 ? 0xffffffffu : rng.below(nSpheres);
            len[p] = rng.below(4) == 0 ? 0u : 1u + rng.below(64);
        }
        const uint32_t form = rng.below(4);  // 0: empty, 1: up to 16, 2: more, 3: whatever
        uint32_t nIds = form == 0 ? 0u : (form == 1 ? 1u + rng.below(16) : (form == 2 ? 17u + rng.below(300) : rng.below(40)));
        std::vector<uint32_t> forget(nIds);
        bool sky = false, oob = false;
        for (uint32_t k = 0; k < nIds; ++k) {
            const uint32_t r = rng.below(10);
            if (r == 0) forget[k] = 0xffffffffu, sky = true;
            else if (r == 1) forget[k] = nSpheres + rng.below(5) * 31u, oob = true;  // at or above the count: matches nothing
            else if (r == 2) forget[k] = 0xfffffffeu, oob = true;
            else forget[k] = rng.below(nSpheres);
        }
        std::vector<uint32_t> want = len;
        for (uint32_t p = 0; p < npix; ++p)
            for (uint32_t k = 0; k < nIds; ++k)
                if (forget[k] == ids[p] && (ids[p] == 0xffffffffu || ids[p] < nSpheres)) want[p] = 0u;
        const rtedit::ForgetPlan P = rtedit::PlanForget(forget.data(), nIds, nSpheres);
        if (P.table.empty()) ++inlineForms;
        else ++tableForms;
        CHECK(P.table.empty() || (P.set.n_bits <= nSpheres && P.table.size() == rtd::forget_table_words(P.set.n_bits)));
        CHECK(P.set.n_inline <= rtd::kForgetInlineIds);
        empties += nIds == 0, withSky += sky, outOfRange += oob;
        std::vector<uint32_t> got = len;
        CHECK(rt_unit_temporal_forget_host(got.data(), ids.data(), npix, nSpheres, nIds ? forget.data() : nullptr, nIds) == RT_OK);
        CHECK(SameBytes(got, want));
    }
    CHECK(inlineForms > 0 && tableForms > 0 && empties > 0 && withSky > 0 && outOfRange > 0);
    g_case = 0;
    uint32_t one = 5, id = 0;
    CHECK(rt_unit_temporal_forget_host(nullptr, &id, 1, 4, &id, 1) == RT_ERR_INVALID_ARG);
    CHECK(rt_unit_temporal_forget_host(&one, nullptr, 1, 4, &id, 1) == RT_ERR_INVALID_ARG);
    CHECK(rt_unit_temporal_forget_host(&one, &id, 1, 4, nullptr, 1) == RT_ERR_INVALID_ARG && one == 5);
    CHECK(rt_unit_temporal_forget_host(nullptr, nullptr, 0, 4, nullptr, 0) == RT_OK);
    CHECK(rt_unit_temporal_forget_host(&one, &id, 1, 4, &id, 1) == RT_OK && one == 0);
    std::printf("forget twin: 3000 cases (inline sets %u, table sets %u, empty %u, with the sky %u, with ids out of range %u)\n", inlineForms, tableForms, empties,
                withSky, outOfRange);
}

}  // namespace

int main() {
    MaterialTables();
    Forget();
    std::printf("shading_edit_selftest ok\n");
    return 0;
}
