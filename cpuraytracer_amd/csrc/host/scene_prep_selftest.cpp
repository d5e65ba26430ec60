// scene_prep_selftest.cpp -- the scene preparation (rt_scene_prep.h) in a program of its own: no device, no Python, no files.
// Generates scenes from a fixed seed -- every layout kind, the sizes either side of a group of four, negative radii, coincident
// centres, light lists of every length -- and checks the STRUCTURE of what PrepareScene returns: lengths, permutations, prefix
// tables, the range of every 16-bit id.  Whether the scan's bounds are conservative is not its business (the fuzz tests own that);
// of the shadow indices it checks the plain inclusion: every sphere's exact footprint lies in cells that list it.
// The material domain (MaterialFault): one offender per clause, the first offender of a table, unread fields left alone.
// Exit status 0 and one line per scene, or the first failed condition and status 1.  Also built with AddressSanitizer and
// UBSan (make scene_prep_selftest_san): the index arithmetic of the builders then runs under both.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

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
    float uni(float lo, float hi) { return lo + (hi - lo) * (float)((next() >> 40) * (1.0 / 16777216.0)); }
};

struct Scene {
    std::string name;
    std::vector<rt_sphere> sp;
};

const char* g_scene = "";
std::string g_lights;

#define CHECK(cond)                                                                                          \
    do {                                                                                                     \
        if (!(cond)) {                                                                                       \
            std::printf("FAILED %s, %s: %s (%s:%d)\n", g_scene, g_lights.c_str(), #cond, __FILE__, __LINE__); \
            std::exit(1);                                                                                    \
        }                                                                                                    \
    } while (0)

std::vector<Scene> MakeScenes() {
    Rng rng{20240607};
    std::vector<Scene> out;
    auto scattered = [&](const char* name, uint32_t n, float box, float rlo, float rhi) {
        Scene s{name, {}};
        for (uint32_t k = 0; k < n; ++k) s.sp.push_back({rng.uni(-box, box), rng.uni(-box, box), rng.uni(-box, box), rng.uni(rlo, rhi)});
        out.push_back(s);
    };
    scattered("one", 1, 1.f, 0.5f, 1.f);
    scattered("three", 3, 2.f, 0.2f, 1.f);
    scattered("four", 4, 2.f, 0.2f, 1.f);
    scattered("five", 5, 2.f, 0.2f, 1.f);
    {   // mixed sizes and signs; the largest spheres of all are among the negative ones
        scattered("mixed300", 300, 20.f, 0.1f, 1.5f);
        std::vector<rt_sphere>& sp = out.back().sp;
        for (size_t k = 0; k < sp.size(); k += 3) sp[k].r = -sp[k].r;
        sp[0].r = -40.f;
        sp[1].r = 25.f;
        sp[2].r = -0.01f;
    }
    {   // a flat layer of small spheres under a few big ones: the cell grid
        Scene s{"layer2000", {}};
        s.sp.push_back({0.f, -1000.f, 0.f, 1000.f});
        s.sp.push_back({-4.f, 1.f, 0.f, -1.f});
        s.sp.push_back({4.f, 1.f, 0.f, 1.f});
        for (int a = -22; a < 22; ++a)
            for (int b = -22; b < 22; ++b) {
                const float r = 0.2f * (rng.next() & 1u ? 1.f : -1.f);
                s.sp.push_back({a + rng.uni(0.f, 0.9f), 0.2f, b + rng.uni(0.f, 0.9f), r});
            }
        out.push_back(s);
    }
    {   // a cubic lattice: too clumped per cell column for the grid, too many groups for the flat scan -- the hierarchy
        Scene s{"lattice10k", {}};
        for (int a = 0; a < 22; ++a)
            for (int b = 0; b < 22; ++b)
                for (int c = 0; c < 21; ++c) s.sp.push_back({(float)a, (float)b, (float)c, 0.3f});
        out.push_back(s);
    }
    {
        Scene s{"coincident", {}};
        for (int k = 0; k < 41; ++k) s.sp.push_back({1.f, 2.f, 3.f, (k & 1 ? -1.f : 1.f) * (0.5f + 0.01f * (float)(k % 7))});
        out.push_back(s);
    }
    return out;
}

std::vector<std::vector<rt_light>> MakeLightLists() {
    const rt_light axis{{0.f, 1.f, 0.f}, {1.f, 1.f, 1.f}, 2.f};
    const rt_light axisX{{-1.f, 0.f, 0.f}, {1.f, 0.5f, 0.25f}, 1.f};
    const rt_light oblique{{0.48f, 0.6f, -0.64f}, {1.f, 1.f, 1.f}, 1.f};
    const rt_light none{{0.f, 0.f, 0.f}, {1.f, 1.f, 1.f}, 1.f};  // not a direction: no index for this light
    std::vector<std::vector<rt_light>> out = {{axis}, {oblique, none}, {}};
    for (uint32_t k = 0; k < RT_MAX_LIGHTS; ++k) out[2].push_back(k % 4 == 0 ? none : (k % 4 == 1 ? axis : (k % 4 == 2 ? oblique : axisX)));
    return out;
}

std::vector<rt_material> MakeMaterials(uint32_t n, bool bytes, Rng& rng) {
    std::vector<rt_material> m(n);
    std::memset(m.data(), 0, n * sizeof(rt_material));
    for (uint32_t k = 0; k < n; ++k) {
        m[k].type = (uint32_t)(rng.next() & 3u);
        m[k].tex_type = (uint32_t)(rng.next() & 1u);
        m[k].smoothness = rng.uni(0.f, 1.f);
        m[k].ior = 1.5f;
        m[k].tiling = 4.f;
        m[k].luminance = 3.f;
        for (int c = 0; c < 3; ++c) {
            m[k].rgb0[c] = bytes ? (float)(rng.next() & 255u) * (1.0f / 255.0f) : rng.uni(0.f, 1.f);
            m[k].rgb1[c] = (float)(rng.next() & 255u) * (1.0f / 255.0f);
        }
    }
    return m;
}

void CheckShadowGrid(const ShadowGrid& G, const SceneLayout& L, const std::vector<rt_sphere>& sp, bool isDirection) {
    if (!isDirection) CHECK(!G.enabled);
    if (!G.enabled) return;
    CHECK(G.nx >= 1 && G.ny >= 1);
    CHECK(G.cellStart.size() == (size_t)G.nx * G.ny + 1);
    CHECK(G.cellStart.front() == 0);
    CHECK(G.cellStart.back() == G.entries.size());
    for (size_t c = 1; c < G.cellStart.size(); ++c) CHECK(G.cellStart[c - 1] <= G.cellStart[c]);
    for (uint16_t e : G.entries) CHECK(e < L.scan.size() && L.orig[e] != 0xffffffffu);
    for (uint16_t e : G.global) CHECK(e < L.scan.size() && L.orig[e] != 0xffffffffu);
    // inclusion, in plain double precision: the bounding square of every sphere's exact footprint -- the disc of radius |r| about
    // the centre's projection -- lies inside the grid, in cells that all list the sphere; or the sphere is in the global list
    std::vector<char> inGlobal(L.scan.size(), 0);
    for (uint16_t e : G.global) inGlobal[e] = 1;
    auto listed = [&](size_t c, size_t e) {
        for (size_t k = G.cellStart[c]; k < G.cellStart[c + 1]; ++k)
            if (G.entries[k] == e) return true;
        return false;
    };
    for (size_t e = 0; e < L.scan.size(); ++e) {
        if (L.orig[e] == 0xffffffffu || inGlobal[e]) continue;
        const rt_sphere& q = sp[L.orig[e]];
        const double r = std::fabs((double)q.r);
        const double u = (double)q.cx * G.e1[0] + (double)q.cy * G.e1[1] + (double)q.cz * G.e1[2];
        const double v = (double)q.cx * G.e2[0] + (double)q.cy * G.e2[1] + (double)q.cz * G.e2[2];
        const double x0 = std::floor((u - r - (double)G.u0) * (double)G.invCell), x1 = std::floor((u + r - (double)G.u0) * (double)G.invCell);
        const double y0 = std::floor((v - r - (double)G.v0) * (double)G.invCell), y1 = std::floor((v + r - (double)G.v0) * (double)G.invCell);
        CHECK(x0 >= 0.0 && y0 >= 0.0 && x1 < (double)G.nx && y1 < (double)G.ny);
        for (size_t y = (size_t)y0; y <= (size_t)y1; ++y)
            for (size_t x = (size_t)x0; x <= (size_t)x1; ++x) CHECK(listed(y * G.nx + x, e));
    }
}

// returns the layout kind: 0 flat, 1 grid, 2 hierarchy
int CheckScene(const std::vector<rt_sphere>& sp, const std::vector<rt_material>& mats, const std::vector<rt_light>& lights) {
    const uint32_t n = (uint32_t)sp.size();
    PrepOptions opt;
    opt.sgSph = true;  // (only scenes whose tables stay in global memory get the table)
    CHECK(AllFinite(sp.data(), n, nullptr));
    const PreparedScene P = PrepareScene(sp.data(), mats.data(), n, lights.data(), (uint32_t)lights.size(), opt);
    const SceneLayout& L = P.layout;
    const size_t nPad = (size_t)L.nGroups * 4 + 4;
    CHECK(nPad < 65536);
    CHECK(L.nGroups >= 4 && L.nGroups % 4 == 0);
    CHECK(L.scan.size() == nPad && L.orig.size() == nPad && L.leaf.size() == nPad);
    {   // orig: every sphere exactly once, padding elsewhere
        std::vector<uint32_t> seen(n, 0);
        for (uint32_t o : L.orig) {
            if (o == 0xffffffffu) continue;
            CHECK(o < n);
            ++seen[o];
        }
        for (uint32_t k = 0; k < n; ++k) CHECK(seen[k] == 1);
    }
    {   // the levels tile `tree`
        CHECK(L.nLevels >= 1 && L.nLevels <= rtd::kMaxLevels);
        CHECK(L.levelCnt[0] == L.nGroups);
        uint32_t off = 0;
        for (uint32_t l = 0; l < L.nLevels; ++l) {
            CHECK(L.levelOff[l] == off);
            CHECK(L.levelCnt[l] != 0);
            off += L.levelCnt[l];
        }
        CHECK(off == L.tree.size());
        CHECK(L.levelCnt[L.nLevels - 1] <= opt.treeTop || L.nLevels == rtd::kMaxLevels || L.gridOn);
    }
    CHECK(L.nAlways <= 8);
    CHECK(L.gridQ.empty() || L.gridQ.size() == nPad);
    if (L.gridOn) {
        // cells of the small spheres, which follow the big spheres' one-sphere groups (padded to whole nodes of four groups)
        const size_t base = (size_t)((L.nAlways + 3u) / 4u * 4u) * 4u;
        CHECK(L.nLevels == 1);
        CHECK(L.gridNu >= 1 && L.gridNu <= 254 && L.gridNv >= 1 && L.gridNv <= 254);
        CHECK(L.gridAxU < 3 && L.gridAxV < 3 && L.gridAxU != L.gridAxV);
        CHECK(L.gridCellStart.size() == (size_t)L.gridNu * L.gridNv + 1);
        CHECK(L.gridCellStart.front() == base);
        CHECK(L.gridCellStart.back() == base + (n - L.nAlways));
        CHECK(L.gridCellStart.back() <= nPad);
        for (size_t c = 1; c < L.gridCellStart.size(); ++c) CHECK(L.gridCellStart[c - 1] <= L.gridCellStart[c]);
        for (size_t e = base; e < L.gridCellStart.back(); ++e) CHECK(L.orig[e] != 0xffffffffu);
    } else {
        CHECK(L.gridCellStart.empty() && L.gridQ.empty());
    }
    // per-entry tables
    CHECK(P.radius.size() == nPad && P.mats.size() == nPad && P.mats16.size() == nPad && P.matType.size() == n);
    for (size_t e = 0; e < nPad; ++e) {
        const float want = L.orig[e] == 0xffffffffu ? 0.f : sp[L.orig[e]].r;
        CHECK(std::memcmp(&P.radius[e], &want, 4) == 0);
        if (L.orig[e] != 0xffffffffu) {
            CHECK(std::memcmp(&P.mats[e], &mats[L.orig[e]], sizeof(rt_material)) == 0);
            if (P.mats16Ok) CHECK((P.mats16[e].x & 3u) == mats[L.orig[e]].type);
        }
    }
    for (uint32_t k = 0; k < n; ++k) CHECK(P.matType[k] == mats[k].type);
    // shadow indices
    auto isDirection = [](const rt_light& l) { return l.direction[0] != 0.f || l.direction[1] != 0.f || l.direction[2] != 0.f; };
    CHECK(P.extraShadow.size() + 1 == lights.size());
    CheckShadowGrid(P.shadow, L, sp, isDirection(lights[0]));
    for (size_t k = 1; k < lights.size(); ++k) CheckShadowGrid(P.extraShadow[k - 1], L, sp, isDirection(lights[k]));
    if (P.shadow.enabled && L.InGlobalMemory())
        CHECK(P.sgSph.size() == P.shadow.entries.size() + 1);
    else
        CHECK(P.sgSph.empty());
    for (int h = 0; h < 2; ++h) CHECK(P.singleMask[h] == L.singleMask[h]);
    if (L.nGroups > 128) CHECK(L.singleMask[0] == 0 && L.singleMask[1] == 0);
    return L.gridOn ? 1 : (L.nLevels > 1 ? 2 : 0);
}

// The material domain of include/rt_api.h: every clause refuses its offender under the right field name, records that only
// carry NaN where their type does not read are inside, and a table reports its FIRST offender.
void CheckMaterialDomain() {
    g_scene = "material domain";
    g_lights = "";
    const float nan = std::nanf(""), inf = INFINITY;
    auto rec = [](uint32_t type, uint32_t tex) {
        rt_material m;
        std::memset(&m, 0, sizeof(m));
        m.type = type; m.tex_type = tex;
        m.smoothness = 16.f; m.ior = 1.5f; m.tiling = 4.f; m.luminance = 100.f;
        for (int c = 0; c < 3; ++c) { m.rgb0[c] = 0.5f; m.rgb1[c] = 0.25f; }
        return m;
    };
    auto faultIs = [](const rt_material& m, const char* field) {
        const char* f = MaterialFault(m);
        return field ? (f && !std::strcmp(f, field)) : f == nullptr;
    };
    for (uint32_t type = 0; type < 4; ++type)
        for (uint32_t tex = 0; tex < 2; ++tex) CHECK(faultIs(rec(type, tex), nullptr));
    { rt_material m = rec(4, 0); CHECK(faultIs(m, "type")); m.type = 0xffffffffu; CHECK(faultIs(m, "type")); }
    { rt_material m = rec(1, 2); CHECK(faultIs(m, "tex_type")); }
    for (uint32_t type = 0; type < 3; ++type) { rt_material m = rec(type, 0); m.smoothness = type == 1 ? inf : nan; CHECK(faultIs(m, "smoothness")); }
    { rt_material m = rec(2, 0); m.ior = nan; CHECK(faultIs(m, "ior")); m.ior = -inf; CHECK(faultIs(m, "ior")); }
    { rt_material m = rec(3, 0); m.luminance = inf; CHECK(faultIs(m, "luminance")); }
    for (uint32_t type : {0u, 1u, 3u}) {
        rt_material m = rec(type, 0);
        m.rgb0[type % 3] = nan;
        CHECK(faultIs(m, "rgb0"));
        m = rec(type, 1);
        m.rgb1[2] = inf;
        CHECK(faultIs(m, "rgb1"));
        m = rec(type, 0);
        m.rgb1[0] = nan; m.tiling = nan;  // const texture: neither is read
        CHECK(faultIs(m, nullptr));
        for (float t : {nan, inf, -inf, std::nextafterf(1073741824.0f, inf), -3.0e9f}) {
            m = rec(type, 1);
            m.tiling = t;
            CHECK(faultIs(m, "tiling"));
        }
        for (float t : {1073741824.0f, -1073741824.0f, 0.f, -50.f, 1e6f}) {
            m = rec(type, 1);
            m.tiling = t;
            CHECK(faultIs(m, nullptr));
        }
    }
    {   // what a type does not read is not inspected
        rt_material m = rec(0, 0);
        m.ior = nan; m.luminance = nan; m.tiling = inf;
        CHECK(faultIs(m, nullptr));
        m = rec(2, 1);  // a glass sphere has no texture: tex_type must still be a texture kind, the texture's fields are unread
        m.tiling = 3.0e9f; m.luminance = nan;
        for (int c = 0; c < 3; ++c) m.rgb0[c] = m.rgb1[c] = nan;
        CHECK(faultIs(m, nullptr));
        m = rec(3, 0);
        m.smoothness = nan; m.ior = inf;
        CHECK(faultIs(m, nullptr));
    }
    {   // a table: the first offender, with its field; untouched outputs when there is none
        std::vector<rt_material> tab(7, rec(0, 1));
        uint32_t which = 99;
        const char* field = "untouched";
        CHECK(MaterialsInDomain(tab.data(), 7, &which, &field) && which == 99 && !std::strcmp(field, "untouched"));
        tab[5].type = 9;
        tab[3].tiling = nan;
        CHECK(!MaterialsInDomain(tab.data(), 7, &which, &field) && which == 3 && !std::strcmp(field, "tiling"));
        CHECK(!MaterialsInDomain(tab.data(), 7, nullptr, nullptr));
        const std::string msg = MaterialFaultMessage("rt_scene_upload", "sphere 3", tab[3], field);
        CHECK(msg.find("sphere 3") != std::string::npos && msg.find("tiling") != std::string::npos);
    }
    std::printf("ok material domain\n");
}

}  // namespace

int main() {
    static const char* const kKind[3] = {"flat", "grid", "hierarchy"};
    Rng rng{77};
    const std::vector<std::vector<rt_light>> lightLists = MakeLightLists();
    bool seen[3] = {false, false, false};
    for (const Scene& s : MakeScenes()) {
        g_scene = s.name.c_str();
        int kind = -1;
        // (a scene of thousands of spheres takes seconds to lay out: that one sees the longest light list only)
        for (size_t li = s.sp.size() > 5000 ? lightLists.size() - 1 : 0; li < lightLists.size(); ++li) {
            g_lights = std::to_string(lightLists[li].size()) + " light(s)";
            const std::vector<rt_material> mats = MakeMaterials((uint32_t)s.sp.size(), li != 1, rng);
            const int k = CheckScene(s.sp, mats, lightLists[li]);
            CHECK(kind < 0 || k == kind);  // the layout does not depend on lights or materials
            kind = k;
        }
        seen[kind] = true;
        std::printf("ok %-12s %6zu spheres  %s\n", g_scene, s.sp.size(), kKind[kind]);
    }
    g_scene = "all scenes";
    g_lights = "";
    CHECK(seen[0] && seen[1] && seen[2]);
    CheckMaterialDomain();
    std::printf("scene_prep_selftest: ok\n");
    return 0;
}
