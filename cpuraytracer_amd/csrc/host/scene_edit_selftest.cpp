// scene_edit_selftest.cpp -- the scene record, the decisions and the staging plans of rt_scene_edit.h in a program of its
// own: no device, no Python.
//   1. Every refusal of rt_scene_upload, the five edits and the two getters from a record filled by hand: the code, the words (written
//      out here as the entries have always said them) and the record's bytes unchanged.
//   2. The same-record rule: the record's own bytes are "same" for every edit, -0.0f against 0.0f is "changed", an empty light list is
//      "same", the camera's padding is neither inspected nor compared, the material table and the sky are reported apart.
//   3. Decide, then commit, over seeded random scripts of uploads and edits: the record equals a model that stores the last accepted
//      arguments, and a refused or same-record step changes nothing.
//   4. The plans' layout: the material tables at 0, 48 and 64 bytes times the entry count, the forget table as one item, an index's
//      tables in order on 16-byte boundaries, a table beyond its room refused; the figures of the rooms and of the bound.
//   (The bound against the plans of generated scenes and light lists is checked where those are generated: light_turn_selftest.cpp and
//   shading_edit_selftest.cpp.)
// Exit status 0 and a summary, or the first failed condition and status 1.  Also built with AddressSanitizer and UBSan
// (make scene_edit_selftest_san).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../../include/rt_api.h"
#include "rt_scene_edit.h"
#include "rt_scene_prep.h"

using namespace rtscene;

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

const float kNaN = std::numeric_limits<float>::quiet_NaN(), kInf = std::numeric_limits<float>::infinity();

template <typename T>
void Put(std::string& s, const T& v) {
    s.append(reinterpret_cast<const char*>(&v), sizeof(T));
}
template <typename T>
void Put(std::string& s, const std::vector<T>& v) {
    Put(s, v.size());
    if (!v.empty()) s.append(reinterpret_cast<const char*>(v.data()), v.size() * sizeof(T));
}
// everything a record holds, member by member (none of the members has padding)
std::string Bytes(const Record& r) {
    std::string s;
    Put(s, r.n), Put(s, r.spheres), Put(s, r.materials), Put(s, r.sky), Put(s, r.camera), Put(s, r.nLights), Put(s, r.exposure);
    for (uint32_t k = 0; k < r.nLights; ++k) Put(s, r.lights[k]);  // (the slots behind the count hold nothing)
    const rtprep::SceneLayout& L = r.shadowLayout;
    Put(s, L.scan), Put(s, L.orig), Put(s, L.nGroups), Put(s, L.nLevels), Put(s, L.gridOn);
    const rtprep::PrepOptions& o = r.prepOpt;
    Put(s, o.treeTop), Put(s, o.shadowGrid), Put(s, o.shadowCellsLds), Put(s, o.shadowCellsGlobal), Put(s, o.sgSph);
    return s;
}

rt_camera MakeCamera(Rng& rng) {
    rt_camera c{};
    float* f = reinterpret_cast<float*>(&c);
    for (size_t k = 0; k < sizeof(c) / sizeof(float); ++k) f[k] = rng.uni(-4.f, 4.f);
    return c;
}
rt_light MakeLight(Rng& rng) {
    rt_light l{};
    for (int c = 0; c < 3; ++c) l.direction[c] = rng.uni(-1.f, 1.f), l.color[c] = rng.uni(0.f, 1.f);
    l.luminance = rng.uni(0.f, 10.f);
    return l;
}
rt_material MakeMaterial(Rng& rng) {
    rt_material m{};
    m.type = rng.below(4), m.tex_type = rng.below(2);
    m.smoothness = rng.uni(0.f, 1.f), m.ior = rng.uni(1.1f, 2.f), m.tiling = rng.uni(-8.f, 8.f), m.luminance = rng.uni(0.f, 20.f);
    for (int c = 0; c < 3; ++c) m.rgb0[c] = rng.uni(0.f, 1.f), m.rgb1[c] = rng.uni(0.f, 1.f);
    return m;
}

// ---------------------------------------------------------------------------------------------------------------- 1 and 2
struct Hand {
    Record rec;
    std::string before;
    Hand() {
        Rng rng{7};
        rec.n = 3;
        rec.spheres = {{0.f, 0.f, 0.f, 1.f}, {2.f, 0.f, 0.f, 0.5f}, {0.f, -100.f, 0.f, 99.f}};
        for (int k = 0; k < 3; ++k) rec.materials.push_back(MakeMaterial(rng));
        rec.sky = MakeMaterial(rng);
        rec.sky.type = RT_MAT_EMISSIVE;
        rec.camera = MakeCamera(rng);
        rec.nLights = 2;
        rec.lights[0] = MakeLight(rng), rec.lights[1] = MakeLight(rng);
        rec.lights[1].color[2] = 0.f;
        rec.exposure = 1.5f;
        rec.shadowLayout.orig = {2u, 0u, 1u, 0xffffffffu};
        before = Bytes(rec);
    }
    void Refused(const Decision& d, int code, const char* message) const {
        if (d.verdict != Verdict::Refused || d.code != code || d.message != message)
            std::printf("expected %d \"%s\"\n     got %d \"%s\" (verdict %d)\n", code, message, d.code, d.message.c_str(), (int)d.verdict);
        CHECK(d.verdict == Verdict::Refused && d.code == code && d.message == message);
        CHECK(Bytes(rec) == before);
        ++refusals;
    }
    void Is(const Decision& d, Verdict v) const {
        CHECK(d.verdict == v && d.code == RT_OK && d.message.empty());
        CHECK(Bytes(rec) == before);
    }
    mutable uint32_t refusals = 0;
};

void Refusals() {
    const Hand h;
    const Record* r = &h.rec;
    const rt_camera cam = r->camera;
    const rt_material* mats = r->materials.data();
    const rt_light* lights = r->lights;
    rt_camera camOut{};
    rt_light lightsOut[RT_MAX_LIGHTS] = {};
    uint32_t count = 77;

    // ---- no scene: the five edits and the two getters
    h.Refused(DecideSetCamera(r, false, &cam), RT_ERR_NO_SCENE, "rt_set_camera: no scene uploaded");
    h.Refused(DecideSetMaterials(r, false, mats, 3, &r->sky), RT_ERR_NO_SCENE, "rt_set_materials: no scene uploaded");
    h.Refused(DecideSetLights(r, false, lights, 2), RT_ERR_NO_SCENE, "rt_set_lights: no scene uploaded");
    h.Refused(DecideTurnLights(r, false, lights, 2), RT_ERR_NO_SCENE, "rt_turn_lights: no scene uploaded");
    h.Refused(DecideSetExposure(r, false, 1.f), RT_ERR_NO_SCENE, "rt_set_exposure: no scene uploaded");
    h.Refused(GetCamera(r, false, &camOut), RT_ERR_NO_SCENE, "rt_get_camera: no scene uploaded");
    h.Refused(GetLights(r, false, lightsOut, RT_MAX_LIGHTS, &count), RT_ERR_NO_SCENE, "rt_get_lights: no scene uploaded");
    CHECK(count == 77);
    // ---- null arguments (a null record: the entry had no context)
    h.Refused(DecideSetCamera(nullptr, false, &cam), RT_ERR_INVALID_ARG, "rt_set_camera: null argument");
    h.Refused(DecideSetCamera(r, true, nullptr), RT_ERR_INVALID_ARG, "rt_set_camera: null argument");
    h.Refused(DecideSetMaterials(nullptr, false, mats, 3, &r->sky), RT_ERR_INVALID_ARG, "rt_set_materials: null argument");
    h.Refused(DecideSetMaterials(r, true, nullptr, 3, &r->sky), RT_ERR_INVALID_ARG, "rt_set_materials: null argument");
    h.Refused(DecideSetMaterials(r, true, mats, 3, nullptr), RT_ERR_INVALID_ARG, "rt_set_materials: null argument");
    h.Refused(DecideSetLights(nullptr, false, lights, 2), RT_ERR_INVALID_ARG, "rt_set_lights: null argument");
    h.Refused(DecideSetLights(r, true, nullptr, 2), RT_ERR_INVALID_ARG, "rt_set_lights: null argument");
    h.Refused(DecideTurnLights(nullptr, false, lights, 2), RT_ERR_INVALID_ARG, "rt_turn_lights: null argument");
    h.Refused(DecideTurnLights(r, true, nullptr, 2), RT_ERR_INVALID_ARG, "rt_turn_lights: null argument");
    h.Refused(DecideSetExposure(nullptr, false, 1.f), RT_ERR_INVALID_ARG, "rt_set_exposure: null ctx");
    h.Refused(GetCamera(nullptr, false, &camOut), RT_ERR_INVALID_ARG, "rt_get_camera: null argument");
    h.Refused(GetCamera(r, true, nullptr), RT_ERR_INVALID_ARG, "rt_get_camera: null argument");
    h.Refused(GetLights(nullptr, false, lightsOut, 8, &count), RT_ERR_INVALID_ARG, "rt_get_lights: null argument");
    h.Refused(GetLights(r, true, lightsOut, 8, nullptr), RT_ERR_INVALID_ARG, "rt_get_lights: null argument");
    h.Refused(GetLights(r, true, nullptr, 8, &count), RT_ERR_INVALID_ARG, "rt_get_lights: null argument");
    CHECK(count == 77);
    // ---- the getters' answers
    h.Refused(GetLights(r, true, lightsOut, 1, &count), RT_ERR_INVALID_ARG, "rt_get_lights: capacity too small for 2 lights");
    CHECK(count == 2);  // (written before the capacity is judged)
    count = 77;
    h.Is(GetLights(r, true, nullptr, 0, &count), Verdict::Same);  // the count alone
    CHECK(count == 2);
    h.Is(GetLights(r, true, lightsOut, 2, &count), Verdict::Same);
    CHECK(std::memcmp(lightsOut, r->lights, 2 * sizeof(rt_light)) == 0);
    h.Is(GetCamera(r, true, &camOut), Verdict::Same);
    CHECK(std::memcmp(&camOut, &r->camera, sizeof(rt_camera)) == 0);

    // ---- counts
    h.Refused(DecideSetMaterials(r, true, mats, 2, &r->sky), RT_ERR_INVALID_ARG, "rt_set_materials: 2 records for a scene of 3 spheres");
    h.Refused(DecideSetLights(r, true, lights, 1), RT_ERR_INVALID_ARG, "rt_set_lights: 1 lights for a scene uploaded with 2");
    h.Refused(DecideTurnLights(r, true, lights, 3), RT_ERR_INVALID_ARG, "rt_turn_lights: 3 lights for a scene uploaded with 2");
    h.Refused(DecideTurnLights(r, true, nullptr, 0), RT_ERR_INVALID_ARG, "rt_turn_lights: 0 lights for a scene uploaded with 2");

    // ---- the camera: each of the six fields, every component of it, NaN and infinity; the padding is not looked at
    const struct {
        const char* message;
        size_t first, count;  // in floats
    } fields[] = {{"rt_set_camera: origin is not finite", 0, 3},
                  {"rt_set_camera: x is not finite", 4, 3},
                  {"rt_set_camera: y is not finite", 8, 3},
                  {"rt_set_camera: origin_image_plane is not finite", 12, 3},
                  {"rt_set_camera: aperture is not finite", 16, 1},
                  {"rt_set_camera: focal_length is not finite", 17, 1}};
    for (const auto& f : fields)
        for (size_t k = 0; k < f.count; ++k)
            for (float bad : {kNaN, kInf, -kInf}) {
                rt_camera c = cam;
                reinterpret_cast<float*>(&c)[f.first + k] = bad;
                h.Refused(DecideSetCamera(r, true, &c), RT_ERR_INVALID_ARG, f.message);
            }
    for (size_t pad : {3u, 7u, 11u, 15u}) {
        rt_camera c = cam;
        reinterpret_cast<float*>(&c)[pad] = kNaN;
        h.Is(DecideSetCamera(r, true, &c), Verdict::Same);  // accepted, and not compared either
        reinterpret_cast<float*>(&c)[0] += 1.f;
        h.Is(DecideSetCamera(r, true, &c), Verdict::Changed);
    }
    {  // the first offending field is the one named
        rt_camera c = cam;
        c.focal_length = kNaN, c.y[1] = kInf;
        h.Refused(DecideSetCamera(r, true, &c), RT_ERR_INVALID_ARG, "rt_set_camera: y is not finite");
    }

    // ---- materials and the sky outside the domain
    {
        std::vector<rt_material> m = r->materials;
        m[1].type = 7;
        h.Refused(DecideSetMaterials(r, true, m.data(), 3, &r->sky), RT_ERR_INVALID_ARG,
                  "rt_set_materials: the material of sphere 1 is outside the material domain: type = 7 (rt_material_type is 0..3)");
        m = r->materials;
        m[2].type = RT_MAT_EMISSIVE, m[2].tex_type = 0, m[2].luminance = kNaN;
        h.Refused(DecideSetMaterials(r, true, m.data(), 3, &r->sky), RT_ERR_INVALID_ARG,
                  "rt_set_materials: the material of sphere 2 is outside the material domain: luminance is not finite");
        rt_material sky = r->sky;
        sky.tex_type = 2;
        h.Refused(DecideSetMaterials(r, true, mats, 3, &sky), RT_ERR_INVALID_ARG,
                  "rt_set_materials: the material of the sky is outside the material domain: tex_type = 2 (rt_texture_type is 0..1)");
        sky = r->sky;
        sky.tex_type = RT_TEX_CHECKER, sky.tiling = 4e9f;
        h.Refused(DecideSetMaterials(r, true, mats, 3, &sky), RT_ERR_INVALID_ARG,
                  "rt_set_materials: the material of the sky is outside the material domain: tiling is not finite or beyond 2^30 in magnitude");
        m[0].type = 9;  // the table is judged before the sky
        h.Refused(DecideSetMaterials(r, true, m.data(), 3, &sky), RT_ERR_INVALID_ARG,
                  "rt_set_materials: the material of sphere 0 is outside the material domain: type = 9 (rt_material_type is 0..3)");
    }

    // ---- lights
    const char* kDirection =
        "rt_set_lights: light 1 has another direction than the uploaded one: a direction change needs an rt_scene_upload (the light's shadow index is built for "
        "its direction)";
    for (float bad : {kNaN, kInf}) {
        rt_light l[2] = {lights[0], lights[1]};
        l[1].color[1] = bad;
        h.Refused(DecideSetLights(r, true, l, 2), RT_ERR_INVALID_ARG, "rt_set_lights: light 1 has a colour or a luminance that is not finite");
        h.Refused(DecideTurnLights(r, true, l, 2), RT_ERR_INVALID_ARG, "rt_turn_lights: light 1 has a colour or a luminance that is not finite");
        l[1] = lights[1], l[0].luminance = bad;
        h.Refused(DecideSetLights(r, true, l, 2), RT_ERR_INVALID_ARG, "rt_set_lights: light 0 has a colour or a luminance that is not finite");
        h.Refused(DecideTurnLights(r, true, l, 2), RT_ERR_INVALID_ARG, "rt_turn_lights: light 0 has a colour or a luminance that is not finite");
        l[0] = lights[0], l[1].direction[2] = bad;
        h.Refused(DecideTurnLights(r, true, l, 2), RT_ERR_INVALID_ARG, "rt_turn_lights: light 1 has a direction that is not finite");
        h.Refused(DecideSetLights(r, true, l, 2), RT_ERR_INVALID_ARG, kDirection);  // (to rt_set_lights it is another direction)
        l[1].color[0] = kNaN;  // the direction is judged before the colour
        h.Refused(DecideTurnLights(r, true, l, 2), RT_ERR_INVALID_ARG, "rt_turn_lights: light 1 has a direction that is not finite");
    }
    {
        rt_light l[2] = {lights[0], lights[1]};
        l[1].direction[0] += 0.25f;
        h.Refused(DecideSetLights(r, true, l, 2), RT_ERR_INVALID_ARG, kDirection);
        h.Is(DecideTurnLights(r, true, l, 2), Verdict::Changed);
        // ... compared with the directions set last: after a committed turn the turned one is accepted and the uploaded one refused
        Record turned = h.rec;
        CommitLights(turned, l);
        CHECK(DecideSetLights(&turned, true, l, 2).verdict == Verdict::Same);
        const Decision d = DecideSetLights(&turned, true, lights, 2);
        CHECK(d.verdict == Verdict::Refused && d.code == RT_ERR_INVALID_ARG && d.message == kDirection);
    }

    // ---- exposure
    for (float bad : {kNaN, kInf, -kInf}) h.Refused(DecideSetExposure(r, true, bad), RT_ERR_INVALID_ARG, "rt_set_exposure: the exposure is not finite");

    // ---- the upload
    const rt_sphere* sp = r->spheres.data();
    const char* kNull = "rt_scene_upload: null pointer or empty scene";
    h.Refused(DecideUpload(nullptr, sp, mats, 3, &cam, lights, 2, &r->sky), RT_ERR_INVALID_ARG, kNull);
    h.Refused(DecideUpload(r, nullptr, mats, 3, &cam, lights, 2, &r->sky), RT_ERR_INVALID_ARG, kNull);
    h.Refused(DecideUpload(r, sp, nullptr, 3, &cam, lights, 2, &r->sky), RT_ERR_INVALID_ARG, kNull);
    h.Refused(DecideUpload(r, sp, mats, 3, nullptr, lights, 2, &r->sky), RT_ERR_INVALID_ARG, kNull);
    h.Refused(DecideUpload(r, sp, mats, 3, &cam, nullptr, 2, &r->sky), RT_ERR_INVALID_ARG, kNull);
    h.Refused(DecideUpload(r, sp, mats, 3, &cam, lights, 2, nullptr), RT_ERR_INVALID_ARG, kNull);
    h.Refused(DecideUpload(r, sp, mats, 0, &cam, lights, 2, &r->sky), RT_ERR_INVALID_ARG, kNull);
    h.Is(DecideUpload(r, sp, mats, 3, &cam, nullptr, 0, &r->sky), Verdict::Changed);  // no lights and no list: a scene
    h.Is(DecideUpload(r, sp, mats, 3, &cam, lights, 2, &r->sky), Verdict::Changed);   // the same arguments: an upload all the same
    h.Refused(DecideUpload(r, sp, mats, 3, &cam, lights, RT_MAX_LIGHTS + 1, &r->sky), RT_ERR_INVALID_ARG, "rt_scene_upload: more than RT_MAX_LIGHTS lights");
    {
        std::vector<rt_sphere> s = r->spheres;
        s[2].r = kInf;
        h.Refused(DecideUpload(r, s.data(), mats, 3, &cam, lights, 2, &r->sky), RT_ERR_INVALID_ARG,
                  "rt_scene_upload: sphere 2 has a centre or a radius that is not finite");
        s[1].cy = kNaN;
        h.Refused(DecideUpload(r, s.data(), mats, 3, &cam, lights, 2, &r->sky), RT_ERR_INVALID_ARG,
                  "rt_scene_upload: sphere 1 has a centre or a radius that is not finite");
        std::vector<rt_material> m = r->materials;
        m[0].tex_type = 5;
        h.Refused(DecideUpload(r, sp, m.data(), 3, &cam, lights, 2, &r->sky), RT_ERR_INVALID_ARG,
                  "rt_scene_upload: the material of sphere 0 is outside the material domain: tex_type = 5 (rt_texture_type is 0..1)");
        h.Refused(DecideUpload(r, s.data(), m.data(), 3, &cam, lights, 2, &r->sky), RT_ERR_INVALID_ARG,
                  "rt_scene_upload: sphere 1 has a centre or a radius that is not finite");  // the spheres are judged first
        rt_material sky = r->sky;
        sky.luminance = -kInf;
        h.Refused(DecideUpload(r, sp, mats, 3, &cam, lights, 2, &sky), RT_ERR_INVALID_ARG,
                  "rt_scene_upload: the material of the sky is outside the material domain: luminance is not finite");
    }
    std::printf("refusals: %u, each with its code, its words and the record unchanged\n", h.refusals);
}

void SameRecord() {
    const Hand h;
    const Record* r = &h.rec;
    h.Is(DecideSetCamera(r, true, &r->camera), Verdict::Same);
    h.Is(DecideSetMaterials(r, true, r->materials.data(), 3, &r->sky), Verdict::Same);
    h.Is(DecideSetLights(r, true, r->lights, 2), Verdict::Same);
    h.Is(DecideTurnLights(r, true, r->lights, 2), Verdict::Same);
    h.Is(DecideSetExposure(r, true, r->exposure), Verdict::Same);
    CHECK(SameBits(&kNaN, &kNaN, sizeof(float)) && SameBits(nullptr, nullptr, 0));
    // -0.0f against 0.0f: changed, in every edit
    Record z = h.rec;
    z.camera.x[1] = 0.f, z.materials[1].rgb0[2] = 0.f, z.sky.luminance = 0.f, z.lights[1].color[2] = 0.f, z.lights[0].direction[1] = 0.f, z.exposure = 0.f;
    {
        rt_camera c = z.camera;
        c.x[1] = -0.f;
        CHECK(DecideSetCamera(&z, true, &c).verdict == Verdict::Changed);
        rt_light l[2] = {z.lights[0], z.lights[1]};
        l[1].color[2] = -0.f;
        CHECK(DecideSetLights(&z, true, l, 2).verdict == Verdict::Changed && DecideTurnLights(&z, true, l, 2).verdict == Verdict::Changed);
        l[1] = z.lights[1], l[0].direction[1] = -0.f;
        CHECK(DecideTurnLights(&z, true, l, 2).verdict == Verdict::Changed && DecideSetLights(&z, true, l, 2).verdict == Verdict::Refused);
        CHECK(DecideSetExposure(&z, true, -0.f).verdict == Verdict::Changed && DecideSetExposure(&z, true, 0.f).verdict == Verdict::Same);
    }
    // the material table and the sky, apart: all four combinations (and every byte of a record counts, read by its type or not)
    for (int table = 0; table < 2; ++table)
        for (int sky = 0; sky < 2; ++sky) {
            std::vector<rt_material> m = z.materials;
            rt_material s = z.sky;
            if (table) m[1].rgb0[2] = -0.f;
            if (sky) s.luminance = -0.f;
            const Decision d = DecideSetMaterials(&z, true, m.data(), 3, &s);
            CHECK(d.verdict == (table || sky ? Verdict::Changed : Verdict::Same) && d.table == (table != 0) && d.sky == (sky != 0));
            Record after = z;
            CommitMaterials(after, d, m.data(), s);
            CHECK(std::memcmp(after.materials.data(), m.data(), 3 * sizeof(rt_material)) == 0 && std::memcmp(&after.sky, &s, sizeof s) == 0);
        }
    {
        std::vector<rt_material> m = z.materials;
        m[0].type = RT_MAT_EMISSIVE, m[0].ior = 1.25f;  // ior: not read by an emissive record, compared all the same
        Record e = z;
        e.materials = m;
        m[0].ior = 1.5f;
        const Decision d = DecideSetMaterials(&e, true, m.data(), 3, &e.sky);
        CHECK(d.verdict == Verdict::Changed && d.table && !d.sky);
    }
    // no lights: the same, for both entries, with or without a list
    Record dark = h.rec;
    dark.nLights = 0;
    for (const rt_light* l : {(const rt_light*)nullptr, (const rt_light*)h.rec.lights}) {
        CHECK(DecideSetLights(&dark, true, l, 0).verdict == Verdict::Same);
        CHECK(DecideTurnLights(&dark, true, l, 0).verdict == Verdict::Same);
    }
    std::printf("same record: every edit, -0.0f against 0.0f, the table and the sky apart, no lights\n");
}

// ---------------------------------------------------------------------------------------------------------------- 3
void Scripts() {
    Rng rng{20261021};
    Record rec, model;
    bool hasScene = false;
    uint32_t verdicts[6][3] = {}, beforeScene = 0;
    const uint32_t kSteps = 6000;
    for (g_case = 0; g_case < kSteps; ++g_case) {
        const uint32_t op = (g_case == 40 || rng.below(12) == 0) ? 0u : 1u + rng.below(5);
        const uint32_t how = rng.below(4);  // 0: the record's own values, 1: something the entry refuses, else: new values
        const std::string before = Bytes(rec);
        Decision d;
        if (op == 0) {
            const uint32_t n = 1 + rng.below(12), nl = rng.below(4);
            std::vector<rt_sphere> sp(n);
            std::vector<rt_material> m(n);
            for (uint32_t k = 0; k < n; ++k) sp[k] = {rng.uni(-9.f, 9.f), rng.uni(-9.f, 9.f), rng.uni(-9.f, 9.f), rng.uni(0.1f, 1.2f)}, m[k] = MakeMaterial(rng);
            rt_light l[RT_MAX_LIGHTS] = {};
            for (uint32_t k = 0; k < nl; ++k) l[k] = MakeLight(rng);
            const rt_camera cam = MakeCamera(rng);
            const rt_material sky = MakeMaterial(rng);
            const float exposure = rng.uni(0.1f, 4.f);
            if (how == 1) sp[rng.below(n)].cx = kNaN;
            d = DecideUpload(&rec, sp.data(), m.data(), n, &cam, nl ? l : nullptr, nl, &sky);
            CHECK(d.verdict == (how == 1 ? Verdict::Refused : Verdict::Changed));
            if (d.verdict == Verdict::Changed) {
                rtprep::PrepOptions opt;
                opt.sgSph = rng.below(2) == 0;
                const rtprep::PreparedScene P = rtprep::PrepareScene(sp.data(), m.data(), n, l, nl, opt);
                CommitUpload(rec, sp.data(), m.data(), n, cam, l, nl, sky, exposure, P.layout, opt);
                model = Record{};  // the model: the arguments, stored
                model.n = n, model.spheres = sp, model.materials = m, model.sky = sky, model.camera = cam, model.nLights = nl, model.exposure = exposure;
                for (uint32_t k = 0; k < nl; ++k) model.lights[k] = l[k];
                model.shadowLayout = rtprep::ShadowLayoutOf(P.layout, opt), model.prepOpt = opt;
                CHECK(model.shadowLayout.orig.size() == P.layout.scan.size());
                hasScene = true;
            }
        } else if (op == 1) {
            rt_camera cam = how == 0 ? rec.camera : MakeCamera(rng);
            if (how == 1) cam.aperture = kInf;
            d = DecideSetCamera(&rec, hasScene, &cam);
            if (d.verdict == Verdict::Changed) CommitCamera(rec, cam), model.camera = cam;
        } else if (op == 2) {
            std::vector<rt_material> m = rec.materials;
            rt_material sky = rec.sky;
            const uint32_t n = how == 1 && rng.below(2) ? rec.n + 1 : rec.n;
            m.resize(n ? n : 1u, rt_material{});  // (never a null table: that is another refusal)
            if (how >= 2) {
                if (rng.below(3) != 0 && n) m[rng.below(n)] = MakeMaterial(rng);
                else sky = MakeMaterial(rng);
            }
            if (how == 1 && n == rec.n) sky.type = 4;
            d = DecideSetMaterials(&rec, hasScene, m.data(), n, &sky);
            if (d.verdict == Verdict::Changed) CommitMaterials(rec, d, m.data(), sky), model.materials = m, model.sky = sky;
        } else if (op == 3 || op == 4) {
            rt_light l[RT_MAX_LIGHTS];
            for (uint32_t k = 0; k < RT_MAX_LIGHTS; ++k) l[k] = rec.lights[k];
            uint32_t nl = rec.nLights;
            if (how >= 2 && nl) {
                rt_light& x = l[rng.below(nl)];
                const rt_light fresh = MakeLight(rng);
                for (int c = 0; c < 3; ++c) x.color[c] = fresh.color[c];
                if (op == 4 && rng.below(2)) std::memcpy(x.direction, fresh.direction, sizeof x.direction);
            }
            if (how == 1) {
                if (nl && rng.below(2)) l[rng.below(nl)].luminance = kNaN;
                else ++nl;
            }
            d = op == 3 ? DecideSetLights(&rec, hasScene, l, nl) : DecideTurnLights(&rec, hasScene, l, nl);
            if (d.verdict == Verdict::Changed) {
                CommitLights(rec, l);
                for (uint32_t k = 0; k < nl; ++k) model.lights[k] = l[k];
            }
        } else {
            const float e = how == 0 ? rec.exposure : (how == 1 ? kNaN : rng.uni(0.1f, 4.f));
            d = DecideSetExposure(&rec, hasScene, e);
            if (d.verdict == Verdict::Changed) CommitExposure(rec, e), model.exposure = e;
        }
        if (op != 0) {
            beforeScene += !hasScene;
            const Verdict want = !hasScene || how == 1 ? Verdict::Refused : (how == 0 ? Verdict::Same : Verdict::Changed);
            const bool noLights = (op == 3 || op == 4) && rec.nLights == 0;  // (nothing to change: the same)
            CHECK(d.verdict == want || (noLights && hasScene && how >= 2 && d.verdict == Verdict::Same));
            if (want == Verdict::Refused) CHECK(d.code == (hasScene ? RT_ERR_INVALID_ARG : RT_ERR_NO_SCENE));
        }
        CHECK((Bytes(rec) == before) == (d.verdict != Verdict::Changed) || op == 0);  // refused or the same record: nothing changed
        CHECK(Bytes(rec) == Bytes(model));
        CHECK((d.verdict == Verdict::Refused) == (d.code != RT_OK) && (d.verdict == Verdict::Refused) == !d.message.empty());
        ++verdicts[op][(int)d.verdict];
    }
    for (int op = 0; op < 6; ++op) CHECK(verdicts[op][(int)Verdict::Refused] > 0 && verdicts[op][(int)Verdict::Changed] > 0);
    for (int op = 1; op < 6; ++op) CHECK(verdicts[op][(int)Verdict::Same] > 0);
    CHECK(beforeScene > 0);
    g_case = kSteps;
    std::printf("scripts: %u steps (uploads %u; refused / same / changed: camera %u/%u/%u, materials %u/%u/%u, set_lights %u/%u/%u, turn_lights %u/%u/%u, "
                "exposure %u/%u/%u), %u edits before the first scene\n",
                kSteps, verdicts[0][2], verdicts[1][0], verdicts[1][1], verdicts[1][2], verdicts[2][0], verdicts[2][1], verdicts[2][2], verdicts[3][0], verdicts[3][1],
                verdicts[3][2], verdicts[4][0], verdicts[4][1], verdicts[4][2], verdicts[5][0], verdicts[5][1], verdicts[5][2], beforeScene);
}

// ---------------------------------------------------------------------------------------------------------------- 4
void CheckLayout(const StagePlan& plan) {
    size_t at = 0;
    for (const StageItem& it : plan.items) {
        CHECK(it.offset == at && it.offset % 16 == 0 && it.bytes <= it.dst.room);
        at += (it.bytes + 15) / 16 * 16;
    }
    CHECK(plan.total == at && plan.status == RT_OK && plan.message.empty());
}

void Plans() {
    Rng rng{5};
    char devMats, devMats16, devTypes, devBits;  // destinations: addresses that are handed through and never looked through
    const size_t kRoomy = (size_t)1 << 30;
    for (g_case = 0; g_case < 40; ++g_case) {
        const uint32_t n = 1 + rng.below(60);
        std::vector<rt_sphere> sp(n);
        std::vector<rt_material> m(n);
        const bool packable = g_case % 2 == 0;
        for (uint32_t k = 0; k < n; ++k) {
            sp[k] = {rng.uni(-9.f, 9.f), rng.uni(-9.f, 9.f), rng.uni(-9.f, 9.f), rng.uni(0.1f, 1.2f)};
            m[k] = rt_material{};
            m[k].rgb0[0] = packable ? 1.f : 0.123456f;
        }
        const rtprep::PreparedScene P = rtprep::PrepareScene(sp.data(), m.data(), n, nullptr, 0, rtprep::PrepOptions{});
        const size_t nPad = P.layout.orig.size();
        const rtprep::PreparedMaterials M = rtprep::PrepareMaterials(m.data(), n, P.layout.orig.data(), nPad);
        CHECK(M.mats16Ok == packable);
        const StagePlan plan = PlanMaterialStage(M, {&devMats, nPad * 48}, {&devMats16, nPad * 16}, {&devTypes, (size_t)n * 4});
        CheckLayout(plan);
        CHECK(plan.items.size() == 3);
        CHECK(plan.items[0].offset == 0 && plan.items[1].offset == nPad * 48 && plan.items[2].offset == nPad * 64);
        CHECK(plan.items[0].bytes == nPad * 48 && plan.items[1].bytes == nPad * 16 && plan.items[2].bytes == (size_t)n * 4);
        CHECK(plan.items[0].src == M.mats.data() && plan.items[1].src == M.mats16.data() && plan.items[2].src == M.matType.data());
        CHECK(plan.items[0].dst.ptr == &devMats && plan.items[2].dst.ptr == &devTypes);
        CHECK(plan.items[1].dst.ptr == (packable ? &devMats16 : nullptr));  // a table that is not valid is copied nowhere
        StageShape shape;
        shape.nPad = nPad, shape.n = n;
        CHECK(plan.total <= StageBytesMax(shape, rtprep::PrepOptions{}));
        const StagePlan tight = PlanMaterialStage(M, {&devMats, nPad * 48}, {&devMats16, nPad * 16 - 1}, {&devTypes, kRoomy});
        CHECK(tight.status == RT_ERR_HIP && tight.message == "rt_set_materials: a table is larger than the room the upload reserved for it");
    }
    for (uint32_t words : {1u, 3u, 37u, 2048u}) {
        const std::vector<uint32_t> table(words, 0x5a5a5a5au);
        const StagePlan plan = PlanForgetStage(table, {&devBits, kForgetTableWords * 4});
        CheckLayout(plan);
        CHECK(plan.items.size() == 1 && plan.items[0].bytes == 4 * (size_t)words && plan.items[0].src == table.data() && plan.items[0].dst.ptr == &devBits);
        CHECK(plan.total <= StageBytesMax(StageShape{}, rtprep::PrepOptions{}));
    }
    CHECK(PlanForgetStage(std::vector<uint32_t>(2049, 0u), {&devBits, kForgetTableWords * 4}).status == RT_ERR_HIP);
    // an index's tables, in the order light 0 -- lights 1 .. -- the far tier -- sgSph, the disabled ones left out
    {
        g_case = 100;
        std::vector<rt_sphere> sp;
        for (int a = -6; a < 6; ++a)
            for (int b = -6; b < 6; ++b) sp.push_back({(float)a, 0.3f, (float)b, 0.3f});
        sp.push_back({0.f, -1000.f, 0.f, 1000.f});
        const std::vector<rt_material> m(sp.size(), rt_material{});
        rt_light l[3] = {};
        l[0].direction[1] = 1.f, l[1].direction[0] = 0.6f, l[1].direction[1] = 0.8f;
        l[2].direction[1] = 3.f;  // no direction: no index
        rtprep::PrepOptions opt;
        const rtprep::PreparedScene P = rtprep::PrepareScene(sp.data(), m.data(), (uint32_t)sp.size(), l, 3, opt);
        const rtprep::PreparedShadows S = rtprep::PrepareShadows(sp.data(), rtprep::ShadowLayoutOf(P.layout, opt), l, 3, opt);
        CHECK(S.shadow.enabled && S.extraShadow.size() == 2 && S.extraShadow[0].enabled && !S.extraShadow[1].enabled);
        auto dest = [](uint32_t maxCells) {
            const ShadowRoom r = ShadowRoomOf(maxCells);
            return IndexDest{{nullptr, r.cellWords * 2}, {nullptr, r.entries * 2}, {nullptr, r.global * 2}};
        };
        const IndexDest extra[2] = {dest(opt.shadowCellsGlobal), dest(opt.shadowCellsGlobal)};
        const IndexDest light0 = dest(Light0CellsMax(P.layout.InGlobalMemory(), opt));
        const StagePlan plan = PlanShadowStage(S, light0, extra, dest(opt.shadowCellsGlobal), {nullptr, 0});
        CheckLayout(plan);
        CHECK(plan.items.size() == (S.shadowFar.enabled ? 9u : 6u));
        CHECK(plan.items[0].src == S.shadow.cellStart.data() && plan.items[0].bytes == S.shadow.cellStart.size() * 2);
        CHECK(plan.items[1].src == S.shadow.entries.data() && plan.items[2].src == S.shadow.global.data());
        CHECK(plan.items[3].src == S.extraShadow[0].cellStart.data() && plan.items[5].bytes == S.extraShadow[0].global.size() * 2);
        if (S.shadowFar.enabled) CHECK(plan.items[6].src == S.shadowFar.cellStart.data());
        StageShape shape;
        shape.nPad = P.layout.scan.size(), shape.n = (uint32_t)sp.size(), shape.nIdx = 3, shape.inGlobalMemory = P.layout.InGlobalMemory();
        CHECK(plan.total > 0 && plan.total <= StageBytesMax(shape, opt));
        IndexDest small = light0;
        small.entries.room = S.shadow.entries.size() * 2 - 2;
        const StagePlan refused = PlanShadowStage(S, small, extra, dest(opt.shadowCellsGlobal), {nullptr, 0});
        CHECK(refused.status == RT_ERR_HIP && refused.message == "rt_turn_lights: a table is larger than the room the upload reserved for it");
        // nothing enabled: nothing to stage
        opt.shadowGrid = false;
        const rtprep::PreparedShadows none = rtprep::PrepareShadows(sp.data(), rtprep::ShadowLayoutOf(P.layout, opt), l, 3, opt);
        const StagePlan empty = PlanShadowStage(none, light0, extra, dest(opt.shadowCellsGlobal), {nullptr, 0});
        CHECK(empty.items.empty() && empty.total == 0 && empty.status == RT_OK);
    }
    // the rooms and the bound, in figures
    const ShadowRoom r64 = ShadowRoomOf(64), r256 = ShadowRoomOf(256);
    CHECK(r64.cellWords == 64 * 64 + 1 && r256.cellWords == 256 * 256 + 1 && r64.entries == 65535 && r64.global == 65 && r256.entries == 65535 && r256.global == 65);
    rtprep::PrepOptions opt;
    CHECK(Light0CellsMax(false, opt) == 64 && Light0CellsMax(true, opt) == 256);
    CHECK(StageBytesMax(StageShape{}, opt) == kForgetTableWords * 4 && kForgetTableWords == 2048);
    auto up = [](size_t b) { return (b + 15) / 16 * 16; };
    const size_t lists = up(65535 * 2) + up(65 * 2), small = up(4097 * 2) + lists, large = up(65537 * 2) + lists;
    StageShape shape;
    shape.nPad = 8, shape.n = 5, shape.nIdx = 2;
    CHECK(StageBytesMax(shape, opt) == small + 2 * large);
    shape.inGlobalMemory = true;
    CHECK(StageBytesMax(shape, opt) == 3 * large);
    opt.sgSph = true;
    CHECK(StageBytesMax(shape, opt) == 3 * large + up(65535 * 16));
    shape.nIdx = 0, shape.nPad = 4000, shape.n = 3997;
    CHECK(StageBytesMax(shape, opt) == 4000 * 64 + up(3997 * 4));
    std::printf("plans: the material tables at 0, 48 nPad and 64 nPad, the forget table as one item, the indices in order on 16-byte boundaries\n");
}

}  // namespace

int main() {
    Refusals();
    SameRecord();
    Scripts();
    Plans();
    std::printf("scene_edit_selftest ok\n");
    return 0;
}
