// rt_scene_edit.cpp -- the scene record, the decisions of the upload and the edits, and the staging plan (rt_scene_edit.h).  Plain C++.
#include "rt_scene_edit.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace rtscene {

namespace {

Decision Refuse(int code, std::string message) {
    Decision d;
    d.verdict = Verdict::Refused, d.code = code, d.message = std::move(message);
    return d;
}
Decision Changed(bool table = false, bool sky = false) {
    Decision d;
    d.verdict = Verdict::Changed, d.table = table, d.sky = sky;
    return d;
}
Decision NoScene(const char* who) { return Refuse(RT_ERR_NO_SCENE, std::string(who) + ": no scene uploaded"); }

// The 14 floats of a camera record that the renderer reads, with their names; the fourth components are padding.
struct CameraField {
    const char* name;
    size_t offset;
    uint32_t count;
};
const CameraField kCameraFields[] = {{"origin", offsetof(rt_camera, origin), 3},
                                     {"x", offsetof(rt_camera, x), 3},
                                     {"y", offsetof(rt_camera, y), 3},
                                     {"origin_image_plane", offsetof(rt_camera, origin_image_plane), 3},
                                     {"aperture", offsetof(rt_camera, aperture), 1},
                                     {"focal_length", offsetof(rt_camera, focal_length), 1}};
const char* FieldOf(const rt_camera& c, const CameraField& f) { return reinterpret_cast<const char*>(&c) + f.offset; }

bool Finite3(const float v[3]) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }

// the material domain over a table and the sky, in the words of `who` (the rule itself is rt_scene_prep.cpp's)
bool MaterialsRefused(const char* who, const rt_material* materials, uint32_t n, const rt_material& sky, Decision* out) {
    uint32_t bad = 0;
    const char* field = nullptr;
    if (!rtprep::MaterialsInDomain(materials, n, &bad, &field))
        *out = Refuse(RT_ERR_INVALID_ARG, rtprep::MaterialFaultMessage(who, "sphere " + std::to_string(bad), materials[bad], field));
    else if ((field = rtprep::MaterialFault(sky)) != nullptr)
        *out = Refuse(RT_ERR_INVALID_ARG, rtprep::MaterialFaultMessage(who, "the sky", sky, field));
    else
        return false;
    return true;
}

size_t Align16(size_t bytes) { return (bytes + 15u) & ~(size_t)15u; }

struct PlanBuilder {
    StagePlan plan;
    const char* who;
    void Add(const void* src, size_t bytes, const TableDest& dst) {
        if (bytes > dst.room && plan.status == RT_OK)
            plan.status = RT_ERR_HIP, plan.message = std::string(who) + ": a table is larger than the room the upload reserved for it";
        plan.items.push_back({src, bytes, plan.total, dst});
        plan.total += Align16(bytes);
    }
    void Add(const rtprep::ShadowGrid& G, const IndexDest& dst) {
        if (!G.enabled) return;  // (a disabled index is copied nowhere: its constants are zero in the records)
        Add(G.cellStart.data(), G.cellStart.size() * sizeof(uint16_t), dst.cells);
        Add(G.entries.data(), G.entries.size() * sizeof(uint16_t), dst.entries);
        Add(G.global.data(), G.global.size() * sizeof(uint16_t), dst.global);
    }
};

// the slot's share of an index at its room
size_t IndexBytesMax(uint32_t maxCells) {
    const ShadowRoom r = ShadowRoomOf(maxCells);
    return Align16(r.cellWords * sizeof(uint16_t)) + Align16(r.entries * sizeof(uint16_t)) + Align16(r.global * sizeof(uint16_t));
}

}  // namespace

bool SameBits(const void* a, const void* b, size_t bytes) { return bytes == 0 || std::memcmp(a, b, bytes) == 0; }

// ------------------------------------------------------------------------------------------------------------------ decisions
Decision DecideUpload(const Record* rec, const rt_sphere* spheres, const rt_material* materials, uint32_t n, const rt_camera* camera,
                      const rt_light* lights, uint32_t n_lights, const rt_material* sky) {
    if (!rec || !spheres || !materials || !camera || (!lights && n_lights != 0) || !sky || n == 0)
        return Refuse(RT_ERR_INVALID_ARG, "rt_scene_upload: null pointer or empty scene");
    if (n_lights > RT_MAX_LIGHTS) return Refuse(RT_ERR_INVALID_ARG, "rt_scene_upload: more than RT_MAX_LIGHTS lights");
    uint32_t bad = 0;
    if (!rtprep::AllFinite(spheres, n, &bad))
        return Refuse(RT_ERR_INVALID_ARG, "rt_scene_upload: sphere " + std::to_string(bad) + " has a centre or a radius that is not finite");
    Decision d;
    if (MaterialsRefused("rt_scene_upload", materials, n, *sky, &d)) return d;
    return Changed();
}

Decision DecideSetCamera(const Record* rec, bool hasScene, const rt_camera* camera) {
    if (!rec || !camera) return Refuse(RT_ERR_INVALID_ARG, "rt_set_camera: null argument");
    if (!hasScene) return NoScene("rt_set_camera");
    for (const CameraField& f : kCameraFields)
        for (uint32_t k = 0; k < f.count; ++k) {
            float v;
            std::memcpy(&v, FieldOf(*camera, f) + k * sizeof(float), sizeof(float));
            if (!std::isfinite(v)) return Refuse(RT_ERR_INVALID_ARG, std::string("rt_set_camera: ") + f.name + " is not finite");
        }
    for (const CameraField& f : kCameraFields)
        if (!SameBits(FieldOf(*camera, f), FieldOf(rec->camera, f), f.count * sizeof(float))) return Changed();
    return Decision{};  // the same record: not an event (rt_set_sampler's precedent)
}

Decision DecideSetMaterials(const Record* rec, bool hasScene, const rt_material* materials, uint32_t n, const rt_material* sky) {
    if (!rec || !materials || !sky) return Refuse(RT_ERR_INVALID_ARG, "rt_set_materials: null argument");
    if (!hasScene) return NoScene("rt_set_materials");
    if (n != rec->n)
        return Refuse(RT_ERR_INVALID_ARG, "rt_set_materials: " + std::to_string(n) + " records for a scene of " + std::to_string(rec->n) + " spheres");
    Decision d;
    if (MaterialsRefused("rt_set_materials", materials, n, *sky, &d)) return d;
    // all 48 bytes of each record (the device tables hold them whole)
    const bool table = !SameBits(materials, rec->materials.data(), (size_t)n * sizeof(rt_material));
    const bool skyChanged = !SameBits(sky, &rec->sky, sizeof(rt_material));
    return table || skyChanged ? Changed(table, skyChanged) : Decision{};
}

Decision DecideLights(const Record* rec, bool hasScene, const char* who, bool mayTurn, const rt_light* lights, uint32_t n_lights) {
    const std::string name(who);
    if (!rec || (!lights && n_lights != 0)) return Refuse(RT_ERR_INVALID_ARG, name + ": null argument");
    if (!hasScene) return NoScene(who);
    if (n_lights != rec->nLights)
        return Refuse(RT_ERR_INVALID_ARG, name + ": " + std::to_string(n_lights) + " lights for a scene uploaded with " + std::to_string(rec->nLights));
    bool same = true;
    for (uint32_t k = 0; k < n_lights; ++k) {
        const rt_light& l = lights[k];
        const rt_light& was = rec->lights[k];
        const bool sameDirection = SameBits(l.direction, was.direction, sizeof l.direction);
        if (mayTurn && !Finite3(l.direction)) return Refuse(RT_ERR_INVALID_ARG, name + ": light " + std::to_string(k) + " has a direction that is not finite");
        if (!mayTurn && !sameDirection)
            return Refuse(RT_ERR_INVALID_ARG, name + ": light " + std::to_string(k) +
                                                  " has another direction than the uploaded one: a direction change needs an rt_scene_upload (the light's shadow index is built for its direction)");
        if (!std::isfinite(l.luminance) || !Finite3(l.color))
            return Refuse(RT_ERR_INVALID_ARG, name + ": light " + std::to_string(k) + " has a colour or a luminance that is not finite");
        same = same && sameDirection && SameBits(l.color, was.color, sizeof l.color) && SameBits(&l.luminance, &was.luminance, sizeof(float));
    }
    return same ? Decision{} : Changed();  // (n_lights == 0: the same)
}

Decision DecideSetExposure(const Record* rec, bool hasScene, float exposure_scale) {
    if (!rec) return Refuse(RT_ERR_INVALID_ARG, "rt_set_exposure: null ctx");
    if (!hasScene) return NoScene("rt_set_exposure");
    if (!std::isfinite(exposure_scale)) return Refuse(RT_ERR_INVALID_ARG, "rt_set_exposure: the exposure is not finite");
    return SameBits(&exposure_scale, &rec->exposure, sizeof(float)) ? Decision{} : Changed();
}

Decision GetCamera(const Record* rec, bool hasScene, rt_camera* out) {
    if (!rec || !out) return Refuse(RT_ERR_INVALID_ARG, "rt_get_camera: null argument");
    if (!hasScene) return NoScene("rt_get_camera");
    *out = rec->camera;
    return Decision{};
}

Decision GetLights(const Record* rec, bool hasScene, rt_light* out, uint32_t capacity, uint32_t* n_lights) {
    if (!rec || !n_lights || (!out && capacity != 0)) return Refuse(RT_ERR_INVALID_ARG, "rt_get_lights: null argument");
    if (!hasScene) return NoScene("rt_get_lights");
    *n_lights = rec->nLights;
    if (capacity == 0) return Decision{};  // the count alone
    if (capacity < rec->nLights) return Refuse(RT_ERR_INVALID_ARG, "rt_get_lights: capacity too small for " + std::to_string(rec->nLights) + " lights");
    for (uint32_t k = 0; k < rec->nLights; ++k) out[k] = rec->lights[k];
    return Decision{};
}

// ------------------------------------------------------------------------------------------------------------------ commits
void CommitUpload(Record& rec, const rt_sphere* spheres, const rt_material* materials, uint32_t n, const rt_camera& camera, const rt_light* lights,
                  uint32_t n_lights, const rt_material& sky, float exposure_scale, const rtprep::SceneLayout& layout, const rtprep::PrepOptions& opt) {
    rec.n = n;
    rec.spheres.assign(spheres, spheres + n);
    rec.materials.assign(materials, materials + n);
    rec.sky = sky;
    rec.camera = camera;
    rec.nLights = n_lights;
    CommitLights(rec, lights);
    rec.exposure = exposure_scale;
    rec.shadowLayout = rtprep::ShadowLayoutOf(layout, opt);
    rec.prepOpt = opt;
}
void CommitCamera(Record& rec, const rt_camera& camera) { rec.camera = camera; }
void CommitMaterials(Record& rec, const Decision& d, const rt_material* materials, const rt_material& sky) {
    if (d.table) rec.materials.assign(materials, materials + rec.n);
    rec.sky = sky;
}
void CommitLights(Record& rec, const rt_light* lights) {
    for (uint32_t k = 0; k < rec.nLights; ++k) rec.lights[k] = lights[k];
}
void CommitExposure(Record& rec, float exposure_scale) { rec.exposure = exposure_scale; }

// ------------------------------------------------------------------------------------------------------------------ staging
StagePlan PlanMaterialStage(const rtprep::PreparedMaterials& M, TableDest mats, TableDest mats16, TableDest matType) {
    PlanBuilder b{{}, "rt_set_materials"};
    if (!M.mats16Ok) mats16.ptr = nullptr;  // (the launch plan then reads no packed table)
    b.Add(M.mats.data(), M.mats.size() * sizeof(rt_material), mats);
    b.Add(M.mats16.data(), M.mats16.size() * sizeof(rtprep::U4), mats16);
    b.Add(M.matType.data(), M.matType.size() * sizeof(uint32_t), matType);
    return b.plan;
}

StagePlan PlanShadowStage(const rtprep::PreparedShadows& S, const IndexDest& light0, const IndexDest* extra, const IndexDest& far, TableDest sgSph) {
    PlanBuilder b{{}, "rt_turn_lights"};
    b.Add(S.shadow, light0);
    for (size_t k = 0; k < S.extraShadow.size(); ++k) b.Add(S.extraShadow[k], extra[k]);
    b.Add(S.shadowFar, far);
    if (!S.sgSph.empty()) b.Add(S.sgSph.data(), S.sgSph.size() * sizeof(rtprep::F4), sgSph);
    return b.plan;
}

StagePlan PlanForgetStage(const std::vector<uint32_t>& table, TableDest bits) {
    PlanBuilder b{{}, "rt_temporal_forget"};
    b.Add(table.data(), table.size() * sizeof(uint32_t), bits);
    return b.plan;
}

size_t StageBytesMax(const StageShape& shape, const rtprep::PrepOptions& opt) {
    const size_t forget = Align16(kForgetTableWords * sizeof(uint32_t));
    const size_t materials = Align16(shape.nPad * sizeof(rt_material)) + Align16(shape.nPad * sizeof(rtprep::U4)) + Align16(shape.n * sizeof(uint32_t));
    // light 0's first index, then one index in global memory per further light and one for light 0's far tier: nIdx of those
    size_t shadows = 0;
    if (shape.nIdx != 0u) {
        shadows = IndexBytesMax(Light0CellsMax(shape.inGlobalMemory, opt)) + (size_t)shape.nIdx * IndexBytesMax(opt.shadowCellsGlobal);
        if (opt.sgSph && shape.inGlobalMemory) shadows += Align16(rtprep::kShadowSphRecordsMax * sizeof(rtprep::F4));
    }
    return std::max(forget, std::max(materials, shadows));
}

}  // namespace rtscene
