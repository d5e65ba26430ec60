// rt_scene_edit.h -- what a context remembers of its scene as the caller gave it, what rt_scene_upload and the edits that change one part
// of it without an upload (rt_set_camera, rt_set_materials, rt_set_lights, rt_turn_lights, rt_set_exposure) refuse, ignore or accept, and
// how the tables an edit copies are laid into a pinned staging slot.  No HIP: rt_capi.hip asks for a decision, does
// the device work and commits; host/scene_edit_selftest.cpp checks all of it in a stand-alone program.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../../include/rt_api.h"
#include "rt_scene_prep.h"

namespace rtscene {

// ---- the record: the arguments of the last accepted upload, each part replaced by the last accepted edit of it.  Read by the decisions,
// the getters and whoever needs the caller's own values; changed only by the Commit functions below.
struct Record {
    uint32_t n = 0;                      // spheres
    std::vector<rt_sphere> spheres;
    std::vector<rt_material> materials;  // by ORIGINAL sphere index
    rt_material sky{};
    rt_camera camera{};
    rt_light lights[RT_MAX_LIGHTS] = {};
    uint32_t nLights = 0;                // as the caller counted them
    float exposure = 0.f;
    // what the edits rebuild tables over: the part of the upload's layout that rtprep::PrepareShadows and PrepareMaterials look at
    // (rtprep::ShadowLayoutOf), and the upload's preparation options (the environment is not read again)
    rtprep::SceneLayout shadowLayout;
    rtprep::PrepOptions prepOpt;
};

// ---- the decisions.  Each is a function of the record, of whether a scene is uploaded and of the caller's arguments, and changes
// nothing.  rec == nullptr: the entry was called without a context.
enum class Verdict {
    Refused,  // code and message say why; nothing may happen
    Same,     // the record's own bytes again: not an event, nothing may happen
    Changed,  // the entry does its device work and then commits
};
struct Decision {
    Verdict verdict = Verdict::Same;
    int code = RT_OK;
    std::string message;
    bool table = false, sky = false;  // DecideSetMaterials, Changed: which of the material table and the sky record differ
};

// Every comparison of a decision: bit for bit, so -0.0f differs from 0.0f and a NaN equals itself.
bool SameBits(const void* a, const void* b, size_t bytes);

// (never Same.  The refusal of layouts beyond 65,535 scan entries needs the prepared layout and is rt_scene_upload's own.)
Decision DecideUpload(const Record* rec, const rt_sphere* spheres, const rt_material* materials, uint32_t n, const rt_camera* camera,
                      const rt_light* lights, uint32_t n_lights, const rt_material* sky);
// The 14 floats the renderer reads are inspected and compared; the fourth components of the four vectors are padding and are neither.
Decision DecideSetCamera(const Record* rec, bool hasScene, const rt_camera* camera);
Decision DecideSetMaterials(const Record* rec, bool hasScene, const rt_material* materials, uint32_t n, const rt_material* sky);
// The one validator of a light list.  who: the entry's name; mayTurn: a direction may differ from the one set last (it must be finite),
// else a direction that differs is refused.
Decision DecideLights(const Record* rec, bool hasScene, const char* who, bool mayTurn, const rt_light* lights, uint32_t n_lights);
inline Decision DecideSetLights(const Record* rec, bool hasScene, const rt_light* lights, uint32_t n_lights) {
    return DecideLights(rec, hasScene, "rt_set_lights", false, lights, n_lights);
}
inline Decision DecideTurnLights(const Record* rec, bool hasScene, const rt_light* lights, uint32_t n_lights) {
    return DecideLights(rec, hasScene, "rt_turn_lights", true, lights, n_lights);
}
Decision DecideSetExposure(const Record* rec, bool hasScene, float exposure_scale);

// The getters, whole: Refused, or Same with the answer written (a refused call writes nothing but GetLights' count, which is written
// before the capacity is judged).
Decision GetCamera(const Record* rec, bool hasScene, rt_camera* out);
Decision GetLights(const Record* rec, bool hasScene, rt_light* out, uint32_t capacity, uint32_t* n_lights);

// ---- the commits: one per entry, called after the device work has been ordered without error.
void CommitUpload(Record& rec, const rt_sphere* spheres, const rt_material* materials, uint32_t n, const rt_camera& camera, const rt_light* lights,
                  uint32_t n_lights, const rt_material& sky, float exposure_scale, const rtprep::SceneLayout& layout, const rtprep::PrepOptions& opt);
void CommitCamera(Record& rec, const rt_camera& camera);
void CommitMaterials(Record& rec, const Decision& d, const rt_material* materials, const rt_material& sky);
void CommitLights(Record& rec, const rt_light* lights);  // rt_set_lights and rt_turn_lights: the count is the record's
void CommitExposure(Record& rec, float exposure_scale);

// ---- the staging plan: where the tables of one edit lie in a pinned slot, and where each goes from there.
// The largest table rt_temporal_forget copies: one bit per id a scene can hold.
constexpr uint32_t kForgetMaxIds = 65536;
constexpr uint32_t kForgetTableWords = kForgetMaxIds / 32u;

// Room for the three tables of a shadow index of ANY direction, in 16-bit elements: the builder's own bounds (rt_scene_prep.h), read by
// whoever reserves device memory for an index and by the slot's bound below.  (entries, global: the lists with their spare element.)
struct ShadowRoom {
    size_t cellWords, entries, global;
};
constexpr ShadowRoom ShadowRoomOf(uint32_t maxCells) {
    return {rtprep::ShadowCellWordsMax(maxCells), rtprep::kShadowEntriesEnd, rtprep::kShadowGlobalMax + 1};
}
// The cell limit of light 0's first index: staged into LDS by the flat scan's kernels, else read in global memory.
inline uint32_t Light0CellsMax(bool inGlobalMemory, const rtprep::PrepOptions& opt) { return inGlobalMemory ? opt.shadowCellsGlobal : opt.shadowCellsLds; }

// A destination as the caller hands it in: the pointer is never looked through here.
struct TableDest {
    void* ptr = nullptr;  // null: the item is laid into the slot and copied nowhere
    size_t room = 0;      // bytes reserved at ptr
};
struct IndexDest {
    TableDest cells, entries, global;
};
struct StageItem {
    const void* src;
    size_t bytes;
    size_t offset;  // in the slot, a multiple of 16
    TableDest dst;
};
struct StagePlan {
    std::vector<StageItem> items;  // in the order their copies are ordered on the stream
    size_t total = 0;              // bytes of the slot the items take (0: nothing to stage)
    int status = RT_OK;            // not RT_OK: a table is larger than its room, `message` says whose; nothing may be copied
    std::string message;
};
// The three material tables: offsets 0, 48 and 64 bytes times the entry count.  The packed table is copied only where it is valid.
StagePlan PlanMaterialStage(const rtprep::PreparedMaterials& M, TableDest mats, TableDest mats16, TableDest matType);
// The tables of every enabled index -- light 0's, extra[k - 1] for light k >= 1, the far tier's -- and the sgSph records where there are any.
StagePlan PlanShadowStage(const rtprep::PreparedShadows& S, const IndexDest& light0, const IndexDest* extra, const IndexDest& far, TableDest sgSph);
StagePlan PlanForgetStage(const std::vector<uint32_t>& table, TableDest bits);

// What both slots must hold, from the upload alone: no plan of a later edit of that scene exceeds it.  A default StageShape is no scene
// at all (rt_create): the forget table.  nIdx: the lights that may have an index (0 where the shadow indices are switched off).
struct StageShape {
    size_t nPad = 0;  // scan entries
    uint32_t n = 0, nIdx = 0;
    bool inGlobalMemory = false;
};
size_t StageBytesMax(const StageShape& shape, const rtprep::PrepOptions& opt);

}  // namespace rtscene
