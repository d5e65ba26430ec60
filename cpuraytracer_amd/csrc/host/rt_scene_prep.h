// rt_scene_prep.h -- what a scene becomes before it reaches the device: the clustered layout of the scan (rt_scan.h), the
// shadow indices (rt_shade.h shadow_query) and the per-entry tables, as plain values on the host.  No HIP: rt_capi.hip copies a
// PreparedScene to the device, host/scene_prep_selftest.cpp checks its structure in a stand-alone program.
#pragma once

#include <stdint.h>

#include <string>
#include <vector>

#include "../../../include/rt_api.h"
#include "../rt_layout_consts.h"
#include "rt_error.h"

namespace rtprep {

// Sixteen bytes, laid out like HIP's float4 / uint4, which the device reads them as.
struct F4 {
    float x, y, z, w;
};
struct U4 {
    uint32_t x, y, z, w;
};

uint32_t EnvU32(const char* name, uint32_t dflt);

// Every setting the preparation takes from outside.  FromEnv() reads the environment at each call ("the environment of the
// moment": tests change the variables between calls).
struct PrepOptions {
    uint32_t treeTop = 128;           // RT_TREE_TOP (4..128): largest top level the matrix-core filter takes (four tiles of 32)
    bool shadowGrid = true;           // RT_SHADOW_GRID=0 keeps every shadow ray on the scan
    uint32_t shadowCellsLds = 64;     // cells per axis of an index staged into LDS next to the tables (flat scan, first light)
    uint32_t shadowCellsGlobal = 256; // RT_SHADOW_CELLS: ... of an index that stays in global memory (BuildShadowGrid)
    bool sgSph = false;               // RT_SG_SPH=1 (experiments): PreparedScene::sgSph
    bool singleDirect = true;         // RT_SINGLE_DIRECT=0 clears PreparedScene::singleMask
    double gridDensity = 1.0;         // RT_GRID_DENSITY (experiments): spheres per cell the cell grid aims at
    bool grid = true;                 // RT_GRID=0: always the bounds hierarchy
    bool gridForce = false;           // RT_GRID=2 (experiments): the cell grid for every scene it can be built for
    bool bigApart = true;             // RT_ALWAYS_BIG set: false -- no grid, and the big spheres stay inside the hierarchy
    bool treeBox = true;              // RT_TREE_BOX_OFF set: no box around the hierarchy
    static PrepOptions FromEnv();
};

// Clustered storage for the scan (rt_scan.h): spheres split by a k-d median tree into groups of four, unusually
// large spheres alone, every group with a conservative bounding sphere for the matrix-core filter.
struct SceneLayout {
    std::vector<F4> scan;         // 4 * nGroups + 4 entries
    std::vector<uint32_t> orig;   // same length
    std::vector<F4> leaf;         // same length: conservative bound of each single sphere (sphere-level filter)
    std::vector<F4> tree;         // bounds of every level, level 0 (the groups) first
    uint32_t levelOff[rtd::kMaxLevels] = {0}, levelCnt[rtd::kMaxLevels] = {0};
    uint32_t nLevels = 1;         // level nLevels-1 is the top level (<= topMax nodes), filtered on the matrix cores
    uint32_t nGroups = 0;         // = levelCnt[0], a multiple of 4
    float boundNorm = 0.f;        // max |C| + R
    unsigned long long singleMask[2] = {0ull, 0ull};  // groups of one sphere, in the flat scan's bitmap coordinates
    uint32_t nAlways = 0;         // hierarchy scan: leading big-sphere groups kept out of the hierarchy (tested for every ray)
    float treeBox[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};  // box around the spheres in the hierarchy (lo, hi, max |coordinate|)
    bool treeBoxOn = false;
    // cell-grid scan (rt_scan.h scan_list_grid): the small spheres sorted by home cell behind the big ones
    bool gridOn = false;
    std::vector<uint16_t> gridCellStart;  // [nu * nv + 1]
    uint32_t gridNu = 0, gridNv = 0, gridAxU = 0, gridAxV = 2;
    float gridG0u = 0.f, gridG0v = 0.f, gridInvH = 0.f, gridRmaxOverH = 0.f, gridBigNorm = 0.f;
    std::vector<uint32_t> gridQ;  // quantised one-sphere bounds per scan entry (rt_scan.h GridQuant), empty: none
    float gridQc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    bool InGlobalMemory() const { return gridOn || nLevels > 1; }  // cell-grid and hierarchy scans: the tables stay out of LDS
};

// Footprints of the spheres in the plane perpendicular to a light, binned into a uniform grid (rt_shade.h shadow_query).
struct ShadowGrid {
    std::vector<uint16_t> cellStart, entries, global;
    uint32_t nx = 0, ny = 0;
    float e1[3] = {0, 0, 0}, e2[3] = {0, 0, 0}, u0 = 0, v0 = 0, invCell = 0, p0sq = 0;
    bool enabled = false;
};

// The bounds of an index's tables whatever the light's direction (BuildShadowGridTier gives up, or halves maxCells, beyond them).  One
// place for the builder's tests and for whoever reserves room for an index whose direction is not yet known (rt_turn_lights).
constexpr size_t kShadowEntriesEnd = 65535;  // cell starts are 16-bit: an index has fewer entries than this
constexpr size_t kShadowGlobalMax = 64;      // ... and at most this many in its global list
constexpr size_t ShadowCellWordsMax(uint32_t maxCells) { return (size_t)maxCells * maxCells + 1; }  // cellStart: nx * ny + 1, nx, ny <= maxCells
constexpr size_t kShadowSphRecordsMax = kShadowEntriesEnd;  // sgSph: entries + 1

// Everything rt_scene_upload copies to the device.
struct PreparedScene {
    SceneLayout layout;
    // radius and material of every scan entry, in clustered order: the hit processing indexes them with the entry it
    // found, with no detour through the original index (one dependent load less; material i still belongs to sphere i).
    // The radii are the caller's signed ones (the normals divide by them); padding entries are zero.
    std::vector<float> radius;
    std::vector<rt_material> mats;
    std::vector<U4> mats16;         // the same table in 16 bytes per entry (rt_shade.h load_material16) ...
    bool mats16Ok = false;          // ... when every material of the scene fits the form
    std::vector<uint32_t> matType;  // material type by ORIGINAL sphere index (rt_tile_order_kernel classifies first hits by it)
    ShadowGrid shadow;                     // the first light's index (not enabled: no lights, switched off, or the scene does not suit)
    std::vector<ShadowGrid> extraShadow;   // one per light 1 .. n_lights - 1
    ShadowGrid shadowFar;                  // the first light's tier-2 index: hit points with p0sq(shadow) < |p|^2 <= p0sq(shadowFar); not enabled: none
    std::vector<F4> sgSph;                 // PrepOptions::sgSph: the scan record of every entry of `shadow` (+ one that never hits), else empty
    unsigned long long singleMask[2] = {0ull, 0ull};  // layout.singleMask, or zero (PrepOptions::singleDirect)
};

// A centre or a radius that is not finite: no bound can be built from it (the callers refuse the scene).
bool AllFinite(const rt_sphere* sp, uint32_t n, uint32_t* which);

// The material domain (include/rt_api.h at rt_material): type <= 3, tex_type <= 1, every field the record's type READS finite
// (smoothness: types 0-2; ior: type 2; luminance: type 3; rgb0: types 0, 1, 3; rgb1 and tiling: under a checker texture on types
// 0, 1, 3), and |tiling| <= 2^30 under a checker texture.  Fields the type does not read are not inspected.  nullptr: the
// record is inside the domain; else the name of its first offending field.
const char* MaterialFault(const rt_material& m);
// ... over a table: false, *which = the first offending record and *field = MaterialFault of it
bool MaterialsInDomain(const rt_material* mats, uint32_t n, uint32_t* which, const char** field);
// What the callers refuse a record with: "<who>: <what> is outside the material domain: <field> ..." (what: "sphere 7", "sky")
std::string MaterialFaultMessage(const char* who, const std::string& what, const rt_material& m, const char* field);

void BuildLayout(const rt_sphere* spheres, uint32_t n, const PrepOptions& opt, SceneLayout& L);
void BuildShadowGrid(const rt_sphere* spheres, const SceneLayout& L, const float lightDir[3], uint32_t maxCells, ShadowGrid& G);
// tier 1: the same; tier 2: the index for the hit points beyond tier 1's radius (rt_scene_prep.cpp states its radius and why)
// counts (optional): which of the builder's branches the call took, added to what is there (host/light_turn_selftest.cpp)
struct ShadowBuildCounts {
    uint64_t built = 0;          // calls from outside (the halving rule's own calls are not counted again)
    uint64_t notADirection = 0;  // |L| outside (0.5, 2): no index
    uint64_t basisSwitch = 0;    // |Lx| dominates: the basis starts from the y axis
    uint64_t noTier2 = 0;        // tier 2 asked for and P2 <= P0
    uint64_t onlyHuge = 0;       // no ordinary sphere: the 1 x 1 grid, everything in the global list
    uint64_t spilled = 0;        // footprints beyond the grid's extent -> global list
    uint64_t wide = 0;           // footprints over more than an eighth of the cells -> global list
    uint64_t halved = 0;         // too many entries and maxCells > 64: built again at maxCells / 2
    uint64_t gaveUp = 0;         // too many entries at 64 cells, or a global list beyond kShadowGlobalMax: no index
    uint64_t enabled = 0;
};
void BuildShadowGridTier(const rt_sphere* spheres, const SceneLayout& L, const float lightDir[3], uint32_t maxCells, uint32_t tier, ShadowGrid& G,
                         ShadowBuildCounts* counts = nullptr);

// The three tables that hold the materials, and nothing else of a scene: the 48-byte records in scan-entry order (padding entries
// zero), the same packed into 16 bytes where every record fits, and the type by ORIGINAL sphere index.  orig: the layout's table of
// nEntries scan entries (0xffffffff: padding).  The one writer of these tables: PrepareScene calls it with its own layout, and
// rt_set_materials with the layout kept from the upload, so an edit's tables are the upload's by construction.
struct PreparedMaterials {
    std::vector<rt_material> mats;
    std::vector<U4> mats16;  // nEntries records either way; past the first record that does not fit they are zero
    bool mats16Ok = false;
    std::vector<uint32_t> matType;
};
PreparedMaterials PrepareMaterials(const rt_material* materials, uint32_t n, const uint32_t* orig, size_t nEntries);

// Everything of a scene that a light's direction reaches: light 0's index, one index per further light, light 0's tier-2 index and the
// optional sgSph table (PreparedScene's members of the same names).  The one writer of these tables: PrepareScene calls it with its own
// layout, rt_turn_lights with the part of the layout kept from the upload (ShadowLayoutOf), so a turn's tables are an upload's by
// construction.  Reads of `opt`: shadowGrid, the two cell limits, sgSph.  lights may be null where n_lights == 0.
struct PreparedShadows {
    ShadowGrid shadow;
    std::vector<ShadowGrid> extraShadow;
    ShadowGrid shadowFar;
    std::vector<F4> sgSph;
};
PreparedShadows PrepareShadows(const rt_sphere* spheres, const SceneLayout& layout, const rt_light* lights, uint32_t n_lights, const PrepOptions& opt,
                               ShadowBuildCounts* counts = nullptr);
// What PrepareShadows reads of a layout, and nothing else of it: orig, nGroups, what InGlobalMemory() tests, and the scan records
// where opt.sgSph asks for them.
SceneLayout ShadowLayoutOf(const SceneLayout& layout, const PrepOptions& opt);

// spheres: n > 0, all finite (AllFinite).  A layout of 65,536 scan entries or more cannot be indexed by the 16-bit ids of the
// tables behind it: then only `layout` is filled, and the caller refuses the scene.
PreparedScene PrepareScene(const rt_sphere* spheres, const rt_material* materials, uint32_t n, const rt_light* lights, uint32_t n_lights,
                           const PrepOptions& opt);

uint32_t RowsetLocalRows(rt_rowset rs);
// ... or 0 where the row set reaches beyond the image's H rows
uint32_t RowsetRowsWithin(rt_rowset rs, uint32_t H);
// ... or 0 where the strip of a W x H image has more than 2^31 pixels: what the unit entries refuse as a "bad row set"
uint32_t UnitStripRows(rt_rowset rs, uint32_t W, uint32_t H);
// out[k] for k < n: the scan entry of original sphere k, shifted right by `shift` (2: its group in the flat scan), 0xffffffff: none
void EntryOfSphere(const uint32_t* orig, size_t nEntries, uint32_t n, uint32_t shift, uint32_t* out);

}  // namespace rtprep
