// rt_launch_plan.h -- what a launch of the trace kernels is, decided without a device: the dynamic LDS image (rt_kernels.h lays it
// out, rt_layout_consts.h holds the sizes both sides use), the TraceParams fields that describe it, the grid, and which of the
// instantiated variants (rt_trace_variants.h) runs.  Plain C++ with no HIP header and no environment: rt_capi.hip fills the inputs
// from its context and the RT_* knobs, applies the plan and launches; rt_unit_launch_plan and host/launch_plan_selftest.cpp run
// the same functions with no GPU.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../rt_trace_variants.h"

namespace rtplan {

constexpr size_t kLdsPerCu = 160 * 1024;  // what a workgroup can have, and what the workgroups of a CU share

// The uploaded scene, as far as a launch depends on it (TraceParams' scene part).
struct SceneShape {
    uint32_t n_padded = 0;           // scan entries
    uint32_t n_levels = 1;           // levels of the bounds hierarchy ...
    uint32_t top_cnt = 0, top_off = 0;  // ... and its top level: nodes, and first node in the table of all levels
    bool grid = false;               // the scene was laid out for the cell-grid scan ...
    uint32_t grid_nu = 0, grid_nv = 0;
    bool grid_quant = false;         // ... and has quantised one-sphere bounds
    bool sg_enabled = false;         // light 0 has a shadow index
    uint32_t sg_nx = 0, sg_ny = 0, sg_nentries = 0, sg_nglobal = 0;
    bool mats16 = false;             // the materials exist packed into 16 bytes
    uint32_t n_lights = 1;
};
// The context's settings (rt_create reads them from the environment once).
struct Settings {
    uint32_t cuCount = 0, blocksPerCu = 4, blockThreads = 256;
    bool useMfma = true, matsInLds = true, useRayCache = true, useStash = true, treeInLds = true, forceGlobal = false;
};
// The experiment knobs a launch reads (RT_MATS16, RT_MATS_L2, RT_STASH_CAP, RT_STASH_PROCESS, RT_GRID_QUANT, RT_GRID_SG_LDS,
// RT_QUEUE_BLOCK, RT_QUEUE_STATIC), at their defaults.
struct Knobs {
    uint32_t mats16 = 0, matsL2 = 1, stashCap = 63, stashProcess = 63, gridQuant = 0, gridSgLds = 0, queueBlock = 0, queueStatic = 1;
};
enum class Mode { Ordinary, Carry };  // Carry: the frame-pipelining kernel (its caller sets the queue fields and resets the cursors)
struct Ask {
    uint32_t total_paths = 0, max_depth = 0;
    Mode mode = Mode::Ordinary;
};

// Which scan a scene gets under these settings: hierarchy, flat (matrix-core filter over the groups, every table in LDS), cell
// grid, or else the VALU scan with (ldsTables) or without its tables in LDS.
struct ScanChoice {
    bool tree, flat, ldsTables, grid, gridLds;
    size_t candBytes, leafBytes;
};
// globSlots: float4 slots of the shadow index's global list in front of the tables (rt_layout_consts.h sg_glob_slots).  A trace
// launch passes what it stages; the tile masks, the closest-hit unit and the feature pass stage none and pass 0 -- within about
// 1 KiB of the 160 KiB limit their `flat` can therefore differ from the trace launch's (known).
ScanChoice ChooseScan(const SceneShape& S, const Settings& C, uint32_t globSlots);

// The queue of fresh paths (rt_params.h): the first static_blocks blocks of every launched wave are static, the remaining paths
// are cut into eight shards of whole blocks.
struct QueueCut {
    uint32_t queue_block = 0, static_blocks = 0, dyn_begin = 0, dyn_blocks = 0;
};
QueueCut CutQueue(uint32_t totalPaths, uint32_t wavesLaunched, uint32_t queueBlock, uint32_t staticBlocks);

// Launches that are refused: a scene the 16-bit lists cannot index; a pipelined launch of a scene that does not get the carrying
// variant; and three combinations the plan itself should not arrive at (internal errors).
enum class Refusal { None, TooManyEntries, NoPipelining, MatsL2NoStash, GridSgNoStash, GridQuantNoStash };
struct TracePlan {
    Refusal refusal = Refusal::None;
    int status = 0;                 // RT_OK, or the refusal's error code ...
    const char* message = nullptr;  // ... and its text; nothing else is valid then
    uint32_t blocks = 0;
    size_t ldsBytes = 0;
    // what the RT_VERBOSE line prints
    bool tree = false, flat = false, grid = false, gridLds = false, ldsTables = false, cacheOn = false;
    size_t candBytes = 0, tablesBytes = 0, leafBytes = 0, opsBytes = 0, sgBytes = 0, treeBytes = 0;
    // TraceParams fields
    uint32_t mats_in_lds = 0, mats16_mode = 0, sg_glob16 = 0, sg_in_lds = 0, tree_in_lds = 0, grid_in_lds = 0;
    uint32_t ray_cache_off16 = 0, ray_cache_stride16 = 0, stash_cap = 0, stash_process = 0;
    QueueCut queue;             // Mode::Ordinary only
    bool lastTraceSky = false;  // the kernel finishes empty-list planes itself (rt_kernels.h kSky)
    bool pipelines = false;     // Mode::Carry: this scene under these settings gets the variant that implements frame pipelining
    TraceKernelId kernel{};
};
TracePlan PlanTrace(const SceneShape& S, const Settings& C, const Knobs& K, const Ask& A);

// Far-hit state (rt_kernels.h kFarState): whether the planned kernel runs as its row's LEAN function (rt_trace_variants.h
// RT_TRACE_LEAN_VARIANTS), which answers the shadow ray of a hit point beyond the shadow index inside hit processing and keeps no
// per-path traversal count.  What is asked of the launch beyond the plan's inputs:
struct FarStateAsk {
    bool pathList = false;    // the launch traces an explicit path list (rt_unit_trace) ...
    bool travOut = false;     // ... or wants per-path traversal counts (TraceParams::trav_out)
    bool shadowGrid = true;   // the context builds shadow indices (RT_SHADOW_GRID is not 0)
    bool forceFull = false;   // RT_FAR_STATE=1: the kernels with far-hit state, everywhere (A/B runs, knob tests)
};
// Lean: an ordinary picture launch -- no path list, no trav_out -- of a scene whose light 0 has a shadow index, on a row of the lean
// list, with the knob at rest.  Everything else keeps the full state: a disabled index (a light list without one, RT_SHADOW_GRID=0:
// every shadow ray then takes the scan, which IS the far-hit state), path lists and rt_unit_trace, the frame-pipelining kernel, the
// cell-grid and hierarchy scans, the kernels without hit stash.  Does not change the plan: image, grid and kernel word are the row's.
bool FarStateLean(const SceneShape& S, const Ask& A, const TracePlan& P, const FarStateAsk& F);
// ... for a packed case of rt_unit_launch_plan (false for a case PlanPacked refuses): rt_unit_far_state_plan
bool FarStateLeanPacked(const uint32_t* in, const FarStateAsk& F);

// The unit kernels (k_unit_closest, rt_features_kernel): the scan a trace launch would run, 256 threads, the LDS image of four
// waves with the hit-processing tables left out.
struct ScanOnlyPlan {
    ScanKernelId kernel;
    size_t ldsBytes;
    uint32_t tree_in_lds;
};
ScanOnlyPlan PlanScanOnly(const SceneShape& S, const Settings& C);

// rt_unit_launch_plan's words (include/rt_api.h documents them)
constexpr uint32_t kCaseWords = 28, kPlanWords = 28;
int PlanPacked(const uint32_t* in, uint32_t* out);  // one case; RT_ERR_INVALID_ARG (nothing written) for inputs no context can have
// The two halves of those words on their own: PlanPacked answers through PackPlan, and the launcher (rt_capi.hip LaunchTrace) keeps
// the case it planned and the plan it applied through both, for rt_unit_last_trace_launch.  PackCase is the inverse of PlanPacked's
// reading of a case: PlanPacked(PackCase(S, C, K, A)) == PackPlan(PlanTrace(S, C, K, A), PlanScanOnly(S, C)) for every context.
uint32_t KernelWord(const TraceKernelId& k);  // word [25]
void PackCase(const SceneShape& S, const Settings& C, const Knobs& K, const Ask& A, uint32_t* in);
void PackPlan(const TracePlan& P, const ScanOnlyPlan& U, uint32_t* out);

}  // namespace rtplan
