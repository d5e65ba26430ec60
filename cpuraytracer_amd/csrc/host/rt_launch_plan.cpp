// rt_launch_plan.cpp -- see rt_launch_plan.h.  The order of the image's parts is the order rt_kernels.h carves them in: scene
// constants, per-wave work lists, the shadow index's global list, scene tables, one-sphere bounds, filter operands, shadow index,
// hierarchy, cells, quantised bounds, packed materials, and last the per-wave hit stashes or path caches.
#include "rt_launch_plan.h"

#include "../../../include/rt_api.h"
#include "../rt_layout_consts.h"

namespace rtplan {

namespace {

size_t Round16(size_t b) { return (b + 15) / 16 * 16; }
// scan records (16 B), original indices (4 B) and radii (4 B) per scan entry, and the 48-byte materials
size_t TableBytes(uint32_t nPadded, bool mats) { return (size_t)nPadded * (16 + 4) + (mats ? (size_t)nPadded * 48 : 0) + (size_t)nPadded * 4; }
size_t OpsBytes(uint32_t nGroups) { return (size_t)rtd::mfma_tiles_for(nGroups) * rtd::kOpsPerTile * 4; }
size_t CellBytes(const SceneShape& S) { return ((size_t)S.grid_nu * S.grid_nv + 1) * 2; }
size_t ShadowIndexBytes(const SceneShape& S) { return Round16(((size_t)S.sg_nx * S.sg_ny + 1 + S.sg_nentries + S.sg_nglobal) * 2); }

TracePlan Refuse(Refusal why) {
    static const struct {
        int code;
        const char* message;
    } kRefusals[] = {
        {RT_OK, nullptr},
        {RT_ERR_INVALID_ARG, "scenes beyond 65,000 spheres are not supported by the 16-bit candidate lists"},
        {RT_ERR_INVALID_ARG, "frame pipelining needs the flat LDS variant of the trace kernel"},
        {RT_ERR_HIP, "internal: materials through L2 without the stash variant"},
        {RT_ERR_HIP, "internal: the grid variant with the shadow index in LDS needs the hit stash"},
        {RT_ERR_HIP, "internal: quantised grid bounds without the stash variant"},
    };
    TracePlan P;
    P.refusal = why;
    P.status = kRefusals[(int)why].code;
    P.message = kRefusals[(int)why].message;
    return P;
}

}  // namespace

ScanChoice ChooseScan(const SceneShape& S, const Settings& C, uint32_t globSlots) {
    ScanChoice V{};
    const size_t tables = TableBytes(S.n_padded, C.matsInLds);
    const bool useLds = !C.forceGlobal && tables <= 48 * 1024 && S.n_padded < 65536;
    const uint32_t wavesPerBlock = C.blockThreads / 64;
    V.grid = C.useMfma && S.grid;                     // cell-grid scan (the scene was laid out for it at upload): tables in global memory (L2)
    V.tree = C.useMfma && !V.grid && S.n_levels > 1;  // deeper hierarchy: tables stay in global memory (L2)
    // the scene constants' slot comes first in the image, then the per-wave regions, then the shadow index's global list
    V.candBytes = rtd::kConstBytes + (size_t)wavesPerBlock * (V.grid ? rtd::kWaveGridBytes : (V.tree ? rtd::kWaveCandBytes : rtd::kWaveListBytes)) +
                  (size_t)globSlots * 16;
    // one-sphere bounds, staged next to the scan table: the flat scan's copy has kFlatLeafStride float4 per group (rt_scan.h), the grid's is dense
    V.leafBytes = (size_t)(S.n_padded / 4u) * (V.grid ? 4u : rtd::kFlatLeafStride) * 16;
    V.flat = !V.tree && !V.grid && useLds && C.useMfma && (V.candBytes + tables + V.leafBytes + OpsBytes(S.top_cnt)) <= kLdsPerCu;
    V.ldsTables = useLds && !V.tree && !V.grid;
    // a grid scene whose tables all fit LDS next to the grid scan's work lists (small scenes laid out for the grid: RT_GRID=2)
    V.gridLds = V.grid && useLds && C.matsInLds && C.blockThreads == 1024 && V.candBytes + tables + V.leafBytes + CellBytes(S) + 16 <= 128 * 1024;
    return V;
}

QueueCut CutQueue(uint32_t totalPaths, uint32_t wavesLaunched, uint32_t queueBlock, uint32_t staticBlocks) {
    QueueCut Q;
    Q.queue_block = queueBlock;
    Q.static_blocks = staticBlocks;
    const uint64_t total = totalPaths, qb = queueBlock;
    uint64_t begin = (uint64_t)wavesLaunched * qb * staticBlocks;
    if (begin > total) begin = total;
    Q.dyn_begin = (uint32_t)begin;
    Q.dyn_blocks = (uint32_t)((total - begin + qb - 1) / qb);
    return Q;
}

TracePlan PlanTrace(const SceneShape& S, const Settings& C, const Knobs& K, const Ask& A) {
    if (S.n_padded >= 65536) return Refuse(Refusal::TooManyEntries);
    TracePlan P;
    const bool ordinary = A.mode == Mode::Ordinary;
    P.mats_in_lds = C.matsInLds ? 1u : 0u;
    // packed materials (decided below, once it is known where the variant reads its materials from).  RT_MATS16: 0 (default) never, 1
    // from global memory wherever the 48-byte table would be read from there, 2 also staged into LDS by the flat stash variant.
    // Measured (C2, three interleaved rounds): 48-byte records through L2 9,983 / packed from global memory 9,972 / packed in LDS
    // with a 56-record stash 9,977 Msamples/s -- the material read is not what a hit waits for; C5: 7,579 -> 7,596; the unpacking adds 62 lane-operations per
    // sample (+1.3 % of the kernel's VALU instructions, tools/phase_budget.py): same time for more instructions, so it stays off.
    const bool want16 = S.mats16 && K.mats16 != 0u;
    P.sg_glob16 = S.sg_enabled ? rtd::sg_glob_slots(S.sg_nglobal) : 0u;

    // ---- the grid: one wave holds 64 paths; no more waves than there is work for, no more blocks than are resident at once
    const uint32_t maxBlocks = C.cuCount * C.blocksPerCu;
    const uint64_t wavesNeeded = ((uint64_t)A.total_paths + 63) / 64;
    const uint32_t wavesPerBlock = C.blockThreads / 64;
    uint32_t blocks = (uint32_t)((wavesNeeded + wavesPerBlock - 1) / wavesPerBlock);
    if (blocks > maxBlocks) blocks = maxBlocks;
    if (blocks == 0) blocks = 1;
    if (!ordinary) blocks = maxBlocks;  // carried paths may outnumber the fresh ones (a flush has none)
    P.blocks = blocks;
    if (ordinary) {
        // 128-path blocks; 256 once a wave will take more than ~32 of them anyway (measured: +0.7 % at 1200x800 spp 128, +0.8 % on C4,
        // +0.9 % on grid10k, neutral at spp 48, -1.7 % at spp 16, where the finer blocks balance the short launch's end better)
        uint32_t qb = K.queueBlock / 64u * 64u;
        if (qb == 0u) qb = (uint64_t)A.total_paths >= 8192ull * blocks * wavesPerBlock ? 2u * rtd::kQueueBlock : rtd::kQueueBlock;
        P.queue = CutQueue(A.total_paths, blocks * wavesPerBlock, qb, K.queueStatic);
    }

    // ---- the image: per-wave work lists + the scene tables when they fit + the filter operand image
    const ScanChoice V = ChooseScan(S, C, P.sg_glob16);
    const bool tree = V.tree, flat = V.flat, ldsTables = V.ldsTables, grid = V.grid;
    const size_t candBytes = V.candBytes, leafBytes = V.leafBytes, tables = TableBytes(S.n_padded, C.matsInLds), opsBytes = OpsBytes(S.top_cnt);
    const bool bigGroup = C.blockThreads == 1024;
    bool gridLds = V.gridLds;
    size_t sgBytes = ((flat || gridLds) && S.sg_enabled) ? ShadowIndexBytes(S) : 0;
    if (candBytes + tables + leafBytes + (flat ? opsBytes : 0) + sgBytes + (gridLds ? CellBytes(S) + 16 : 0) > kLdsPerCu) {
        sgBytes = 0;                         // index stays in global memory (L2)
        if (S.sg_enabled) gridLds = false;  // ... and the all-in-LDS grid variant needs it there
    }
    P.sg_in_lds = sgBytes ? 1u : 0u;
    size_t treeBytes = tree ? (size_t)(S.top_off + S.top_cnt) * 16 : 0;
    if (!C.treeInLds || candBytes + opsBytes + treeBytes > kLdsPerCu) treeBytes = 0;
    P.tree_in_lds = treeBytes ? 1u : 0u;
    // (the cells go to LDS in the 1024-thread variants; smaller workgroups -- a knob for experiments -- read them through L2)
    size_t gridBytes = (grid && bigGroup) ? Round16(CellBytes(S)) : 0;
    if (candBytes + gridBytes > kLdsPerCu) gridBytes = 0;
    P.grid_in_lds = gridBytes ? 1u : 0u;
    // what only the ordinary 1024-thread hit-stash kernels over a grid scene with its tables in global memory can take next to the cells
    const bool gridExtras = grid && !gridLds && gridBytes != 0 && C.useStash && ordinary && bigGroup && A.max_depth < 65536u;
    // ... RT_GRID_QUANT=1 (experiments; BASELINE configs[4]'s "LDS-tiled sphere list"): the QUANTISED one-sphere bounds behind the
    // cells (rt_scan.h GridQuant: the step loop then reads no global memory) when they leave room for a stash of at least 16 records.
    // Measured on grid10k (4096^2, spp 64): 40 KB of bounds leave 38 stash records
    // instead of 63; 7.59 -> 7.10 Gsamples/s, of which -3.8 % is the smaller stash (float4 bounds at 38 records: 7.31) and -2.8 %
    // the 17 extra operations per tested sphere that unpack the record -- the float4 bounds hit L1 95 % of the time, and what the
    // L1 serves per cycle was not the limit it looked like (profiles/r04_c5_placement.json).  Default off.
    // (The room is tested against the whole 160 KiB, the stash's capacity below against the budget of ONE of blocksPerCu blocks:
    // where they disagree the launch is refused -- ADVICE.md item 3, kept as it is.)
    size_t gridQBytes = 0;
    if (gridExtras && S.grid_quant && K.gridQuant != 0u && K.gridSgLds == 0u && K.stashCap >= 16u) {
        const size_t qb = Round16((size_t)S.n_padded * 4);
        if (candBytes + gridBytes + qb + (size_t)wavesPerBlock * 16 * rtd::kStashDwords * 4 + 256 <= kLdsPerCu) gridQBytes = qb;
    }
    // ... RT_GRID_SG_LDS=1 (experiments): the shadow index when that leaves a stash of at least 24 records.  Measured on grid10k:
    // 48.6 KB of index leave 31 records instead of 63: -5 % (6.47 vs 6.82 Gsamples/s) -- the full stash is worth more than the three
    // dependent L2 reads per shadow query it would save.
    bool gridSgLds = false;
    if (gridExtras && S.sg_enabled && K.gridSgLds != 0u) {
        const size_t sgb = ShadowIndexBytes(S);
        if (candBytes + gridBytes + sgb + (size_t)wavesPerBlock * 24 * rtd::kStashDwords * 4 + 256 <= kLdsPerCu) {
            gridSgLds = true;
            sgBytes = sgb;
        }
    }
    size_t ldsBytes = candBytes + ((ldsTables || gridLds) ? tables : 0) + ((flat || gridLds) ? leafBytes : 0) + ((flat || tree) ? opsBytes : 0) + sgBytes +
                      treeBytes + gridBytes + gridQBytes;
    ldsBytes = Round16(ldsBytes);

    // ---- the per-wave regions go last.  Hit stash (rt_kernels.h, kStash): the matrix-core variants at 1024 threads regroup their
    // hit processing through a per-wave stash of up to 63 hit records in the room the path cache would take -- as many records as
    // the LDS left over holds (RT_STASH=0: the path-cache variants; RT_STASH_CAP: fewer records).  depth shares its register with
    // the scan entry, hence max_depth < 65536.
    const size_t budget = kLdsPerCu / C.blocksPerCu;
    auto capFor = [&](size_t imageBytes) -> uint32_t {  // records per wave that fit behind an image of this size
        if (budget <= imageBytes) return 0u;
        const size_t room = (budget - imageBytes) / wavesPerBlock / 16 * 16;
        uint32_t c = (uint32_t)(room / (rtd::kStashDwords * 4));
        c = c > 63u ? 63u : c;
        return c > K.stashCap ? K.stashCap : c;
    };
    const bool stashKernel = C.useStash && ordinary && (flat || tree || grid) && bigGroup && A.max_depth < 65536u;
    // flat variant with the hit-processing tables provably in LDS (typed pointers: no flat loads) when they all fit
    const bool hitLds = flat && C.matsInLds && (sgBytes != 0 || !S.sg_enabled);
    uint32_t cap = capFor(ldsBytes);
    // Flat variant: when the material table's 48 bytes per sphere would buy at least eight more records per wave, the
    // materials are read through L2 instead (kMatsL2; measured on the cover scene: 44 -> 63 records, +1 %; RT_MATS_L2=0: never).
    // Decided on the candidate image WITHOUT touching ldsBytes: the smaller image is committed only together with the stash
    // variant that is built for it (the other flat kernels stage the material table and need its room).
    bool matsL2 = false;
    if (stashKernel && hitLds && K.matsL2 != 0u) {
        const size_t matBytes = (size_t)S.n_padded * 48;
        const uint32_t cap2 = matBytes <= ldsBytes ? capFor(ldsBytes - matBytes) : 0u;
        if (cap2 >= cap + 8u && cap2 >= 16u) {
            matsL2 = true;
            ldsBytes -= matBytes;
            cap = cap2;
            // ... and, RT_MATS16=2, their packed form into the room that leaves, when the stash keeps at least 48 records with it
            const size_t m16Bytes = (size_t)S.n_padded * 16;
            const uint32_t cap3 = capFor(ldsBytes + m16Bytes);
            if (want16 && K.mats16 >= 2u && cap3 >= 48u) {
                P.mats16_mode = 2u;
                ldsBytes += m16Bytes;
                cap = cap3;
            }
        }
    }
    const bool useStash = stashKernel && cap >= 16u;
    if (useStash) {
        P.stash_cap = cap;
        P.stash_process = K.stashProcess < cap ? K.stashProcess : cap;  // experiments: process hits from this many + 1 lanes on
        P.ray_cache_off16 = (uint32_t)(ldsBytes / 16);
        P.ray_cache_stride16 = (cap * rtd::kStashDwords * 4 + 15) / 16;
        ldsBytes += (size_t)wavesPerBlock * P.ray_cache_stride16 * 16;
    }
    if (matsL2 && !useStash) return Refuse(Refusal::MatsL2NoStash);
    // every other variant that reads its materials from GLOBAL memory takes the packed record from there (one 16-byte read per
    // hit instead of three); variants with the 48-byte table in LDS keep it
    const bool matsGlobal = matsL2 || tree || (grid && !gridLds) || !C.matsInLds || (!flat && !ldsTables && !gridLds);
    if (want16 && P.mats16_mode == 0u && matsGlobal) P.mats16_mode = 1u;
    // per-wave caches of prepared paths, when there is room left (RT_RAY_CACHE=0 disables them)
    if (!useStash && C.useRayCache && ldsBytes + (size_t)wavesPerBlock * rtd::kRayCacheBytes <= budget) {
        P.ray_cache_off16 = (uint32_t)(ldsBytes / 16);
        P.ray_cache_stride16 = rtd::kRayCacheBytes / 16;
        ldsBytes += (size_t)wavesPerBlock * rtd::kRayCacheBytes;
    }
    P.ldsBytes = ldsBytes;
    P.tree = tree, P.flat = flat, P.grid = grid, P.gridLds = gridLds, P.ldsTables = ldsTables;
    P.cacheOn = P.ray_cache_off16 != 0 && !useStash;
    P.candBytes = candBytes, P.tablesBytes = ldsTables ? tables : 0, P.leafBytes = flat ? leafBytes : 0, P.opsBytes = (flat || tree) ? opsBytes : 0;
    P.sgBytes = sgBytes, P.treeBytes = treeBytes;

    // ---- the kernel
    const bool cached = P.ray_cache_off16 != 0;
    TraceKernelId k{};
    k.lights = S.n_lights != 1u;
    k.kThreads = bigGroup ? 1024 : (C.blockThreads == 512 ? 512 : 256);
    if (!ordinary) {
        P.pipelines = hitLds && cached && bigGroup;
        if (!P.pipelines) return Refuse(Refusal::NoPipelining);
        k.kLds = k.kCache = k.kHitLds = k.kCarry = true;
        k.kScan = 1;
    } else if (grid) {
        const bool cellsLds = P.grid_in_lds != 0;  // (implies 1024 threads)
        k.kScan = 3;
        k.kLds = gridLds && cellsLds;
        if (!k.kLds && gridSgLds) {
            if (!useStash) return Refuse(Refusal::GridSgNoStash);
            k.kSgLds = true;
        } else if (!k.kLds && gridQBytes != 0) {
            if (!useStash) return Refuse(Refusal::GridQuantNoStash);
            k.kGridQ = true;
        }
        k.kHitLds = cellsLds;
        k.kStash = useStash && cellsLds;
        k.kCache = cached && (cellsLds || !bigGroup);  // (1024 threads without the cells in LDS: the one variant without either)
    } else {
        k.kScan = tree ? 2 : (flat ? 1 : 0);
        k.kLds = ldsTables;
        k.kHitLds = tree ? P.tree_in_lds != 0 : hitLds;
        k.kCache = cached;
        k.kStash = useStash;
        k.kMatsL2 = matsL2;
    }
    P.kernel = k;
    P.lastTraceSky = ordinary && useStash && !grid && !tree;  // kStash && kScan == 1 && !kCarry
    return P;
}

bool FarStateLean(const SceneShape& S, const Ask& A, const TracePlan& P, const FarStateAsk& F) {
    if (P.status != RT_OK || A.mode != Mode::Ordinary || F.forceFull) return false;
    if (F.pathList || F.travOut) return false;       // the lean kernels count no traversals per path
    if (!S.sg_enabled || !F.shadowGrid) return false;  // without an index every shadow ray waits for the scan: that is the far-hit state
    return FindLeanVariant(P.kernel) >= 0;
}

ScanOnlyPlan PlanScanOnly(const SceneShape& S, const Settings& C) {
    const ScanChoice V = ChooseScan(S, C, 0u);
    ScanOnlyPlan P{};
    const size_t waves = 256 / 64;
    P.ldsBytes = waves * (V.grid ? rtd::kWaveGridBytes : (V.tree ? rtd::kWaveCandBytes : rtd::kWaveListBytes));
    if (V.grid) {
        P.kernel = {false, 3};
    } else if (V.tree) {
        P.kernel = {false, 2};
        P.ldsBytes += OpsBytes(S.top_cnt);
        const size_t treeBytes = (size_t)(S.top_off + S.top_cnt) * 16;
        P.tree_in_lds = (C.treeInLds && P.ldsBytes + treeBytes <= kLdsPerCu) ? 1u : 0u;
        if (P.tree_in_lds) P.ldsBytes += treeBytes;
    } else {
        P.kernel = {V.ldsTables, V.flat ? 1 : 0};
        if (V.ldsTables) P.ldsBytes += TableBytes(S.n_padded, false);
        if (V.flat) P.ldsBytes += V.leafBytes + OpsBytes(S.top_cnt);
    }
    return P;
}

namespace {

// a packed case as its four records; false for inputs no context can have
bool UnpackCase(const uint32_t* in, SceneShape& S, Settings& C, Knobs& K, Ask& A) {
    S.n_padded = in[0], S.n_levels = in[1], S.top_cnt = in[2], S.top_off = in[3];
    S.grid = in[4] & 1u, S.grid_quant = in[4] & 2u, S.sg_enabled = in[4] & 4u, S.mats16 = in[4] & 8u;
    S.grid_nu = in[5], S.grid_nv = in[6];
    S.sg_nx = in[7], S.sg_ny = in[8], S.sg_nentries = in[9], S.sg_nglobal = in[10];
    S.n_lights = in[11];
    C.cuCount = in[12], C.blocksPerCu = in[13], C.blockThreads = in[14];
    C.useMfma = in[15] & 1u, C.matsInLds = in[15] & 2u, C.useRayCache = in[15] & 4u, C.useStash = in[15] & 8u, C.treeInLds = in[15] & 16u,
    C.forceGlobal = in[15] & 32u;
    K.mats16 = in[16], K.matsL2 = in[17], K.stashCap = in[18], K.stashProcess = in[19], K.gridQuant = in[20], K.gridSgLds = in[21],
    K.queueBlock = in[22], K.queueStatic = in[23];
    A.total_paths = in[24], A.max_depth = in[25];
    if (in[26] > 1u || in[27] != 0u || (in[4] >> 4) != 0u || (in[15] >> 6) != 0u) return false;
    A.mode = in[26] ? Mode::Carry : Mode::Ordinary;
    // what rt_create and rt_scene_upload guarantee
    if (C.blocksPerCu == 0u || C.blocksPerCu > 8u || C.blockThreads < 64u || C.blockThreads > 1024u || C.blockThreads % 64u != 0u || C.cuCount == 0u ||
        C.cuCount > 4096u || S.n_levels == 0u || S.n_levels > rtd::kMaxLevels || S.grid_nu > 65535u || S.grid_nv > 65535u || S.sg_nx > 65535u ||
        S.sg_ny > 65535u)
        return false;
    return true;
}

}  // namespace

int PlanPacked(const uint32_t* in, uint32_t* out) {
    SceneShape S;
    Settings C;
    Knobs K;
    Ask A;
    if (!UnpackCase(in, S, C, K, A)) return RT_ERR_INVALID_ARG;
    PackPlan(PlanTrace(S, C, K, A), PlanScanOnly(S, C), out);
    return RT_OK;
}

bool FarStateLeanPacked(const uint32_t* in, const FarStateAsk& F) {
    SceneShape S;
    Settings C;
    Knobs K;
    Ask A;
    if (!UnpackCase(in, S, C, K, A)) return false;
    return FarStateLean(S, A, PlanTrace(S, C, K, A), F);
}

uint32_t KernelWord(const TraceKernelId& k) {
    return (k.lights ? 1u : 0u) | (k.kLds ? 2u : 0u) | (k.kThreads == 1024 ? 2u : (k.kThreads == 512 ? 1u : 0u)) << 2 | (uint32_t)k.kScan << 4 |
           (k.kCache ? 1u << 6 : 0u) | (k.kHitLds ? 1u << 7 : 0u) | (k.kCarry ? 1u << 8 : 0u) | (k.kStash ? 1u << 9 : 0u) |
           (k.kMatsL2 ? 1u << 10 : 0u) | (k.kSgLds ? 1u << 11 : 0u) | (k.kGridQ ? 1u << 12 : 0u) | (FindTraceVariant(k) >= 0 ? 1u << 31 : 0u);
}

void PackCase(const SceneShape& S, const Settings& C, const Knobs& K, const Ask& A, uint32_t* in) {
    in[0] = S.n_padded, in[1] = S.n_levels, in[2] = S.top_cnt, in[3] = S.top_off;
    in[4] = (S.grid ? 1u : 0u) | (S.grid_quant ? 2u : 0u) | (S.sg_enabled ? 4u : 0u) | (S.mats16 ? 8u : 0u);
    in[5] = S.grid_nu, in[6] = S.grid_nv;
    in[7] = S.sg_nx, in[8] = S.sg_ny, in[9] = S.sg_nentries, in[10] = S.sg_nglobal;
    in[11] = S.n_lights;
    in[12] = C.cuCount, in[13] = C.blocksPerCu, in[14] = C.blockThreads;
    in[15] = (C.useMfma ? 1u : 0u) | (C.matsInLds ? 2u : 0u) | (C.useRayCache ? 4u : 0u) | (C.useStash ? 8u : 0u) | (C.treeInLds ? 16u : 0u) |
             (C.forceGlobal ? 32u : 0u);
    in[16] = K.mats16, in[17] = K.matsL2, in[18] = K.stashCap, in[19] = K.stashProcess, in[20] = K.gridQuant, in[21] = K.gridSgLds;
    in[22] = K.queueBlock, in[23] = K.queueStatic;
    in[24] = A.total_paths, in[25] = A.max_depth;
    in[26] = A.mode == Mode::Carry ? 1u : 0u;
    in[27] = 0u;
}

void PackPlan(const TracePlan& P, const ScanOnlyPlan& U, uint32_t* out) {
    for (uint32_t w = 0; w < kPlanWords; ++w) out[w] = 0u;
    out[26] = (U.kernel.kLds ? 1u : 0u) | (uint32_t)U.kernel.kScan << 1 | U.tree_in_lds << 3 | (FindScanVariant(U.kernel) >= 0 ? 1u << 4 : 0u);
    out[27] = (uint32_t)U.ldsBytes;
    out[0] = (uint32_t)P.status;
    out[1] = (uint32_t)P.refusal;
    if (P.status != RT_OK) return;
    out[2] = P.blocks, out[3] = (uint32_t)P.ldsBytes;
    out[4] = (uint32_t)P.candBytes, out[5] = (uint32_t)P.tablesBytes, out[6] = (uint32_t)P.leafBytes, out[7] = (uint32_t)P.opsBytes;
    out[8] = (uint32_t)P.sgBytes, out[9] = (uint32_t)P.treeBytes;
    out[10] = (P.tree ? 1u : 0u) | (P.flat ? 2u : 0u) | (P.grid ? 4u : 0u) | (P.gridLds ? 8u : 0u) | (P.ldsTables ? 16u : 0u) | (P.cacheOn ? 32u : 0u) |
              (P.lastTraceSky ? 64u : 0u) | (P.pipelines ? 128u : 0u);
    out[11] = P.mats_in_lds, out[12] = P.mats16_mode, out[13] = P.sg_glob16, out[14] = P.sg_in_lds, out[15] = P.tree_in_lds, out[16] = P.grid_in_lds;
    out[17] = P.ray_cache_off16, out[18] = P.ray_cache_stride16, out[19] = P.stash_cap, out[20] = P.stash_process;
    out[21] = P.queue.queue_block, out[22] = P.queue.static_blocks, out[23] = P.queue.dyn_begin, out[24] = P.queue.dyn_blocks;
    out[25] = KernelWord(P.kernel);
}

}  // namespace rtplan
