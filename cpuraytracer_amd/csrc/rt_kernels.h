// rt_kernels.h — HIP kernels of the render-loop hot path for MI355X (gfx950 / CDNA4).
// Device functions live in rt_params.h (parameters, ray generation), rt_scan.h (filter + resolve), rt_shade.h (hit
// processing, shadow index) and rt_device_math.h (DirectXMath restatements, Halton, RNG, elementary functions).
//
// What runs where (reference file:line -> kernel):
//   GenerateRays            spheres-app.cpp:132-161  -> gen_primary_ray()           (64 paths at a time into a per-wave LDS cache)
//   for_each(par) trace     spheres-app.cpp:177-184  -> rt_trace_kernel             (persistent-threads megakernel)
//   GetHitColor recursion   spheres-app.cpp:238-257  -> per-lane state machine in rt_trace_kernel
//   BvhNode/Sphere::Intersect ray-tracing.cpp:42-84,174-214 -> scan_list_mfma() (filter + pooled resolve) / scan_list_deferred()
//   Material::Scatter x3    material.cpp:20-164      -> scatter_only()
//   DirectionalLight::Shade light.cpp:11-42          -> shadow_query() (exact footprint index) + shade_value()
//   hdr[id] += L*exposure   spheres-app.cpp:182-183  -> rt_accumulate_kernel        (ordered in s)
//   tonemap transform(par)  spheres-app.cpp:196-214  -> rt_resolve_kernel
//
// Design (DESIGN.md §5 has the long form and the conservativeness argument):
//   * one work-item per (pixel, sample) PATH; a wave keeps 64 paths in flight and refills finished
//     lanes (ballot + prefix count) from a per-wave LDS cache of 64 prepared paths that all 64 lanes
//     generate together from the wave's block of a global queue, so lanes stay full despite path
//     lengths of 1..51 closest-hit scans;
//   * shadow rays are answered at the hit by an exact footprint index (spheres binned in the plane
//     perpendicular to the sun); far hit points fall back to a second scan ("needs shadow scan"
//     lane state) — the same booleans as the reference's any-hit either way;
//   * the scan is a conservative FILTER followed by an EXACT resolve.  Spheres are stored in k-d
//     groups of four with a bounding sphere each; "which ray may hit which group" is a K = 4 dense
//     contraction evaluated on the matrix cores with split-bf16 operands
//     (v_mfma_f32_32x32x16_bf16); rejected bits are shifted into register bitmaps, the wave's
//     (ray, group) pairs are pooled in an LDS work list, filtered per sphere with the same
//     conservative formula, and the surviving (ray, sphere) pairs evaluate Sphere::Intersect in the
//     reference's operation order, merged per ray with an LDS 64-bit minimum.  The image equals an
//     exhaustive scan bit for bit; scene tables, operand image, work lists and scene constants live
//     in LDS (measured: VALU ops with SGPR sources issue at half rate on gfx950, so scene data must
//     arrive in VGPRs);
//   * xoshiro128** state in 4 VGPRs per lane;
//   * per-path results go to an HBM sample buffer [tile of 64 pixels][sample][pixel] (12 B each) and are summed in
//     increasing s by rt_accumulate_kernel: the reference's summation order, bit for bit.
#pragma once

#include "rt_params.h"
#include "rt_scan.h"
#include "rt_shade.h"
#include "rt_tile_mask.h"
#include "rt_noise.h"
#include "rt_features.h"

namespace rtd {

enum : uint32_t { kIdle = 0u, kNeedClosest = 1u, kNeedShadow = 2u, kHaveHit = 3u };  // kHaveHit: hit-stash variant only (below)

// Hit stash (kStash variants of rt_trace_kernel): one record per closest hit that waits for its hit processing --
// hit position, ray direction, throughput, radiance, stream state, sample slot, depth | scan entry << 16, traversals.
// Field k of record r sits at dword k * cap + r of the wave's region: consecutive records, consecutive banks.
static_assert(kStashDwords == 4 * 3 + 4 + 3, "rt_layout_consts.h: four three-vectors, the stream state, slot, depth | entry, traversals");

// Work-item index -> (column i, global row j, sample s) and the path's slot in the sample buffer: the explicit path
// list of the unit tests, or the tiled order below over the rows of this shard.  slot = index either way.
// The tiled order's arithmetic for any source of its constants (member names of TraceParams): the kernel arguments, or the copy the
// kernels without far-hit state read back from LDS (LeanCoords below), which never have a path list.
template <class P>
RT_DEV void tiled_coordinates(const P& p, uint32_t q, uint32_t& i, uint32_t& j, uint32_t& s, uint32_t& slot) {
    // storage order = [tile of 64 local pixels][sample of the pass][pixel in tile] (the last tile is as wide as the
    // pixels left): a wave's block of 128 consecutive work-items is two sample planes of one tile, so its 12-byte
    // results fill whole cache lines, and rt_accumulate_kernel reads 768 contiguous bytes per plane.  The WORK order
    // is the same with the full tiles permuted by tile_order (expensive tiles first, sky last: rt_tile_order_kernel),
    // so that the 51-segment paths are not the last ones a launch starts; the partial tile stays last.
    const uint32_t tileSpan = 64u * p.spp_pass;
    const uint32_t nFull = p.npix_local >> 6;
    const uint32_t tileW = fastdiv(q, p.fd_tile);
    uint32_t pl, k;
    slot = q;
    if (tileW < nFull) {
        const uint32_t rem = q - tileW * tileSpan;
        const uint32_t tile = p.tile_order ? p.tile_order[tileW] : tileW;
        k = rem >> 6;
        pl = (tile << 6) + (rem & 63u);
        slot = tile * tileSpan + rem;
    } else {
        RT_SITE(K_PARTIAL);
        const uint32_t rem = q - nFull * tileSpan;
        const uint32_t wl = p.npix_local - (nFull << 6);
        k = rem / wl;
        pl = (nFull << 6) + (rem - k * wl);
    }
    s = p.s0 + k;
    const uint32_t lr = fastdiv(pl, p.fd_w);
    i = pl - lr * p.W;
    j = rowset_global_row(p.rs, lr, p.fd_rows);
    slot += p.sample_base;  // the call's region of the sample ring (0 without frame pipelining)
}
RT_DEV void path_coordinates(const TraceParams& p, uint32_t q, uint32_t& i, uint32_t& j, uint32_t& s, uint32_t& slot) {
    if (p.path_list) {
        RT_SITE(K_PATHLIST);
        i = p.path_list[3 * q];
        j = p.path_list[3 * q + 1];
        s = p.path_list[3 * q + 2];
        slot = q;
    } else {
        tiled_coordinates(p, q, i, j, s, slot);
    }
}
// What tiled_coordinates and the fresh-plane code read of a launch, read back from LDS (rt_params.h, "the launch constants of the
// kernels without far-hit state"): a and b are chunks 0 and 1.  kUniform: as scalars (the wave-uniform control code of K_GEN_TILE);
// else as each lane's own temporaries (the per-lane index arithmetic, where an SGPR source would halve the VALU rate).
struct LeanCoords {
    const uint32_t* tile_order;
    const uint32_t* tile_masks;
    const uint16_t* tile_spheres;
    FastDiv fd_tile, fd_w, fd_rows;
    uint32_t npix_local, spp_pass, sample_base, sky_skip, W, s0;
    uint64_t seed;
    rt_rowset rs;
};
template <bool kUniform>
RT_DEV LeanCoords lean_coords(const SceneConsts& K, const uint32_t* a, const uint32_t* b) {
    auto w = [](const uint32_t* at) -> uint32_t { return kUniform ? lds_uniform(at) : *at; };
    LeanCoords c;
    c.tile_order = lds_global<const uint32_t>(a + kLeanPlaneTileOrder, kUniform);
    c.tile_masks = lds_global<const uint32_t>(a + kLeanPlaneTileMasks, kUniform);
    c.tile_spheres = lds_global<const uint16_t>(a + kLeanPlaneTileSpheres, kUniform);
    c.fd_tile = FastDiv{w(a + kLeanPlaneFdTile), w(a + kLeanPlaneFdTile + 1)};
    c.fd_w = FastDiv{w(a + kLeanPlaneFdW), w(a + kLeanPlaneFdW + 1)};
    c.fd_rows = FastDiv{w(b + kLeanQueueFdRows), w(b + kLeanQueueFdRows + 1)};
    c.npix_local = w(a + kLeanPlaneNpix); c.spp_pass = w(a + kLeanPlaneSpp); c.sample_base = w(a + kLeanPlaneSampleBase);
    c.sky_skip = w(a + kLeanPlaneSkySkip);
    c.W = w(&K.W); c.s0 = w(&K.s0);
    c.seed = (uint64_t)w(a + kLeanPlaneSeed) | (uint64_t)w(a + kLeanPlaneSeed + 1) << 32;
    c.rs.first_row = w(b + kLeanQueueRsFirst); c.rs.num_rows = 0u; c.rs.block_rows = w(b + kLeanQueueRsBlockRows);
    c.rs.shard = w(b + kLeanQueueRsShard); c.rs.nshards = w(b + kLeanQueueRsNshards);
    return c;
}

// Scene tables as the scan and the hit processing read them: LDS copies when the launch staged them, else global (L2).
struct SceneTabs {
    const float4* scan;
    const uint32_t* orig;
    const float4* leaf;
    const float* rad;
    const rt_material* mats;
    const uint4* mats16;    // packed materials in LDS (kMatsL2 variants with p.mats16_mode == 2), else null
    const float* ops;       // filter operand image of the top level (matrix-core scans)
    const float4* tree;
    const uint16_t *sgCell, *sgEntries, *sgGlobal;
    const uint16_t* gridCells;  // cell-grid scan: first scan entry per cell
    const uint32_t* gridQ;      // ... and (kGridQ) the quantised one-sphere bounds in LDS
    uint32_t nTop, nTiles;
};

// Workgroup prologue shared by the megakernel and the closest-hit unit kernel: copy the scene tables the variant keeps in
// LDS to tabBase (16-byte aligned pieces: scan | one-sphere bounds (flat matrix-core scan only) | orig | materials (48 B =
// 3 float4) | radii | filter operands | shadow index; tree mode: operands | all levels of bounds) and build the filter's
// operand image.  Every thread of the workgroup must call it.
// kHitLds: flat matrix-core variant -- the material table and the shadow index are in LDS too; hierarchy variant -- all
// levels of bounds are in LDS.  Their pointers are assigned unconditionally so that the compiler can prove the address space -- a pointer that is LDS or global
// depending on a run-time flag becomes a FLAT load, and every flat load waits for vmcnt(0) AND lgkmcnt(0), i.e. also
// for the previous iteration's sample stores.  The host launches it only when p.mats_in_lds and (p.sg_in_lds or no index).
// kMatsL2 (with kHitLds): the material table is NOT staged -- it is read through L2 with a global-address-space pointer, and
// the 48 bytes per sphere it would take go to the hit stash (on the cover scene 44 -> 63 records per wave).
// kSgLds (cell-grid scan with its tables in global memory): the shadow index is staged behind the cells (typed LDS pointers).
template <bool kLds, int kScan, bool kHitLds = false, bool kMatsL2 = false, bool kSgLds = false, bool kGridQ = false>
RT_DEV void stage_scene(const TraceParams& p, float4* tabBase, SceneTabs& T) {
    constexpr bool kMfma = kScan == 1 || kScan == 2;
    T.gridCells = p.grid_cell_start;
    T.gridQ = nullptr;
    T.scan = p.scan;
    T.orig = p.orig;
    T.leaf = p.leaf;
    T.rad = p.radius;
    T.mats = p.mats;
    T.mats16 = nullptr;
    T.ops = nullptr;
    T.tree = p.tree;
    T.sgCell = p.sg_cell_start;
    T.sgEntries = p.sg_entries;
    T.sgGlobal = p.sg_global;
    const uint32_t topLevel = p.n_levels - 1u;
    const uint32_t nTop = p.level_cnt[topLevel];
    const uint32_t nTiles = mfma_tiles_for(nTop);  // even; nTop <= 128 => at most four
    T.nTop = nTop;
    T.nTiles = nTiles;
    if (kLds) {
        float4* ldsScan = tabBase;
        float4* ldsLeaf = ldsScan + p.n_padded;
        constexpr bool kLeafLds = kScan == 1 || kScan == 3;  // the scans that test one-sphere bounds from LDS
        // (the flat scan keeps the bounds at kFlatLeafStride float4 per group of four: rt_scan.h)
        constexpr uint32_t kLeafStride = kScan == 1 ? kFlatLeafStride : 4u;
        uint32_t* ldsOrig = reinterpret_cast<uint32_t*>(ldsLeaf + (kLeafLds ? (p.n_padded / 4u) * kLeafStride : 0u));
        float4* ldsMat = reinterpret_cast<float4*>(ldsOrig + p.n_padded);  // n_padded is a multiple of 4
        const uint32_t nMatLds = kMatsL2 ? 0u : ((kHitLds || p.mats_in_lds) ? p.n_padded : 0u);
        // (kMatsL2: the 48-byte table stays in global memory; its 16-byte packed form takes the place when the launch says so)
        const uint32_t nMat16 = (kMatsL2 && p.mats16_mode == 2u) ? p.n_padded : 0u;
        float* ldsRad = reinterpret_cast<float*>(ldsMat + (size_t)nMatLds * 3 + nMat16);
        const float4* gMat = reinterpret_cast<const float4*>(p.mats);
        for (uint32_t k = threadIdx.x; k < p.n_padded; k += blockDim.x) {
            ldsScan[k] = p.scan[k];
            ldsOrig[k] = p.orig[k];
            if (kLeafLds) ldsLeaf[(k >> 2) * kLeafStride + (k & 3u)] = p.leaf[k];
        }
        for (uint32_t k = threadIdx.x; k < nMatLds * 3; k += blockDim.x) ldsMat[k] = gMat[k];
        if (kMatsL2) {
            const float4* g16 = reinterpret_cast<const float4*>(p.mats16);
            for (uint32_t k = threadIdx.x; k < nMat16; k += blockDim.x) ldsMat[k] = g16[k];
            T.mats16 = reinterpret_cast<const uint4*>(ldsMat);
        }
        for (uint32_t k = threadIdx.x; k < p.n_padded; k += blockDim.x) ldsRad[k] = p.radius[k];
        if (kScan == 3) {
            // cell-grid scan with every table in LDS (kHitLds by construction): the cells' first entries, then the shadow index
            uint16_t* gc = reinterpret_cast<uint16_t*>(ldsRad + p.n_padded);
            const uint32_t ng = p.grid_nu * p.grid_nv + 1u;
            for (uint32_t k = threadIdx.x; k < ng; k += blockDim.x) gc[k] = p.grid_cell_start[k];
            T.gridCells = gc;
            uint16_t* g = gc + ((ng + 7u) & ~7u);  // 16-byte steps
            const uint32_t nc = p.sg_nx * p.sg_ny + 1u;
            if (p.sg_enabled) {
                for (uint32_t k = threadIdx.x; k < nc; k += blockDim.x) g[k] = p.sg_cell_start[k];
                for (uint32_t k = threadIdx.x; k < p.sg_nentries; k += blockDim.x) g[nc + k] = p.sg_entries[k];
                for (uint32_t k = threadIdx.x; k < p.sg_nglobal; k += blockDim.x) g[nc + p.sg_nentries + k] = p.sg_global[k];
            }
            T.sgCell = g;
            T.sgEntries = g + nc;
            T.sgGlobal = g + nc + p.sg_nentries;
        }
        if (kMfma) {
            float* ldsOps = ldsRad + p.n_padded;  // a multiple of 4
            build_mfma_operands(p.tree + p.level_off[topLevel], nTop, nTiles, ldsOps, threadIdx.x, blockDim.x);
            T.ops = ldsOps;
            if (kHitLds) {
                // typed LDS pointers, staged only when the scene has an index (the pointers are never read otherwise)
                uint16_t* g = reinterpret_cast<uint16_t*>(ldsOps + (size_t)nTiles * kOpsPerTile);
                const uint32_t nc = p.sg_nx * p.sg_ny + 1u;
                if (p.sg_enabled) {
                    for (uint32_t k = threadIdx.x; k < nc; k += blockDim.x) g[k] = p.sg_cell_start[k];
                    for (uint32_t k = threadIdx.x; k < p.sg_nentries; k += blockDim.x) g[nc + k] = p.sg_entries[k];
                    for (uint32_t k = threadIdx.x; k < p.sg_nglobal; k += blockDim.x) g[nc + p.sg_nentries + k] = p.sg_global[k];
                }
                T.sgCell = g;
                T.sgEntries = g + nc;
                T.sgGlobal = g + nc + p.sg_nentries;
            } else if (p.sg_enabled && p.sg_in_lds) {  // shadow index after the operand image
                uint16_t* g = reinterpret_cast<uint16_t*>(ldsOps + (size_t)nTiles * kOpsPerTile);
                const uint32_t nc = p.sg_nx * p.sg_ny + 1u;
                for (uint32_t k = threadIdx.x; k < nc; k += blockDim.x) g[k] = p.sg_cell_start[k];
                for (uint32_t k = threadIdx.x; k < p.sg_nentries; k += blockDim.x) g[nc + k] = p.sg_entries[k];
                for (uint32_t k = threadIdx.x; k < p.sg_nglobal; k += blockDim.x) g[nc + p.sg_nentries + k] = p.sg_global[k];
                T.sgCell = g;
                T.sgEntries = g + nc;
                T.sgGlobal = g + nc + p.sg_nentries;
            }
        }
        __syncthreads();
        T.scan = ldsScan;
        T.orig = ldsOrig;
        if (kLeafLds) T.leaf = ldsLeaf;
        T.rad = ldsRad;
        if (kMatsL2) T.mats = p.mats;  // (a kernel argument: global address space, no flat loads)
        else if (kHitLds) T.mats = reinterpret_cast<const rt_material*>(ldsMat);
        else if (p.mats_in_lds) T.mats = reinterpret_cast<const rt_material*>(ldsMat);
    } else if (kScan == 3) {
        // cell-grid scan: the exact tables stay in global memory (L2); the cells' first entries live in LDS (kHitLds: typed pointer)
        if (kHitLds) {
            uint16_t* g = reinterpret_cast<uint16_t*>(tabBase);
            const uint32_t ng = p.grid_nu * p.grid_nv + 1u;
            for (uint32_t k = threadIdx.x; k < ng; k += blockDim.x) g[k] = p.grid_cell_start[k];
            T.gridCells = g;
            if (kGridQ) {  // the quantised bounds behind the cells (16-byte steps): 4 bytes per scan entry
                uint32_t* q = reinterpret_cast<uint32_t*>(g + ((ng + 7u) & ~7u));
                for (uint32_t k = threadIdx.x; k < p.n_padded; k += blockDim.x) q[k] = p.grid_qrec[k];
                T.gridQ = q;
            }
            if (kSgLds) {  // the shadow index behind the cells (16-byte steps); the host launches this flavour only when the scene has one
                uint16_t* sgl = g + ((ng + 7u) & ~7u);
                const uint32_t nc = p.sg_nx * p.sg_ny + 1u;
                for (uint32_t k = threadIdx.x; k < nc; k += blockDim.x) sgl[k] = p.sg_cell_start[k];
                for (uint32_t k = threadIdx.x; k < p.sg_nentries; k += blockDim.x) sgl[nc + k] = p.sg_entries[k];
                for (uint32_t k = threadIdx.x; k < p.sg_nglobal; k += blockDim.x) sgl[nc + p.sg_nentries + k] = p.sg_global[k];
                T.sgCell = sgl;
                T.sgEntries = sgl + nc;
                T.sgGlobal = sgl + nc + p.sg_nentries;
            }
            __syncthreads();
        }
    } else if (kMfma) {
        // exact tables stay in global memory (L2); the top level's operand image and, when they fit, all bounds live in LDS
        float* ldsOps = reinterpret_cast<float*>(tabBase);
        build_mfma_operands(p.tree + p.level_off[topLevel], nTop, nTiles, ldsOps, threadIdx.x, blockDim.x);
        T.ops = ldsOps;
        if (kHitLds) {  // hierarchy scan: every level of bounds is in LDS (typed pointer: the descent's node reads are ds_read, not flat)
            float4* ldsTree = reinterpret_cast<float4*>(ldsOps + (size_t)nTiles * kOpsPerTile);
            const uint32_t nNodes = p.level_off[topLevel] + nTop;
            for (uint32_t k = threadIdx.x; k < nNodes; k += blockDim.x) ldsTree[k] = p.tree[k];
            T.tree = ldsTree;
        }
        __syncthreads();
    }
}

// Next block of fresh paths for this wave (rt_params.h, "the queue of fresh paths"); false when every shard is empty.
// What one wave learns about an empty shard it tells its workgroup (SceneConsts::dry_mask, LDS): when a launch runs out of
// work, 4,096 waves asking 8 cursors each are 32,000 requests that the memory side serves one behind the other -- they
// alone were the last 0.4 ms of a launch (tools/timeline_waves.py: a claim took 160-400 us there).
RT_DEV uint32_t dry_shards(SceneConsts* ldsK) {
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(&ldsK->dry_mask, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
}
RT_DEV void mark_dry(SceneConsts* ldsK, uint32_t lane, uint32_t k) {
    if (lane == 0) __hip_atomic_fetch_or(&ldsK->dry_mask, 1u << k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// (P: the kernel arguments, or the lean kernels' LeanQueue read back from LDS -- the queue's members under TraceParams' names)
struct LeanQueue {
    uint32_t* shard_heads;
    uint32_t total_paths, dyn_begin, dyn_blocks, queue_block;
};
RT_DEV LeanQueue lean_queue(const uint32_t* b) {
    return LeanQueue{lds_global<uint32_t>(b + kLeanQueueHeads), lds_uniform(b + kLeanQueueTotal), lds_uniform(b + kLeanQueueDynBegin),
                     lds_uniform(b + kLeanQueueDynBlocks), lds_uniform(b + kLeanQueueBlock)};
}
template <class P>
RT_DEV bool claim_block(const P& p, SceneConsts* ldsK, uint32_t lane, uint32_t qb, uint32_t& blkNext, uint32_t& blkEnd,
                        uint32_t& shard) {
    RT_SITE(K_CLAIM);
    uint32_t dry = dry_shards(ldsK);
    for (uint32_t a = 0; a < kQueueShards; ++a) {
        const uint32_t k = (blockIdx.x + a) & (kQueueShards - 1u);
        if ((dry >> k) & 1u) continue;
        uint32_t* head = p.shard_heads + kShardStrideWords * k;
        uint32_t c = 0;
        if (lane == 0) c = __hip_atomic_load(head, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        c = (uint32_t)__builtin_amdgcn_readfirstlane((int)c);
        if (c * kQueueShards + k >= p.dyn_blocks) {
            mark_dry(ldsK, lane, k);
            continue;
        }
        if (lane == 0) c = atomicAdd(head, 1u);
        c = (uint32_t)__builtin_amdgcn_readfirstlane((int)c);
        const uint32_t b = c * kQueueShards + k;  // shard k owns the blocks k, k + 8, k + 16, ...
        if (b < p.dyn_blocks) {
            blkNext = p.dyn_begin + b * qb;
            blkEnd = (blkNext + qb) < p.total_paths ? (blkNext + qb) : p.total_paths;
            shard = k;  // where the claim succeeded (the caller claims ahead from the same shard)
            return true;
        }
        mark_dry(ldsK, lane, k);
        dry = dry_shards(ldsK);  // what the others found in the meantime
    }
    shard = kQueueShards;
    return false;
}

// ============================================================================ megakernel
// Persistent threads: every wave loops { refill idle lanes from the queue; one list scan for all
// lanes; per-lane state transition } until the queue is empty and all its lanes are idle.  Waves
// never synchronise with each other after the LDS staging barrier, and every wave's loop ends when
// the (bounded, monotonically consumed) queue is exhausted and its at most 64 paths of at most
// max_depth+1 segments have finished.
// kScan: 0 = VALU sign filter per group (any scene size), 1 = matrix-core filter over the groups (tables in LDS),
// 2 = matrix-core filter over the top level of the bounds hierarchy + per-lane descent (tables through L2).
// kCarry: frame pipelining (rt_params.h): resume the paths the previous trace kernel carried out, end as soon as the
// fresh queue is empty and carry the unfinished paths into the next kernel.
// kStash: REGROUPED HIT PROCESSING (within the wave).  Four closest-hit scans in ten end in the sky, so hit
// processing -- Material::Scatter, the shadow index, DirectionalLight::Shade: 40 % of an iteration -- ran with 36 of 64
// lanes.  Here a lane whose scan found a hit only RECORDS it (state kHaveHit: position in `ro`, scan entry in the high half
// of `depth`) and the wave processes hits when at least stash_cap + 1 lanes hold one; with fewer it pushes them to a
// per-wave stash in LDS (the region the prepared-path cache occupies in the other variants), all 64 lanes generate the next
// 64 fresh paths straight into registers, scan, and the lanes that missed pop stashed hits until the wave is full of
// hits.  Scans run with ~59 live rays, hit processing with ~58 lanes instead of 36.  Every path sees the same sequence of
// operations on the same values as before: only WHEN a hit is processed changes, never what is computed.
// kLights (trace_body only): false = ONE light, the reference's scene (rt_trace_kernel); true = the scene's LIST of lights
// (rt_trace_kernel_lights: Material::Shade's loop, material.cpp:4-13).  Two entry kernels over one body, so that the single-light
// kernels' code and register allocation are exactly what they were without the list.
// kGridQ (cell-grid scan, global tables): the quantised one-sphere bounds are staged into LDS behind the cells (rt_scan.h GridQuant).
// kFarState: true = a hit point beyond the shadow index's radius waits one iteration in kNeedShadow and takes a lane of the next scan
// (one light), carrying pend, nextDir, contAfterShadow and pathScattered across the loop; and every path counts its traversals for
// trav_out.  false (the flat hit-stash kernels of picture launches, rt_trace_kernel_lean below): such a hit is answered inside
// processHit -- by light 0's second index (p.far_index), or by the any-hit over every entry -- so that none of that state, nor
// pathTrav with its stash dword (dword 18 stays in the record, unread and unwritten), lives across an iteration: nextDir is then
// written by Scatter and read a few lines on, in the same hit processing.  Same arithmetic on the same values, same counts: only where
// the far shadow ray is answered changes.  (The kFarState == true code is the text it was, so that those kernels keep their code.)
template <bool kLights, bool kLds, int kThreads, int kScan, bool kCache, bool kHitLds, bool kCarry, bool kStash, bool kMatsL2, bool kSgLds, bool kGridQ,
          bool kFarState = true>
__device__ __forceinline__ void trace_body(const TraceParams& p) {
    static_assert(kFarState || (kLds && kScan == 1 && kStash && !kCarry), "without far-hit state: the flat LDS hit-stash family, no frame pipelining");
    static_assert(!kGridQ || (kScan == 3 && !kLds && kHitLds && !kSgLds), "quantised bounds: the global-tables grid variant");
    static_assert(!kSgLds || (kScan == 3 && !kLds && kHitLds), "shadow index in LDS next to the grid's cells: the global-tables grid variant");
    static_assert(!kMatsL2 || (kHitLds && kStash && kLds), "materials through L2: a flavour of the all-in-LDS stash variants");
    constexpr bool kMfma = kScan == 1 || kScan == 2;  // matrix-core filter; kScan == 3: cell-grid scan (rt_scan.h scan_list_grid)
    static_assert(!kCarry || (kCache && kHitLds && kScan == 1), "frame pipelining is built for the flat LDS variant only");
    static_assert(!kStash || (kCache && !kCarry), "the hit stash takes the LDS region of the prepared-path cache");
    static_assert(!kHitLds || kScan != 0, "kHitLds belongs to the matrix-core and grid variants");
#ifdef RT_TIMELINE
    const unsigned long long tl0 = __builtin_amdgcn_s_memrealtime();  // 100 MHz; diagnostic build only
    uint32_t tlCarriedIn = 0;
#endif
    RT_SITE(K_WAVE);
    extern __shared__ float4 smem[];
    // [0, kConstBytes): the scene constants; then the per-wave regions; then the tables
    SceneConsts* ldsK = reinterpret_cast<SceneConsts*>(smem);
    if (threadIdx.x == 0) fill_consts(p, *ldsK);
    // kFarState == false: the launch constants the loop reads go to LDS as well (rt_params.h) and are read back where they are used;
    // `leanHot` is a fixed address, chunk(k) costs one more LDS read for its offset
    constexpr bool kLean = !kFarState;
    static_assert(!kLean || kThreads / kWaveSize >= (int)kLeanChunks, "one hit-stash region per chunk of lean launch constants");
    const uint32_t* ldsWords = reinterpret_cast<const uint32_t*>(smem);
    const uint32_t* leanHot = ldsWords + kLeanHotOffset / 4u;
    if (kLean && threadIdx.x == 0) fill_lean_consts(p, reinterpret_cast<uint32_t*>(smem));
    auto chunk = [&](uint32_t k) -> const uint32_t* { return ldsWords + (leanHot[kLeanHotTail] + k * leanHot[kLeanHotStride]); };
    // the elementary functions' tables behind the constants (log | exp2 | sincos, as MathTabs indexes them)
    unsigned long long* ldsMath = reinterpret_cast<unsigned long long*>(smem + kSceneConstBytes / 16);
    {
        const MathTabs g = default_math_tabs();
        for (uint32_t k = threadIdx.x; k < kMathTabWords; k += blockDim.x)
            ldsMath[k] = k < 94u ? g.log[k] : (k < 127u ? g.exp2[k - 94u] : g.sincos[k - 127u]);
    }
#ifdef RT_NO_LDS_MATH
    const MathTabs mt = default_math_tabs();
#else
    const MathTabs mt{ldsMath, ldsMath + 94, ldsMath + 127};
#endif
    uint16_t* candBase = reinterpret_cast<uint16_t*>(smem + kConstBytes / 16);
    constexpr uint32_t kWaveRegion = wave_region_bytes<kScan>();  // the work lists of the flat, hierarchy or grid scan
    // the shadow index's global list (rt_params.h sg_glob_slots): spheres, then ids, in front of the tables
    float4* globSph = smem + kConstBytes / 16 + (kThreads / kWaveSize) * (kWaveRegion / 16);
    uint16_t* globIds = reinterpret_cast<uint16_t*>(globSph + p.sg_nglobal);
    if (p.sg_glob16 != 0u)
        for (uint32_t k = threadIdx.x; k < p.sg_nglobal; k += blockDim.x) {
            const uint32_t id = p.sg_global[k];
            globSph[k] = p.scan[id];
            globIds[k] = (uint16_t)id;
        }
    float4* tabBase = globSph + p.sg_glob16;
    SceneTabs T;
    stage_scene<kLds, kScan, kHitLds, kMatsL2, kSgLds, kGridQ>(p, tabBase, T);  // ends with a workgroup barrier when it staged anything
    const float4* scanTab = T.scan;
    const uint32_t* origTab = T.orig;
    const float4* leafTab = T.leaf;
    const float* radTab = T.rad;
    const rt_material* matTab = T.mats;
    const uint4* mat16Lds = T.mats16;
    const float* mfmaOps = T.ops;
    const float4* treeTab = T.tree;
    const uint16_t* sgCell = T.sgCell;
    const uint16_t* sgEntries = T.sgEntries;
    const uint16_t* sgGlobal = T.sgGlobal;
    const uint16_t* gridCells = T.gridCells;
    const uint32_t* gridQ = T.gridQ;
    const uint32_t nTop = T.nTop, nTiles = T.nTiles;

    const uint32_t lane = threadIdx.x & (kWaveSize - 1);
    uint16_t* waveCand = candBase + (threadIdx.x / kWaveSize) * (kWaveRegion / 2);
    uint16_t* cand = waveCand + lane;
    __syncthreads();  // the constants block (and, above, the staged tables) are visible to every wave from here on
#ifdef RT_TIMELINE
    const unsigned long long tl1 = __builtin_amdgcn_s_memrealtime();
#endif
    const SceneConsts& K = *ldsK;
    const V3 sunDir = v3(K.sun_dir[0], K.sun_dir[1], K.sun_dir[2]);
    const float aSun = dot3(sunDir, sunDir);  // the `a` of every shadow ray (ray-tracing.cpp:46)

    // per-lane path state
    V3 ro = v3(0.f, 0.f, 0.f), rd = v3(0.f, 0.f, 1.f);  // current ray
    V3 thr = v3(1.f, 1.f, 1.f), rad = v3(0.f, 0.f, 0.f);
    V3 pend = v3(0.f, 0.f, 0.f), nextDir = v3(0.f, 0.f, 0.f);
    StreamDraws draws{Rng{1u, 0u, 0u, 0u}};
    uint32_t q = 0, depth = 0, state = kIdle, pathTrav = 0;  // q = the path's slot in the sample buffer
    uint32_t seq8 = 0;  // kCarry: low byte of the sequence number of the path's region (its call)
    uint32_t carried = 0;  // kCarry: paths this wave carries out (wave-uniform)
    uint32_t itersHere = 0;  // kCarry: iterations of this wave in this launch
    const uint32_t gwave = blockIdx.x * (kThreads / kWaveSize) + threadIdx.x / kWaveSize;  // this wave's index in the grid
    const uint32_t kBlk = kLean ? 0u : p.queue_block;  // paths per queue block (a multiple of 64); lean: read where a block is taken
    bool contAfterShadow = false, pathScattered = false;
    uint32_t nTrav = 0, nSeg = 0;

    // wave-uniform queue window and prepared-path cache (48-byte slots: origin, direction, stream state, path index)
    uint32_t blkNext = 0, blkEnd = 0, cachePos = 0, cacheCnt = 0;
    bool queueEmpty = false;
    uint32_t pendShard = kQueueShards;  // shard of the block claimed ahead (kQueueShards: none), wave-uniform
    uint32_t pendCount = 0;             // lane 0: what that claim returned
    if (kCarry) {
        // the wave's own carried paths (rt_params.h): no cursor, no atomics
        const uint32_t nIn = p.cont_in_n[gwave];
#ifdef RT_TIMELINE
        tlCarriedIn = nIn;
#endif
        if (lane < nIn) {
            const ContEntry* e = p.cont_in + ((size_t)gwave * kWaveSize + lane);
            const float4 A = e->a, B = e->b, Cc = e->c, D = e->d, E = e->e;
            ro = v3(A.x, A.y, A.z);
            rd = v3(A.w, B.x, B.y);
            thr = v3(B.z, B.w, Cc.x);
            rad = v3(Cc.y, Cc.z, Cc.w);
            draws.rng = Rng{__float_as_uint(D.x), __float_as_uint(D.y), __float_as_uint(D.z), __float_as_uint(D.w)};
            q = __float_as_uint(E.x);
            depth = __float_as_uint(E.y);
            seq8 = __float_as_uint(E.z);
            pathTrav = __float_as_uint(E.w);
            const float4 F = e->f, G = e->g;
            pend = v3(F.x, F.y, F.z);
            nextDir = v3(F.w, G.x, G.y);
            const uint32_t fl = __float_as_uint(G.z);
            state = fl & 3u;
            contAfterShadow = (fl & 4u) != 0u;
            pathScattered = (fl & 8u) != 0u;
        }
    }
    {
        // the wave's first block(s) of fresh paths are static: block `gwave`; the shards start behind those.  (The carrying
        // kernel uses half-size blocks: a wave can only start paths as lanes fall idle, so a wave whose lanes are held by long
        // paths should own little unstarted work when the queue runs dry -- it must start all of it before it may leave.)
        const uint32_t span = p.queue_block * p.static_blocks;  // (before the loop: the kernel arguments in every kernel)
        const uint32_t b0 = gwave * span;
        blkNext = b0 < p.total_paths ? b0 : p.total_paths;
        blkEnd = (b0 + span) < p.total_paths ? (b0 + span) : p.total_paths;
    }
    // per-wave region behind the tables: the prepared-path cache, or (kStash) the hit stash, p.ray_cache_stride16 float4 per wave
    float4* rayCache = kCache ? smem + p.ray_cache_off16 + (threadIdx.x / kWaveSize) * p.ray_cache_stride16 : nullptr;
    uint32_t stashCnt = 0;  // kStash: records in the wave's stash (wave-uniform)

    unsigned long long dbgScan[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#ifdef RT_TIMELINE
    unsigned long long tlDrain = 0ull;  // when this wave had nothing left to start
    uint32_t drainIters = 0;            // iterations after that
    unsigned long long tlLastClaim = 0ull;
    uint32_t tlBorn = 0;  // per lane: when its path was started
    uint32_t tlBlocks = 0, tlLastBlock = 0, tlIters = 0;
#endif
    (void)dbgScan;
#ifdef RT_STAMPS
    unsigned long long cyRefill = 0, cyScan = 0, cyTrans = 0, cyIters = 0, cyHit[6] = {0, 0, 0, 0, 0, 0};
#endif
    // Next block of fresh paths for this wave; false when every shard is empty.  The block was claimed AHEAD, when the
    // previous one was taken: the atomic's round trip (two of them with the look, ~4 us under load, 117 times per wave on
    // C2) ran under the work on a whole block instead of stalling the wave.  A claim that came back beyond the shard's end
    // falls through to a fresh look.
    // (Q: the queue's constants under TraceParams' names and the block size -- the kernel arguments, or, without far-hit state, what
    // lean_queue reads back from LDS once per block of 128 paths)
    auto takeBlock = [&](const auto& Q, uint32_t qb) -> bool {
        bool got = false;
        if (pendShard < kQueueShards) {
            const uint32_t c = (uint32_t)__builtin_amdgcn_readfirstlane((int)pendCount);
            const uint32_t b = c * kQueueShards + pendShard;
            if (b < Q.dyn_blocks) {
                blkNext = Q.dyn_begin + b * qb;
                blkEnd = (blkNext + qb) < Q.total_paths ? (blkNext + qb) : Q.total_paths;
                got = true;
            } else {
                mark_dry(ldsK, lane, pendShard);
                pendShard = kQueueShards;  // that shard is dry
            }
        }
        if (!got && !claim_block(Q, ldsK, lane, qb, blkNext, blkEnd, pendShard)) return false;
        // (not in the frame-pipelining kernel: a wave must start everything it owns before it may carry out)
        if (kCarry) pendShard = kQueueShards;
        if (pendShard < kQueueShards && ((dry_shards(ldsK) >> pendShard) & 1u)) pendShard = kQueueShards;
        if (pendShard < kQueueShards && lane == 0) pendCount = atomicAdd(Q.shard_heads + kShardStrideWords * pendShard, 1u);  // claim ahead
        return true;
    };
    auto nextBlock = [&]() -> bool {
        RT_SITE(K_NEXTBLOCK);
        if constexpr (kLean) {
            const LeanQueue Q = lean_queue(chunk(1));
            return takeBlock(Q, Q.queue_block);
        } else {
            return takeBlock(p, kBlk);
        }
    };
    // A finished path: GetHitColor * exposureAdjustment, spheres-app.cpp:183; one 12-byte store
    auto finishPath = [&]() {
        RT_SITE(K_FINISH);
        const float expo = K.exposure;
        float* const samples = kLean ? lds_global<float>(leanHot + kLeanHotSamples, false) : p.samples;
        *reinterpret_cast<float3*>(samples + (size_t)q * 3) = make_float3(rad.x * expo, rad.y * expo, rad.z * expo);
        if (kFarState && p.trav_out) p.trav_out[q] = pathTrav;  // (a launch with trav_out takes a kFarState kernel: host/rt_launch_plan.cpp)
        state = kIdle;
#ifdef RT_TIMELINE
        if (!kCarry && tlDrain != 0ull && gwave < 4096u) {
            unsigned int* w = g_tlLast + 4u * gwave;
            w[0] = tlBorn; w[1] = depth; w[2] = q; w[3] = pathTrav;
        }
#endif
    };
#ifdef RT_STAMPS
    unsigned long long thA = 0, thB = 0;
#endif
    // kFarState == false: light 0's shadow question for a hit point beyond its first index (|p|^2 = pp > sg_p0sq): the second index
    // within its radius; beyond that, or where the scene has none, the any-hit over every entry.  All three answer "does any entry
    // yield an accepted root", which is what the shadow scan answered.
    auto farShadow = [&](V3 pos, float pp) -> bool {
        RT_SITE(H_FARHIT);
        // (reached only without far-hit state: the scene's light records and entry count come out of LDS, chunk 2)
        const uint32_t* rare = chunk(2);
        const LightRec* F = lds_uniform(rare + kLeanRareFarIndex) != 0u
                                ? lds_global<const LightRec>(rare + kLeanRareExtraLights) + (lds_uniform(rare + kLeanRareNLights) - 1u)
                                : nullptr;
        if (F != nullptr && pp <= F->sg_p0sq)
            return shadow_query(*F, scanTab, F->cell_start, F->entries, F->global, false, globSph, globIds, (const float4*)nullptr, pos, sunDir, aSun);
        return any_hit_all(scanTab, lds_uniform(rare + kLeanRareNPadded), pos, sunDir, aSun);
    };
    // Hit processing of one closest hit (scan entry idx at pos) for a lane in state kNeedClosest: Scatter, the shadow
    // query, Emit + Shade, and the path's next state (GetHitColor, spheres-app.cpp:238-257).
    auto processHit = [&](int idx, V3 pos, bool& finished) {
        RT_SITE(H_PROCESS);
        const float4 S = scanTab[idx];
        const float radius = radTab[idx];  // radius and material tables are in scan-entry (clustered) order
        // the packed 16-byte record where the launch provides it: from LDS (kMatsL2 variants, mode 2) or from global memory (mode 1)
        const uint32_t hotFlags = kLean ? lds_uniform(leanHot + kLeanHotFlags) : 0u;
        const uint32_t mats16Mode = kLean ? (hotFlags & 255u) : p.mats16_mode;
        const bool globInLds = kLean ? (hotFlags & 256u) != 0u : p.sg_glob16 != 0u;
        const uint4* const mats16 = kLean ? lds_global<const uint4>(leanHot + kLeanHotMats16, false) : p.mats16;
        const Mat m = (kMatsL2 && mats16Mode == 2u) ? load_material16(mat16Lds, idx)
                                                     : (mats16Mode == 1u ? load_material16(mats16, idx) : load_material(matTab, idx));
        const V3 center = v3(S.x, S.y, S.z);
        const V3 nrm = div3_signed(pos - center, radius);  // ray-tracing.cpp:62 (true divide by the SIGNED radius: r < 0 turns the normal inward)
        V3 atten, local, localOcc, tex;
        RT_STAMP(th0);
        const bool scattered = scatter_only(m, rd, nrm, draws, atten, nextDir, tex, mt, K.sampler);  // Scatter first: it draws (spheres-app.cpp:246)
        RT_STAMP(th1);
        const bool cont = (depth < (kLean ? leanHot[kLeanHotMaxDepth] : p.max_depth)) && scattered;  // spheres-app.cpp:247
        if (kLights) {
            // Material::Shade over the scene's LIST of lights (material.cpp:4-13): directLighting = 0, += light->Shade(...) in list
            // order; every light casts its shadow ray (one traversal each), answered by the light's own footprint index -- or, for
            // a hit point outside it, by the any-hit over every entry.  (One light -- the reference's scene -- takes the path below.)
            RT_SITE(H_MULTI);
            V3 emitOnly;
            shade_value(K, m, tex, pos, nrm, false, emitOnly, localOcc, mt);  // Emit + 0
            V3 direct = v3(0.f, 0.f, 0.f);
            const float pp = dot3(pos, pos);
            const uint32_t nLights = kLean ? lds_uniform(chunk(2) + kLeanRareNLights) : p.n_lights;
            const LightRec* const extraLights = kLean ? lds_global<const LightRec>(chunk(2) + kLeanRareExtraLights) : p.extra_lights;
            const uint32_t nPadded = kLean ? lds_uniform(chunk(2) + kLeanRareNPadded) : p.n_padded;
            for (uint32_t k = 0; k < nLights; ++k) {
                bool occ;
                V3 sh;
                if (k == 0u) {
                    occ = (K.sg_enabled && pp <= K.sg_p0sq)
                              ? shadow_query(K, scanTab, sgCell, sgEntries, sgGlobal, globInLds, globSph, globIds, (!kLds && kScan >= 2) ? p.sg_sph : nullptr, pos, sunDir, aSun)
                              : (kFarState ? any_hit_all(scanTab, nPadded, pos, sunDir, aSun) : farShadow(pos, pp));
                    sh = occ ? v3(0.f, 0.f, 0.f) : shade_only(K, m, tex, pos, nrm, mt);
                } else {
                    const LightRec& Lk = extraLights[k - 1u];
                    const V3 dirK = v3(Lk.sun_dir[0], Lk.sun_dir[1], Lk.sun_dir[2]);
                    const float aK = dot3(dirK, dirK);
                    occ = (Lk.sg_enabled && pp <= Lk.sg_p0sq)
                              ? shadow_query(Lk, scanTab, Lk.cell_start, Lk.entries, Lk.global, false, globSph, globIds, (const float4*)nullptr, pos, dirK, aK)
                              : any_hit_all(scanTab, nPadded, pos, dirK, aK);
                    sh = occ ? v3(0.f, 0.f, 0.f) : shade_only(Lk, m, tex, pos, nrm, mt);
                }
                ++nTrav;
                if (kFarState) ++pathTrav;
                direct = direct + sh;  // (an occluded light's Shade is XM_Zero, light.cpp:15-18)
            }
            rad = rad + thr * (emitOnly + direct);  // radiance += throughput * (Emit + Shade)
            if (cont) {
                thr = thr * atten;
                ro = pos;
                rd = nextDir;
                ++depth;
            } else {
                finished = true;
            }
            return;
        }
        const bool useIndex = K.sg_enabled && dot3(pos, pos) <= K.sg_p0sq;
        bool occluded = false;
        if (useIndex) occluded = shadow_query(K, scanTab, sgCell, sgEntries, sgGlobal, globInLds, globSph, globIds, (!kLds && kScan >= 2) ? p.sg_sph : nullptr, pos, sunDir, aSun);
        else if (!kFarState) occluded = farShadow(pos, dot3(pos, pos));
        RT_STAMP(th2);
        // the Blinn-Phong value (two normalisations, two pows) is only needed when the sun is visible or unknown
        shade_value(K, m, tex, pos, nrm, !occluded, local, localOcc, mt);
        RT_STAMP(th3);
#ifdef RT_STAMPS
        thA = th0;
        thB = th3;
#endif
        RT_ACC(cyHit[0], th0, th1);
        RT_ACC(cyHit[1], th1, th2);
        RT_ACC(cyHit[2], th2, th3);
        if (useIndex || !kFarState) {
            RT_SITE(H_INDEXED);
            // shadow ray answered by the exact footprint index (or, kFarState == false, in place above): no second scan for this hit
            ++nTrav;  // the shadow ray still counts as a traversal of the scene (matches the oracle's counter)
            if (kFarState) ++pathTrav;
            if (kLean) {
                // The same update without branches.  The addend is chosen by a select and the SUM is what the predicate keeps or
                // drops -- an occluded lane that scattered keeps its radiance untouched, it does not add +0 (rad can be -0 only in
                // theory, but the bits are the contract).  A path that ends here is stored by finishPath from rad and q alone, so
                // its throughput, ray and depth may take the values of a continuing path: nothing reads them again.
                const bool add = !occluded || !scattered;
                const V3 sum = rad + thr * v3(occluded ? localOcc.x : local.x, occluded ? localOcc.y : local.y, occluded ? localOcc.z : local.z);
                rad = v3(add ? sum.x : rad.x, add ? sum.y : rad.y, add ? sum.z : rad.z);
                thr = thr * atten;
                ro = pos;
                rd = nextDir;
                ++depth;
                finished = !cont;
                return;
            }
            if (!occluded) rad = rad + thr * local;           // radiance += throughput * (Emit + Shade)
            else if (!scattered) rad = rad + thr * localOcc;  // occluded: throughput * (Emit + 0)
            if (cont) {
                thr = thr * atten;
                ro = pos;
                rd = nextDir;
                ++depth;
            } else {
                finished = true;
            }
        } else {
            RT_SITE(H_FARHIT);
            pend = thr * local;
            // a path that does not scatter ends here, so its nextDir registers carry throughput * (Emit + 0),
            // the value the reference adds when the sun is occluded (0 for every non-emissive material)
            pathScattered = scattered;
            if (!scattered) nextDir = thr * localOcc;
            contAfterShadow = cont;
            thr = thr * atten;
            ro = pos;  // shadow ray and scattered ray both start at hit.pos
            rd = sunDir;
            state = kNeedShadow;
        }
    };
    // Tile masks (rt_tile_mask.h; flat hit-stash variants): when the 64 fresh paths of K_GEN are one full tile at one sample, the scan
    // that follows in the same iteration holds that tile's 64 primary rays and nothing else, and takes the tile's candidate words.
    constexpr bool kPrim = kStash && kScan == 1;
    // ... and a tile whose sphere list is EMPTY is finished in K_GEN without rays (below; never in the frame-pipelining kernel)
    constexpr bool kSky = kPrim && !kCarry;
    for (;;) {
        RT_SITE(K_ITER);
        RT_STAMP(ts0);
        uint32_t primTile = 0xffffffffu;  // wave-uniform: the tile whose mask this iteration's scan takes (none)
        // kOneExit (the kernels without far-hit state): the loop has ONE exit, at its end, and no `continue` -- an iteration with nothing to scan skips the scan and the
        // transitions through a wave-uniform `if` and the wave leaves when `leanAgain` is false.  With the exit in the middle of
        // the body (the text the other kernels keep) the compiler linearises the loop as one with a divergent exit: a break mask
        // accumulated every iteration, the scan and the transitions under a saved exec mask, and 22 register copies for the loop's
        // phi nodes at its head.  Same iterations, same work in each.
        constexpr bool kOneExit = kLean;
        bool leanSkippedSky = false, leanNoScan = false, leanAgain = true;
        // ------------------------------------------------ refill idle lanes (ballot + prefix)
        // New paths come from a per-wave cache of 64 prepared paths in LDS: when it runs empty ALL 64 lanes generate
        // the next 64 paths of the wave's queue block at once (index arithmetic, stream seeding, Camera::GetRay with
        // its two normalisations: ~350 instructions at full lane utilisation instead of once per handful of idle
        // lanes), and an idle lane just pops a 48-byte slot.  In-flight paths are untouched: the generation only uses
        // temporaries.  Without room for the cache in LDS (kCache == false) idle lanes generate their own path.
        uint64_t idleMask = __ballot(state == kIdle);
        if (kStash) {
            float* stash = reinterpret_cast<float*>(rayCache);
            // <= 63 records of kStashDwords dwords (lean: a lane's temporary out of LDS, used in its address arithmetic only)
            const uint32_t cap = kLean ? leanHot[kLeanHotStashCap] : p.stash_cap;
            // (1) idle lanes take stashed hits (newest first)
            if (stashCnt != 0u && idleMask != 0ull) {
                RT_SITE(K_POP);
                const uint32_t nIdle = (uint32_t)__popcll(idleMask);
                const uint32_t n = stashCnt < nIdle ? stashCnt : nIdle;
                const uint32_t r = prefix_count(idleMask);
                if (state == kIdle && r < n) {
                    RT_SITE(K_POP_LANE);
                    const float* e = stash + (stashCnt - 1u - r);
                    if constexpr (kLean) {
                        // field after field by stepping a 32-bit LDS address: with the cap a lane's temporary, e[k * cap] would be a
                        // 64-bit multiply-add per field
                        float f[kStashDwords - 1u];
                        for (uint32_t k = 0; k < kStashDwords - 1u; ++k) {
                            f[k] = *e;
                            e += cap;
                        }
                        ro = v3(f[0], f[1], f[2]);
                        rd = v3(f[3], f[4], f[5]);
                        thr = v3(f[6], f[7], f[8]);
                        rad = v3(f[9], f[10], f[11]);
                        draws.rng = Rng{__float_as_uint(f[12]), __float_as_uint(f[13]), __float_as_uint(f[14]), __float_as_uint(f[15])};
                        q = __float_as_uint(f[16]);
                        depth = __float_as_uint(f[17]);
                    } else {
                        ro = v3(e[0], e[cap], e[2u * cap]);
                        rd = v3(e[3u * cap], e[4u * cap], e[5u * cap]);
                        thr = v3(e[6u * cap], e[7u * cap], e[8u * cap]);
                        rad = v3(e[9u * cap], e[10u * cap], e[11u * cap]);
                        draws.rng = Rng{__float_as_uint(e[12u * cap]), __float_as_uint(e[13u * cap]), __float_as_uint(e[14u * cap]),
                                        __float_as_uint(e[15u * cap])};
                        q = __float_as_uint(e[16u * cap]);
                        depth = __float_as_uint(e[17u * cap]);
                        if (kFarState) pathTrav = __float_as_uint(e[18u * cap]);
                    }
                    state = kHaveHit;
                }
                stashCnt -= n;
            }
            // (2) process the hits when (nearly) every lane holds one; with fewer and nothing to scan, make room for 64 fresh paths
            const uint64_t hitMask = __ballot(state == kHaveHit);
            const uint32_t nHit = (uint32_t)__popcll(hitMask);
            bool process = nHit > (kLean ? lds_uniform(leanHot + kLeanHotStashProcess) : p.stash_process);
            if (!process && nHit != 0u && __ballot(state == kNeedClosest || (kFarState && state == kNeedShadow)) == 0ull) {
                if (blkNext == blkEnd && !queueEmpty && !nextBlock()) queueEmpty = true;
                if (blkNext == blkEnd) {
                    process = true;  // no fresh paths left: the hits are processed as they are
                } else {
                    RT_SITE(K_PUSH);
                    // (the stash is empty here: had records been left after (1), no lane would be idle, so with nothing to
                    // scan all 64 would hold a hit)
                    wave_lds_handoff();  // the pops above have read their records
                    if (state == kHaveHit) {
                        RT_SITE(K_PUSH_LANE);
                        float* e = stash + prefix_count(hitMask);
                        if constexpr (kLean) {
                            const float f[kStashDwords - 1u] = {ro.x, ro.y, ro.z, rd.x, rd.y, rd.z, thr.x, thr.y, thr.z, rad.x, rad.y, rad.z,
                                                                __uint_as_float(draws.rng.s0), __uint_as_float(draws.rng.s1), __uint_as_float(draws.rng.s2),
                                                                __uint_as_float(draws.rng.s3), __uint_as_float(q), __uint_as_float(depth)};
                            for (uint32_t k = 0; k < kStashDwords - 1u; ++k) {  // (stepping the address: as in the pop)
                                *e = f[k];
                                e += cap;
                            }
                        } else {
                            e[0] = ro.x; e[cap] = ro.y; e[2u * cap] = ro.z;
                            e[3u * cap] = rd.x; e[4u * cap] = rd.y; e[5u * cap] = rd.z;
                            e[6u * cap] = thr.x; e[7u * cap] = thr.y; e[8u * cap] = thr.z;
                            e[9u * cap] = rad.x; e[10u * cap] = rad.y; e[11u * cap] = rad.z;
                            e[12u * cap] = __uint_as_float(draws.rng.s0); e[13u * cap] = __uint_as_float(draws.rng.s1);
                            e[14u * cap] = __uint_as_float(draws.rng.s2); e[15u * cap] = __uint_as_float(draws.rng.s3);
                            e[16u * cap] = __uint_as_float(q);
                            e[17u * cap] = __uint_as_float(depth);
                            if (kFarState) e[18u * cap] = __uint_as_float(pathTrav);
                        }
                        state = kIdle;
                    }
                    stashCnt = nHit;
                    wave_lds_handoff();  // records are popped by other lanes than the ones that pushed them
                }
            }
            if (process) {
                RT_SITE(K_PROCESS);
                bool finished = false;
                if (state == kHaveHit) {
                    const int hidx = (int)(depth >> 16);
                    depth &= 0xffffu;
                    state = kNeedClosest;
                    processHit(hidx, ro, finished);
                }
                if (finished) finishPath();
            }
            // (3) fresh paths: whenever every lane is idle -- at the start and after each push -- all 64 lanes generate the
            // next 64 paths of the wave's queue block straight into their registers (index arithmetic, stream seeding,
            // Camera::GetRay with its two normalisations at full lane utilisation, no LDS round trip)
            if (__ballot(state != kIdle) == 0ull) {
                if (blkNext == blkEnd && !queueEmpty && !nextBlock()) queueEmpty = true;
                if (blkNext != blkEnd) {
                    RT_SITE(K_GEN);
#ifdef RT_TIMELINE
                    {
                        const uint32_t tlBlk = kLean ? lds_uniform(chunk(1) + kLeanQueueBlock) : kBlk;  // (kBlk is 0 in a lean kernel)
                        if (blkNext % tlBlk == 0u) {
                            tlLastClaim = __builtin_amdgcn_s_memrealtime();
                            ++tlBlocks;
                            tlLastBlock = blkNext / tlBlk;
                        }
                    }
#endif
                    const uint32_t nGen = (blkEnd - blkNext) < (uint32_t)kWaveSize ? (blkEnd - blkNext) : (uint32_t)kWaveSize;
                    if (kPrim) {
                        // (lean: this plane's constants as scalars out of LDS; else the kernel arguments themselves)
                        const uint32_t* const leanA = kLean ? chunk(0) : nullptr;
                        const uint32_t* const leanB = kLean ? chunk(1) : nullptr;
                        auto planeConsts = [&]() -> decltype(auto) {
                            if constexpr (kLean) return lean_coords<true>(K, leanA, leanB);
                            else return (p);
                        };
                        decltype(auto) pc = planeConsts();
                        // one full tile at one sample (path_coordinates: tile spans are multiples of 64), and the tile has a mask
                        if (pc.tile_masks != nullptr && nGen == (uint32_t)kWaveSize && (blkNext & 63u) == 0u) {
                            RT_SITE(K_GEN_TILE);
                            const uint32_t tw = fastdiv(blkNext, pc.fd_tile);
                            if (tw < (pc.npix_local >> 6)) {
                                const uint32_t tile = (uint32_t)__builtin_amdgcn_readfirstlane((int)(pc.tile_order ? pc.tile_order[tw] : tw));
                                const uint32_t flags = (uint32_t)__builtin_amdgcn_readfirstlane((int)pc.tile_masks[kTileMaskWords * tile + 4u]);
                                if (flags & 1u) {
                                    primTile = tile;
                                    if (pc.tile_spheres != nullptr) {
                                        const uint32_t nList = (uint32_t)__builtin_amdgcn_readfirstlane((int)pc.tile_spheres[(size_t)kTileSphereHalfs * tile]);
                                        // bit 31: the tile has a sphere list as well (tile < 2^25: the strip has at most 2^31 pixels)
                                        if (nList != kTileSphereNone) primTile = tile | 0x80000000u;
                                        if (kSky && nList == 0u && pc.sky_skip != 0u) {
                                            // An EMPTY list: the list holds every sphere a primary ray of the tile can have a root in
                                            // (rt_tile_mask.h), so all 64 paths miss on their first scan and end as
                                            // (0 + 1 * sky) * exposure -- K_TRANS_MISS and finishPath, whatever the jitter and the lens
                                            // sample.  The wave stores that for every plane of this tile its block still holds (same
                                            // expressions, same bits; one traversal and one segment per path, one direct scan per
                                            // plane) without rays, scan or transition.  Every lane stays idle: back to the top of the
                                            // loop, which pops what the stash holds and comes here again for the paths behind them.
                                            const uint32_t tileSpan = 64u * pc.spp_pass;
                                            const uint32_t rem = blkNext - tw * tileSpan;
                                            const uint32_t inTile = (tileSpan - rem) >> 6, inBlock = (blkEnd - blkNext) >> 6;
                                            const uint32_t nSky = inTile < inBlock ? inTile : inBlock;  // >= 1
                                            const V3 sky = v3(K.sky_emit[0], K.sky_emit[1], K.sky_emit[2]);
                                            const V3 skyRad = v3(0.f, 0.f, 0.f) + v3(1.f, 1.f, 1.f) * sky;
                                            const float expo = K.exposure;
                                            const float3 smp = make_float3(skyRad.x * expo, skyRad.y * expo, skyRad.z * expo);
                                            // path_coordinates' slot of path blkNext + lane (no path list here: the launch sets sky_skip)
                                            const uint32_t slot = tile * tileSpan + rem + pc.sample_base + lane;
                                            float* const samples = kLean ? lds_global<float>(leanHot + kLeanHotSamples) : p.samples;
                                            for (uint32_t k = 0; k < nSky; ++k) {
                                                *reinterpret_cast<float3*>(samples + (size_t)(slot + 64u * k) * 3) = smp;
                                                // (no launch with tile tables sets trav_out today, and none without far-hit state ever does)
                                                if (kFarState && p.trav_out) p.trav_out[slot + 64u * k] = 1u;
                                            }
                                            nTrav += nSky;
                                            nSeg += nSky;
                                            if (lane == 0) {
                                                __hip_atomic_fetch_add(&ldsK->prim_direct, nSky, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                                                __hip_atomic_fetch_add(&ldsK->prim_sky, nSky, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                                            }
                                            blkNext += 64u * nSky;
                                            if (kOneExit) leanSkippedSky = true;  // (every lane is idle: nothing below runs)
                                            else continue;
                                        }
                                    }
                                }
                            }
                        }
                    }
                    if (lane < nGen && !(kOneExit && leanSkippedSky)) {
                        RT_SITE(K_GEN_LANE);
                        uint32_t i, j, sN;
                        if constexpr (kLean) {
                            // every constant of the index arithmetic is the lane's own temporary out of LDS; no path list, and the
                            // launch provides the ray-generation tables (rt_capi.hip LaunchTrace)
                            const LeanCoords c = lean_coords<false>(K, chunk(0), chunk(1));
                            tiled_coordinates(c, blkNext + lane, i, j, sN, q);
                            draws.rng = rng_seed(c.seed, j * c.W + i, sN);
                            gen_primary_ray<true>(K, i, j, sN, ro, rd);
                        } else {
                            path_coordinates(p, blkNext + lane, i, j, sN, q);
                            draws.rng = rng_seed(p.seed, j * p.W + i, sN);
                            gen_primary_ray(K, i, j, sN, ro, rd);
                        }
                        thr = v3(1.f, 1.f, 1.f);
                        rad = v3(0.f, 0.f, 0.f);
                        depth = 0;
                        pathTrav = 0;
                        state = kNeedClosest;
#ifdef RT_TIMELINE
                        tlBorn = (uint32_t)(__builtin_amdgcn_s_memrealtime() - tl0);
#endif
                    }
                    if (!(kOneExit && leanSkippedSky)) blkNext += nGen;
                }
            }
        } else if (kCache) {
            while (idleMask != 0ull) {
                if (cachePos == cacheCnt) {
                    if (queueEmpty) break;
                    if (blkNext == blkEnd && !nextBlock()) {
                        queueEmpty = true;
                        break;
                    }
#ifdef RT_TIMELINE
                    if (blkNext % kBlk == 0u) {
                        tlLastClaim = __builtin_amdgcn_s_memrealtime();
                        ++tlBlocks;
                        tlLastBlock = blkNext / kBlk;
#ifdef RT_TIMELINE_RING
                        if (!kCarry && gwave < 4096u && lane == 0)
                            g_tlRing[16u * gwave + (tlBlocks & 15u)] = ((tlLastClaim - tl0) << 24) | (unsigned long long)(__popcll(__ballot(state != kIdle)) & 127) << 17 | (tlLastBlock >> 3);
#endif
                    }
#endif
                    const uint32_t nGen = (blkEnd - blkNext) < (uint32_t)kWaveSize ? (blkEnd - blkNext) : (uint32_t)kWaveSize;
                    wave_lds_handoff();  // every slot of the previous batch has been popped
                    if (lane < nGen) {
                        const uint32_t qn = blkNext + lane;
                        uint32_t i, j, s, slotn;
                        path_coordinates(p, qn, i, j, s, slotn);
                        const Rng g = rng_seed(p.seed, j * p.W + i, s);
                        V3 go, gd;
                        gen_primary_ray(K, i, j, s, go, gd);
                        float4* slot = rayCache + 3u * lane;
                        slot[0] = make_float4(go.x, go.y, go.z, gd.x);
                        slot[1] = make_float4(gd.y, gd.z, __uint_as_float(g.s0), __uint_as_float(g.s1));
                        slot[2] = make_float4(__uint_as_float(g.s2), __uint_as_float(g.s3), __uint_as_float(slotn), 0.f);
                    }
                    blkNext += nGen;
                    cacheCnt = nGen;
                    cachePos = 0;
                    wave_lds_handoff();  // slots are popped by other lanes than the ones that filled them
                }
                const uint32_t avail = cacheCnt - cachePos;
                const uint32_t want = (uint32_t)__popcll(idleMask);
                const uint32_t rank = prefix_count(idleMask);
                if (state == kIdle && rank < avail) {
                    const float4* slot = rayCache + 3u * (cachePos + rank);
                    const float4 A = slot[0], B = slot[1], C = slot[2];
                    ro = v3(A.x, A.y, A.z);
                    rd = v3(A.w, B.x, B.y);
                    draws.rng = Rng{__float_as_uint(B.z), __float_as_uint(B.w), __float_as_uint(C.x), __float_as_uint(C.y)};
                    q = __float_as_uint(C.z);
                    thr = v3(1.f, 1.f, 1.f);
                    rad = v3(0.f, 0.f, 0.f);
                    depth = 0;
                    pathTrav = 0;
                    if (kCarry) seq8 = p.region_seq & 255u;
                    state = kNeedClosest;
#ifdef RT_TIMELINE
                    tlBorn = (uint32_t)(__builtin_amdgcn_s_memrealtime() - tl0);
#endif
                }
                cachePos += want < avail ? want : avail;
                idleMask = __ballot(state == kIdle);
            }
        } else {
            while (idleMask != 0ull && !queueEmpty) {
                if (blkNext == blkEnd) {
                    uint32_t shardUnused = 0;
                    if (!claim_block(p, ldsK, lane, kBlk, blkNext, blkEnd, shardUnused)) {
                        queueEmpty = true;
                        break;
                    }
                }
                const uint32_t avail = blkEnd - blkNext;
                const uint32_t want = (uint32_t)__popcll(idleMask);
                const uint32_t rank = prefix_count(idleMask);
                if (state == kIdle && rank < avail) {
                    uint32_t i, j, s;
                    path_coordinates(p, blkNext + rank, i, j, s, q);
                    draws.rng = rng_seed(p.seed, j * p.W + i, s);
                    gen_primary_ray(K, i, j, s, ro, rd);
                    thr = v3(1.f, 1.f, 1.f);
                    rad = v3(0.f, 0.f, 0.f);
                    depth = 0;
                    pathTrav = 0;
                    state = kNeedClosest;
                }
                blkNext += want < avail ? want : avail;
                idleMask = __ballot(state == kIdle);
            }
        }
        if (__ballot(state != kIdle) == 0ull) {
            // queue empty and every lane drained -- but hits may still wait in the stash: a wave of 64 hits whose paths ALL
            // ended at that hit (a tile looking at an emissive sphere) leaves every lane idle with records behind it
            if (kOneExit) {
                leanNoScan = true;
                leanAgain = __builtin_amdgcn_readfirstlane((int)stashCnt) != 0 || leanSkippedSky;  // (a finished empty-list tile: back to the top for the paths behind it)
            } else {
                if (kStash && stashCnt != 0u) continue;  // back to the top: the idle lanes pop them (at most 63: one more round)
                break;
            }
        }
#ifdef RT_TIMELINE
        ++tlIters;
        if (queueEmpty && cachePos == cacheCnt) {
            if (tlDrain == 0ull) tlDrain = __builtin_amdgcn_s_memrealtime();
            ++drainIters;
        }
#endif
        if (kCarry) {
            ++itersHere;
            // Nothing left to start: carry the live paths into the next call's kernel instead of running their tail here.
            // A lane is carried between two scans, whichever it waits for (closest hit, or the shadow scan of a far hit point),
            // but not when its region is max_carry_age calls old (its slot of the sample ring is about to be reused): such
            // paths make the wave iterate on (<= 102 iterations).
            // (min_iters: a wave without fresh work must still advance the paths it was handed, or they would be passed from
            // kernel to kernel untouched until the age limit makes some wave run their whole tail)
            const bool nothingToStart = queueEmpty && cachePos == cacheCnt && p.carry != 0u && itersHere >= p.min_iters;
            const bool carriable = state == kIdle || ((p.region_seq - seq8) & 255u) < p.max_carry_age;
            if (nothingToStart && __ballot(!carriable) == 0ull) {
                const uint64_t liveMask = __ballot(state != kIdle);
                carried = (uint32_t)__popcll(liveMask);
                uint32_t age1 = 0;  // 1 + region age of this lane's carried path
                if (state != kIdle) {
                    ContEntry* e = p.cont_out + ((size_t)gwave * kWaveSize + prefix_count(liveMask));
                    e->a = make_float4(ro.x, ro.y, ro.z, rd.x);
                    e->b = make_float4(rd.y, rd.z, thr.x, thr.y);
                    e->c = make_float4(thr.z, rad.x, rad.y, rad.z);
                    e->d = make_float4(__uint_as_float(draws.rng.s0), __uint_as_float(draws.rng.s1), __uint_as_float(draws.rng.s2),
                                       __uint_as_float(draws.rng.s3));
                    e->e = make_float4(__uint_as_float(q), __uint_as_float(depth), __uint_as_float(seq8), __uint_as_float(pathTrav));
                    e->f = make_float4(pend.x, pend.y, pend.z, nextDir.x);
                    e->g = make_float4(nextDir.y, nextDir.z, __uint_as_float(state | (contAfterShadow ? 4u : 0u) | (pathScattered ? 8u : 0u)), 0.f);
                    age1 = 1u + ((p.region_seq - seq8) & 255u);
                }
                for (int off = 32; off > 0; off >>= 1) {
                    const uint32_t o2 = (uint32_t)__shfl_xor((int)age1, off);
                    age1 = o2 > age1 ? o2 : age1;
                }
                if (lane == 0) atomicMax(&ldsK->exit_age_max, age1);  // LDS: the workgroup's oldest carried region
                break;
            }
        }

        if (!(kOneExit && leanNoScan)) {
        RT_STAMP(ts1);
        // ------------------------------------------------ one list scan for every live lane
        float tmin = 0.f;
        int idx = -1;
        const bool live = kStash ? (state == kNeedClosest || (kFarState && state == kNeedShadow)) : (state != kIdle);  // (lanes holding a hit wait)
        if (kMfma) {
            // every lane takes part: lane l also supplies operands for, and filters half the spheres of,
            // the ray owned by lane l^32, whether or not its own ray is live
            const uint32_t* tileMask = nullptr;
            if (kPrim && primTile != 0xffffffffu && (primTile & 0x80000000u) != 0u) {
                // the tile's sphere list: every lane tests its own ray against the listed spheres (rt_scan.h scan_tile_spheres)
                if (lane == 0) __hip_atomic_fetch_add(&ldsK->prim_direct, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                const uint16_t* const tileSpheres = kLean ? lds_global<const uint16_t>(chunk(0) + kLeanPlaneTileSpheres) : p.tile_spheres;
                scan_tile_spheres(scanTab, origTab, tileSpheres + (size_t)kTileSphereHalfs * (primTile & 0x7fffffffu), ro, rd, live, tmin, idx, lane);
            } else {
            if (kPrim && primTile != 0xffffffffu) {
                tileMask = (kLean ? lds_global<const uint32_t>(chunk(0) + kLeanPlaneTileMasks) : p.tile_masks) + kTileMaskWords * primTile;
                // statistics (rt_unit_tile_masks): one LDS add per masked scan into the workgroup's constants block -- no register
                // lives across the persistent loop for it (two wave-uniform counters cost the kernel two VGPR spills and 1.1 %)
                if (lane == 0) __hip_atomic_fetch_add(&ldsK->prim_masked, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
            scan_list_mfma<kScan == 2, kPrim>(scanTab, leafTab, origTab, mfmaOps, nTiles, nTop, treeTab, p.level_off, p.n_levels, p.bound_norm, p.single_mask, p.n_always, p.tree_box_on ? p.tree_box : nullptr, ro, rd,
                                       live, tmin, idx, waveCand, lane, dbgScan, tileMask);
            }
        } else if (kScan == 3) {
            const GridParams G{gridCells, p.grid_nu, p.grid_nv, p.grid_ax_u, p.grid_ax_v, p.grid_g0u, p.grid_g0v, p.grid_inv_h, p.grid_rmax_over_h, p.grid_big_norm};
            const GridQuant Q{gridQ, p.grid_q[0], p.grid_q[1], p.grid_q[2], p.grid_q[3], p.grid_q[4], p.grid_q[5], p.grid_q[6], p.grid_q[7]};
            scan_list_grid<kGridQ>(scanTab, leafTab, origTab, G, gridCells, p.n_always, p.tree_box, p.bound_norm, ro, rd, live, tmin, idx, waveCand, lane, Q);
        } else if (live) {
            scan_list_deferred(scanTab, origTab, p.n_padded, ro, rd, tmin, idx, cand);
        }
        if (live) {
            ++nTrav;
            if (kFarState) ++pathTrav;
        }

        RT_STAMP(ts2);
        // ------------------------------------------------ state transitions
        bool finished = false;
#ifdef RT_STAMPS
        thA = 0;
        thB = 0;
#endif
        if (state == kNeedClosest) {
            ++nSeg;
            if (idx < 0) {
                RT_SITE(K_TRANS_MISS);
                // miss: sky Emissive::Emit (spheres-app.cpp:255)
                const V3 sky = v3(K.sky_emit[0], K.sky_emit[1], K.sky_emit[2]);
                rad = rad + thr * sky;
                finished = true;
            } else if (kStash) {
                RT_SITE(K_TRANS_HIT);
                // the hit waits for a full wave of hits: position (XMVectorMultiplyAdd(t, dir, origin), ray-tracing.cpp:57) in
                // place of the origin, scan entry beside the depth
                ro = tmin * rd + ro;
                depth |= (uint32_t)idx << 16;
                state = kHaveHit;
            } else {
                processHit(idx, tmin * rd + ro, finished);  // XMVectorMultiplyAdd(t, dir, origin), ray-tracing.cpp:57
            }
        } else if (kFarState && state == kNeedShadow) {
            RT_SITE(K_TRANS_SHADOW);
            if (idx < 0) rad = rad + pend;              // sun visible: radiance += throughput * (Emit + Shade)
            else if (!pathScattered) rad = rad + nextDir;  // occluded: radiance += throughput * (Emit + 0)
            if (contAfterShadow) {
                rd = nextDir;
                ++depth;
                state = kNeedClosest;
            } else {
                finished = true;
            }
        }
        if (finished) finishPath();
        RT_STAMP(ts3);
#ifdef RT_STAMPS
        if (thA != 0) {  // lanes that processed a hit this iteration (uniform enough: lane 0 reports)
            cyHit[3] += thA - ts2;
            cyHit[4] += ts3 - thB;
            cyHit[5] += 1;
        }
#endif
        RT_ACC(cyRefill, ts0, ts1);
        RT_ACC(cyScan, ts1, ts2);
        RT_ACC(cyTrans, ts2, ts3);
#ifdef RT_STAMPS
        cyIters += 1;
#endif
        }
        if (kOneExit && !leanAgain) break;
    }

    if (kCarry) {
        // the wave that leaves last tells the commit kernel which region is the oldest with paths still in flight
        if (lane == 0) {
            p.cont_out_n[gwave] = carried;
            const uint32_t ticket = atomicAdd(&ldsK->exit_ticket, 1u);
            if (ticket == (uint32_t)(kThreads / kWaveSize) - 1u) {
                const uint32_t m = atomicMax(&ldsK->exit_age_max, 0u);
                if (m != 0u) atomicMin(&p.ctl->oldest_open, p.region_seq - (m - 1u));
            }
        }
    }
#ifdef RT_TIMELINE
    if (lane == 0) {
        const unsigned long long tl2 = __builtin_amdgcn_s_memrealtime();
        // one 64-byte record per wave, plain stores: shared counters here would be 4,096 x n same-line atomics at ~11 ns
        // each when the waves leave together -- the instrument would make the tail it is meant to measure
        if (gwave < 4096u) {
            unsigned long long* w = g_tlWave + 8u * gwave;
            w[0] = tl0; w[1] = kCarry ? tl1 : (tlDrain != 0ull ? tlDrain : tl2); w[2] = tl2; w[3] = tlBlocks; w[4] = kCarry ? carried : tlLastBlock;
            w[5] = kCarry ? ((tlLastClaim - tl0) << 8 | (unsigned long long)tlCarriedIn) : tlLastClaim; w[6] = tlIters; w[7] = drainIters;
        }
    }
#endif
    // counters: wave reduce, one atomic pair per wave
    unsigned long long t = nTrav, s = nSeg;
    for (int off = 32; off > 0; off >>= 1) {
        t += __shfl_down(t, off);
        s += __shfl_down(s, off);
    }
#ifdef RT_STAMPS
    {
        unsigned long long it = dbgScan[2];
        for (int off = 32; off > 0; off >>= 1) it += __shfl_down(it, off);
        if (lane == 0) atomicAdd(&g_dbg[6], it);
    }
#endif
    if (lane == 0) {
        // (behind the loop the kernel arguments would do, but reading them here keeps them alive in scalar registers across it)
        unsigned long long* const counters = kLean ? lds_global<unsigned long long>(chunk(1) + kLeanQueueCounters, false) : p.counters;
        const bool haveMasks = kLean ? (chunk(0)[kLeanPlaneTileMasks] | chunk(0)[kLeanPlaneTileMasks + 1]) != 0u : p.tile_masks != nullptr;
        atomicAdd(&counters[0], t);
        atomicAdd(&counters[1], s);
        if (kPrim && haveMasks) {
            // the wave that leaves last adds the workgroup's count of masked scans (every other wave's adds precede its ticket)
            const uint32_t ticket = __hip_atomic_fetch_add(&ldsK->exit_ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (ticket == (uint32_t)(kThreads / kWaveSize) - 1u)
            {
                // (a directly resolved scan took its tile's tables as well: [3] counts both kinds, [4] the direct ones)
                const unsigned long long nDirect = __hip_atomic_load(&ldsK->prim_direct, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                atomicAdd(&counters[3], nDirect + (unsigned long long)__hip_atomic_load(&ldsK->prim_masked, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
                atomicAdd(&counters[4], nDirect);
                if (kSky) atomicAdd(&counters[5], (unsigned long long)__hip_atomic_load(&ldsK->prim_sky, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
            }
        }
#ifdef RT_STAMPS
        atomicAdd(&g_dbg[0], cyRefill);
        atomicAdd(&g_dbg[1], cyScan);
        atomicAdd(&g_dbg[2], cyTrans);
        atomicAdd(&g_dbg[3], cyIters);
        atomicAdd(&g_dbg[4], dbgScan[0]);
        atomicAdd(&g_dbg[5], dbgScan[1]);
        atomicAdd(&g_dbg[7], dbgScan[3]);
        atomicAdd(&g_dbg[8], dbgScan[4]);
        atomicAdd(&g_dbg[9], dbgScan[5]);
        atomicAdd(&g_dbg[10], dbgScan[6]);
        atomicAdd(&g_dbg[11], dbgScan[7]);
        atomicAdd(&g_dbg[12], cyHit[0]);
        atomicAdd(&g_dbg[13], cyHit[1]);
        atomicAdd(&g_dbg[14], cyHit[2]);
        atomicAdd(&g_dbg[15], cyHit[3]);
        atomicAdd(&g_dbg[16], cyHit[4]);
        atomicAdd(&g_dbg[17], cyHit[5]);
#endif
    }
}

template <bool kLds, int kThreads, int kScan, bool kCache, bool kHitLds = false, bool kCarry = false, bool kStash = false, bool kMatsL2 = false,
          bool kSgLds = false, bool kGridQ = false>
__global__ void __launch_bounds__(kThreads, 1) rt_trace_kernel(const TraceParams p) {
    trace_body<false, kLds, kThreads, kScan, kCache, kHitLds, kCarry, kStash, kMatsL2, kSgLds, kGridQ>(p);
}
// ... and for scenes whose light list has another length than one (rt_scene_upload, n_lights != 1)
template <bool kLds, int kThreads, int kScan, bool kCache, bool kHitLds = false, bool kCarry = false, bool kStash = false, bool kMatsL2 = false,
          bool kSgLds = false, bool kGridQ = false>
__global__ void __launch_bounds__(kThreads, 1) rt_trace_kernel_lights(const TraceParams p) {
    trace_body<true, kLds, kThreads, kScan, kCache, kHitLds, kCarry, kStash, kMatsL2, kSgLds, kGridQ>(p);
}

// ... and the flat LDS hit-stash kernels without far-hit state (trace_body, kFarState == false; rt_trace_variants.h RT_TRACE_LEAN_VARIANTS),
// as entries of their own: the kernels above keep their names and their code
template <bool kLds, int kThreads, int kScan, bool kCache, bool kHitLds, bool kCarry, bool kStash, bool kMatsL2, bool kSgLds, bool kGridQ>
__global__ void __launch_bounds__(kThreads, 1) rt_trace_kernel_lean(const TraceParams p) {
    trace_body<false, kLds, kThreads, kScan, kCache, kHitLds, kCarry, kStash, kMatsL2, kSgLds, kGridQ, false>(p);
}
template <bool kLds, int kThreads, int kScan, bool kCache, bool kHitLds, bool kCarry, bool kStash, bool kMatsL2, bool kSgLds, bool kGridQ>
__global__ void __launch_bounds__(kThreads, 1) rt_trace_kernel_lights_lean(const TraceParams p) {
    trace_body<true, kLds, kThreads, kScan, kCache, kHitLds, kCarry, kStash, kMatsL2, kSgLds, kGridQ, false>(p);
}

// ============================================================ ray-generation tables (A1, A9)
// jitter[k] = Halton2D(s0+k; 2,3) (spheres-app.cpp:140), lens[k] = HaltonSampleDisk(k0+k; 4,5) (:152)
// The first threads also set the queue cursors (and, frame pipelining, the control block) for the trace kernel that follows.
__global__ void __launch_bounds__(256) rt_raygen_tables_kernel(float2* jitter, uint32_t s0, uint32_t nJitter, float2* lens, uint32_t k0,
                                                               uint32_t nLens, uint32_t sampler, uint32_t* shardHeads = nullptr,
                                                               FrameCtl* ctl = nullptr) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (shardHeads && k < kQueueShards) shardHeads[kShardStrideWords * k] = 0u;
    if (ctl && k == 0) ctl->oldest_open = 0xffffffffu;
    if (k < nJitter) jitter[k] = make_float2(halton(s0 + k, 2), halton(s0 + k, 3));
    if (k < nLens) {
        float lx, ly;
        halton_disk_4_5(k0 + k, lx, ly, sampler);
        lens[k] = make_float2(lx, ly);
    }
}

// ====================================================== work order of the tiles (scheduling only)
// A persistent launch ends with the tail of whatever it started last; if those are 51-segment paths through the glass
// spheres, most of the chip waits for them (2 % of a C2 launch, 11 % at spp 16).  Three pilot rays per full tile (its first,
// middle and last pixel, sample 1) are traced through the production scan when an accumulation starts; the tile's class is
// the most expensive material among their first hits -- nothing, anything else, metal, glass (and, below them all, the tiles whose
// sphere list is empty: rt_tile_class_kernel) -- and the launches of the
// accumulation take the tiles by descending class: the sky, whose paths end after one scan, comes last.  Results do not
// depend on the order (every path has its own slot and stream); only the schedule does.
#ifndef RT_PILOTS_PER_TILE
#define RT_PILOTS_PER_TILE 3
#endif
constexpr uint32_t kPilotsPerTile = RT_PILOTS_PER_TILE;  // evenly spaced over the tile's 64 pixels, both ends included
__global__ void __launch_bounds__(256) rt_pilot_rays_kernel(const TraceParams p, uint32_t nFull, float* rays) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nFull * kPilotsPerTile) return;
    const uint32_t tile = t / kPilotsPerTile, which = t - tile * kPilotsPerTile;
    const uint32_t pl = (tile << 6) + (which * 63u + (kPilotsPerTile - 1u) / 2u) / (kPilotsPerTile - 1u);
    const uint32_t lr = pl / p.W;
    V3 o, d;
    gen_primary_ray(p, pl - lr * p.W, rowset_global_row(p.rs, lr), 1u, o, d);
    float* w = rays + 6 * (size_t)t;
    w[0] = o.x; w[1] = o.y; w[2] = o.z; w[3] = d.x; w[4] = d.y; w[5] = d.z;
}
// hits: rt_unit_closest_hit records (10 floats; [1] = original sphere index as bits, < 0 = miss), kPilotsPerTile per tile
RT_DEV uint32_t pilot_class(const float* hits, uint32_t t, const uint32_t* matTypeByOrig) {
    uint32_t c = 0;
    for (uint32_t k = 0; k < kPilotsPerTile; ++k) {
        const int oidx = __float_as_int(hits[10 * ((size_t)t * kPilotsPerTile + k) + 1]);
        if (oidx >= 0) {
            const uint32_t ty = matTypeByOrig[oidx];
            const uint32_t ck = ty == RT_MAT_DIELECTRIC_TRANSPARENT ? 3u : (ty == RT_MAT_METAL ? 2u : 1u);
            c = ck > c ? ck : c;
        }
    }
    return c;
}
// A tile next to a glass tile -- left, right, in the row above or below -- counts as glass too: the cap of a glass sphere
// that sticks out into the sky can be narrower than the pilots' spacing, and its 51-segment paths, started with the sky in
// the launch's last half millisecond, were the last three waves of a C2 launch (+1 % of its duration; tools/timeline_bulk.py).
// skyFlags (may be null; rt_sky_tiles_kernel below): a tile whose sphere list is EMPTY gets a class of its own below the sky, AFTER
// the neighbour rule -- the pilots guess, the empty list proves that no path of the tile meets anything.  The stored class is
// 0 for such a tile and 1 + the pilots' class for every other, so that the sorted order ends with exactly the flagged tiles.
constexpr uint32_t kTileClasses = 5;
__global__ void __launch_bounds__(256) rt_tile_class_kernel(const float* hits, uint32_t nFull, uint32_t W, const uint32_t* matTypeByOrig,
                                                            uint8_t* cls, const uint8_t* skyFlags = nullptr) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nFull) return;
    uint32_t c = pilot_class(hits, t, matTypeByOrig);
    if (c != 3u) {
        const int64_t first = (int64_t)t << 6;
        const int64_t near[6] = {first - 64, first + 64, first - (int64_t)W, first - (int64_t)W + 63, first + (int64_t)W, first + (int64_t)W + 63};
        for (int k = 0; k < 6; ++k) {
            const int64_t n = near[k] >> 6;  // the tile of that pixel
            if (near[k] >= 0 && n < (int64_t)nFull && pilot_class(hits, (uint32_t)n, matTypeByOrig) == 3u) c = 3u;
        }
    }
    cls[t] = (uint8_t)((skyFlags != nullptr && skyFlags[t] != 0u) ? 0u : c + 1u);
}
// Stable counting sort of the tiles by descending class; one workgroup, thread k owns a contiguous run of tiles.
__global__ void __launch_bounds__(1024) rt_tile_order_kernel(const uint8_t* cls, uint32_t nFull, uint32_t* order) {
    __shared__ uint32_t waveTot[16][kTileClasses];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    const uint32_t per = (nFull + 1023u) / 1024u;
    const uint32_t t0 = tid * per < nFull ? tid * per : nFull, t1 = (t0 + per) < nFull ? (t0 + per) : nFull;
    uint32_t cnt[kTileClasses] = {0u, 0u, 0u, 0u, 0u};
    for (uint32_t t = t0; t < t1; ++t) {
        const uint32_t c = cls[t];
        for (uint32_t k = 0; k < kTileClasses; ++k) cnt[k] += c == k ? 1u : 0u;
    }
    uint32_t pos[kTileClasses];  // where this thread's tiles of class k start
    for (uint32_t k = 0; k < kTileClasses; ++k) {
        uint32_t incl = cnt[k];
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t v = (uint32_t)__shfl_up((int)incl, off);
            if ((int)lane >= off) incl += v;
        }
        if (lane == 63u) waveTot[w][k] = incl;
        pos[k] = incl - cnt[k];
    }
    __syncthreads();
    uint32_t base = 0;
    for (int k = (int)kTileClasses - 1; k >= 0; --k) {
        uint32_t before = 0, tot = 0;
        for (uint32_t v = 0; v < 16u; ++v) {
            before += v < w ? waveTot[v][k] : 0u;
            tot += waveTot[v][k];
        }
        pos[k] += base + before;
        base += tot;
    }
    for (uint32_t t = t0; t < t1; ++t) {
        const uint32_t c = cls[t];
        uint32_t at = 0;
        for (uint32_t k = 0; k < kTileClasses; ++k) {
            at = c == k ? pos[k] : at;
            pos[k] += c == k ? 1u : 0u;
        }
        order[at] = t;
    }
}

// ====================================================== candidate masks of the tiles' primary rays
// rt_tile_mask.h: one wave per full tile, lane l decides groups l and l + 64 of the flat scan's top level; the two ballots are
// permuted into the scan's word layout (bit N from the top of word k = group kBase[k] + N + (N & 16), kBase = 0, 64, 16, 80) and
// lane 0 writes the tile's eight words with two 16-byte stores.  A tile with more than `limit` candidate groups, or one the
// construction does not apply to, gets flags = 0 and keeps the matrix-core filter.
static_assert(kTileMaskPerRay == 2.0 * (double)kMarginRel, "the masks bound the filter's own per-ray margin");
// Sphere lists (rt_tile_mask.h; lists may be null): the lanes then test the member entries of the candidate groups, 64 entries a round
// in ascending order, and append the listed ones behind the record's count (ballot + prefix offsets).
__global__ void __launch_bounds__(256) rt_tile_mask_kernel(const TraceParams p, uint32_t nFull, uint32_t limit, uint32_t* __restrict__ words,
                                                           uint32_t sphLimit, uint16_t* __restrict__ lists) {
    const uint32_t tile = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (tile >= nFull) return;  // wave-uniform
    RT_SITE(T_MASK);
    const TileMaskCam c = tile_mask_cam(p.cam_o, p.cam_x, p.cam_y, p.cam_oip, p.aperture, p.focal, p.W, p.H);
    const uint32_t topLevel = p.n_levels - 1u;
    const uint32_t nTop = p.level_cnt[topLevel];
    const float4* bounds = p.tree + p.level_off[topLevel];
    int r0 = 0, r1 = 0;
    if (lane < nTop) {
        const float4 B = bounds[lane];
        const float b[4] = {B.x, B.y, B.z, B.w};
        r0 = tile_group_reached(c, p.rs, tile, b);
    }
    if (lane + 64u < nTop && nTop <= 128u) {
        const float4 B = bounds[lane + 64u];
        const float b[4] = {B.x, B.y, B.z, B.w};
        r1 = tile_group_reached(c, p.rs, tile, b);
    }
    const uint64_t m0 = __ballot(r0 > 0), m1 = __ballot(r1 > 0);
    const bool bad = __ballot(r0 < 0 || r1 < 0) != 0ull || nTop > 128u;
    if (lane == 0) {
        auto wordA = [](uint64_t m) { return __builtin_bitreverse32((uint32_t)m & 0xffffu) | (__builtin_bitreverse32((uint32_t)(m >> 32) & 0xffffu) >> 16); };
        auto wordB = [](uint64_t m) { return __builtin_bitreverse32((uint32_t)(m >> 16) & 0xffffu) | (__builtin_bitreverse32((uint32_t)(m >> 48) & 0xffffu) >> 16); };
        const uint32_t cnt = (uint32_t)(__popcll(m0) + __popcll(m1));
        uint4* w = reinterpret_cast<uint4*>(words + (size_t)kTileMaskWords * tile);
        w[0] = make_uint4(wordA(m0), wordA(m1), wordB(m0), wordB(m1));
        w[1] = make_uint4(tile_mask_flags(bad, cnt, limit), cnt, 0u, 0u);
    }
    if (lists != nullptr) {  // wave-uniform
        RT_SITE(T_SPHERES);
        uint16_t* rec = lists + (size_t)kTileSphereHalfs * tile;
        const bool masked = tile_mask_flags(bad, (uint32_t)(__popcll(m0) + __popcll(m1)), limit) != 0u && sphLimit != 0u && sphLimit <= kTileSphereMax;
        uint32_t nS = 0;
        for (uint32_t e0 = 0; masked && e0 < 4u * nTop && nS <= sphLimit; e0 += 64u) {
            const uint32_t e = e0 + lane, g = e >> 2;
            bool in = false;
            if (g < nTop && e < p.n_padded) {
                const int gr = (int)(((g < 64u ? m0 : m1) >> (g & 63u)) & 1ull);
                const float4 B = p.leaf[e];
                const float b[4] = {B.x, B.y, B.z, B.w};
                in = tile_entry_listed(c, p.rs, tile, gr, p.orig[e], b);
            }
            const uint64_t m = __ballot(in);
            const uint32_t at = nS + prefix_count(m);
            if (in && at < sphLimit) rec[1u + at] = (uint16_t)e;
            nS += (uint32_t)__popcll(m);
        }
        if (lane == 0) rec[0] = (uint16_t)((masked && nS <= sphLimit) ? nS : kTileSphereNone);
    }
}

// ====================================================== tiles kept out of the trace queue
// A full tile whose sphere list is EMPTY can only see the sky: every sample of every pixel of it is the one constant
// (0 + 1 * sky) * exposure (K_GEN above).  Where an accumulation starts, this kernel writes -- into buffers of the accumulation's own,
// not the mask tables, which rt_unit_tile_masks may rebuild for another picture -- flags[tile] = 1 iff the tile's list header is 0,
// info[0] += the number of flagged tiles (zeroed by the caller) and info[1..3] = the constant sample, formed by the V3 expressions
// of the miss transition and finishPath, so that a -0 channel, a NaN or an infinity keeps the bits the traced path gives it.
// rt_tile_class_kernel puts the flagged tiles last in work order, the host then leaves them out of the queue, and the tile-aware
// accumulation below adds the constant for them instead of reading the sample buffer.
__global__ void __launch_bounds__(256) rt_sky_tiles_kernel(const TraceParams p, const uint16_t* __restrict__ lists, uint32_t nFull,
                                                           uint8_t* __restrict__ flags, uint32_t* __restrict__ info) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const bool empty = t < nFull && lists[(size_t)kTileSphereHalfs * t] == 0u;
    if (t < nFull) flags[t] = empty ? 1u : 0u;
    const uint32_t n = (uint32_t)__popcll(__ballot(empty));
    if ((threadIdx.x & 63u) == 0u && n != 0u) atomicAdd(&info[0], n);
    if (t == 0u) {
        const V3 sky = v3(p.sky_emit[0], p.sky_emit[1], p.sky_emit[2]);
        const V3 skyRad = v3(0.f, 0.f, 0.f) + v3(1.f, 1.f, 1.f) * sky;
        const float expo = p.exposure;
        info[1] = __float_as_uint(skyRad.x * expo);
        info[2] = __float_as_uint(skyRad.y * expo);
        info[3] = __float_as_uint(skyRad.z * expo);
    }
}
// After a launch whose queue left flagged tiles out: what the trace kernel would have added to the counters for those tiles' planes
// -- one traversal and one segment per path ([0], [1]) and, where the kernel is one that finishes such planes without rays (kSky;
// else planes = 0: the other kernels keep no tile statistics), one table-taking, direct, ray-less scan per plane ([3], [4], [5]).
__global__ void __launch_bounds__(64) rt_sky_counters_kernel(unsigned long long* counters, unsigned long long paths, unsigned long long planes) {
    const uint32_t k = threadIdx.x;
    if (k < 2u) counters[k] += paths;
    else if (k >= 3u && k < 6u) counters[k] += planes;
}

// ============================================================== ordered accumulation (A16)
// hdr[pixel] += sample(pixel, s) for s = s0 .. s0+spp-1 in that order (spheres-app.cpp:182-183).
// kMoments (rt_set_noise_estimate on): the second moments beside it, sq[pixel] += RN(sample^2) for the same planes in the same order
// (rt_noise.h); hdr and sq are carried in registers and written once, and the hdr arithmetic is the same statements, so the strip
// has the same bits either way.
// kTiles: a pixel of a flagged tile (rt_sky_tiles_kernel) does not read the sample buffer -- whose planes of that tile the trace
// launch may not have written -- but performs the same `count` sequential adds of the constant sample skyC.  A tile is one wave:
// the branch is wave-uniform.
template <bool kMoments, bool kTiles>
RT_DEV void accumulate_body(const float* __restrict__ samples, float* __restrict__ hdr, float* __restrict__ sq, uint32_t npix, uint32_t spp,
                            uint32_t first, uint32_t count, const uint8_t* __restrict__ skyFlags, const float* __restrict__ skyC) {
    const uint32_t pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= npix) return;
    float r = hdr[3 * (size_t)pix], g = hdr[3 * (size_t)pix + 1], b = hdr[3 * (size_t)pix + 2];
    float qr = 0.f, qg = 0.f, qb = 0.f;
    if (kMoments) {
        qr = sq[3 * (size_t)pix];
        qg = sq[3 * (size_t)pix + 1];
        qb = sq[3 * (size_t)pix + 2];
    }
    // tiled buffer [tile of 64 pixels][sample][pixel in tile] (path_coordinates): the 64 lanes of a wave read 768
    // contiguous bytes per sample plane; eight planes in flight, the adds stay sequential in s.  first / count: the planes
    // [first, first + count) of the buffer's spp (render-ahead batching adds the planes of one call at a time).
    const uint32_t nFull = npix >> 6, tile = pix >> 6;
    const uint32_t stride = tile < nFull ? 64u : npix - (nFull << 6);
    const float3* sp = reinterpret_cast<const float3*>(samples) + (size_t)tile * 64u * spp + (pix - (tile << 6));
    uint32_t s = first < spp ? first : spp;
    const uint32_t end = count > spp - s ? spp : s + count;
    if (kTiles && tile < nFull && skyFlags[tile] != 0u) {
        const float cx = skyC[0], cy = skyC[1], cz = skyC[2];
        const float cxx = cx * cx, cyy = cy * cy, czz = cz * cz;  // rounded first, added second (rt_noise.h)
        for (; s < end; ++s) {
            r += cx;
            g += cy;
            b += cz;
            if (kMoments) {
                qr = qr + cxx;
                qg = qg + cyy;
                qb = qb + czz;
            }
        }
    }
    for (; s + 8 <= end; s += 8) {
        float3 v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = sp[(size_t)(s + k) * stride];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            r += v[k].x;
            g += v[k].y;
            b += v[k].z;
            if (kMoments) {
                // the contract (rt_noise.h): the square rounds to binary32 FIRST, the add rounds second -- never an fmaf
                qr = qr + (v[k].x * v[k].x);
                qg = qg + (v[k].y * v[k].y);
                qb = qb + (v[k].z * v[k].z);
            }
        }
    }
    for (; s < end; ++s) {
        const float3 v = sp[(size_t)s * stride];
        r += v.x;
        g += v.y;
        b += v.z;
        if (kMoments) {
            qr = qr + (v.x * v.x);  // two roundings, as above
            qg = qg + (v.y * v.y);
            qb = qb + (v.z * v.z);
        }
    }
    hdr[3 * (size_t)pix] = r;
    hdr[3 * (size_t)pix + 1] = g;
    hdr[3 * (size_t)pix + 2] = b;
    if (kMoments) {
        sq[3 * (size_t)pix] = qr;
        sq[3 * (size_t)pix + 1] = qg;
        sq[3 * (size_t)pix + 2] = qb;
    }
}
__global__ void __launch_bounds__(256) rt_accumulate_kernel(const float* __restrict__ samples, float* __restrict__ hdr, uint32_t npix,
                                                            uint32_t spp, uint32_t first = 0, uint32_t count = 0xffffffffu) {
    accumulate_body<false, false>(samples, hdr, nullptr, npix, spp, first, count, nullptr, nullptr);
}
__global__ void __launch_bounds__(256) rt_accumulate_moments_kernel(const float* __restrict__ samples, float* __restrict__ hdr,
                                                                    float* __restrict__ sq, uint32_t npix, uint32_t spp, uint32_t first = 0,
                                                                    uint32_t count = 0xffffffffu) {
    accumulate_body<true, false>(samples, hdr, sq, npix, spp, first, count, nullptr, nullptr);
}
// ... and their tile-aware forms, launched whenever the running accumulation has flags
__global__ void __launch_bounds__(256) rt_accumulate_tiles_kernel(const float* __restrict__ samples, float* __restrict__ hdr, uint32_t npix,
                                                                  uint32_t spp, uint32_t first, uint32_t count,
                                                                  const uint8_t* __restrict__ skyFlags, const float* __restrict__ skyC) {
    accumulate_body<false, true>(samples, hdr, nullptr, npix, spp, first, count, skyFlags, skyC);
}
__global__ void __launch_bounds__(256) rt_accumulate_moments_tiles_kernel(const float* __restrict__ samples, float* __restrict__ hdr,
                                                                          float* __restrict__ sq, uint32_t npix, uint32_t spp, uint32_t first,
                                                                          uint32_t count, const uint8_t* __restrict__ skyFlags,
                                                                          const float* __restrict__ skyC) {
    accumulate_body<true, true>(samples, hdr, sq, npix, spp, first, count, skyFlags, skyC);
}

// ================================================================ noise estimate (rt_noise.h)
// out[pixel] = (absolute, relative) standard error of the pixel mean after n samples
__global__ void __launch_bounds__(256) rt_noise_map_kernel(const float* __restrict__ hdr, const float* __restrict__ sq, uint32_t npix, uint32_t n,
                                                           float floor, float2* __restrict__ out) {
    const uint32_t pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= npix) return;
    const float h[3] = {hdr[3 * (size_t)pix], hdr[3 * (size_t)pix + 1], hdr[3 * (size_t)pix + 2]};
    const float q[3] = {sq[3 * (size_t)pix], sq[3 * (size_t)pix + 1], sq[3 * (size_t)pix + 2]};
    float e[2];
    noise_estimate(h, q, n, floor, e);
    out[pix] = make_float2(e[0], e[1]);
}
// red[k] = pixels whose relative error is above thr.t[k] (k < thr.n), red[kNoiseMaxThresholds] = bit pattern of the largest finite
// relative error.  Integer atomics only (a sum of counts, a maximum of non-negative floats' patterns): the answer does not depend
// on the order the waves arrive in.  red is zeroed by the caller.
__global__ void __launch_bounds__(256) rt_noise_summary_kernel(const float* __restrict__ hdr, const float* __restrict__ sq, uint32_t npix, uint32_t n,
                                                               float floor, NoiseThresholds thr, uint32_t* __restrict__ red) {
    const uint32_t pix = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = pix < npix;
    float rel = 0.f;
    if (live) {
        const float h[3] = {hdr[3 * (size_t)pix], hdr[3 * (size_t)pix + 1], hdr[3 * (size_t)pix + 2]};
        const float q[3] = {sq[3 * (size_t)pix], sq[3 * (size_t)pix + 1], sq[3 * (size_t)pix + 2]};
        float e[2];
        noise_estimate(h, q, n, floor, e);
        rel = e[1];
    }
    const uint32_t bits = __float_as_uint(rel);
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t k = 0; k < thr.n && k < kNoiseMaxThresholds; ++k) {
        const uint32_t c = (uint32_t)__popcll(__ballot(live && noise_above(rel, bits, thr.t[k])));
        if (lane == 0 && c != 0u) atomicAdd(&red[k], c);
    }
    uint32_t m = (live && noise_is_finite(bits)) ? bits : 0u;
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)m, off);
        m = o > m ? o : m;
    }
    if (lane == 0 && m != 0u) atomicMax(&red[kNoiseMaxThresholds], m);
}

// ================================================== ordered accumulation of pipelined regions (A16)
// Frame pipelining: add every region that is complete -- sequence numbers committed+1 .. min(newest, oldest_open - 1) -- to
// the HDR strip, region by region and sample by sample in increasing s (spheres-app.cpp:182-183).  The commit point is kept
// TWICE (FrameCtl): commit kernel number k reads entry k & 1 and its block 0 writes the new point to entry (k + 1) & 1, which
// nobody reads before the next commit kernel -- no closing ticket, no "last block".  Every block therefore reads the same
// committed_seq / oldest_open: the entry it reads is not written during this kernel, oldest_open only by the trace kernels.
struct RegionTable {
    uint32_t seq[kMaxFramesInFlight];  // by ring slot (sequence % regions): the call that owns it
    uint32_t spp[kMaxFramesInFlight];  // ... and its samples per pixel
};
__global__ void __launch_bounds__(256) rt_commit_kernel(const float* __restrict__ ring, float* __restrict__ hdr, uint32_t npix,
                                                        uint32_t regionEntries, uint32_t nRing, RegionTable rt, FrameCtl* ctl,
                                                        uint32_t newestSeq, uint32_t commitNo) {
    const uint32_t committed = ctl->committed_seq[commitNo & 1u], open = ctl->oldest_open;
    uint32_t limit = newestSeq;
    if (open != 0xffffffffu && open - 1u < limit) limit = open - 1u;
    if (limit < committed) limit = committed;
    if (blockIdx.x == 0 && threadIdx.x == 0) {  // the other entry: nobody reads it before the next commit kernel
        uint32_t add = 0;
        for (uint32_t q = committed + 1u; q <= limit; ++q) add += rt.spp[q % nRing];
        ctl->committed_seq[(commitNo + 1u) & 1u] = limit;
        ctl->committed_samples[(commitNo + 1u) & 1u] = ctl->committed_samples[commitNo & 1u] + add;
    }
    if (limit == committed) return;
    for (uint32_t pix = blockIdx.x * blockDim.x + threadIdx.x; pix < npix; pix += gridDim.x * blockDim.x) {
        float r = hdr[3 * (size_t)pix], g = hdr[3 * (size_t)pix + 1], b = hdr[3 * (size_t)pix + 2];
        const uint32_t nFull = npix >> 6, tile = pix >> 6;
        const uint32_t stride = tile < nFull ? 64u : npix - (nFull << 6);
        for (uint32_t q = committed + 1u; q <= limit; ++q) {
            const uint32_t slot = q % nRing, spp = rt.spp[slot];
            // the region's buffer is tiled like the one-shot sample buffer: [tile of 64 pixels][sample][pixel in tile]
            const float3* sp = reinterpret_cast<const float3*>(ring) + (size_t)slot * regionEntries + (size_t)tile * 64u * spp + (pix - (tile << 6));
            for (uint32_t s = 0; s < spp; ++s) {
                const float3 v = sp[(size_t)s * stride];
                r += v.x;
                g += v.y;
                b += v.z;
            }
        }
        hdr[3 * (size_t)pix] = r;
        hdr[3 * (size_t)pix + 1] = g;
        hdr[3 * (size_t)pix + 2] = b;
    }
}

// ====================================================================== resolve (A17)
// hdr / n, ACES fit, gamma 1/2.2, XMStoreColor (spheres-app.cpp:186-214); output R,G,B bytes.
RT_DEV float tonemap_channel(float h, float n) {
    const float a = 2.51f, b = 0.03f, c = 2.43f, d = 0.59f, e = 0.14f;
    float color = h / n;
    color = sat1((color * (a * color + b)) / (color * (c * color + d) + e));
    color = rt_powf(color, 1 / 2.2f);
    return color;
}
// committedSamples (frame pipelining): the number of samples in the strip is only known on the device
__global__ void __launch_bounds__(256) rt_resolve_kernel(const float* __restrict__ hdr, uint8_t* __restrict__ ldr, uint32_t npix,
                                                         uint32_t nSamples, const uint32_t* committedSamples = nullptr) {
    const uint32_t pix = blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= npix) return;
    if (committedSamples) nSamples = *committedSamples > 0u ? *committedSamples : 1u;
    const float n = (float)nSamples;
    for (int ch = 0; ch < 3; ++ch) ldr[3 * (size_t)pix + ch] = (uint8_t)rne_u8(tonemap_channel(hdr[3 * (size_t)pix + ch], n));
}

// ============================================================ feature buffers (rt_features.h)
// First-hit albedo, normal, depth, coverage and object id of the samples [s0, s1) of every local pixel, summed on the device.
// The ray is gen_primary_ray's, the hit the PRODUCTION scan's -- the same table staging and the same scan functions as
// k_unit_closest below, i.e. as the variant of rt_trace_kernel that rt_render launches for the scene -- and the sample's values
// are rt_features.h feature_sample's.  One wave owns 64 consecutive local pixels (a tile; lanes past npix stay in the
// wave-cooperative scans with live == false), workgroups are persistent over the tiles, the tables are staged once per workgroup,
// and the loop over s runs here with the eight sums and the id in registers: a continuing call (cont) loads the pixel's sums
// first and goes on adding in order, so any split of a sample range gives the bits of one call.  One read-modify-write of the
// strip per call, as two aligned 16-byte halves per pixel; no per-sample buffer in global memory.  The material of the hit
// sphere comes from the table the hit processing reads (p.mats, per scan entry), through L2: one record per lane and sample.
// Nothing rt_render relies on is read or written: the ray-generation tables are the feature pass's own.
struct FeatureParams {
    float* feat;        // [npix][8] sums (16-byte aligned)
    uint32_t* ids;      // [npix] id of the sample added last
    uint32_t npix;      // local pixels of the strip
    uint32_t s0, s1;    // sample indices [s0, s1), 1-based
    uint32_t cont;      // 1: the strip holds the sums of the samples before s0
    float sky[3];       // feature_sky_albedo of the scene's sky
};
template <bool kLds, int kScan>
__global__ void __launch_bounds__(256) rt_features_kernel(const TraceParams p, const FeatureParams f) {
    extern __shared__ float4 smem[];
    constexpr uint32_t kWaveRegion = wave_region_bytes<kScan>();
    constexpr uint32_t kWaves = 256 / kWaveSize;
    uint16_t* candBase = reinterpret_cast<uint16_t*>(smem);
    float4* tabBase = smem + kWaves * (kWaveRegion / 16);
    SceneTabs T;
    stage_scene<kLds, kScan>(p, tabBase, T);
    __syncthreads();
    const uint32_t lane = threadIdx.x & (kWaveSize - 1);
    const uint32_t wave = threadIdx.x / kWaveSize;
    uint16_t* waveCand = candBase + wave * (kWaveRegion / 2);
    const uint32_t nTiles = (f.npix + 63u) >> 6;
    const V3 sky = v3(f.sky[0], f.sky[1], f.sky[2]);
    for (uint32_t tile = blockIdx.x * kWaves + wave; tile < nTiles; tile += gridDim.x * kWaves) {
        const uint32_t pl = (tile << 6) + lane;
        const bool live = pl < f.npix;
        uint32_t i = 0, j = 0;
        if (live) {
            const uint32_t lr = fastdiv(pl, p.fd_w);
            i = pl - lr * p.W;
            j = rowset_global_row(p.rs, lr, p.fd_rows);
        }
        float acc[kFeatureChannels];
        for (uint32_t c = 0; c < kFeatureChannels; ++c) acc[c] = 0.f;
        uint32_t id = kFeatureNoId;
        float4* strip = reinterpret_cast<float4*>(f.feat) + 2 * (size_t)pl;
        if (live && f.cont) {
            const float4 a = strip[0], b = strip[1];
            acc[0] = a.x; acc[1] = a.y; acc[2] = a.z; acc[3] = a.w;
            acc[4] = b.x; acc[5] = b.y; acc[6] = b.z; acc[7] = b.w;
            id = f.ids[pl];
        }
        for (uint32_t s = f.s0; s < f.s1; ++s) {
            V3 o = v3(0.f, 0.f, 0.f), d = v3(0.f, 0.f, 1.f);
            if (live) gen_primary_ray(p, i, j, s, o, d);
            float tmin = 0.f;
            int idx = -1;
            if (kScan == 3) {
                const GridParams G{T.gridCells, p.grid_nu, p.grid_nv, p.grid_ax_u, p.grid_ax_v, p.grid_g0u, p.grid_g0v, p.grid_inv_h, p.grid_rmax_over_h, p.grid_big_norm};
                scan_list_grid(T.scan, T.leaf, T.orig, G, T.gridCells, p.n_always, p.tree_box, p.bound_norm, o, d, live, tmin, idx, waveCand, lane);
            } else if (kScan != 0) {
                unsigned long long dbg[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                (void)dbg;
                scan_list_mfma<kScan == 2>(T.scan, T.leaf, T.orig, T.ops, T.nTiles, T.nTop, T.tree, p.level_off, p.n_levels, p.bound_norm, p.single_mask, p.n_always,
                                           p.tree_box_on ? p.tree_box : nullptr, o, d, live, tmin, idx, waveCand, lane, dbg);
            } else if (live) {
                scan_list_deferred(T.scan, T.orig, p.n_padded, o, d, tmin, idx, waveCand + lane);
            }
            if (live) {
                const bool hit = idx >= 0;
                Mat m{};
                uint32_t oidx = kFeatureNoId;
                V3 nrm = v3(0.f, 0.f, 0.f);
                if (hit) {  // the hit record, as k_unit_closest forms it
                    const float4 S = T.scan[idx];
                    const V3 pos = tmin * d + o;
                    nrm = (pos - v3(S.x, S.y, S.z)) / T.rad[idx];
                    oidx = T.orig[idx];
                    m = feature_material(p.mats[idx]);
                }
                float v[kFeatureChannels];
                uint32_t sid;
                feature_sample(hit, m, oidx, tmin, nrm, 0.5f * nrm.x + 0.5f, 0.5f * nrm.z + 0.5f, sky, v, sid);
                for (uint32_t c = 0; c < kFeatureChannels; ++c) acc[c] = acc[c] + v[c];
                id = sid;
            }
        }
        if (live) {
            strip[0] = make_float4(acc[0], acc[1], acc[2], acc[3]);
            strip[1] = make_float4(acc[4], acc[5], acc[6], acc[7]);
            f.ids[pl] = id;
        }
    }
}

// ================================================================== unit-test kernels
__global__ void k_unit_halton(const uint32_t* index, uint32_t base, uint32_t n, float* out) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) out[k] = halton(index[k], base);
}
__global__ void k_unit_math(uint32_t op, const float* x, const float* y, uint32_t n, float* out) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    float r = 0.f;
    if (op == 0) r = rt_sinf(x[k]);
    else if (op == 1) r = rt_cosf(x[k]);
    else if (op == 2) r = rt_powf(x[k], y[k]);
    else if (op == 3) r = rt_tanf(x[k]);
#if RT_MARKSTEIN
    else if (op == 4) r = recip_rn(x[k]);  // must equal 1.0f / x for normal x in [2^-100, 2^100]
    else if (op == 5) {                      // the quotient the hit processing forms (guarded): must equal x / y
        const V3 q = div3(v3(x[k], 0.f, -x[k]), y[k]);
        r = q.x;
    }
#else
    else if (op == 4) r = 1.0f / x[k];
    else if (op == 5) r = x[k] / y[k];
#endif
    else if (op == 6) r = x[k] / y[k];      // the compiler's IEEE division, on the device
    else if (op == 7) r = sqrt_rn(x[k]);    // the square root the path takes (guarded): must equal the IEEE root for every x
#if RT_FAST_SQRT
    else if (op == 8) r = sqrt_rn_core(x[k]);  // ... its fast form alone: the IEEE root for x in [2^-80, inf)
#else
    else if (op == 8) r = __builtin_sqrtf(x[k]);
#endif
    else if (op == 9) r = __builtin_sqrtf(x[k]);  // the compiler's IEEE square root, on the device
    out[k] = r;
}
__global__ void k_unit_primary(const TraceParams p, const uint32_t* ijs, uint32_t n, float* out) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    V3 o, d;
    gen_primary_ray(p, ijs[3 * k], ijs[3 * k + 1], ijs[3 * k + 2], o, d);
    float* w = out + 6 * (size_t)k;
    w[0] = o.x; w[1] = o.y; w[2] = o.z; w[3] = d.x; w[4] = d.y; w[5] = d.z;
}
// Closest hit through the PRODUCTION scan of the uploaded scene: the same table staging (stage_scene) and the same
// scan function (scan_list_mfma flat / hierarchy, or scan_list_deferred) as the variant of rt_trace_kernel that
// rt_render launches for this scene, 64 rays per wave.  LDS image: per-wave work-list regions, then the tables.
template <bool kLds, int kScan>
__global__ void __launch_bounds__(256) k_unit_closest(const TraceParams p, const float* rays, uint32_t n, float* out) {
    extern __shared__ float4 smem[];
    constexpr uint32_t kWaveRegion = wave_region_bytes<kScan>();
    uint16_t* candBase = reinterpret_cast<uint16_t*>(smem);
    float4* tabBase = smem + (256 / kWaveSize) * (kWaveRegion / 16);
    SceneTabs T;
    stage_scene<kLds, kScan>(p, tabBase, T);
    __syncthreads();
    const uint32_t lane = threadIdx.x & (kWaveSize - 1);
    uint16_t* waveCand = candBase + (threadIdx.x / kWaveSize) * (kWaveRegion / 2);
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = k < n;
    V3 o = v3(0.f, 0.f, 0.f), d = v3(0.f, 0.f, 1.f);
    if (live) {
        const float* r = rays + 6 * (size_t)k;
        o = v3(r[0], r[1], r[2]);
        d = v3(r[3], r[4], r[5]);
    }
    float tmin = 0.f;
    int idx = -1;
    unsigned long long dbg[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    (void)dbg;
    if (kScan == 3) {
        const GridParams G{T.gridCells, p.grid_nu, p.grid_nv, p.grid_ax_u, p.grid_ax_v, p.grid_g0u, p.grid_g0v, p.grid_inv_h, p.grid_rmax_over_h, p.grid_big_norm};
        scan_list_grid(T.scan, T.leaf, T.orig, G, T.gridCells, p.n_always, p.tree_box, p.bound_norm, o, d, live, tmin, idx, waveCand, lane);
    } else if (kScan != 0) {
        scan_list_mfma<kScan == 2>(T.scan, T.leaf, T.orig, T.ops, T.nTiles, T.nTop, T.tree, p.level_off, p.n_levels, p.bound_norm, p.single_mask, p.n_always, p.tree_box_on ? p.tree_box : nullptr, o, d, live,
                                   tmin, idx, waveCand, lane, dbg);
    } else if (live) {
        scan_list_deferred(T.scan, T.orig, p.n_padded, o, d, tmin, idx, waveCand + lane);
    }
    if (!live) return;
    float* w = out + 10 * (size_t)k;
    for (int c = 0; c < 10; ++c) w[c] = 0.f;
    const int oidx = idx >= 0 ? (int)T.orig[idx] : -1;
    w[1] = __int_as_float(oidx);
    if (idx >= 0) {
        const float4 S = T.scan[idx];
        const V3 pos = tmin * d + o;
        const V3 nrm = (pos - v3(S.x, S.y, S.z)) / T.rad[idx];
        w[0] = tmin;
        w[2] = pos.x; w[3] = pos.y; w[4] = pos.z;
        w[5] = nrm.x; w[6] = nrm.y; w[7] = nrm.z;
        w[8] = 0.5f * nrm.x + 0.5f;
        w[9] = 0.5f * nrm.z + 0.5f;
    }
}

// Camera::GetRay for given (uv, lens offset) pairs: in 4 floats, out origin xyz + direction xyz.
__global__ void k_unit_camera(const TraceParams p, const float* uvoff, uint32_t n, float* out) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const float uvx = uvoff[4 * k], uvy = uvoff[4 * k + 1], lensx = uvoff[4 * k + 2], lensy = uvoff[4 * k + 3];
    V3 o, d;
    camera_get_ray(p, uvx, uvy, lensx, lensy, o, d);
    float* w = out + 6 * (size_t)k;
    w[0] = o.x; w[1] = o.y; w[2] = o.z; w[3] = d.x; w[4] = d.y; w[5] = d.z;
}
// Material::Scatter + Emit + unoccluded DirectionalLight::Shade for one material record.
// in: ray dir 3, pos 3, normal 3, draws 3 (12 floats); out: scattered, atten 3, dir 3, draws used, local 3 (11 floats)
__global__ void k_unit_scatter(const TraceParams p, const rt_material* mat, const float* in, uint32_t n, float* out) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const float* q = in + 12 * (size_t)k;
    const Mat m = load_material(mat, 0);
    ScriptedDraws draws{{q[9], q[10], q[11]}, 0u};
    V3 atten, dir, local, localOcc;
    const bool sc = scatter_and_shade(p, m, v3(q[0], q[1], q[2]), v3(q[3], q[4], q[5]), v3(q[6], q[7], q[8]), draws, atten, dir, local, localOcc, p.sampler);
    float* w = out + 11 * (size_t)k;
    w[0] = sc ? 1.f : 0.f;
    w[1] = atten.x; w[2] = atten.y; w[3] = atten.z;
    w[4] = dir.x; w[5] = dir.y; w[6] = dir.z;
    w[7] = (float)draws.used;
    w[8] = local.x; w[9] = local.y; w[10] = local.z;
}
// The shadow question of the hit processing (processHit above) for given points and light `light` of the scene's list, over the
// uploaded tables: out = bit 0 occluded | bit 1 answered by any_hit_all (index off, or |p|^2 > sg_p0sq).  globLds: the index's
// global list from an LDS copy of (spheres, ids), staged as rt_trace_kernel's prologue stages globSph / globIds (dynamic LDS:
// sg_glob_slots(global entries) float4); else from its id list.  tier 2 (light 0 only): the question as the kernels without far-hit state
// ask it (trace_body farShadow) -- a point beyond the first index goes to the second one within ITS radius: bit 2 set, bit 1 clear.
__global__ void __launch_bounds__(256) k_unit_shadow(const TraceParams p, uint32_t light, uint32_t globLds, const float* pts, uint32_t n, uint8_t* out,
                                                     uint32_t tier) {
    extern __shared__ float4 smem[];
    const LightRec* Lk = light != 0u ? p.extra_lights + (light - 1u) : nullptr;
    const bool enabled = (Lk ? Lk->sg_enabled : p.sg_enabled) != 0u;
    const uint32_t nGlob = enabled ? (Lk ? Lk->sg_nglobal : p.sg_nglobal) : 0u;
    const uint16_t* glob = Lk ? Lk->global : p.sg_global;
    float4* globSph = smem;
    uint16_t* globIds = reinterpret_cast<uint16_t*>(globSph + nGlob);
    const bool inLds = globLds != 0u && enabled;
    if (inLds)
        for (uint32_t k = threadIdx.x; k < nGlob; k += blockDim.x) {
            const uint32_t id = glob[k];
            globSph[k] = p.scan[id];
            globIds[k] = (uint16_t)id;
        }
    __syncthreads();
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const V3 pos = v3(pts[3 * (size_t)k], pts[3 * (size_t)k + 1], pts[3 * (size_t)k + 2]);
    const float pp = dot3(pos, pos);
    bool useIndex, occ, useFar = false;
    if (Lk == nullptr) {
        const V3 sunDir = v3(p.sun_dir[0], p.sun_dir[1], p.sun_dir[2]);
        const float aSun = dot3(sunDir, sunDir);
        useIndex = p.sg_enabled && pp <= p.sg_p0sq;
        const LightRec* F = tier >= 2u ? far_index_rec(p) : nullptr;
        useFar = !useIndex && F != nullptr && pp <= F->sg_p0sq;
        occ = useIndex ? shadow_query(p, p.scan, p.sg_cell_start, p.sg_entries, p.sg_global, inLds, globSph, globIds, p.sg_sph, pos, sunDir, aSun)
              : useFar ? shadow_query(*F, p.scan, F->cell_start, F->entries, F->global, false, globSph, globIds, (const float4*)nullptr, pos, sunDir, aSun)
                       : any_hit_all(p.scan, p.n_padded, pos, sunDir, aSun);
    } else {
        const V3 dirK = v3(Lk->sun_dir[0], Lk->sun_dir[1], Lk->sun_dir[2]);
        const float aK = dot3(dirK, dirK);
        useIndex = Lk->sg_enabled && pp <= Lk->sg_p0sq;
        occ = useIndex ? shadow_query(*Lk, p.scan, Lk->cell_start, Lk->entries, Lk->global, inLds, globSph, globIds, (const float4*)nullptr, pos, dirK, aK)
                       : any_hit_all(p.scan, p.n_padded, pos, dirK, aK);
    }
    out[k] = (uint8_t)((occ ? 1u : 0u) | ((useIndex || useFar) ? 0u : 2u) | (useFar ? 4u : 0u));
}
// Resolve for given HDR triples (tonemap unit test): in 3 floats, out 3 bytes
__global__ void k_unit_tonemap(const float* hdr, uint32_t n, uint32_t nSamples, uint8_t* out) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    for (int ch = 0; ch < 3; ++ch) out[3 * (size_t)k + ch] = (uint8_t)rne_u8(tonemap_channel(hdr[3 * (size_t)k + ch], (float)nSamples));
}

}  // namespace rtd
