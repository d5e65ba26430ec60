// rt_layout_consts.h -- the constants the scene preparation on the host (host/rt_scene_prep.cpp) shares with the kernels that read
// its tables (rt_params.h, rt_scan.h).  Plain C++: no HIP header, so that the host unit builds without one.
#pragma once

#include <stdint.h>

namespace rtd {

constexpr uint32_t kMaxLevels = 6;  // levels of group bounds (4-ary): 128 * 4^5 groups at most
// K of the filter margins (units of eps * a * G; the host folds the same K into each bound): the matrix-core level needs
// 101*16 (exact-path rounding, amplified by the member offsets) + ~600 (split-bf16 operands); levels tested on the VALU
// in f32 need 101*16 + 30; a one-sphere bound (offset 0) needs 16 + 30.
constexpr float kMarginK = 4096.f, kMarginKValu = 2048.f, kMarginKLeaf = 64.f;

// ---- the dynamic LDS image of the trace kernels: what the launch plan on the host (host/rt_launch_plan.cpp) sizes and the kernels
// lay out.  Each value has its one definition here; where it follows from something only the device code knows (a struct, the
// experiment macros of rt_scan.h) the number stands here and a static_assert beside that something holds it to it.
constexpr uint32_t kSceneConstBytes = 256;                    // SceneConsts at the start of the image (rt_params.h) ...
constexpr uint32_t kConstBytes = kSceneConstBytes + 8 * 256;  // ... followed by the elementary functions' tables (255 words)
constexpr uint32_t kWaveListBytes = 2816;  // per wave, flat and VALU scan: item pools + per-ray best keys (rt_scan.h kPoolA, kPoolB)
constexpr uint32_t kWaveCandBytes = 3328;  // per wave, hierarchy scan: (ray, node) and (ray, sphere) lists + keys (kTreeWork, kTreeExact)
constexpr uint32_t kWaveGridBytes = 4480;  // per wave, cell-grid scan: (ray, slab) items, exact list + keys (kGridWork, kGridExact)
constexpr uint32_t kFlatLeafStride = 5;    // float4 slots per group in the flat scan's LDS copy of the one-sphere bounds (rt_scan.h: why five)
constexpr uint32_t kOpsPerTile = 8 * 64;   // dwords of the group operand image per 32-group tile
constexpr uint32_t kStashDwords = 19;      // dwords of a hit-stash record (rt_kernels.h)
constexpr uint32_t kRayCacheBytes = 64 * 48;  // per-wave cache of prepared paths
constexpr uint32_t kQueueBlock = 128;  // paths a wave takes from the global queue per claim (claimed one block ahead: rt_kernels.h)
// tiles of the filter's operand image for nTop groups: always an even number (bitmap words cover two tiles; rt_scan.h)
constexpr uint32_t mfma_tiles_for(uint32_t nTop) { return (((nTop + 31u) / 32u) + 1u) & ~1u; }
// The shadow index's GLOBAL list (spheres whose footprint covers much of the grid: the floor, the big spheres; <= 64) is walked by
// every query: its spheres and ids sit in LDS in every variant -- 18 bytes each -- so that the walk reads them directly instead of
// chasing id -> sphere through the tables (two dependent L2 reads per pair of entries in the large-scene variants).
constexpr uint32_t sg_glob_slots(uint32_t nGlobal) { return nGlobal ? nGlobal + (nGlobal * 2u + 15u) / 16u : 0u; }

}  // namespace rtd
