// rt_denoise_launch.h -- what rt_capi.hip sees of the denoiser's translation unit (rt_denoise.hip): one launcher over plain
// pointers.  The kernels live in a unit of their own so that the device code of rt_capi.hip -- the trace variants and their
// register allocation -- stays what it was (DESIGN.md "Denoise").
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../rt_denoise.h"
#include "../rt_rowset_map.h"
#include "../rt_temporal.h"

namespace rtdn {

constexpr uint32_t kTileW = 32, kTileH = 8;  // a 256-thread workgroup owns a 32 x 8 pixel tile: a wave is two rows of 32
constexpr uint32_t kStageLdsLimit = 64u * 1024u;  // the staged form runs where three planes of tile + halo fit this
enum Form : uint32_t { kFormNone = 0, kFormDirect = 1, kFormStaged = 2 };

// Bytes of LDS the staged form takes at a step: three float4 planes of (32 + 4 step) x (8 + 4 step) pixels.
inline uint32_t StageBytes(uint32_t step) { return (kTileW + 4u * step) * (kTileH + 4u * step) * 3u * 16u; }
// The measured cut (profiles/denoise_timing.txt): staging pays at these steps.  RT_DENOISE_STAGE overrides it.
inline bool StageByDefault(uint32_t step) { return step <= 2u; }
// stageKnob: -1 unset, 0 never staged, 1 staged wherever the LDS image fits
inline bool Staged(uint32_t step, int stageKnob) {
    if (StageBytes(step) > kStageLdsLimit) return false;
    return stageKnob < 0 ? StageByDefault(step) : stageKnob != 0;
}

struct Strips {
    const float* hdr;   // [npix][3]
    const float* sq;    // [npix][3]
    const float* feat;  // [npix][8], 16-byte aligned
    uint32_t n, m;      // samples in hdr / sq, samples in feat
    uint32_t W, rows;
    void* state[2];     // [npix] float4 (c.rgb, v), ping and pong
    void* guide[2];     // [npix] float4 each: (albedo rgb, normal x), (normal y, normal z, depth, coverage)
    float* den;         // [npix][3] out
    float* denVar;      // [npix] out
};

// A call of the denoiser is a point on three independent axes, each described once here (Job below puts them together).
//
// 1. Where a pixel's current-frame inputs lie.  In image order (parts == NULL), or -- the parts form, rt_denoise_shards* -- hdr, sq
//    and feat of Strips and Temporal::ids are the gathered parts of a row-sharded picture, [nshards] parts of rowsMax x W pixels each,
//    and W x rows is the IMAGE's row range; row j of it is the row of the part that ../rt_rowset_map.h names.  The prepare pass reads
//    through the mapping; everything it writes, the history and everything the levels touch are in image order.
struct ShardLayout {
    uint32_t rowsMax, blockRows, nshards;
};

// 2. Where v0 comes from.  The second moments (spatialRadius == 0), or -- the spatial source, ../rt_denoise.h -- the (2 radius + 1)^2
//    window around the pixel, radius 1..3: rt_denoise_prepare_spatial_kernel (over parts: _spatial_shards_kernel) runs first and writes Strips::state[0] and Strips::guide;
//    Strips::sq is not read and may be NULL.  committed: NULL, or a device word that holds the strip's sample count where only the
//    device knows it (frames in flight: rt_resolve's rule, 0 reads as 1); Strips::n is then not read.  LDS of that pass at a radius:
inline uint32_t SpatialLdsBytes(uint32_t radius) { return (kTileW + 2u * radius) * (kTileH + 2u * radius) * 3u * 16u; }

// 3. What the history does.  Nothing (temporal == NULL), or -- the temporal form, ../rt_temporal.h -- the prepare pass also reprojects
//    every pixel into the history's camera, gathers the history there (fetch: nearest or bilinear), validates and blends, and writes
//    the new history -- one pass.  Level 0 then reads the new history's state and guides where they lie: Strips::state[0] and
//    Strips::guide are idle until level 1 writes state[0], so only a spatial pass, which writes them for the temporal pass to read,
//    needs the guide strips reserved.  The history is never updated in place: prev and next are different sets of buffers.
struct TemporalSet {
    void* state;     // [npix] float4 (c.rgb, v) before the levels
    void* guide[2];  // [npix] float4 each, as Strips::guide
    uint32_t* ids;   // [npix]
    uint32_t* len;   // [npix] frames blended into state (>= 1)
};
struct Temporal {
    const uint32_t* ids;   // [npix] the feature strips' ids of this frame
    rtd::TemporalGeom geom;  // geom.num_rows == Strips::rows
    rtd::TemporalCam cam, camPrev;
    rtd::TemporalParams params;
    uint32_t fetch;        // rtd::kTemporalFetchNearest or kTemporalFetchBilinear: which prepare kernel reads the history
    bool hasPrev;          // false: an empty history (prev is not read)
    TemporalSet prev, next;
    uint32_t* target;      // [npix] out
};

struct Job {
    Strips strips;
    const ShardLayout* parts;   // axis 1
    uint32_t spatialRadius;     // axis 2
    const uint32_t* committed;
    const Temporal* temporal;   // axis 3
};
// Enqueues the spatial pass if asked for, the one prepare kernel the axes select and one a-trous launch per level on the stream (a
// hipStream_t).  forms[l] = the form level l took.  Returns a hipError_t as int (0 = success); nothing is waited for.  Every product of
// the axes runs.  Parts with a spatial radius: the spatial pass reads hdr and feat through the mapping (committed is not read: the parts
// are a snapshot, n is Strips::n), and a temporal pass after it reads only Temporal::ids there -- the planes it takes lie in image order.
int Launch(void* stream, const Job& j, const rtd::DenoiseParams& P, int stageKnob, uint32_t forms[rtd::kDenoiseMaxLevels]);

}  // namespace rtdn

// What rt_denoise_shards and rt_unit_denoise_shards_host refuse, checked once (rt_denoise_host.cpp): the shape, the sample counts and
// the parameters (NULL: the defaults), which are returned in P.  The struct's own pointers are looked at only with devicePointers.
// spatial (rt_denoise_shards_variance and its twins under the spatial source): sq is not looked at and may be NULL, and the parts need
// n >= 1 instead of n >= 2; nothing else differs.
struct rt_shard_parts;
struct rt_denoise_params;
// ... and what rt_denoise_shards_temporal and rt_unit_temporal_shards_host refuse: all of that for frame->parts, the frame's own
// fields (ids only with devicePointers), the fetch and the temporal parameters (NULL: that fetch's defaults), returned in T.  On
// RT_OK *G is the geometry of the parts' row range in the W x H image.
struct rt_shard_frame;
struct rt_temporal_params;
namespace rtdn {
// Where row y of the image's row range starts in the gathered parts, in pixels: the host twins' reading of the mapping.
size_t PartsRowStart(const ShardLayout& parts, uint32_t W, uint32_t y);
int CheckShardParts(const char* who, const rt_shard_parts* parts, const rt_denoise_params* params, bool devicePointers, rtd::DenoiseParams* P,
                    bool spatial = false);
int CheckShardFrame(const char* who, const rt_shard_frame* frame, const rt_denoise_params* params, const rt_temporal_params* tparams, uint32_t fetch,
                    bool devicePointers, rtd::DenoiseParams* P, rtd::TemporalParams* T, rtd::TemporalGeom* G, bool spatial = false);
}
