// rt_capi.hip — C-ABI implementation (include/rt_api.h) over the HIP kernels in rt_kernels.h.
// Builds into librt_hip.so with hipcc --offload-arch=gfx950.  No CPU fallback exists: every entry
// point that needs the device fails with RT_ERR_NO_DEVICE / RT_ERR_HIP when it is absent.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <set>
#include <string>
#include <unordered_map>
#include <array>
#include <initializer_list>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/rt_api.h"
#include "host/rt_camera_launch.h"
#include "host/rt_denoise_host.h"
#include "host/rt_edit_launch.h"
#include "host/rt_denoise_launch.h"
#include "host/rt_launch_plan.h"
#include "host/rt_scene_edit.h"
#include "host/rt_scene_prep.h"
#include "host/rt_sequence.h"
#include "host/rt_tile_tables.h"
#include "rt_kernels.h"

using rtprep::EnvU32;
using rtprep::Fail;

// the prepared tables are copied to the device as they lie: the device reads float4 / uint4 where the host wrote F4 / U4
static_assert(sizeof(rtprep::F4) == sizeof(float4) && offsetof(rtprep::F4, y) == offsetof(float4, y) && offsetof(rtprep::F4, z) == offsetof(float4, z) &&
                  offsetof(rtprep::F4, w) == offsetof(float4, w),
              "rtprep::F4 is laid out like float4");
static_assert(sizeof(rtprep::U4) == sizeof(uint4) && offsetof(rtprep::U4, y) == offsetof(uint4, y) && offsetof(rtprep::U4, z) == offsetof(uint4, z) &&
                  offsetof(rtprep::U4, w) == offsetof(uint4, w),
              "rtprep::U4 is laid out like uint4");

namespace {

#define RT_HIP(call)                                                                                             \
    do {                                                                                                         \
        hipError_t e_ = (call);                                                                                  \
        if (e_ != hipSuccess) {                                                                                  \
            return Fail(e_ == hipErrorOutOfMemory ? RT_ERR_OUT_OF_MEMORY : RT_ERR_HIP,                           \
                        std::string(#call) + ": " + hipGetErrorString(e_) + " (" __FILE__ ":" + std::to_string(__LINE__) + ")"); \
        }                                                                                                        \
    } while (0)

// Device memory with one owner: freed when its owner goes -- a member of rt_ctx inside `delete ctx` (rt_destroy), a local of a unit
// entry at its return -- and never copied.
template <typename T>
struct DevBuf {
    T* ptr = nullptr;
    size_t count = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { Release(); }
    int Reserve(size_t n) {
        if (n <= count) return RT_OK;
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr;
        count = 0;
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&ptr), n * sizeof(T));
        if (e != hipSuccess) {
            (void)hipGetLastError();  // the failure is reported here; later hipGetLastError() checks must not see it again
            return Fail(RT_ERR_OUT_OF_MEMORY, std::string("hipMalloc: ") + hipGetErrorString(e));
        }
        count = n;
        return RT_OK;
    }
    // Room for src.size() + extra elements, and the vector's content copied to its start (S: T's layout on the host).
    template <typename S>
    int Upload(const std::vector<S>& src, size_t extra = 0) {
        static_assert(sizeof(S) == sizeof(T), "a table is copied to the device as it lies");
        const int rc = Reserve(src.size() + extra);
        if (rc != RT_OK) return rc;
        if (!src.empty()) RT_HIP(hipMemcpy(ptr, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
        return RT_OK;
    }
    // The unit entries' round trip: room for n elements filled from host memory; and n elements back, once the stream has run dry.
    int UploadFrom(const T* src, size_t n) {
        const int rc = Reserve(n);
        if (rc != RT_OK) return rc;
        RT_HIP(hipMemcpy(ptr, src, n * sizeof(T), hipMemcpyHostToDevice));
        return RT_OK;
    }
    int DownloadTo(T* dst, size_t n, hipStream_t stream) const {
        RT_HIP(hipStreamSynchronize(stream));
        RT_HIP(hipMemcpy(dst, ptr, n * sizeof(T), hipMemcpyDeviceToHost));
        return RT_OK;
    }
    void Release() {
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr;
        count = 0;
    }
};
static_assert(!std::is_copy_constructible<DevBuf<float>>::value, "a DevBuf is the one owner of its memory");

// Room for the three tables of an index of ANY direction: the builder's own bounds (host/rt_scene_edit.h ShadowRoomOf), so that
// rt_turn_lights never allocates under running kernels -- and an index that is disabled now has its buffers all the same, a turn can
// enable it.
int ReserveShadowGrid(uint32_t maxCells, DevBuf<uint16_t>& cells, DevBuf<uint16_t>& entries, DevBuf<uint16_t>& global) {
    const rtscene::ShadowRoom room = rtscene::ShadowRoomOf(maxCells);
    int rc;
    if ((rc = cells.Reserve(room.cellWords)) != RT_OK) return rc;
    if ((rc = entries.Reserve(room.entries)) != RT_OK) return rc;
    return global.Reserve(room.global);
}
// A shadow index's three tables (the id lists with one spare element, so that an empty list still has an address): the actual bytes,
// into buffers that ReserveShadowGrid has sized.
int UploadShadowGrid(const rtprep::ShadowGrid& G, DevBuf<uint16_t>& cells, DevBuf<uint16_t>& entries, DevBuf<uint16_t>& global) {
    int rc;
    if ((rc = cells.Upload(G.cellStart)) != RT_OK) return rc;
    if ((rc = entries.Upload(G.entries, 1)) != RT_OK) return rc;
    return global.Upload(G.global, 1);
}
// ... and the same buffers as a staging plan's destinations (host/rt_scene_edit.h): the pointer and the room reserved at it
template <typename T>
rtscene::TableDest DestOf(const DevBuf<T>& b) {
    return {b.ptr, b.count * sizeof(T)};
}
rtscene::IndexDest IndexDestOf(const DevBuf<uint16_t>& cells, const DevBuf<uint16_t>& entries, const DevBuf<uint16_t>& global) {
    return {DestOf(cells), DestOf(entries), DestOf(global)};
}

}  // namespace

struct rt_ctx {
    int device = 0;
    hipStream_t ownStream = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t streamEv = nullptr;  // rt_set_stream: the end of the old stream's work, which the new stream waits for (never the host)
    std::vector<hipEvent_t> passEv;  // three timing events per sample-range pass of rt_render, grown on demand
    int cuCount = 0;
    size_t ldsPerBlockMax = 0;
    uint64_t workspaceLimit = 8ull << 30;

    // how rt_render calls are sequenced (host/rt_sequence.h): has-scene, the mode settings, the running accumulation, the pending batch
    // and the planes traced ahead.  Read freely here; changed only through rtseq's events and step reports.
    rtseq::State seq;

    // scene: what the caller gave, as of the last upload or edit (host/rt_scene_edit.h: read freely, changed only through rtscene's
    // commits), and what it became on the device
    rtscene::Record scene;
    DevBuf<float4> scan, tree, leaf;
    DevBuf<uint32_t> orig;
    DevBuf<uint16_t> sgCells, sgEntries, sgGlobal;
    DevBuf<float4> sgSph;  // large scenes: the scan record of every shadow-index entry (rt_params.h sg_sph)
    // lights 1 .. n_lights-1 (rt_params.h LightRec): their records and their shadow indices, in global memory
    struct ExtraLight {
        DevBuf<uint16_t> cells, entries, global;
    };
    ExtraLight extraIdx[RT_MAX_LIGHTS];
    DevBuf<rtd::LightRec> lightRecs;
    // light 0's second shadow index (rt_params.h far_index): its tables, in global memory like an extra light's; its record is the
    // last of lightRecs
    ExtraLight farIdx;
    DevBuf<uint16_t> gridCells;  // cell-grid scan: first scan entry per cell
    DevBuf<uint32_t> gridQ;      // ... and the quantised one-sphere bounds per scan entry (rt_scan.h GridQuant)
    bool useShadowGrid = true;  // RT_SHADOW_GRID=0 keeps every shadow ray on the scan
    DevBuf<float> radius;
    DevBuf<rt_material> mats;
    DevBuf<uint4> mats16;     // the same table packed into 16 bytes per entry (rt_shade.h load_material16), when the scene allows it
    bool mats16Ok = false;
    rtd::TraceParams base{};  // scene part filled at upload; the part an edit reaches again by that edit
    // Pinned staging for the copies an edit or rt_temporal_forget orders on the stream: two slots used in turn, each with an event
    // recorded behind its copies.  A slot is written again only once that event has completed -- the one host wait an edit may take,
    // and it takes it only when two newer edits are still queued.  Sized at the upload (never under running kernels).
    struct Stage {
        void* host = nullptr;  // pinned
        size_t bytes = 0;
        hipEvent_t ev = nullptr;
        bool queued = false;   // copies out of `host` were ordered and ev recorded behind them
    } stage[2];
    uint32_t stageNext = 0;
    DevBuf<uint32_t> forgetBits;  // rt_temporal_forget's table form: kForgetTableWords words, reserved at rt_create

    // accumulation: the strips of seq's running accumulation
    uint32_t sampler = 0;      // RT_SAMPLER_* flags of the next / running accumulation (rt_set_sampler)
    DevBuf<float> hdr;         // [W*rows*3]
    DevBuf<float> sq;          // [W*rows*3] sums of squared samples, valid with hdr while seq.noise is on (rt_noise.h)
    DevBuf<float> noiseMap;    // [W*rows*2] output of rt_noise_map
    DevBuf<uint32_t> noiseRed; // [kNoiseMaxThresholds + 1] counts and maximum of rt_noise_summary
    DevBuf<uint8_t> ldr;       // [W*rows*3]
    DevBuf<float> samples;     // workspace [pixels*spp_pass*3]
    DevBuf<uint32_t> queue;    // [1]
    DevBuf<unsigned long long> counters;  // [2]
    DevBuf<float2> jitterTab, lensTab;    // ray-generation tables of the current pass
    double lastResolveMs = 0.0;

    // feature buffers (rt_render_features; rt_features.h): strips, ray-generation tables and sequencing of their own -- nothing
    // here is read or written by rt_render, and nothing of rt_render's by the feature pass
    bool featCleared = false;     // rt_clear_features was called: the next rt_render_features may start at any s0
    uint32_t featCount = 0;       // samples per pixel in the strips (0: nothing accumulated)
    uint32_t featNext = 0;        // the s0 that continues the accumulation (the previous call's s1)
    rtseq::PictureKey featPic;    // the picture the strips are of ...
    uint32_t featRows = 0;        // ... and its local rows
    DevBuf<float> feat;           // [W*rows*8] sums of albedo rgb, normal xyz, depth, coverage
    DevBuf<uint32_t> featIds;     // [W*rows] id of the sample added last
    DevBuf<float2> featJitter, featLens;  // ray-generation tables of the feature pass

    // denoise (rt_denoise; rt_denoise.h, rt_denoise.hip): a snapshot of the filtered picture in strips of its own
    bool denValid = false;        // den / denVar / denLdr hold the last rt_denoise's result (voided by rt_scene_upload)
    uint32_t denW = 0, denRows = 0;
    uint32_t denForms[rtd::kDenoiseMaxLevels] = {0, 0, 0, 0, 0};  // rtdn::Form of each level of the last rt_denoise
    DevBuf<float> denState[2];    // [W*rows*4] (c.rgb, v) of a level, ping and pong
    DevBuf<float> denGuide[2];    // [W*rows*4] each: (albedo rgb, normal x), (normal y, normal z, depth, coverage)
    DevBuf<float> den, denVar;    // [W*rows*3], [W*rows]
    DevBuf<uint8_t> denLdr;       // [W*rows*3] the resolve of den with n_samples = 1

    // temporal accumulation (rt_denoise_temporal; rt_temporal.h): the history, state of its own that rt_scene_upload keeps.  Two sets
    // used ping-pong -- a call reads set tmpCur and writes the other, which then becomes tmpCur -- and never updated in place.
    struct TemporalSet {
        DevBuf<float> state, guide[2];  // [W*rows*4] each
        DevBuf<uint32_t> ids, len;      // [W*rows]
    };
    bool tmpValid = false;        // set tmpCur holds a history of the picture below, taken with tmpCam
    uint32_t tmpCur = 0;
    rtseq::PictureKey tmpPic;
    rtd::TemporalCam tmpCam{};
    TemporalSet tmpSet[2];
    DevBuf<uint32_t> tmpTarget;   // [W*rows] of the last call

    // tuning (env: RT_BLOCKS_PER_CU, RT_FORCE_GLOBAL_TABLES)
    uint32_t blocksPerCu = 4;
    uint32_t blockThreads = 256;
    bool useMfma = true;  // matrix-core pre-filter for the list scan (RT_SCAN=valu disables)
    bool matsInLds = true;   // RT_MATS_LDS=0 leaves the material table in global memory (frees 48 B/sphere of LDS)
    bool useRayCache = true;
    bool useStash = true;  // regrouped hit processing through a per-wave hit stash (rt_kernels.h kStash); RT_STASH=0: off
    bool treeInLds = true;      // RT_TREE_LDS=0: the hierarchy's bounds are read through L2
    uint32_t treeTop = 128;  // largest top level the matrix-core filter takes (4 tiles of 32); RT_TREE_TOP overrides
    bool forceGlobal = false;

    // the launcher's own account (rt_unit_last_trace_launch): the packed inputs and plan of the most recent LaunchTrace, in the words of
    // rt_unit_launch_plan, and the launches since rt_create
    uint32_t lastCaseWords[rtplan::kCaseWords] = {}, lastPlanWords[rtplan::kPlanWords] = {};
    uint32_t traceLaunches = 0;
    bool lastTraceLean = false;  // ... and whether it ran its row's kernel without far-hit state (rt_unit_last_trace_far_state)

    // The per-tile tables: candidate masks and sphere lists of the primary rays (BuildTileMasks; rt_tile_mask.h), work order and
    // empty-list flags (BuildTileOrder), the flagged tiles' count.  What of them is valid, for which picture and limits, and what a
    // call may use is host/rt_tile_tables.h's to say: read and changed only through rttile's plans, reports and events.
    rttile::State tiles;
    DevBuf<uint32_t> tileMasks;    // kTileMaskWords per full tile
    DevBuf<uint16_t> tileSpheres;  // kTileSphereHalfs per full tile (built together with the masks)
    DevBuf<float> pilotRays, pilotHits;
    DevBuf<uint32_t> tileOrder, matType;
    DevBuf<uint8_t> tileClass;
    DevBuf<uint8_t> skyFlags;     // [full tiles]
    DevBuf<uint32_t> skyInfo;     // [0] flagged tiles, [1..3] the constant sample's bits
    // the count's way to the host (rt_kernels.h rt_sky_tiles_kernel): pinned memory and an event that is only ever QUERIED
    uint32_t* skyCountHost = nullptr;  // pinned
    hipEvent_t skyEv = nullptr;
    // the last render's account, for the unit entries
    struct TileAccount {
        bool lastTraceSky = false;  // the last ordinary LaunchTrace took a kernel that finishes empty-list planes itself (rt_kernels.h kSky)
        uint32_t skyExcluded = 0;   // tiles the last rt_render that launched a trace kernel kept out of its queue (rt_unit_sky_excluded)
        uint64_t freshScans = 0;    // blocks of 64 fresh paths launched by the last rt_render that ran passes (rt_unit_tile_masks)
    } tileAcct;

    // frame pipelining (rt_set_frame_pipelining; rt_params.h): regions of a sample ring, two continuation buffers (seq.pipeDepth: the
    // calls a path may be carried across)
    bool pipeOpen = false;      // pipelined calls have been submitted since the last flush
    uint32_t pipeSeq = 0;       // sequence number of the newest region
    uint32_t pipeSppCap = 0, pipeNpix = 0, pipeRing = 0;  // geometry of the ring: samples per region, pixels, regions
    uint32_t pipeInSel = 0;     // which continuation buffer the next trace kernel reads
    uint32_t pipeCommits = 0;   // commit kernels launched since the pipeline started (FrameCtl: which entry is current)
    uint32_t pipeMaxDepth = 0;  // max_depth and seed of the running pipeline (a flush re-launches with them)
    uint64_t pipeSeed = 0;
    rtd::RegionTable pipeRegions{};
    DevBuf<float> ring;
    DevBuf<rtd::ContEntry> cont[2];
    DevBuf<uint32_t> contN[2];  // carried paths per wave
    DevBuf<rtd::FrameCtl> ctl;
};

// ---- launches.  What a launch IS -- its dynamic LDS image, the TraceParams fields that describe it, its grid, and which of the
// instantiated variants runs -- is planned by host/rt_launch_plan.cpp, in plain C++ that tests reach without a device
// (rt_unit_launch_plan).  Here the plan's inputs are gathered from the context, the scene and the environment of the moment, its
// fields applied and the kernel looked up in the tables below, which expand the one list of variants (rt_trace_variants.h).
static rtplan::SceneShape ShapeOf(const rtd::TraceParams& tp) {
    rtplan::SceneShape S;
    S.n_padded = tp.n_padded;
    S.n_levels = tp.n_levels;
    S.top_cnt = tp.level_cnt[tp.n_levels - 1];
    S.top_off = tp.level_off[tp.n_levels - 1];
    S.grid = tp.grid_cell_start != nullptr;
    S.grid_nu = tp.grid_nu, S.grid_nv = tp.grid_nv;
    S.grid_quant = tp.grid_qrec != nullptr;
    S.sg_enabled = tp.sg_enabled != 0u;
    S.sg_nx = tp.sg_nx, S.sg_ny = tp.sg_ny, S.sg_nentries = tp.sg_nentries, S.sg_nglobal = tp.sg_nglobal;
    S.mats16 = tp.mats16 != nullptr;
    S.n_lights = tp.n_lights;
    return S;
}
static rtplan::Settings SettingsOf(const rt_ctx* ctx) {
    rtplan::Settings C;
    C.cuCount = (uint32_t)ctx->cuCount, C.blocksPerCu = ctx->blocksPerCu, C.blockThreads = ctx->blockThreads;
    C.useMfma = ctx->useMfma, C.matsInLds = ctx->matsInLds, C.useRayCache = ctx->useRayCache, C.useStash = ctx->useStash;
    C.treeInLds = ctx->treeInLds, C.forceGlobal = ctx->forceGlobal;
    return C;
}
static rtplan::Knobs KnobsFromEnv() {  // read at every launch: tests change them between calls
    rtplan::Knobs K;
    K.mats16 = EnvU32("RT_MATS16", K.mats16), K.matsL2 = EnvU32("RT_MATS_L2", K.matsL2);
    K.stashCap = EnvU32("RT_STASH_CAP", K.stashCap), K.stashProcess = EnvU32("RT_STASH_PROCESS", K.stashProcess);
    K.gridQuant = EnvU32("RT_GRID_QUANT", K.gridQuant), K.gridSgLds = EnvU32("RT_GRID_SG_LDS", K.gridSgLds);
    K.queueBlock = EnvU32("RT_QUEUE_BLOCK", K.queueBlock), K.queueStatic = EnvU32("RT_QUEUE_STATIC", K.queueStatic);
    return K;
}
static void SetQueue(rtd::TraceParams& tp, const rtplan::QueueCut& q) {
    tp.queue_block = q.queue_block, tp.static_blocks = q.static_blocks, tp.dyn_begin = q.dyn_begin, tp.dyn_blocks = q.dyn_blocks;
}

// ---- how the host's records become launch parameters, each written down once.  P is rtd::TraceParams (light 0, the unit kernels) or
// rtd::LightRec (lights 1 ..): the member names are equal (rt_params.h).
// A shadow index's constants; a disabled index sets them zero, whatever the builder left in it and whatever p held (rt_turn_lights
// switches indices off and on in place).  Where its three tables lie differs by caller and stays there.
template <typename P>
static void SetShadowGrid(P& p, const rtprep::ShadowGrid& built) {
    const rtprep::ShadowGrid none;
    const rtprep::ShadowGrid& G = built.enabled ? built : none;
    p.sg_enabled = G.enabled ? 1u : 0u;
    for (int c = 0; c < 3; ++c) {
        p.sg_e1[c] = G.e1[c];
        p.sg_e2[c] = G.e2[c];
    }
    p.sg_u0 = G.u0, p.sg_v0 = G.v0, p.sg_inv_cell = G.invCell, p.sg_p0sq = G.p0sq;
    p.sg_nx = G.nx, p.sg_ny = G.ny, p.sg_nglobal = (uint32_t)G.global.size();
}
template <typename P>
static void SetLight(P& p, const rt_light& light) {
    for (int c = 0; c < 3; ++c) {
        p.sun_dir[c] = light.direction[c];
        p.sun_rad[c] = light.luminance * light.color[c];  // m_luminance * m_color, light.cpp:27
    }
}
// ---- what the lights and their shadow indices become, written once for rt_scene_upload and rt_turn_lights.  The indices' tables lie
// in buffers the upload reserved at the builder's bounds (ReserveShadowGrid), so their addresses are known before anything is copied.
// The records behind base.extra_lights: lights 1 .. with their index each, then the far-tier record -- an empty light that carries
// light 0's second index -- while that index exists.
template <typename Prepared>  // rtprep::PreparedScene (the upload) or rtprep::PreparedShadows (a turn): the members have the same names
static std::vector<rtd::LightRec> LightRecords(const rt_ctx* ctx, const Prepared& S, const rt_light* lights, uint32_t n_lights,
                                               const float camO[3]) {
    auto indexed = [](const rtprep::ShadowGrid& G, const rt_ctx::ExtraLight& X) {
        rtd::LightRec R{};
        SetShadowGrid(R, G);
        if (G.enabled) R.cell_start = X.cells.ptr, R.entries = X.entries.ptr, R.global = X.global.ptr;
        return R;
    };
    std::vector<rtd::LightRec> recs;
    for (uint32_t k = 1; k < n_lights; ++k) {
        rtd::LightRec R = indexed(S.extraShadow[k - 1], ctx->extraIdx[k]);
        SetLight(R, lights[k]);
        for (int c = 0; c < 3; ++c) R.cam_o[c] = camO[c];
        recs.push_back(R);
    }
    if (S.shadowFar.enabled) recs.push_back(indexed(S.shadowFar, ctx->farIdx));  // (enabled only with light 0's first index: n_lights >= 1)
    return recs;
}
// Light 0 and everything the by-value launch parameters say of the lights: the launch plan reads the index's sizes from here and picks
// the variant and the LDS image.  nRecs: LightRecords' count.
template <typename Prepared>
static void SetSunAndIndices(rt_ctx* ctx, const Prepared& S, const rt_light& sun, size_t nRecs) {
    rtd::TraceParams& b = ctx->base;
    const rtprep::ShadowGrid& SG = S.shadow;
    SetLight(b, sun);
    SetShadowGrid(b, SG);
    b.extra_lights = nRecs ? ctx->lightRecs.ptr : nullptr;
    b.far_index = S.shadowFar.enabled ? 1u : 0u;
    b.sg_cell_start = SG.enabled ? ctx->sgCells.ptr : nullptr;
    b.sg_entries = SG.enabled ? ctx->sgEntries.ptr : nullptr;
    b.sg_global = SG.enabled ? ctx->sgGlobal.ptr : nullptr;
    b.sg_sph = SG.enabled && !S.sgSph.empty() ? ctx->sgSph.ptr : nullptr;
    b.sg_nentries = SG.enabled ? (uint32_t)SG.entries.size() : 0u;  // (for the list's copy into LDS; a LightRec's index stays in global memory)
}
static void SetCamera(rtd::TraceParams& tp, const rt_camera& camera) {
    for (int c = 0; c < 3; ++c) {
        tp.cam_o[c] = camera.origin[c];
        tp.cam_x[c] = camera.x[c];
        tp.cam_y[c] = camera.y[c];
        tp.cam_oip[c] = camera.origin_image_plane[c];
    }
    tp.aperture = camera.aperture;
    tp.focal = camera.focal_length;
}
static void SetSky(rtd::TraceParams& tp, const rt_material& sky) {
    for (int k = 0; k < 3; ++k) tp.sky_emit[k] = sky.luminance * sky.rgb0[k];  // Emissive::Emit, material.cpp:172-175
}
static void SetExposure(rtd::TraceParams& tp, const rtscene::Record& scene) { tp.exposure = scene.exposure; }  // the launch parameter's one writer
static void SetPicture(rtd::TraceParams& tp, const rtseq::PictureKey& pic) { tp.W = pic.W, tp.H = pic.H, tp.rs = pic.rs; }
// The parameters of one pass of the trace kernel: the scene (ctx->base, whose work part is zero: no path list, no tile tables, no
// ray-generation tables, nothing of the pipeline) and the samples [s0, s0 + spp) of the npix local pixels of the picture.  The caller
// adds what is its own.
static rtd::TraceParams PassParams(const rt_ctx* ctx, const rtseq::PictureKey& pic, uint32_t s0, uint32_t spp, uint32_t npix, uint32_t max_depth,
                                   uint64_t seed) {
    rtd::TraceParams tp = ctx->base;
    SetPicture(tp, pic);
    tp.s0 = s0;
    tp.spp_pass = spp;
    tp.total_paths = npix * spp;
    tp.npix_local = npix;
    tp.max_depth = max_depth;
    tp.sampler = ctx->sampler;
    tp.seed = seed;
    tp.counters = ctx->counters.ptr;
    return tp;
}

// The time on the stream since hipEventRecord(ctx->ev[first]), in ms: records ev[first + 1] and waits for it.
static int ElapsedSince(rt_ctx* ctx, int first, double* out_ms) {
    RT_HIP(hipEventRecord(ctx->ev[first + 1], ctx->stream));
    RT_HIP(hipEventSynchronize(ctx->ev[first + 1]));
    float ms = 0.f;
    RT_HIP(hipEventElapsedTime(&ms, ctx->ev[first], ctx->ev[first + 1]));
    *out_ms = ms;
    return RT_OK;
}

// What a reader hands out: strips of the context, each to the caller's buffer where one is given.  The host form waits for the stream
// and copies; the device form enqueues on it.
struct StripCopy {
    void* dst;
    const void* src;
    size_t bytes;
};
static int CopyStrips(rt_ctx* ctx, bool toDevice, std::initializer_list<StripCopy> strips) {
    if (!toDevice) RT_HIP(hipStreamSynchronize(ctx->stream));
    for (const StripCopy& s : strips) {
        if (!s.dst) continue;
        if (toDevice) RT_HIP(hipMemcpyAsync(s.dst, s.src, s.bytes, hipMemcpyDeviceToDevice, ctx->stream));
        else RT_HIP(hipMemcpy(s.dst, s.src, s.bytes, hipMemcpyDeviceToHost));
    }
    return RT_OK;
}

using TraceKernelFn = void (*)(rtd::TraceParams);
using ClosestKernelFn = void (*)(rtd::TraceParams, const float*, uint32_t, float*);
using FeaturesKernelFn = void (*)(rtd::TraceParams, rtd::FeatureParams);
static const struct {
    TraceKernelFn one, lights;  // the single-light kernel and its twin over the light list (rt_kernels.h trace_body)
} kTraceKernels[] = {
#define RT_ROW(...) {&rtd::rt_trace_kernel<__VA_ARGS__>, &rtd::rt_trace_kernel_lights<__VA_ARGS__>},
    RT_TRACE_VARIANTS(RT_ROW)
#undef RT_ROW
};
#define RT_ROW(LDS, M) &rtd::k_unit_closest<LDS, M>,
static const ClosestKernelFn kClosestKernels[] = {RT_SCAN_VARIANTS(RT_ROW)};
#undef RT_ROW
#define RT_ROW(LDS, M) &rtd::rt_features_kernel<LDS, M>,
static const FeaturesKernelFn kFeaturesKernels[] = {RT_SCAN_VARIANTS(RT_ROW)};
#undef RT_ROW
static_assert(sizeof(kTraceKernels) / sizeof(kTraceKernels[0]) == rtplan::kTraceVariantCount, "one row per variant of the list");
// ... and the rows that exist without far-hit state as well (rt_trace_variants.h RT_TRACE_LEAN_VARIANTS), instantiated behind them
static const struct {
    TraceKernelFn one, lights;
} kTraceLeanKernels[] = {
#define RT_ROW(...) {&rtd::rt_trace_kernel_lean<__VA_ARGS__>, &rtd::rt_trace_kernel_lights_lean<__VA_ARGS__>},
    RT_TRACE_LEAN_VARIANTS(RT_ROW)
#undef RT_ROW
};
static_assert(sizeof(kTraceLeanKernels) / sizeof(kTraceLeanKernels[0]) == rtplan::kTraceLeanVariantCount, "one row per variant of the lean list");

// hipFuncAttributeMaxDynamicSharedMemorySize is a property of (device, function), process-wide: every kernel variant is raised
// ONCE per device to the 160 KiB a workgroup can have, so that two contexts with different scenes can never disagree about it
// (a per-context cache of "the last value I set" could skip the call after another context had lowered the limit), and a
// launch-bound 1-spp frame pays the attribute call only the first time.  Never lowered, never set to one launch's size.
static int RaiseLdsLimit(int device, const void* fn, size_t ldsBytes) {
    if (ldsBytes <= 48 * 1024) return RT_OK;  // what every function may have without asking
    static std::mutex mu;
    static std::set<std::pair<int, const void*>> raised;
    std::lock_guard<std::mutex> lock(mu);
    if (raised.count({device, fn})) return RT_OK;
    RT_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)rtplan::kLdsPerCu));
    raised.insert({device, fn});
    return RT_OK;
}

// Launch the megakernel over the total_paths paths described by tp.  Mode::Carry: the variant that implements frame pipelining
// (tp.ctl etc. and the queue fields filled by the caller; the queue cursor lives in tp.ctl and is reset by the preparation kernel).
static int LaunchTrace(rt_ctx* ctx, rtd::TraceParams& tp, rtplan::Mode mode = rtplan::Mode::Ordinary) {
    const rtplan::SceneShape shape = ShapeOf(tp);
    const rtplan::Settings settings = SettingsOf(ctx);
    const rtplan::Knobs knobs = KnobsFromEnv();
    const rtplan::Ask ask{tp.total_paths, tp.max_depth, mode};
    const rtplan::TracePlan P = rtplan::PlanTrace(shape, settings, knobs, ask);
    if (P.status != RT_OK) return Fail(P.status, P.message);
    tp.shard_heads = ctx->queue.ptr;
    tp.fd_tile = rtd::make_fastdiv(tp.spp_pass ? 64u * tp.spp_pass : 1u);  // path_coordinates' divisors (rt_params.h, FastDiv)
    tp.fd_w = rtd::make_fastdiv(tp.W ? tp.W : 1u);
    tp.fd_rows = rtd::make_fastdiv(tp.rs.block_rows ? tp.rs.block_rows : 1u);
    tp.mats_in_lds = P.mats_in_lds, tp.mats16_mode = P.mats16_mode;
    tp.sg_glob16 = P.sg_glob16, tp.sg_in_lds = P.sg_in_lds, tp.tree_in_lds = P.tree_in_lds, tp.grid_in_lds = P.grid_in_lds;
    tp.ray_cache_off16 = P.ray_cache_off16, tp.ray_cache_stride16 = P.ray_cache_stride16;
    tp.stash_cap = P.stash_cap, tp.stash_process = P.stash_process;
    ctx->tileAcct.lastTraceSky = P.lastTraceSky;
    if (std::getenv("RT_VERBOSE"))
        std::fprintf(stderr, "rt_trace launch: tree=%d flat=%d ldsTables=%d blocks=%u threads=%u lds=%zu B (cand %zu, tables %zu, leaf %zu, ops %zu, sg %zu, tree %zu, cache %s, stash %u)\n",
                     (int)P.tree, (int)P.flat + 2 * (int)P.grid + 4 * (int)P.gridLds, (int)P.ldsTables, P.blocks, ctx->blockThreads, P.ldsBytes, P.candBytes, P.tablesBytes, P.leafBytes,
                     P.opsBytes, P.sgBytes, P.treeBytes, P.cacheOn ? "yes" : "no", P.stash_cap);
    if (mode == rtplan::Mode::Ordinary) {
        // queue cursors for this launch (the pipelined path sets them in its preparation kernel)
        SetQueue(tp, P.queue);
        hipLaunchKernelGGL(rtd::rt_raygen_tables_kernel, dim3(1), dim3(64), 0, ctx->stream, (float2*)nullptr, 0u, 0u, (float2*)nullptr, 0u, 0u, 0u,
                           ctx->queue.ptr, (rtd::FrameCtl*)nullptr);
        RT_HIP(hipGetLastError());
    }
    const int row = rtplan::FindTraceVariant(P.kernel);
    if (row < 0) return Fail(RT_ERR_HIP, "internal: the launch plan chose a trace kernel variant that is not instantiated");
    // far-hit state or not (host/rt_launch_plan.h FarStateLean; RT_FAR_STATE is read at every launch, like the other knobs)
    rtplan::FarStateAsk far;
    far.pathList = tp.path_list != nullptr, far.travOut = tp.trav_out != nullptr;
    far.shadowGrid = ctx->useShadowGrid, far.forceFull = EnvU32("RT_FAR_STATE", 0) != 0u;
    const bool lean = rtplan::FarStateLean(shape, ask, P, far);
    // The lean kernels hold no radical-inverse fallback: they read the ray-generation tables, which every launch that can be lean
    // has (rt_render fills them; the one launch without them, rt_unit_trace, has a path list and keeps the far-hit state).  A
    // launch that broke that would read through a null pointer: refused here, never answered by another kernel.
    if (lean && (tp.jitter_tab == nullptr || tp.lens_tab == nullptr))
        return Fail(RT_ERR_HIP, "internal: a trace launch without far-hit state needs the ray-generation tables");
    const int leanRow = lean ? rtplan::FindLeanVariant(P.kernel) : -1;
    const TraceKernelFn fn = lean ? (P.kernel.lights ? kTraceLeanKernels[leanRow].lights : kTraceLeanKernels[leanRow].one)
                                  : (P.kernel.lights ? kTraceKernels[row].lights : kTraceKernels[row].one);
    if (const int rc = RaiseLdsLimit(ctx->device, reinterpret_cast<const void*>(fn), P.ldsBytes)) return rc;
    hipLaunchKernelGGL(fn, dim3(P.blocks), dim3(ctx->blockThreads), P.ldsBytes, ctx->stream, tp);
    RT_HIP(hipGetLastError());
    // what was planned and applied, in rt_unit_launch_plan's words (the plan's own packing: nothing is restated here)
    rtplan::PackCase(shape, settings, knobs, ask, ctx->lastCaseWords);
    rtplan::PackPlan(P, rtplan::PlanScanOnly(shape, settings), ctx->lastPlanWords);
    ctx->lastTraceLean = lean;
    ++ctx->traceLaunches;
    return RT_OK;
}

// The unit kernels' launch (rtplan::PlanScanOnly): the scan variant rt_render would launch for this scene, 64 rays per wave, LDS
// image for four waves, hit-processing tables left out.  Returns the row of the kernel in kClosestKernels / kFeaturesKernels.
static int PlanScanOnlyLaunch(const rt_ctx* ctx, rtd::TraceParams& tp, rtplan::ScanOnlyPlan& P) {
    P = rtplan::PlanScanOnly(ShapeOf(tp), SettingsOf(ctx));
    tp.mats_in_lds = 0;
    tp.sg_in_lds = 0;
    if (P.kernel.kScan == 3) tp.grid_in_lds = 0;
    if (P.kernel.kScan == 2) tp.tree_in_lds = P.tree_in_lds;
    return rtplan::FindScanVariant(P.kernel);
}

// rt_unit_closest_hit's device part.  Also traces the pilot rays of the tile order.
static int LaunchClosest(rt_ctx* ctx, const float* dRays, uint32_t n, float* dOut) {
    rtd::TraceParams tp = ctx->base;
    rtplan::ScanOnlyPlan P;
    const int row = PlanScanOnlyLaunch(ctx, tp, P);
    if (row < 0) return Fail(RT_ERR_HIP, "internal: the launch plan chose a scan that is not instantiated");
    const ClosestKernelFn fn = kClosestKernels[row];
    if (const int rc = RaiseLdsLimit(ctx->device, reinterpret_cast<const void*>(fn), P.ldsBytes)) return rc;
    hipLaunchKernelGGL(fn, dim3((n + 255) / 256), dim3(256), P.ldsBytes, ctx->stream, tp, dRays, n, dOut);
    RT_HIP(hipGetLastError());
    return RT_OK;
}

// The feature pass (rt_kernels.h rt_features_kernel) over the strip's npix local pixels: the scan variant and the LDS image of
// LaunchClosest, persistent workgroups -- as many as are resident at once.
static int LaunchFeatures(rt_ctx* ctx, rtd::TraceParams& tp, const rtd::FeatureParams& fp) {
    rtplan::ScanOnlyPlan P;
    const int row = PlanScanOnlyLaunch(ctx, tp, P);
    if (row < 0) return Fail(RT_ERR_HIP, "internal: the launch plan chose a scan that is not instantiated");
    tp.fd_w = rtd::make_fastdiv(tp.W ? tp.W : 1u);
    tp.fd_rows = rtd::make_fastdiv(tp.rs.block_rows ? tp.rs.block_rows : 1u);
    const size_t ldsBytes = P.ldsBytes, waves = 256 / 64;
    if (ldsBytes > rtplan::kLdsPerCu) return Fail(RT_ERR_HIP, "internal: the feature pass's LDS image exceeds a workgroup's 160 KiB");
    const uint32_t nTiles = (fp.npix + 63u) / 64u;
    size_t perCu = rtplan::kLdsPerCu / (ldsBytes ? ldsBytes : 1);  // workgroups of this image a CU holds, at most 8 (32 waves)
    perCu = perCu > 8 ? 8 : (perCu < 1 ? 1 : perCu);
    uint32_t blocks = (uint32_t)((nTiles + waves - 1) / waves);
    const uint32_t maxBlocks = (uint32_t)ctx->cuCount * (uint32_t)perCu;
    if (blocks > maxBlocks) blocks = maxBlocks;
    if (blocks == 0) blocks = 1;
    const FeaturesKernelFn fn = kFeaturesKernels[row];
    if (const int rc = RaiseLdsLimit(ctx->device, reinterpret_cast<const void*>(fn), ldsBytes)) return rc;
    hipLaunchKernelGGL(fn, dim3(blocks), dim3(256), ldsBytes, ctx->stream, tp, fp);
    RT_HIP(hipGetLastError());
    return RT_OK;
}

// Candidate masks of the full tiles' primary rays for the accumulation that is starting (rt_tile_mask.h): one small kernel on
// the stream, no host wait.  Like the tile order they are a function of the scene (camera included), the image size and the strip,
// and are kept across accumulations of the same picture.  Only the flat matrix-core scan of the hit-stash kernels reads them.
// RT_PRIMARY_MASK=0 (both knobs are read when an accumulation starts): no masks, every scan runs the filter.  RT_PRIMARY_MASK_LIMIT: tiles with more candidate groups
// than this keep the filter.  RT_PRIMARY_SPHERES: tiles with a mask and at most this many reachable spheres also get a sphere list and
// resolve their primary rays directly (rt_scan.h scan_tile_spheres); 0 = no lists, values above kTileSphereMax are clamped.
// RT_SKY_SKIP=0 (read by rt_render where an accumulation starts): tiles whose list is empty generate and scan their rays like every
// other listed tile (rt_kernels.h kSky).  RT_SKY_EXCLUDE=0 (read there too): those tiles are not flagged -- every launch queues every tile
// and the accumulation reads every plane from the sample buffer (BuildTileOrder).
static uint32_t TileSphereLimitFromEnv() {
    const uint32_t v = EnvU32("RT_PRIMARY_SPHERES", rtd::kTileSphereLimitDefault);
    return v > rtd::kTileSphereMax ? rtd::kTileSphereMax : v;
}
static rttile::Knobs TileKnobsFromEnv() {
    rttile::Knobs K;
    K.primaryMask = EnvU32("RT_PRIMARY_MASK", 1u) != 0u;
    K.primaryMaskLimit = EnvU32("RT_PRIMARY_MASK_LIMIT", rtd::kTileMaskLimitDefault);
    K.primarySpheres = TileSphereLimitFromEnv();
    K.skipSky = EnvU32("RT_SKY_SKIP", 1u) != 0u;
    K.excludeSky = EnvU32("RT_SKY_EXCLUDE", 1u) != 0u;
    return K;
}
static int BuildTileMasks(rt_ctx* ctx, const rtseq::PictureKey& pic, uint32_t npix, const rttile::Knobs& knobs) {
    const rtd::TraceParams& b = ctx->base;
    const bool sceneTakesMasks = b.n_levels == 1u && b.level_cnt[0] <= 128u && rtplan::ChooseScan(ShapeOf(b), SettingsOf(ctx), 0u).flat;
    const rttile::MaskPlan plan = rttile::PlanMasks(ctx->tiles, pic, npix, knobs, sceneTakesMasks);
    if (plan.answer != rttile::MaskAnswer::Build) return RT_OK;
    const uint32_t nFull = plan.nFull, sphLimit = plan.sphLimit;
    int rc;
    if ((rc = ctx->tileMasks.Reserve((size_t)nFull * rtd::kTileMaskWords)) != RT_OK) return rc;
    if (sphLimit != 0u && (rc = ctx->tileSpheres.Reserve((size_t)nFull * rtd::kTileSphereHalfs)) != RT_OK) return rc;
    rtd::TraceParams tp = b;
    SetPicture(tp, pic);
    hipLaunchKernelGGL(rtd::rt_tile_mask_kernel, dim3((nFull + 3) / 4), dim3(256), 0, ctx->stream, tp, nFull, plan.limit, ctx->tileMasks.ptr,
                       sphLimit, sphLimit != 0u ? ctx->tileSpheres.ptr : nullptr);
    RT_HIP(hipGetLastError());
    rttile::MasksBuilt(ctx->tiles, pic, plan);
    return RT_OK;
}

// Work order of the full tiles for the accumulation that is starting (rt_kernels.h, rt_tile_order_kernel): three pilot rays per
// tile through the production scan, then a stable sort by the most expensive first-hit material.  All on the stream, no host wait.
// Runs AFTER BuildTileMasks: where the tiles have sphere lists (and RT_SKY_SKIP and RT_SKY_EXCLUDE are on) the tiles with an empty
// list are flagged first (rt_sky_tiles_kernel) and sorted behind all others, and their number is copied to pinned host memory
// behind an event, for the later calls that find it complete (SkyCountPoll) to leave them out of the queue.
// What is flagged, ordered and copied, and under which key it is kept, is rttile::PlanOrder's answer; a rebuild that fails half way
// leaves everything dropped (OrderBuilt is reported last).
static void DropTileOrder(rt_ctx* ctx) {
    rttile::Dropped(ctx->tiles);
    (void)rtseq::TileTablesDropped(ctx->seq);  // (planes traced ahead go with the flags: nothing beyond the sequencer's own state)
}
static void SkyCountPoll(rt_ctx* ctx) {
    if (!rttile::CountToAwait(ctx->tiles)) return;
    const hipError_t e = hipEventQuery(ctx->skyEv);
    if (e == hipSuccess) {
        rttile::CountArrived(ctx->tiles, *ctx->skyCountHost);
    } else if (e == hipErrorNotReady) {
        (void)hipGetLastError();  // "not ready" is an answer, not an error of the calls that follow
    } else {
        rttile::CountFailed(ctx->tiles);  // a real error: the count stays unknown, and the error is left for the call that follows to report
    }
}
// The launches of a work order for nFull full tiles of a picture, into the buffers given: the one place they are written down, for
// BuildTileOrder (the context's kept buffers) and rt_unit_tile_order (buffers of the entry's own).  flags: lists (kTileSphereHalfs per
// tile) are read and dst.flags / dst.info written first; order: pilot rays, the production closest-hit scan, classes, the sort.
// Every buffer has room for nFull tiles (rays 6, hits 10 floats per pilot; info 4 words).  On the stream, no host wait.
struct TileOrderDest {
    float* pilotRays = nullptr;
    float* pilotHits = nullptr;
    uint8_t* cls = nullptr;
    uint32_t* order = nullptr;
    uint8_t* flags = nullptr;
    uint32_t* info = nullptr;
};
static int LaunchTileOrder(rt_ctx* ctx, const rtseq::PictureKey& pic, uint32_t nFull, bool flags, bool order, const uint16_t* lists,
                           const TileOrderDest& dst) {
    int rc;
    if (flags) {
        RT_HIP(hipMemsetAsync(dst.info, 0, 4 * sizeof(uint32_t), ctx->stream));
        hipLaunchKernelGGL(rtd::rt_sky_tiles_kernel, dim3((nFull + 255) / 256), dim3(256), 0, ctx->stream, ctx->base, lists, nFull, dst.flags, dst.info);
        RT_HIP(hipGetLastError());
    }
    if (order) {
        const uint32_t nPilot = nFull * rtd::kPilotsPerTile;
        rtd::TraceParams tp = ctx->base;
        SetPicture(tp, pic);
        tp.s0 = 1;
        tp.sampler = ctx->sampler;
        tp.jitter_tab = nullptr;
        tp.lens_tab = nullptr;
        hipLaunchKernelGGL(rtd::rt_pilot_rays_kernel, dim3((nPilot + 255) / 256), dim3(256), 0, ctx->stream, tp, nFull, dst.pilotRays);
        RT_HIP(hipGetLastError());
        if ((rc = LaunchClosest(ctx, dst.pilotRays, nPilot, dst.pilotHits)) != RT_OK) return rc;
        hipLaunchKernelGGL(rtd::rt_tile_class_kernel, dim3((nFull + 255) / 256), dim3(256), 0, ctx->stream, dst.pilotHits, nFull, pic.W,
                           ctx->matType.ptr, dst.cls, flags ? dst.flags : (const uint8_t*)nullptr);
        hipLaunchKernelGGL(rtd::rt_tile_order_kernel, dim3(1), dim3(1024), 0, ctx->stream, dst.cls, nFull, dst.order);
        RT_HIP(hipGetLastError());
    }
    return RT_OK;
}
static int BuildTileOrder(rt_ctx* ctx, const rtseq::PictureKey& pic, uint32_t npix) {
    const rttile::OrderPlan plan = rttile::PlanOrder(ctx->tiles, pic, npix, (uint32_t)ctx->cuCount);
    if (!plan.rebuild) return RT_OK;
    (void)rtseq::TileTablesDropped(ctx->seq);  // (the plan dropped order and flags)
    const uint32_t nFull = plan.nFull;
    int rc;
    if (plan.flags) {
        if (!ctx->skyEv) RT_HIP(hipEventCreateWithFlags(&ctx->skyEv, hipEventDisableTiming));
        if (!ctx->skyCountHost) RT_HIP(hipHostMalloc(reinterpret_cast<void**>(&ctx->skyCountHost), sizeof(uint32_t), hipHostMallocDefault));
        if ((rc = ctx->skyFlags.Reserve(nFull)) != RT_OK) return rc;
        if ((rc = ctx->skyInfo.Reserve(4)) != RT_OK) return rc;
    }
    if (plan.order) {
        const uint32_t nPilot = nFull * rtd::kPilotsPerTile;
        if ((rc = ctx->pilotRays.Reserve((size_t)nPilot * 6)) != RT_OK) return rc;
        if ((rc = ctx->pilotHits.Reserve((size_t)nPilot * 10)) != RT_OK) return rc;
        if ((rc = ctx->tileClass.Reserve(nFull)) != RT_OK) return rc;
        if ((rc = ctx->tileOrder.Reserve(nFull)) != RT_OK) return rc;
    }
    TileOrderDest dst;
    dst.pilotRays = ctx->pilotRays.ptr, dst.pilotHits = ctx->pilotHits.ptr, dst.cls = ctx->tileClass.ptr, dst.order = ctx->tileOrder.ptr;
    dst.flags = ctx->skyFlags.ptr, dst.info = ctx->skyInfo.ptr;
    if ((rc = LaunchTileOrder(ctx, pic, nFull, plan.flags, plan.order, ctx->tileSpheres.ptr, dst)) != RT_OK) return rc;
    if (plan.count) {
        RT_HIP(hipMemcpyAsync(ctx->skyCountHost, ctx->skyInfo.ptr, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        RT_HIP(hipEventRecord(ctx->skyEv, ctx->stream));
    }
    rttile::OrderBuilt(ctx->tiles, pic, plan);
    return RT_OK;
}

// The ray-generation tables of the samples [s0, s0 + spp) of a strip of W columns, in the two buffers given (rt_render's or the feature
// pass's), and tp's account of them: the host half of the indexing contract of rt_params.h -- jitter_tab[s - s0], and lens_tab[k - lens_k0]
// for k = s + i + j over the strip's rows.  queue, ctl: the pipelined form, whose table kernel also resets the queue cursors and the
// control block for the carrying trace kernel that follows.
static int LaunchRaygenTables(rt_ctx* ctx, rtd::TraceParams& tp, DevBuf<float2>& jitter, DevBuf<float2>& lens, uint32_t s0, uint32_t spp, uint32_t W,
                              const rt_rowset& rs, uint32_t* queue = nullptr, rtd::FrameCtl* ctl = nullptr) {
    const uint32_t k0 = s0 + rs.first_row;
    const uint32_t nLens = spp + W + rs.num_rows;
    const uint32_t nmax = spp > nLens ? spp : nLens;
    int rc;
    if ((rc = jitter.Reserve(spp)) != RT_OK || (rc = lens.Reserve(nLens)) != RT_OK) return rc;
    tp.jitter_tab = jitter.ptr;
    tp.lens_tab = lens.ptr;
    tp.lens_k0 = k0;
    hipLaunchKernelGGL(rtd::rt_raygen_tables_kernel, dim3((nmax + 255) / 256), dim3(256), 0, ctx->stream, jitter.ptr, s0, spp, lens.ptr, k0, nLens,
                       ctx->sampler, queue, ctl);
    RT_HIP(hipGetLastError());
    return RT_OK;
}

// ------------------------------------------------------------------------------ frame pipelining
// (rt_params.h "frame pipelining")  Host side: one region of the sample ring per rt_render call, two
// continuation buffers used alternately, and three launches per call: preparation + ray-generation tables, the carrying
// trace kernel, the commit kernel.  Nothing here waits for the device.
static void PipelineDrop(rt_ctx* ctx) { ctx->pipeOpen = false; }  // carried paths and uncommitted regions are abandoned
// What an event of the sequencer voided outside its own state (rtseq::kInFlight ...): dropped here, in one place.
static void DropVoided(rt_ctx* ctx, uint32_t voids);
static uint32_t PipelineWaves(const rt_ctx* ctx) { return (uint32_t)ctx->cuCount * ctx->blocksPerCu * (ctx->blockThreads / 64); }
static void PipelineShards(const rt_ctx* ctx, rtd::TraceParams& tp) {
    // measured (tools/progressive_frames.py, 1-spp frames): 128-path blocks x 1 static beat 64 x 2, 128 x 0, 192 x 1, 256 x 0
    uint32_t qb = EnvU32("RT_PIPE_QUEUE_BLOCK", rtd::kCarryQueueBlock) / 64u * 64u;
    if (qb == 0) qb = 64;
    SetQueue(tp, rtplan::CutQueue(tp.total_paths, PipelineWaves(ctx), qb, EnvU32("RT_PIPE_STATIC_BLOCKS", 1)));
}

static int PipelineTraceAndCommit(rt_ctx* ctx, rtd::TraceParams& tp, uint32_t npix, bool carry) {
    tp.ctl = ctx->ctl.ptr;
    tp.cont_in = ctx->cont[ctx->pipeInSel].ptr;
    tp.cont_in_n = ctx->contN[ctx->pipeInSel].ptr;
    tp.cont_out = ctx->cont[ctx->pipeInSel ^ 1u].ptr;
    tp.cont_out_n = ctx->contN[ctx->pipeInSel ^ 1u].ptr;
    tp.carry = carry ? 1u : 0u;
    tp.region_seq = ctx->pipeSeq;
    tp.max_carry_age = ctx->seq.pipeDepth;
    tp.min_iters = EnvU32("RT_PIPE_MIN_ITERS", 8);
    int rc = LaunchTrace(ctx, tp, rtplan::Mode::Carry);
    if (rc != RT_OK) return rc;
    hipLaunchKernelGGL(rtd::rt_commit_kernel, dim3((npix + 255) / 256), dim3(256), 0, ctx->stream, ctx->ring.ptr, ctx->hdr.ptr, npix,
                       npix * ctx->pipeSppCap, ctx->pipeRing, ctx->pipeRegions, ctx->ctl.ptr, ctx->pipeSeq, ctx->pipeCommits);
    RT_HIP(hipGetLastError());
    ++ctx->pipeCommits;  // the commit point is now entry pipeCommits & 1 of the control block
    ctx->pipeInSel ^= 1u;
    return RT_OK;
}

// Run every carried path to its end and commit every region: afterwards the HDR strip holds seq.accumulated samples.
static int PipelineFlush(rt_ctx* ctx) {
    if (!ctx->pipeOpen) return RT_OK;
    const uint32_t npix = ctx->pipeNpix;
    rtd::TraceParams tp = PassParams(ctx, ctx->seq.pic, 1, 1, npix, ctx->pipeMaxDepth, ctx->pipeSeed);
    tp.total_paths = 0;  // nothing fresh: only the carried paths
    tp.samples = ctx->ring.ptr;
    PipelineShards(ctx, tp);
    hipLaunchKernelGGL(rtd::rt_raygen_tables_kernel, dim3(1), dim3(256), 0, ctx->stream, (float2*)nullptr, 0u, 0u, (float2*)nullptr, 0u, 0u,
                       ctx->sampler, ctx->queue.ptr, ctx->ctl.ptr);
    RT_HIP(hipGetLastError());
    int rc = PipelineTraceAndCommit(ctx, tp, npix, false);
    ctx->pipeOpen = false;
    if (rc != RT_OK) DropVoided(ctx, rtseq::StepFailed(ctx->seq));
    return rc;
}

// One pipelined call: samples [s0, s1) of the strip become region pipeSeq + 1 of the ring.
static int PipelineRender(rt_ctx* ctx, const rtseq::PictureKey& pic, uint32_t npix, uint32_t s0, uint32_t s1, uint32_t max_depth, uint64_t seed) {
    const uint32_t spp = s1 - s0;
    const uint32_t nRing = ctx->seq.pipeDepth + 2u;
    int rc;
    if (ctx->pipeOpen && (ctx->pipeNpix != npix || spp > ctx->pipeSppCap || ctx->pipeRing != nRing || ctx->pipeMaxDepth != max_depth ||
                          ctx->pipeSeed != seed)) {
        if ((rc = PipelineFlush(ctx)) != RT_OK) return rc;  // geometry or parameters changed: start a new pipeline
    }
    if (!ctx->pipeOpen) {
        ctx->pipeNpix = npix;
        ctx->pipeSppCap = spp;
        ctx->pipeRing = nRing;
        ctx->pipeMaxDepth = max_depth;
        ctx->pipeSeed = seed;
        ctx->pipeInSel = 0;
        ctx->pipeRegions = rtd::RegionTable{};
        const size_t waves = PipelineWaves(ctx);
        if ((rc = ctx->ring.Reserve((size_t)nRing * npix * spp * 3)) != RT_OK) return rc;
        for (int k = 0; k < 2; ++k) {
            if ((rc = ctx->cont[k].Reserve(waves * 64)) != RT_OK) return rc;
            if ((rc = ctx->contN[k].Reserve(waves)) != RT_OK) return rc;
            RT_HIP(hipMemsetAsync(ctx->contN[k].ptr, 0, waves * sizeof(uint32_t), ctx->stream));  // nothing carried yet
        }
        if ((rc = ctx->ctl.Reserve(1)) != RT_OK) return rc;
        rtd::FrameCtl init{};
        init.oldest_open = 0xffffffffu;
        init.committed_seq[0] = ctx->pipeSeq;              // everything up to here is in the strip already
        init.committed_samples[0] = ctx->seq.accumulated;
        ctx->pipeCommits = 0;
        RT_HIP(hipMemcpyAsync(ctx->ctl.ptr, &init, sizeof(init), hipMemcpyHostToDevice, ctx->stream));
        RT_HIP(hipStreamSynchronize(ctx->stream));       // `init` is a stack object; once per pipeline start
        ctx->pipeOpen = true;
    }
    const uint32_t seq = ++ctx->pipeSeq;
    const uint32_t slot = seq % nRing;
    ctx->pipeRegions.seq[slot] = seq;
    ctx->pipeRegions.spp[slot] = spp;
    rtd::TraceParams tp = PassParams(ctx, pic, s0, spp, npix, max_depth, seed);
    // natural tile order: a frame's long paths are carried into the next kernel anyway, and starting every wave on the most
    // expensive tiles only lengthens the stretch before the first wave runs dry (measured 0.285 vs 0.253 ms per frame)
    tp.tile_order = nullptr;
    tp.samples = ctx->ring.ptr;
    tp.sample_base = slot * npix * ctx->pipeSppCap;
    PipelineShards(ctx, tp);
    if ((rc = LaunchRaygenTables(ctx, tp, ctx->jitterTab, ctx->lensTab, s0, spp, pic.W, pic.rs, ctx->queue.ptr, ctx->ctl.ptr)) != RT_OK) return rc;
    return PipelineTraceAndCommit(ctx, tp, npix, true);
}

extern "C" {

const char* rt_last_error(void) { return rtprep::LastError(); }
int rt_api_version(void) { return RT_API_VERSION; }

// ---- pinned staging of the edits' tables (rt_ctx::Stage).  What is laid where in a slot, and how large a slot must be, is
// host/rt_scene_edit.h's to say (StagePlan, StageBytesMax); here are the slots themselves and the one copier.
// Both slots hold at least `bytes`.  Called where the stream has run dry or nothing was ever queued (rt_create, rt_scene_upload
// behind its hipStreamSynchronize): a slot that grows is not being read.
static int StageReserve(rt_ctx* ctx, size_t bytes) {
    for (auto& st : ctx->stage) {
        if (!st.ev) RT_HIP(hipEventCreateWithFlags(&st.ev, hipEventDisableTiming));
        if (st.bytes >= bytes) continue;
        if (st.queued) RT_HIP(hipEventSynchronize(st.ev));
        st.queued = false;
        if (st.host) RT_HIP(hipHostFree(st.host));
        st.host = nullptr, st.bytes = 0;
        RT_HIP(hipHostMalloc(&st.host, bytes, hipHostMallocDefault));
        st.bytes = bytes;
    }
    return RT_OK;
}
// The slot whose turn it is, free to be written: waits -- the host, for the slot's event -- only while copies out of it are still
// queued, i.e. while two newer edits have not run yet.
static int StageAcquire(rt_ctx* ctx, size_t bytes, rt_ctx::Stage** out) {
    rt_ctx::Stage& st = ctx->stage[ctx->stageNext & 1u];
    if (st.bytes < bytes) return Fail(RT_ERR_HIP, "shading edit: the staging is smaller than the tables (no upload sized it)");
    if (st.queued) RT_HIP(hipEventSynchronize(st.ev));
    st.queued = false;
    *out = &st;
    return RT_OK;
}
// ... and once its copies are ordered on the stream
static int StageQueued(rt_ctx* ctx, rt_ctx::Stage* st) {
    RT_HIP(hipEventRecord(st->ev, ctx->stream));
    st->queued = true;
    ctx->stageNext ^= 1u;
    return RT_OK;
}
// The tables of a plan, through the slot whose turn it is: each laid at its offset and its copy ordered on the stream -- behind every
// launch that reads the old table -- then the slot's event behind them all.  No allocation, and no host wait but StageAcquire's.
static int StageCopy(rt_ctx* ctx, const rtscene::StagePlan& plan) {
    if (plan.status != RT_OK) return Fail(plan.status, plan.message);
    if (plan.total == 0) return RT_OK;
    rt_ctx::Stage* st = nullptr;
    int rc;
    if ((rc = StageAcquire(ctx, plan.total, &st)) != RT_OK) return rc;
    for (const rtscene::StageItem& it : plan.items) {
        if (it.bytes == 0) continue;
        char* h = static_cast<char*>(st->host) + it.offset;
        std::memcpy(h, it.src, it.bytes);
        if (it.dst.ptr) RT_HIP(hipMemcpyAsync(it.dst.ptr, h, it.bytes, hipMemcpyHostToDevice, ctx->stream));
    }
    return StageQueued(ctx, st);
}

int rt_create(int device_ordinal, rt_ctx** out) {
    if (!out) return Fail(RT_ERR_INVALID_ARG, "rt_create: null out");
    *out = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        return Fail(RT_ERR_NO_DEVICE, std::string("rt_create: no HIP device (") + hipGetErrorString(e) +
                                          "); this library has no CPU fallback");
    if (device_ordinal < 0 || device_ordinal >= count) return Fail(RT_ERR_NO_DEVICE, "rt_create: device ordinal out of range");
    RT_HIP(hipSetDevice(device_ordinal));
    // owned until the end: every early return below releases what has been created so far (rt_destroy copes with
    // half-initialised contexts)
    std::unique_ptr<rt_ctx, void (*)(rt_ctx*)> guard(new rt_ctx(), rt_destroy);
    rt_ctx* ctx = guard.get();
    ctx->device = device_ordinal;
    hipDeviceProp_t prop;
    RT_HIP(hipGetDeviceProperties(&prop, device_ordinal));
    ctx->cuCount = prop.multiProcessorCount;
    ctx->ldsPerBlockMax = prop.sharedMemPerBlock;
    RT_HIP(hipStreamCreateWithFlags(&ctx->ownStream, hipStreamNonBlocking));
    ctx->stream = ctx->ownStream;
    for (auto& ev : ctx->ev) RT_HIP(hipEventCreate(&ev));
    {
        const char* scan = std::getenv("RT_SCAN");
        ctx->useMfma = !(scan && std::strcmp(scan, "valu") == 0);
        ctx->matsInLds = EnvU32("RT_MATS_LDS", 1) != 0;
        ctx->useRayCache = EnvU32("RT_RAY_CACHE", 1) != 0;
        ctx->useStash = EnvU32("RT_STASH", 1) != 0;
        ctx->treeInLds = EnvU32("RT_TREE_LDS", 1) != 0;
        ctx->tiles.orderWanted = EnvU32("RT_TILE_ORDER", 1) != 0;
        // what PrepareScene takes from the context, fixed here (its other settings are read at each upload): one reader for
        // rt_create and for the GPU-less layout queries, so that they describe the layout an upload would build
        const rtprep::PrepOptions opt = rtprep::PrepOptions::FromEnv();
        ctx->useShadowGrid = opt.shadowGrid;
        ctx->treeTop = opt.treeTop;
    }
    // launch geometry (sweeps: profiles/r01_sweep_*.jsonl): the matrix-core scan wants 16 waves per CU in ONE
    // 1024-thread workgroup (one LDS image, 128 VGPRs); the pure-VALU scan runs 4 x 256 threads
    ctx->blocksPerCu = EnvU32("RT_BLOCKS_PER_CU", ctx->useMfma ? 1 : 4);
    if (ctx->blocksPerCu == 0) ctx->blocksPerCu = 1;
    ctx->forceGlobal = EnvU32("RT_FORCE_GLOBAL_TABLES", 0) != 0;
    ctx->blockThreads = EnvU32("RT_BLOCK_THREADS", ctx->useMfma ? 1024 : 256);
    if (ctx->blockThreads != 256 && ctx->blockThreads != 512 && ctx->blockThreads != 1024) ctx->blockThreads = 256;
    int rc = ctx->queue.Reserve(rtd::kQueueShards * rtd::kShardStrideWords);  // eight queue cursors, 128 bytes apart
    if (rc == RT_OK) rc = ctx->counters.Reserve(6);
    if (rc == RT_OK) rc = ctx->forgetBits.Reserve(rtscene::kForgetTableWords);
    if (rc == RT_OK) rc = StageReserve(ctx, rtscene::StageBytesMax(rtscene::StageShape{}, rtprep::PrepOptions{}));  // no scene yet: the forget table
    if (rc != RT_OK) return rc;
    {
        // sample-buffer workspace: sized for this GPU's HBM (288 GB on MI355X), so that BASELINE configs 3 (on one GPU:
        // 11.8 GB) and 5 (12.9 GB) run as ONE pass; RT_WORKSPACE_GIB or rt_set_workspace_limit override
        size_t freeB = 0, totalB = 0;
        RT_HIP(hipMemGetInfo(&freeB, &totalB));
        uint64_t lim = 64ull << 30;
        if (lim > freeB / 2) lim = freeB / 2;
        const uint32_t envGiB = EnvU32("RT_WORKSPACE_GIB", 0);
        if (envGiB) lim = (uint64_t)envGiB << 30;
        if (lim < (1ull << 20)) lim = 1ull << 20;
        ctx->workspaceLimit = lim;
    }
    *out = guard.release();
    return RT_OK;
}

void rt_destroy(rt_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    if (ctx->skyCountHost) (void)hipHostFree(ctx->skyCountHost);
    if (ctx->skyEv) (void)hipEventDestroy(ctx->skyEv);
    for (auto& st : ctx->stage) {
        if (st.host) (void)hipHostFree(st.host);
        if (st.ev) (void)hipEventDestroy(st.ev);
    }
    if (ctx->streamEv) (void)hipEventDestroy(ctx->streamEv);
    for (auto& ev : ctx->ev)
        if (ev) (void)hipEventDestroy(ev);
    for (auto& ev : ctx->passEv)
        if (ev) (void)hipEventDestroy(ev);
    if (ctx->ownStream) (void)hipStreamDestroy(ctx->ownStream);
    // The buffers free themselves inside `delete ctx` (DevBuf), after the stream is gone: nothing on it can still use them, since it
    // was synchronised above, and the device they belong to is still the current one.
    delete ctx;
}

static int BatchFlush(rt_ctx* ctx);  // frame batching (rt_set_frame_batch), next to rt_render

// Before an event that asks for it (rtseq::kSettle...): render the pending batch (kPending), then finish the frames in flight (kInFlight).
static int Settle(rt_ctx* ctx, uint32_t what) {
    int rc = (what & rtseq::kPending) ? BatchFlush(ctx) : RT_OK;
    if (rc == RT_OK && (what & rtseq::kInFlight)) rc = PipelineFlush(ctx);
    return rc;
}
static void DropVoided(rt_ctx* ctx, uint32_t voids) {
    if (voids & rtseq::kInFlight) PipelineDrop(ctx);
    if (voids & rtseq::kTileOrder) DropTileOrder(ctx);
    if (voids & rtseq::kFeatures) ctx->featCount = 0;
    if (voids & rtseq::kDenoised) ctx->denValid = false;
}

int rt_set_stream(rt_ctx* ctx, void* hip_stream) {
    if (!ctx) return Fail(RT_ERR_INVALID_ARG, "rt_set_stream: null ctx");
    RT_HIP(hipSetDevice(ctx->device));
    const int rcs = Settle(ctx, rtseq::kSettleBeforeStream);  // on the old stream
    if (rcs != RT_OK) return rcs;
    const uint32_t voids = rtseq::StreamReplaced(ctx->seq);
    // (the copy of the flags' count must not land in the pinned word after a newer one's: the one place that waits for it, and only
    // when a picture's tables were built and never rendered from again)
    if (rttile::CountToAwait(ctx->tiles)) RT_HIP(hipEventSynchronize(ctx->skyEv));
    DropVoided(ctx, voids);
    const hipStream_t next = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : ctx->ownStream;
    if (next != ctx->stream) {
        // Everything the context has enqueued so far -- the settle above included -- runs before anything it enqueues from here on:
        // an accumulation, the feature strips and the history continue across the switch.  The device waits, the host does not.
        if (!ctx->streamEv) RT_HIP(hipEventCreateWithFlags(&ctx->streamEv, hipEventDisableTiming));
        RT_HIP(hipEventRecord(ctx->streamEv, ctx->stream));
        RT_HIP(hipStreamWaitEvent(next, ctx->streamEv, 0));
    }
    ctx->stream = next;
    return RT_OK;
}

int rt_set_workspace_limit(rt_ctx* ctx, uint64_t bytes) {
    if (!ctx || bytes < (1u << 20)) return Fail(RT_ERR_INVALID_ARG, "rt_set_workspace_limit: need >= 1 MiB");
    ctx->workspaceLimit = bytes;
    return RT_OK;
}

int rt_scene_upload(rt_ctx* ctx, const rt_sphere* spheres, const rt_material* materials, uint32_t n, const rt_camera* camera,
                    const rt_light* lights, uint32_t n_lights, const rt_material* sky, float exposure_scale) {
    // (refused before any side effect: pending frames stay pending, the previous scene stays)
    const rtscene::Decision d = rtscene::DecideUpload(ctx ? &ctx->scene : nullptr, spheres, materials, n, camera, lights, n_lights, sky);
    if (d.verdict == rtscene::Verdict::Refused) return Fail(d.code, d.message);
    // light 0 keeps the single-light kernel path's slots; an empty list is uploaded as one dark light that is never consulted
    const rt_light noLight{{0.f, 1.f, 0.f}, {0.f, 0.f, 0.f}, 0.f};
    const rt_light* sun = n_lights ? lights : &noLight;
    RT_HIP(hipSetDevice(ctx->device));
    int rc;
    if ((rc = Settle(ctx, rtseq::kSettleBeforeScene)) != RT_OK) return rc;
    rtprep::PrepOptions opt = rtprep::PrepOptions::FromEnv();
    opt.treeTop = ctx->treeTop;  // (fixed at rt_create)
    opt.shadowGrid = ctx->useShadowGrid;
    const rtprep::PreparedScene P = rtprep::PrepareScene(spheres, materials, n, lights, n_lights, opt);
    const rtprep::SceneLayout& L = P.layout;
    const rtprep::ShadowGrid& SG = P.shadow;
    // work lists, the shadow index and the closest-hit keys carry scan-entry ids in 16 bits
    if (L.scan.size() >= 65536) return Fail(RT_ERR_INVALID_ARG, "rt_scene_upload: scenes beyond 65,535 scan entries (about 65,000 spheres) are not supported");
    const uint32_t nPad = (uint32_t)L.scan.size();

    // ---- the tables, to the device
    RT_HIP(hipStreamSynchronize(ctx->stream));
    if ((rc = ctx->scan.Upload(L.scan)) != RT_OK) return rc;
    if ((rc = ctx->orig.Upload(L.orig)) != RT_OK) return rc;
    if ((rc = ctx->tree.Upload(L.tree)) != RT_OK) return rc;
    if ((rc = ctx->leaf.Upload(L.leaf)) != RT_OK) return rc;
    if ((rc = ctx->radius.Upload(P.radius)) != RT_OK) return rc;
    if ((rc = ctx->mats.Upload(P.mats)) != RT_OK) return rc;
    ctx->mats16Ok = P.mats16Ok;
    // (the packed table has its full size whether or not this scene packs: a later rt_set_materials that flips mats16Ok only copies)
    if ((rc = P.mats16Ok ? ctx->mats16.Upload(P.mats16) : ctx->mats16.Reserve(P.mats16.size())) != RT_OK) return rc;
    if ((rc = ctx->matType.Upload(P.matType)) != RT_OK) return rc;
    rttile::SceneReplaced(ctx->tiles);  // (their inputs are overwritten: nothing of the tiles' tables is valid)
    (void)rtseq::TileTablesDropped(ctx->seq);
    // The shadow indices -- light 0's (staged into LDS by the flat scan's kernels, else read in global memory), one per further light
    // and light 0's far tier, both in global memory (256 x 256 cells at most) -- each in buffers sized for an index of any direction,
    // the disabled ones included: rt_turn_lights only copies.  So the records know their tables' addresses before the copies.
    const uint32_t nIdx = opt.shadowGrid ? n_lights : 0u;  // lights that may have an index (RT_SHADOW_GRID=0: none, after any turn)
    if (nIdx != 0u) {
        if ((rc = ReserveShadowGrid(rtscene::Light0CellsMax(L.InGlobalMemory(), opt), ctx->sgCells, ctx->sgEntries, ctx->sgGlobal)) != RT_OK) return rc;
        if ((rc = ReserveShadowGrid(opt.shadowCellsGlobal, ctx->farIdx.cells, ctx->farIdx.entries, ctx->farIdx.global)) != RT_OK) return rc;
        if (opt.sgSph && L.InGlobalMemory() && (rc = ctx->sgSph.Reserve(rtprep::kShadowSphRecordsMax)) != RT_OK) return rc;
    }
    for (uint32_t k = 1; k < nIdx; ++k)
        if ((rc = ReserveShadowGrid(opt.shadowCellsGlobal, ctx->extraIdx[k].cells, ctx->extraIdx[k].entries, ctx->extraIdx[k].global)) != RT_OK) return rc;
    // (both staging slots: the largest of what rt_set_materials, rt_turn_lights and rt_temporal_forget copy)
    rtscene::StageShape stageShape;
    stageShape.nPad = nPad, stageShape.n = n, stageShape.nIdx = nIdx, stageShape.inGlobalMemory = L.InGlobalMemory();
    if ((rc = StageReserve(ctx, rtscene::StageBytesMax(stageShape, opt))) != RT_OK) return rc;
    std::vector<rtd::LightRec> recs = LightRecords(ctx, P, lights, n_lights, camera->origin);
    const size_t nRecs = recs.size();
    // (n_lights records lie there from now on, the far tier's slot empty while that index is off: a turn that switches it on writes
    // every field of it but cam_o, which nothing reads of that record and which is zero from here)
    recs.resize(std::max<size_t>(nRecs, n_lights), rtd::LightRec{});
    if (!recs.empty() && (rc = ctx->lightRecs.Upload(recs)) != RT_OK) return rc;
    for (uint32_t k = 1; k < n_lights; ++k) {
        const rtprep::ShadowGrid& G2 = P.extraShadow[k - 1];
        if (G2.enabled && (rc = UploadShadowGrid(G2, ctx->extraIdx[k].cells, ctx->extraIdx[k].entries, ctx->extraIdx[k].global)) != RT_OK) return rc;
    }
    if (P.shadowFar.enabled && (rc = UploadShadowGrid(P.shadowFar, ctx->farIdx.cells, ctx->farIdx.entries, ctx->farIdx.global)) != RT_OK) return rc;
    if (SG.enabled && (rc = UploadShadowGrid(SG, ctx->sgCells, ctx->sgEntries, ctx->sgGlobal)) != RT_OK) return rc;
    if (!P.sgSph.empty() && (rc = ctx->sgSph.Upload(P.sgSph)) != RT_OK) return rc;
    if (L.gridOn) {
        if ((rc = ctx->gridCells.Upload(L.gridCellStart)) != RT_OK) return rc;
        if (!L.gridQ.empty() && (rc = ctx->gridQ.Upload(L.gridQ)) != RT_OK) return rc;
    }

    // ---- the launch parameters' scene part
    rtd::TraceParams& b = ctx->base;
    b = rtd::TraceParams{};
    if (L.gridOn) {
        b.grid_cell_start = ctx->gridCells.ptr;
        b.grid_nu = L.gridNu;
        b.grid_nv = L.gridNv;
        b.grid_ax_u = L.gridAxU;
        b.grid_ax_v = L.gridAxV;
        b.grid_g0u = L.gridG0u;
        b.grid_g0v = L.gridG0v;
        b.grid_inv_h = L.gridInvH;
        b.grid_rmax_over_h = L.gridRmaxOverH;
        b.grid_big_norm = L.gridBigNorm;
        b.grid_qrec = L.gridQ.empty() ? nullptr : ctx->gridQ.ptr;
        for (int c = 0; c < 8; ++c) b.grid_q[c] = L.gridQc[c];
    }
    b.n_lights = n_lights;
    SetSunAndIndices(ctx, P, *sun, nRecs);
    b.scan = ctx->scan.ptr;
    b.orig = ctx->orig.ptr;
    b.leaf = ctx->leaf.ptr;
    b.tree = ctx->tree.ptr;
    b.n_groups = L.nGroups;
    b.n_levels = L.nLevels;
    for (uint32_t k = 0; k < rtd::kMaxLevels; ++k) {
        b.level_off[k] = L.levelOff[k];
        b.level_cnt[k] = L.levelCnt[k];
    }
    b.bound_norm = L.boundNorm;
    b.n_always = L.nAlways;
    for (int k = 0; k < 9; ++k) b.tree_box[k] = L.treeBox[k];
    b.tree_box_on = L.treeBoxOn ? 1u : 0u;
    b.single_mask[0] = P.singleMask[0];
    b.single_mask[1] = P.singleMask[1];
    b.radius = ctx->radius.ptr;
    b.mats = ctx->mats.ptr;
    b.mats16 = ctx->mats16Ok ? ctx->mats16.ptr : nullptr;
    b.n = n;
    b.n_padded = nPad;
    SetCamera(b, *camera);
    SetSky(b, *sky);
    rtscene::CommitUpload(ctx->scene, spheres, materials, n, *camera, lights, n_lights, *sky, exposure_scale, L, opt);
    SetExposure(b, ctx->scene);
    DropVoided(ctx, rtseq::SceneReplaced(ctx->seq));
    return RT_OK;
}

// ---- edits: camera, materials, sky, lights and exposure without an upload (rt_api.h).  What each refuses,
// and when its arguments are the record's own and the call is not an event, is host/rt_scene_edit.h's decision.  An accepted edit
// computes what an upload with the new values computes, runs no scene preparation but its own tables', and takes no host wait but the
// staging's (StageAcquire).  Every entry reads: decide -- return or fail -- hipSetDevice -- settle -- its device work -- commit the
// record -- PictureInputChanged.  A failed settle or launch leaves the record as it was.
static const rtscene::Record* RecordOf(const rt_ctx* ctx) { return ctx ? &ctx->scene : nullptr; }
static bool HasScene(const rt_ctx* ctx) { return ctx && ctx->seq.hasScene; }
static int Answer(const rtscene::Decision& d) { return d.verdict == rtscene::Verdict::Refused ? Fail(d.code, d.message) : RT_OK; }
// The head of an edit.  *go: the edit goes on (changed, and settled without error); else the entry returns what this returned.
static int BeginEdit(rt_ctx* ctx, const rtscene::Decision& d, bool* go) {
    *go = false;
    if (d.verdict != rtscene::Verdict::Changed) return Answer(d);  // (the same record: not an event -- rt_set_sampler's precedent)
    RT_HIP(hipSetDevice(ctx->device));
    const int rc = Settle(ctx, rtseq::kSettleBeforeCamera);  // the pending batch was asked of the old values
    *go = rc == RT_OK;
    return rc;
}
// What a change of the camera voids, and a change of materials, sky, lights or exposure with it -- every picture and every per-tile
// table is a function of each of them (the work order reads matType, the empty-list tiles' constant sample reads sky and exposure):
// decided by the camera's two events, written here once for the five entries.
static void PictureInputChanged(rt_ctx* ctx) {
    rttile::CameraChanged(ctx->tiles);
    (void)rtseq::TileTablesDropped(ctx->seq);
    DropVoided(ctx, rtseq::CameraChanged(ctx->seq));
}

int rt_set_camera(rt_ctx* ctx, const rt_camera* camera) {
    bool go;
    const int rc = BeginEdit(ctx, rtscene::DecideSetCamera(RecordOf(ctx), HasScene(ctx), camera), &go);
    if (!go) return rc;
    // The one piece of device memory that holds the camera: cam_o of lights 1 .. (the far-tier record behind them carries none).  On
    // the stream, behind every launch of the old camera, the origin by value: no host wait, nothing read later.
    const uint32_t extra = ctx->base.n_lights > 1u ? ctx->base.n_lights - 1u : 0u;
    RT_HIP((hipError_t)rtcam::LaunchLightCamera(ctx->stream, ctx->lightRecs.ptr, extra, camera->origin));
    SetCamera(ctx->base, *camera);
    rtscene::CommitCamera(ctx->scene, *camera);
    PictureInputChanged(ctx);
    return RT_OK;
}

int rt_get_camera(rt_ctx* ctx, rt_camera* out) { return Answer(rtscene::GetCamera(RecordOf(ctx), HasScene(ctx), out)); }

int rt_set_materials(rt_ctx* ctx, const rt_material* materials, uint32_t n, const rt_material* sky) {
    const rtscene::Decision d = rtscene::DecideSetMaterials(RecordOf(ctx), HasScene(ctx), materials, n, sky);
    bool go;
    int rc = BeginEdit(ctx, d, &go);
    if (!go) return rc;
    if (d.table) {
        // The three tables, by their one writer over the upload's layout.  Each buffer has had its full size since the upload.
        const std::vector<uint32_t>& orig = ctx->scene.shadowLayout.orig;
        const rtprep::PreparedMaterials M = rtprep::PrepareMaterials(materials, n, orig.data(), orig.size());
        if ((rc = StageCopy(ctx, rtscene::PlanMaterialStage(M, DestOf(ctx->mats), DestOf(ctx->mats16), DestOf(ctx->matType)))) != RT_OK) return rc;
        ctx->mats16Ok = M.mats16Ok;  // (either way round: the launch plan reads the pointer)
        ctx->base.mats16 = M.mats16Ok ? ctx->mats16.ptr : nullptr;
    }
    SetSky(ctx->base, *sky);
    rtscene::CommitMaterials(ctx->scene, d, materials, *sky);
    PictureInputChanged(ctx);
    return RT_OK;
}

int rt_set_lights(rt_ctx* ctx, const rt_light* lights, uint32_t n_lights) {
    bool go;
    const int rc = BeginEdit(ctx, rtscene::DecideSetLights(RecordOf(ctx), HasScene(ctx), lights, n_lights), &go);
    if (!go) return rc;
    // Light 0's radiance is a launch parameter.  Lights 1 .. keep theirs in device memory: patched on the stream, by value, behind
    // every launch of the old radiance (the far-tier record behind them holds an index and no light).
    rtd::LightRec tmp{};
    rtedit::LightRadiance R{};
    for (uint32_t k = 1; k < n_lights; ++k) {
        SetLight(tmp, lights[k]);
        for (int c = 0; c < 3; ++c) R.rad[k - 1][c] = tmp.sun_rad[c];
    }
    RT_HIP((hipError_t)rtedit::LaunchLightRadiance(ctx->stream, ctx->lightRecs.ptr, n_lights - 1u, R));
    SetLight(ctx->base, lights[0]);
    rtscene::CommitLights(ctx->scene, lights);
    PictureInputChanged(ctx);
    return RT_OK;
}

// Turning the lights: direction, colour and luminance of every light as one event.  Of everything a scene becomes, a
// direction reaches the shadow indices alone: they are rebuilt on the host by their one writer over what the upload kept, copied into
// buffers reserved at the builder's bounds, and the records of lights 1 .. and of the far tier are rewritten on the stream by value.
int rt_turn_lights(rt_ctx* ctx, const rt_light* lights, uint32_t n_lights) {
    bool go;
    int rc = BeginEdit(ctx, rtscene::DecideTurnLights(RecordOf(ctx), HasScene(ctx), lights, n_lights), &go);
    if (!go) return rc;
    if (ctx->lightRecs.count < n_lights) return Fail(RT_ERR_HIP, "rt_turn_lights: the light records are fewer than the lights (no upload reserved them)");
    const rtscene::Record& scene = ctx->scene;
    const rtprep::PreparedShadows S = rtprep::PrepareShadows(scene.spheres.data(), scene.shadowLayout, lights, n_lights, scene.prepOpt);
    // The tables of every enabled index: only the actual bytes; the room is the upload's reservation.
    rtscene::IndexDest extra[RT_MAX_LIGHTS];
    for (uint32_t k = 1; k < n_lights; ++k) extra[k - 1] = IndexDestOf(ctx->extraIdx[k].cells, ctx->extraIdx[k].entries, ctx->extraIdx[k].global);
    const rtscene::StagePlan plan = rtscene::PlanShadowStage(S, IndexDestOf(ctx->sgCells, ctx->sgEntries, ctx->sgGlobal), extra,
                                                             IndexDestOf(ctx->farIdx.cells, ctx->farIdx.entries, ctx->farIdx.global), DestOf(ctx->sgSph));
    if ((rc = StageCopy(ctx, plan)) != RT_OK) return rc;
    // The records in device memory, behind the copies and behind every launch that reads the old ones: by value, cam_o left alone.
    const std::vector<rtd::LightRec> recs = LightRecords(ctx, S, lights, n_lights, scene.camera.origin);
    RT_HIP((hipError_t)rtedit::LaunchLightIndex(ctx->stream, ctx->lightRecs.ptr, (uint32_t)recs.size(), recs.data()));
    SetSunAndIndices(ctx, S, lights[0], recs.size());  // light 0, the index's sizes for the launch plan, far_index, extra_lights
    rtscene::CommitLights(ctx->scene, lights);
    PictureInputChanged(ctx);
    return RT_OK;
}

int rt_get_lights(rt_ctx* ctx, rt_light* out, uint32_t capacity, uint32_t* n_lights) {
    return Answer(rtscene::GetLights(RecordOf(ctx), HasScene(ctx), out, capacity, n_lights));
}

int rt_set_exposure(rt_ctx* ctx, float exposure_scale) {
    bool go;
    const int rc = BeginEdit(ctx, rtscene::DecideSetExposure(RecordOf(ctx), HasScene(ctx), exposure_scale), &go);
    if (!go) return rc;
    rtscene::CommitExposure(ctx->scene, exposure_scale);
    SetExposure(ctx->base, ctx->scene);
    PictureInputChanged(ctx);
    return RT_OK;
}

int rt_set_frame_pipelining(rt_ctx* ctx, uint32_t depth) {
    if (!ctx || depth > rtd::kMaxFramesInFlight - 2u) return Fail(RT_ERR_INVALID_ARG, "rt_set_frame_pipelining: depth must be 0..14");
    RT_HIP(hipSetDevice(ctx->device));
    int rc = Settle(ctx, rtseq::kPending);
    if (rc != RT_OK) return rc;
    rc = Settle(ctx, rtseq::kInFlight);  // (failed or not, nothing is in flight any more: the depth is stored)
    DropVoided(ctx, rtseq::PipeliningSettingChanged(ctx->seq, depth));
    return rc;
}

int rt_committed_samples(rt_ctx* ctx, uint32_t* out) {
    if (!ctx || !out) return Fail(RT_ERR_INVALID_ARG, "rt_committed_samples: null argument");
    RT_HIP(hipSetDevice(ctx->device));
    RT_HIP(hipStreamSynchronize(ctx->stream));
    *out = ctx->seq.accumulated;
    if (ctx->pipeOpen) {
        rtd::FrameCtl c{};
        RT_HIP(hipMemcpy(&c, ctx->ctl.ptr, sizeof(c), hipMemcpyDeviceToHost));
        *out = c.committed_samples[ctx->pipeCommits & 1u];
    }
    return RT_OK;
}

int rt_set_sampler(rt_ctx* ctx, uint32_t flags) {
    if (!ctx || (flags & ~(RT_SAMPLER_COSINE_HEMISPHERE | RT_SAMPLER_SQRT_DISK)) != 0u) return Fail(RT_ERR_INVALID_ARG, "rt_set_sampler: unknown flag");
    if (flags != ctx->sampler) DropVoided(ctx, rtseq::SamplerChanged(ctx->seq));
    ctx->sampler = flags;
    return RT_OK;
}

int rt_set_noise_estimate(rt_ctx* ctx, int on) {
    if (!ctx) return Fail(RT_ERR_INVALID_ARG, "rt_set_noise_estimate: null ctx");
    DropVoided(ctx, rtseq::NoiseToggled(ctx->seq, on != 0));
    return RT_OK;
}

int rt_clear(rt_ctx* ctx) {
    if (!ctx) return Fail(RT_ERR_INVALID_ARG, "rt_clear: null ctx");
    DropVoided(ctx, rtseq::Cleared(ctx->seq));
    return RT_OK;
}

static int RenderNow(rt_ctx* ctx, const rtseq::Call& call, rt_stats* out_stats, uint32_t aheadEnd = 0);

// The ordered accumulation of the planes [first, first + count) of the sample buffer: with rt_set_noise_estimate on, the kernel that
// also adds their squares to the strip of second moments (same hdr bits); off, the plain one.
// With flags of the empty-list tiles (BuildTileOrder) the tile-aware forms: the flagged tiles' planes are the constant, whether the
// launch that traced the buffer wrote them or left them out.
static void LaunchAccumulate(rt_ctx* ctx, uint32_t npix, uint32_t spp, uint32_t first, uint32_t count) {
    if (rttile::AccumulateByFlags(ctx->tiles)) {
        const float* skyC = reinterpret_cast<const float*>(ctx->skyInfo.ptr + 1);  // (the constant sample follows the count)
        if (ctx->seq.noise)
            hipLaunchKernelGGL(rtd::rt_accumulate_moments_tiles_kernel, dim3((npix + 255) / 256), dim3(256), 0, ctx->stream, ctx->samples.ptr,
                               ctx->hdr.ptr, ctx->sq.ptr, npix, spp, first, count, ctx->skyFlags.ptr, skyC);
        else
            hipLaunchKernelGGL(rtd::rt_accumulate_tiles_kernel, dim3((npix + 255) / 256), dim3(256), 0, ctx->stream, ctx->samples.ptr,
                               ctx->hdr.ptr, npix, spp, first, count, ctx->skyFlags.ptr, skyC);
    } else if (ctx->seq.noise)
        hipLaunchKernelGGL(rtd::rt_accumulate_moments_kernel, dim3((npix + 255) / 256), dim3(256), 0, ctx->stream, ctx->samples.ptr, ctx->hdr.ptr,
                           ctx->sq.ptr, npix, spp, first, count);
    else
        hipLaunchKernelGGL(rtd::rt_accumulate_kernel, dim3((npix + 255) / 256), dim3(256), 0, ctx->stream, ctx->samples.ptr, ctx->hdr.ptr, npix,
                           spp, first, count);
}

// Frame batching: render the pending sample planes with ONE launch (no statistics, nothing waits for the device).
static int BatchFlush(rt_ctx* ctx) {
    if (!ctx->seq.pend.on) return RT_OK;
    return RenderNow(ctx, rtseq::PendingTaken(ctx->seq), nullptr);
}

// The readers (rtseq::PendingMustRender has the rule): nothing committed yet, or the pending frames START a new accumulation -- they
// are what there is to show, and seq.pic / seq.rows still describe the old strip.
static int RenderPendingForReader(rt_ctx* ctx) { return rtseq::PendingMustRender(ctx->seq) ? BatchFlush(ctx) : RT_OK; }

int rt_set_frame_batch(rt_ctx* ctx, uint32_t frames) {
    if (!ctx || frames == 0 || frames > 4096) return Fail(RT_ERR_INVALID_ARG, "rt_set_frame_batch: frames must be 1..4096");
    RT_HIP(hipSetDevice(ctx->device));
    const int rc = Settle(ctx, rtseq::kSettleBeforeBatchSetting);  // (failed or not, nothing is pending any more: the size is stored)
    DropVoided(ctx, rtseq::BatchSettingChanged(ctx->seq, frames));
    return rc;
}

int rt_set_frame_lookahead(rt_ctx* ctx, uint32_t frames) {
    if (!ctx || frames == 0 || frames > 4096) return Fail(RT_ERR_INVALID_ARG, "rt_set_frame_lookahead: frames must be 1..4096");
    DropVoided(ctx, rtseq::LookaheadSettingChanged(ctx->seq, frames));
    return RT_OK;
}

// What the call does is the sequencer's to say (rtseq::PlanRender: plain, batched, render-ahead; pipelining is decided in RenderNow,
// where the launch plan is at hand); here its steps are carried out in order.
int rt_render(rt_ctx* ctx, uint32_t W, uint32_t H, rt_rowset rs, uint32_t s0, uint32_t s1, uint32_t max_depth, uint64_t seed,
              rt_stats* out_stats) {
    if (!ctx) return Fail(RT_ERR_INVALID_ARG, "rt_render: null ctx");
    rtseq::Call call;
    call.pic = {W, H, rs};
    call.rows = rtprep::RowsetRowsWithin(rs, H);
    call.s0 = s0, call.s1 = s1, call.max_depth = max_depth, call.seed = seed;
    call.wants_stats = out_stats != nullptr;
    const rtseq::Steps steps = rtseq::PlanRender(ctx->seq, call);
    for (uint32_t k = 0; k < steps.n; ++k) {
        const rtseq::Step& step = steps.v[k];
        int rc = RT_OK;
        switch (step.kind) {
            case rtseq::StepKind::AddAhead:  // the planes were traced by an earlier call's launch: one small kernel
                RT_HIP(hipSetDevice(ctx->device));
                LaunchAccumulate(ctx, ctx->seq.pic.W * ctx->seq.rows, ctx->seq.ahead.spp, step.first, step.count);
                RT_HIP(hipGetLastError());
                rtseq::AheadAdded(ctx->seq, step);
                break;
            case rtseq::StepKind::Record: rtseq::Recorded(ctx->seq, call); break;
            case rtseq::StepKind::RenderPending: rc = BatchFlush(ctx); break;
            case rtseq::StepKind::RenderNow: rc = RenderNow(ctx, call, out_stats, step.aheadEnd); break;
            case rtseq::StepKind::Refuse:
                rtseq::RenderBegins(ctx->seq);
                rc = Fail(step.refusal.status, step.refusal.message);
                break;
        }
        if (rc != RT_OK) return rc;
    }
    return RT_OK;
}

// aheadEnd (render-ahead, rt_set_frame_lookahead): trace the planes [s0, aheadEnd) with this call's ONE launch, add only [s0, s1)
// to the strip and keep the rest in the sample buffer for the calls that continue (0: trace [s0, s1) only).  The sequencer admits
// the call and cuts it into passes; the tables, the launches, the events and the statistics are here.
static int RenderNow(rt_ctx* ctx, const rtseq::Call& call, rt_stats* out_stats, uint32_t aheadEnd) {
    rtseq::State& seq = ctx->seq;
    rtseq::RenderBegins(seq);
    const rtseq::Refusal bad = rtseq::CheckCall(seq, call);
    if (bad.status != RT_OK) return Fail(bad.status, bad.message);
    const uint32_t W = call.pic.W, rows = call.rows, s0 = call.s0, s1 = call.s1, max_depth = call.max_depth;
    const rt_rowset rs = call.pic.rs;
    const uint64_t seed = call.seed;
    RT_HIP(hipSetDevice(ctx->device));
    const uint32_t npix = W * rows;
    SkyCountPoll(ctx);  // (before any table is rebuilt: the call that builds the flags never sees their number, whatever the timing)

    const bool pipelined = rtseq::MayPipeline(seq, call) &&
                           rtplan::PlanTrace(ShapeOf(ctx->base), SettingsOf(ctx), KnobsFromEnv(), {npix, ctx->base.max_depth, rtplan::Mode::Carry}).pipelines;
    const uint32_t abandoned = rtseq::AccumulationStarting(seq, call);
    DropVoided(ctx, abandoned);
    if (!abandoned && !pipelined) {  // anything but a pipelined call first settles what is in flight
        int rcf = PipelineFlush(ctx);
        if (rcf != RT_OK) return rcf;
    }
    rtseq::Refusal why;
    switch (rtseq::Admit(seq, call, &why)) {
        case rtseq::Admission::Refused: return Fail(why.status, why.message);
        case rtseq::Admission::Continues: break;
        case rtseq::Admission::Starts: {
            int rc;
            if ((rc = ctx->hdr.Reserve((size_t)npix * 3)) != RT_OK) return rc;
            if ((rc = ctx->ldr.Reserve((size_t)npix * 3)) != RT_OK) return rc;
            RT_HIP(hipMemsetAsync(ctx->hdr.ptr, 0, (size_t)npix * 3 * sizeof(float), ctx->stream));  // app.cpp:112-119
            if (seq.noise) {
                if ((rc = ctx->sq.Reserve((size_t)npix * 3)) != RT_OK) return rc;
                RT_HIP(hipMemsetAsync(ctx->sq.ptr, 0, (size_t)npix * 3 * sizeof(float), ctx->stream));
            }
            rtseq::AccumulationStarted(seq, call);
            const rttile::Knobs knobs = TileKnobsFromEnv();
            rttile::AccumulationStarts(ctx->tiles, knobs);
            if ((rc = BuildTileMasks(ctx, call.pic, npix, knobs)) != RT_OK) return rc;
            if ((rc = BuildTileOrder(ctx, call.pic, npix)) != RT_OK) return rc;  // (after the masks: it flags the tiles whose list is empty)
        }
    }

    if (pipelined) {
        ctx->tileAcct.skyExcluded = 0;  // (the carrying kernel's launch queues every tile)
        int rcp = PipelineRender(ctx, call.pic, npix, s0, s1, max_depth, seed);
        if (rcp != RT_OK) {
            DropVoided(ctx, rtseq::StepFailed(seq));
            return rcp;
        }
        rtseq::Rendered(seq, call, 0, 0);
        return RT_OK;
    }

    // [s0, s1) in passes whose sample buffer fits the workspace limit
    rtseq::PassSplit split = rtseq::SplitPasses(npix, s0, s1, aheadEnd, ctx->workspaceLimit);
    if (split.refused.status != RT_OK) return Fail(split.refused.status, split.refused.message);
    int rc;
    // The default limit is a snapshot of the free memory at rt_create; another context or the caller's allocator may have
    // taken memory since.  A smaller sample buffer only means more passes (bit-identical: the accumulation stays sequential
    // in s), so shrink the pass until the buffer fits before giving up.
    while ((rc = ctx->samples.Reserve((size_t)npix * split.sppPass * 3)) != RT_OK) {
        if (rc != RT_ERR_OUT_OF_MEMORY || !rtseq::ShrinkPass(split)) return rc;
    }

    // Passes run back to back on the stream: trace(k) -> accumulate(k) -> trace(k+1) are ordered by the stream itself
    // (they share the sample buffer), so the host never waits between passes; each pass has its own three timing
    // events, read once at the end when the caller asked for statistics.
    uint32_t passes = 0;
    auto runPasses = [&]() -> int {
        int rc;
        ctx->tileAcct.freshScans = 0;
        // The tables this call's picture may take, and the empty-list tiles that stay out of the queue (rttile::UseFor has the rules).
        // Their share of the counters is added behind each launch; their samples are the accumulation's constant (LaunchAccumulate).
        const uint32_t nFull = npix >> 6;
        const rttile::Use use = rttile::UseFor(ctx->tiles, call.pic, npix);
        const uint32_t nSky = use.nSky;
        RT_HIP(hipMemsetAsync(ctx->counters.ptr, 0, 6 * sizeof(unsigned long long), ctx->stream));
        ctx->tileAcct.skyExcluded = nSky;
        for (rtseq::Pass pass = rtseq::FirstPass(split); pass.spp != 0; pass = rtseq::NextPass(split, pass)) {
            const uint32_t s = pass.s, spp = pass.spp;
            rtd::TraceParams tp = PassParams(ctx, call.pic, s, spp, npix, max_depth, seed);
            tp.tile_order = use.order ? ctx->tileOrder.ptr : nullptr;
            tp.tile_masks = use.masks ? ctx->tileMasks.ptr : nullptr;
            tp.tile_spheres = use.lists ? ctx->tileSpheres.ptr : nullptr;
            tp.sky_skip = use.sky_skip;
            ctx->tileAcct.freshScans += ((uint64_t)tp.total_paths + 63u) / 64u;  // (all tiles: the statistics do not know about the shorter queue)
            if (nSky != 0u) tp.total_paths = (nFull - nSky) * 64u * spp;
            tp.samples = ctx->samples.ptr;
            while (ctx->passEv.size() < 3 * (size_t)(passes + 1)) {
                hipEvent_t e = nullptr;
                RT_HIP(hipEventCreate(&e));
                ctx->passEv.push_back(e);
            }
            hipEvent_t* ev = ctx->passEv.data() + 3 * (size_t)passes;
            RT_HIP(hipEventRecord(ev[0], ctx->stream));
            if ((rc = LaunchRaygenTables(ctx, tp, ctx->jitterTab, ctx->lensTab, s, spp, W, rs)) != RT_OK) return rc;
            if ((rc = LaunchTrace(ctx, tp)) != RT_OK) return rc;
            if (nSky != 0u) {
                const unsigned long long planes = (unsigned long long)nSky * spp;
                hipLaunchKernelGGL(rtd::rt_sky_counters_kernel, dim3(1), dim3(64), 0, ctx->stream, ctx->counters.ptr, planes * 64ull,
                                   ctx->tileAcct.lastTraceSky ? planes : 0ull);
                RT_HIP(hipGetLastError());
            }
            RT_HIP(hipEventRecord(ev[1], ctx->stream));
            LaunchAccumulate(ctx, npix, spp, pass.add_first, pass.add_count);
            RT_HIP(hipGetLastError());
            RT_HIP(hipEventRecord(ev[2], ctx->stream));
            ++passes;
        }
        return RT_OK;
    };
    if ((rc = runPasses()) != RT_OK) {
        DropVoided(ctx, rtseq::StepFailed(seq));  // some passes may already have been added to hdr
        return rc;
    }
    rtseq::Rendered(seq, call, split.aheadEnd, split.sppTrace);
    const uint32_t sppTotal = s1 - s0;

    if (out_stats) {
        // Without a stats request the call stays asynchronous on the stream (progressive 1-spp frames are launch bound:
        // ~0.2 ms of GPU work each); with one it waits for the last pass and reads the event timers.
        float msTrace = 0.f, msAcc = 0.f;
        RT_HIP(hipEventSynchronize(ctx->passEv[3 * (size_t)(passes - 1) + 2]));
        for (uint32_t k = 0; k < passes; ++k) {
            float a = 0.f, b = 0.f;
            RT_HIP(hipEventElapsedTime(&a, ctx->passEv[3 * (size_t)k], ctx->passEv[3 * (size_t)k + 1]));
            RT_HIP(hipEventElapsedTime(&b, ctx->passEv[3 * (size_t)k + 1], ctx->passEv[3 * (size_t)k + 2]));
            msTrace += a;
            msAcc += b;
        }
        unsigned long long c[2] = {0, 0};
        RT_HIP(hipMemcpy(c, ctx->counters.ptr, sizeof(c), hipMemcpyDeviceToHost));
        std::memset(out_stats, 0, sizeof(*out_stats));
        out_stats->samples = (uint64_t)npix * sppTotal;
        out_stats->traversals = c[0];
        out_stats->segments = c[1];
        out_stats->ms_render = msTrace;
        out_stats->ms_accumulate = msAcc;
        out_stats->ms_resolve = 0.0;
        out_stats->local_rows = rows;
        out_stats->passes = passes;
    }
    return RT_OK;
}

int rt_resolve(rt_ctx* ctx, uint32_t n_samples) {
    if (!ctx) return Fail(RT_ERR_INVALID_ARG, "rt_resolve: null ctx");
    if (const int rcb = RenderPendingForReader(ctx)) return rcb;
    if (ctx->seq.accumulated == 0) return Fail(RT_ERR_SEQUENCE, "rt_resolve: nothing accumulated");
    RT_HIP(hipSetDevice(ctx->device));
    const uint32_t n = n_samples ? n_samples : ctx->seq.accumulated;
    const uint32_t npix = ctx->seq.pic.W * ctx->seq.rows;
    RT_HIP(hipEventRecord(ctx->ev[0], ctx->stream));
    // with frames in flight the strip holds FrameCtl::committed_samples samples, a number only the device knows
    const uint32_t* devCount = (ctx->pipeOpen && n_samples == 0) ? &ctx->ctl.ptr->committed_samples[ctx->pipeCommits & 1u] : nullptr;
    hipLaunchKernelGGL(rtd::rt_resolve_kernel, dim3((npix + 255) / 256), dim3(256), 0, ctx->stream, ctx->hdr.ptr, ctx->ldr.ptr, npix, n,
                       devCount);
    RT_HIP(hipGetLastError());
    return ElapsedSince(ctx, 0, &ctx->lastResolveMs);
}

double rt_last_resolve_ms(rt_ctx* ctx) { return ctx ? ctx->lastResolveMs : 0.0; }

// Each reader once, for both of its forms (who: the entry's name for the messages; CopyStrips has the difference).
static int ReadPicture(rt_ctx* ctx, const char* who, bool toDevice, void* hdr_rgb, void* ldr_rgb) {
    if (!ctx) return Fail(RT_ERR_INVALID_ARG, std::string(who) + ": null ctx");
    if (const int rcb = RenderPendingForReader(ctx)) return rcb;
    if (ctx->seq.accumulated == 0) return Fail(RT_ERR_SEQUENCE, std::string(who) + ": nothing rendered");
    RT_HIP(hipSetDevice(ctx->device));
    const size_t npix = (size_t)ctx->seq.pic.W * ctx->seq.rows;
    return CopyStrips(ctx, toDevice, {{hdr_rgb, ctx->hdr.ptr, npix * 3 * sizeof(float)}, {ldr_rgb, ctx->ldr.ptr, npix * 3}});
}
int rt_download(rt_ctx* ctx, float* hdr_rgb, uint8_t* ldr_rgb) { return ReadPicture(ctx, "rt_download", false, hdr_rgb, ldr_rgb); }
int rt_copy_to_device(rt_ctx* ctx, void* dev_hdr_rgb, void* dev_ldr_rgb) { return ReadPicture(ctx, "rt_copy_to_device", true, dev_hdr_rgb, dev_ldr_rgb); }

// ---------------------------------------------------------------- noise estimate (rt_noise.h)
// Like the other readers: a pending batch that starts the picture is rendered first; planes traced ahead never reached the strips.
static int NoiseReady(rt_ctx* ctx, const char* who, uint32_t minSamples) {
    if (!ctx) return Fail(RT_ERR_INVALID_ARG, std::string(who) + ": null ctx");
    if (!ctx->seq.noise) return Fail(RT_ERR_SEQUENCE, std::string(who) + ": rt_set_noise_estimate is off");
    if (const int rcb = RenderPendingForReader(ctx)) return rcb;
    if (ctx->seq.accumulated == 0) return Fail(RT_ERR_SEQUENCE, std::string(who) + ": nothing accumulated");
    if (ctx->seq.accumulated < minSamples) return Fail(RT_ERR_SEQUENCE, std::string(who) + ": the estimate needs at least 2 samples per pixel");
    RT_HIP(hipSetDevice(ctx->device));
    return RT_OK;
}

// The same without the switch, for readers of hdr alone (the spatial variance source): a picture with samples in the strip, as
// rt_resolve(ctx, 0) sees it.  With frames in flight the count is the device's (CommittedWord); nothing in flight is settled.
static int PictureReady(rt_ctx* ctx, const char* who) {
    if (!ctx) return Fail(RT_ERR_INVALID_ARG, std::string(who) + ": null ctx");
    if (const int rcb = RenderPendingForReader(ctx)) return rcb;
    if (ctx->seq.accumulated == 0) return Fail(RT_ERR_SEQUENCE, std::string(who) + ": nothing accumulated");
    RT_HIP(hipSetDevice(ctx->device));
    return RT_OK;
}
static const uint32_t* CommittedWord(const rt_ctx* ctx) { return ctx->pipeOpen ? &ctx->ctl.ptr->committed_samples[ctx->pipeCommits & 1u] : nullptr; }

static int ReadMoments(rt_ctx* ctx, const char* who, bool toDevice, void* sq_rgb) {
    const int rc = NoiseReady(ctx, who, 1);
    if (rc != RT_OK) return rc;
    if (!sq_rgb) return Fail(RT_ERR_INVALID_ARG, std::string(who) + ": null buffer");
    return CopyStrips(ctx, toDevice, {{sq_rgb, ctx->sq.ptr, (size_t)ctx->seq.pic.W * ctx->seq.rows * 3 * sizeof(float)}});
}
int rt_download_moments(rt_ctx* ctx, float* sq_rgb) { return ReadMoments(ctx, "rt_download_moments", false, sq_rgb); }
int rt_copy_moments_to_device(rt_ctx* ctx, void* dev_sq) { return ReadMoments(ctx, "rt_copy_moments_to_device", true, dev_sq); }

int rt_noise_map(rt_ctx* ctx, float floor, float* out_abs_rel) {
    int rc = NoiseReady(ctx, "rt_noise_map", 2);
    if (rc != RT_OK) return rc;
    if (!out_abs_rel) return Fail(RT_ERR_INVALID_ARG, "rt_noise_map: null buffer");
    const uint32_t npix = ctx->seq.pic.W * ctx->seq.rows;
    if ((rc = ctx->noiseMap.Reserve((size_t)npix * 2)) != RT_OK) return rc;
    hipLaunchKernelGGL(rtd::rt_noise_map_kernel, dim3((npix + 255) / 256), dim3(256), 0, ctx->stream, ctx->hdr.ptr, ctx->sq.ptr, npix, ctx->seq.accumulated,
                       floor, reinterpret_cast<float2*>(ctx->noiseMap.ptr));
    RT_HIP(hipGetLastError());
    RT_HIP(hipStreamSynchronize(ctx->stream));
    RT_HIP(hipMemcpy(out_abs_rel, ctx->noiseMap.ptr, (size_t)npix * 2 * sizeof(float), hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_noise_summary(rt_ctx* ctx, float floor, const float* thresholds, uint32_t n_thr, uint32_t* out_counts, float* out_max_rel) {
    int rc = NoiseReady(ctx, "rt_noise_summary", 2);
    if (rc != RT_OK) return rc;
    if (n_thr > rtd::kNoiseMaxThresholds || (n_thr != 0 && (!thresholds || !out_counts)))
        return Fail(RT_ERR_INVALID_ARG, "rt_noise_summary: at most 8 thresholds, with their buffers");
    const uint32_t npix = ctx->seq.pic.W * ctx->seq.rows;
    rtd::NoiseThresholds thr{};
    thr.n = n_thr;
    for (uint32_t k = 0; k < n_thr; ++k) thr.t[k] = thresholds[k];
    if ((rc = ctx->noiseRed.Reserve(rtd::kNoiseMaxThresholds + 1)) != RT_OK) return rc;
    RT_HIP(hipMemsetAsync(ctx->noiseRed.ptr, 0, (rtd::kNoiseMaxThresholds + 1) * sizeof(uint32_t), ctx->stream));
    hipLaunchKernelGGL(rtd::rt_noise_summary_kernel, dim3((npix + 255) / 256), dim3(256), 0, ctx->stream, ctx->hdr.ptr, ctx->sq.ptr, npix,
                       ctx->seq.accumulated, floor, thr, ctx->noiseRed.ptr);
    RT_HIP(hipGetLastError());
    RT_HIP(hipStreamSynchronize(ctx->stream));
    uint32_t red[rtd::kNoiseMaxThresholds + 1];
    RT_HIP(hipMemcpy(red, ctx->noiseRed.ptr, sizeof(red), hipMemcpyDeviceToHost));
    for (uint32_t k = 0; k < n_thr; ++k) out_counts[k] = red[k];
    if (out_max_rel) std::memcpy(out_max_rel, &red[rtd::kNoiseMaxThresholds], sizeof(float));
    return RT_OK;
}

// ---------------------------------------------------------------- feature buffers (rt_features.h)
// Sequencing of its own (featCount / featNext), strips and ray-generation tables of its own: rt_render's accumulation, tile tables,
// pending batches, planes traced ahead and carried paths are neither read nor changed.
int rt_render_features(rt_ctx* ctx, uint32_t W, uint32_t H, rt_rowset rs, uint32_t s0, uint32_t s1, double* out_ms) {
    if (!ctx) return Fail(RT_ERR_INVALID_ARG, "rt_render_features: null ctx");
    if (W == 0 || H == 0 || s0 == 0 || s1 <= s0) return Fail(RT_ERR_INVALID_ARG, "rt_render_features: empty image or sample range");
    if (!ctx->seq.hasScene) return Fail(RT_ERR_NO_SCENE, "rt_render_features: no scene uploaded");
    const uint32_t rows = rtprep::RowsetRowsWithin(rs, H);
    if (rows == 0) return Fail(RT_ERR_INVALID_ARG, "rt_render_features: bad row set");
    const uint64_t npix64 = (uint64_t)W * rows;
    if (npix64 > (1ull << 31) - 64u || (uint64_t)W * H > 0xffffffffull) return Fail(RT_ERR_INVALID_ARG, "rt_render_features: image too large");
    // the lens table is indexed by s + i + j: keep that sum, like the tables' sizes, inside 32 bits
    if ((uint64_t)s1 + W + H > 0xffffffffull) return Fail(RT_ERR_INVALID_ARG, "rt_render_features: sample range too large");
    RT_HIP(hipSetDevice(ctx->device));
    const uint32_t npix = (uint32_t)npix64;
    const rtseq::PictureKey pic{W, H, rs};
    const bool continues = ctx->featCount != 0 && ctx->featPic == pic && s0 == ctx->featNext;
    // (a call that starts at 1 always starts over; one that could continue does; after rt_clear_features any s0 starts)
    const bool starts = s0 == 1 || (ctx->featCleared && !continues);
    if (!starts && !continues) return Fail(RT_ERR_SEQUENCE, "rt_render_features: sample range or row set does not continue the accumulation");
    ctx->featCleared = false;
    int rc;
    if (starts) {
        ctx->featCount = 0;
        if ((rc = ctx->feat.Reserve((size_t)npix * rtd::kFeatureChannels)) != RT_OK) return rc;
        if ((rc = ctx->featIds.Reserve(npix)) != RT_OK) return rc;
        ctx->featPic = pic;
        ctx->featRows = rows;
    }
    const uint32_t spp = s1 - s0;
    rtd::TraceParams tp = ctx->base;
    SetPicture(tp, pic);
    tp.s0 = s0;
    tp.sampler = ctx->sampler;
    tp.npix_local = npix;
    rtd::FeatureParams fp{};
    fp.feat = ctx->feat.ptr;
    fp.ids = ctx->featIds.ptr;
    fp.npix = npix;
    fp.s0 = s0;
    fp.s1 = s1;
    fp.cont = starts ? 0u : 1u;
    const rtd::V3 skyAlbedo = rtd::feature_sky_albedo(rtd::feature_material(ctx->scene.sky));
    fp.sky[0] = skyAlbedo.x;
    fp.sky[1] = skyAlbedo.y;
    fp.sky[2] = skyAlbedo.z;
    auto run = [&]() -> int {
        if (out_ms) RT_HIP(hipEventRecord(ctx->ev[2], ctx->stream));
        int rcl = LaunchRaygenTables(ctx, tp, ctx->featJitter, ctx->featLens, s0, spp, W, rs);
        if (rcl != RT_OK || (rcl = LaunchFeatures(ctx, tp, fp)) != RT_OK) return rcl;
        return out_ms ? ElapsedSince(ctx, 2, out_ms) : RT_OK;
    };
    if ((rc = run()) != RT_OK) {
        ctx->featCount = 0;  // the strips may be half written: the next call must start again
        return rc;
    }
    ctx->featCount += spp;
    ctx->featNext = s1;
    return RT_OK;
}

int rt_feature_samples(rt_ctx* ctx, uint32_t* out) {
    if (!ctx || !out) return Fail(RT_ERR_INVALID_ARG, "rt_feature_samples: null argument");
    *out = ctx->featCount;
    return RT_OK;
}

static int ReadFeatures(rt_ctx* ctx, const char* who, bool toDevice, void* feat8, void* ids) {
    if (!ctx) return Fail(RT_ERR_INVALID_ARG, std::string(who) + ": null ctx");
    if (ctx->featCount == 0) return Fail(RT_ERR_SEQUENCE, std::string(who) + ": nothing accumulated");
    RT_HIP(hipSetDevice(ctx->device));
    const size_t npix = (size_t)ctx->featPic.W * ctx->featRows;
    return CopyStrips(ctx, toDevice, {{feat8, ctx->feat.ptr, npix * rtd::kFeatureChannels * sizeof(float)}, {ids, ctx->featIds.ptr, npix * sizeof(uint32_t)}});
}
int rt_download_features(rt_ctx* ctx, float* feat8, uint32_t* ids) { return ReadFeatures(ctx, "rt_download_features", false, feat8, ids); }
int rt_copy_features_to_device(rt_ctx* ctx, void* dev_feat8, void* dev_ids) { return ReadFeatures(ctx, "rt_copy_features_to_device", true, dev_feat8, dev_ids); }

int rt_clear_features(rt_ctx* ctx) {
    if (!ctx) return Fail(RT_ERR_INVALID_ARG, "rt_clear_features: null ctx");
    ctx->featCount = 0;
    ctx->featCleared = true;
    return RT_OK;
}

// ---------------------------------------------------------------- denoise (rt_denoise.h; kernels and launcher: rt_denoise.hip)
// Readers of hdr, sq and feat that write strips of their own: no sequencing state of rt_render or rt_render_features changes.  An
// entry makes its checks and describes what they leave as a DenoiseCall -- DescribePicture for the context's own picture,
// DescribeParts for gathered parts -- and DenoiseRun does the rest; the messages carry the entry's own name in front, and every refusal
// comes before the first change of state.
// "The picture is ready for the filter": the context's accumulation is a row range with feature strips of the same picture.
static int DenoisePictureReady(const rt_ctx* ctx, const char* who) {
    if (ctx->seq.pic.rs.nshards != 1)
        return Fail(RT_ERR_INVALID_ARG, std::string(who) + ": the local rows of a cyclic row set (nshards != 1) are not neighbours in the image");
    if (ctx->featCount == 0) return Fail(RT_ERR_SEQUENCE, std::string(who) + ": no feature strips (rt_render_features)");
    if (ctx->featPic != ctx->seq.pic) return Fail(RT_ERR_SEQUENCE, std::string(who) + ": the feature strips are of another image or row set than the picture");
    if ((ctx->seq.rows + rtdn::kTileH - 1u) / rtdn::kTileH > 65535u) return Fail(RT_ERR_INVALID_ARG, std::string(who) + ": more than 524,280 rows");
    return RT_OK;
}
// "Reserve and describe the strips" of a W x rows picture: the filter's own (guides: the guide strips too; the temporal step has its
// history's), and the RT_DENOISE_STAGE knob.  The inputs are the caller's to fill.
static int DenoiseStrips(rt_ctx* ctx, uint32_t W, uint32_t rows, bool guides, rtdn::Strips* S, int* knob) {
    const size_t npix = (size_t)W * rows;
    int rc;
    for (int k = 0; k < 2; ++k)
        if ((rc = ctx->denState[k].Reserve(npix * 4)) != RT_OK || (guides && (rc = ctx->denGuide[k].Reserve(npix * 4)) != RT_OK)) return rc;
    if ((rc = ctx->den.Reserve(npix * 3)) != RT_OK || (rc = ctx->denVar.Reserve(npix)) != RT_OK || (rc = ctx->denLdr.Reserve(npix * 3)) != RT_OK) return rc;
    *knob = -1;
    if (const char* e = std::getenv("RT_DENOISE_STAGE")) *knob = std::atoi(e) != 0 ? 1 : 0;
    *S = rtdn::Strips{};
    S->W = W;
    S->rows = rows;
    for (int k = 0; k < 2; ++k) {
        S->state[k] = ctx->denState[k].ptr;
        if (guides) S->guide[k] = ctx->denGuide[k].ptr;
    }
    S->den = ctx->den.ptr;
    S->denVar = ctx->denVar.ptr;
    return RT_OK;
}
// "Time, launch the resolve, publish", on either side of the entry's own launch (launched: what it returned, a hipError_t as int).
static int DenoiseBegin(rt_ctx* ctx, double* out_ms) {
    ctx->denValid = false;  // the strips are being rewritten
    if (out_ms) RT_HIP(hipEventRecord(ctx->ev[2], ctx->stream));
    return RT_OK;
}
static int DenoiseFinish(rt_ctx* ctx, const char* who, const rtdn::Strips& S, int launched, double* out_ms) {
    const uint32_t npix = S.W * S.rows;
    const int he = launched;
    if (he != 0) return Fail(RT_ERR_HIP, std::string(who) + ": launch: " + hipGetErrorString((hipError_t)he));
    hipLaunchKernelGGL(rtd::rt_resolve_kernel, dim3((npix + 255) / 256), dim3(256), 0, ctx->stream, ctx->den.ptr, ctx->denLdr.ptr, npix, 1u, nullptr);
    RT_HIP(hipGetLastError());
    if (out_ms)
        if (const int rc = ElapsedSince(ctx, 2, out_ms)) return rc;
    ctx->denW = S.W;
    ctx->denRows = S.rows;
    ctx->denValid = true;
    return RT_OK;
}

// What the checks leave of a call, along the launcher's three axes (host/rt_denoise_launch.h): the current frame's inputs of a W x rows
// picture -- in image order, or as gathered parts (parts) --, the variance source, and the temporal step's part, filled only where
// temporal: the picture the history is keyed with, its row range, the ids, the camera and the fetch.
struct DenoiseCall {
    uint32_t W, rows;
    const float *hdr, *sq, *feat;
    uint32_t n, m;
    rtdn::ShardLayout layout;   // gathered parts where nshards != 0 (the checks refuse 0 there), else image order
    rtd::DenoiseParams P;
    uint32_t spatialRadius;     // 0: v0 from the moments; else the spatial source's radius
    const uint32_t* committed;  // the spatial pass's device-side sample count, or NULL (CommittedWord)
    bool temporal;
    rtseq::PictureKey pic;
    rtd::TemporalGeom geom;
    const uint32_t* ids;
    rtd::TemporalCam cam;
    rtd::TemporalParams T;
    uint32_t fetch;
};
// The history is the context's: set tmpCur is read, the other set is written and becomes tmpCur once everything is enqueued.
static int DenoiseRun(rt_ctx* ctx, const char* who, const DenoiseCall& c, double* out_ms) {
    int rc;
    const size_t npix = (size_t)c.W * c.rows;
    const bool hasPrev = c.temporal && ctx->tmpValid && ctx->tmpPic == c.pic;
    if (c.temporal) {
        if (!hasPrev) ctx->tmpValid = false;  // (a Reserve below may let the old sets go: they were of another picture)
        for (auto& t : ctx->tmpSet)
            if ((rc = t.state.Reserve(npix * 4)) != RT_OK || (rc = t.guide[0].Reserve(npix * 4)) != RT_OK || (rc = t.guide[1].Reserve(npix * 4)) != RT_OK ||
                (rc = t.ids.Reserve(npix)) != RT_OK || (rc = t.len.Reserve(npix)) != RT_OK)
                return rc;
        if ((rc = ctx->tmpTarget.Reserve(npix)) != RT_OK) return rc;
    }
    rtdn::Job J{};
    rtdn::Strips& S = J.strips;
    int knob;
    // (the guide strips: the temporal pass writes its history's instead, unless a spatial pass writes them for it to read)
    if ((rc = DenoiseStrips(ctx, c.W, c.rows, !c.temporal || c.spatialRadius != 0, &S, &knob)) != RT_OK) return rc;
    S.hdr = c.hdr;
    S.sq = c.sq;
    S.feat = c.feat;
    S.n = c.n;
    S.m = c.m;
    J.parts = c.layout.nshards != 0 ? &c.layout : nullptr;
    J.spatialRadius = c.spatialRadius;
    J.committed = c.committed;
    rtdn::Temporal Q{};
    const uint32_t nxt = (ctx->tmpCur & 1u) ^ 1u;
    if (c.temporal) {
        Q.ids = c.ids;
        Q.geom = c.geom;
        Q.cam = c.cam;
        Q.camPrev = hasPrev ? ctx->tmpCam : Q.cam;
        Q.params = c.T;
        Q.fetch = c.fetch;
        Q.hasPrev = hasPrev;
        const auto setOf = [](rt_ctx::TemporalSet& t) { return rtdn::TemporalSet{t.state.ptr, {t.guide[0].ptr, t.guide[1].ptr}, t.ids.ptr, t.len.ptr}; };
        Q.prev = setOf(ctx->tmpSet[nxt ^ 1u]);
        Q.next = setOf(ctx->tmpSet[nxt]);
        Q.target = ctx->tmpTarget.ptr;
        J.temporal = &Q;
        ctx->tmpValid = false;  // the history is being rewritten, until everything is enqueued
    }
    if ((rc = DenoiseBegin(ctx, out_ms)) != RT_OK) return rc;
    if ((rc = DenoiseFinish(ctx, who, S, rtdn::Launch(ctx->stream, J, c.P, knob, ctx->denForms), out_ms)) != RT_OK || !c.temporal) return rc;
    ctx->tmpCur = nxt;
    ctx->tmpPic = c.pic;
    ctx->tmpCam = c.cam;
    ctx->tmpValid = true;
    return RT_OK;
}

// The context's own picture.  (spatialRadius: 0 -- the variance comes from the strip of second moments: the switch on, n >= 2 -- or the
// radius of the spatial source, which reads the picture itself: n >= 1, sq not read)
// (temporal: with the temporal step; fetch: which prepare kernel reads the history, and whose defaults tparams == NULL takes)
static int DescribePicture(rt_ctx* ctx, const char* who, const rt_denoise_params* params, uint32_t spatialRadius, bool temporal,
                           const rt_temporal_params* tparams, uint32_t fetch, DenoiseCall* c) {
    *c = DenoiseCall{};
    int rc = spatialRadius != 0 ? PictureReady(ctx, who) : NoiseReady(ctx, who, 2);
    if (rc != RT_OK || (rc = rtdn::CheckDenoiseParams(who, params, &c->P)) != RT_OK) return rc;
    if (temporal && (rc = rtdn::CheckTemporalParamsFetch(who, tparams, fetch, &c->T)) != RT_OK) return rc;
    if ((rc = DenoisePictureReady(ctx, who)) != RT_OK) return rc;
    c->W = ctx->seq.pic.W;
    c->rows = ctx->seq.rows;
    if (temporal) {
        c->temporal = true;
        c->pic = ctx->seq.pic;
        c->geom = rtd::TemporalGeom{c->pic.W, c->pic.H, c->pic.rs.first_row, ctx->seq.rows};
        if (!rtd::temporal_geom_ok(c->geom) || ctx->seq.rows != c->pic.rs.num_rows)
            return Fail(RT_ERR_INVALID_ARG, std::string(who) + ": a picture wider or taller than 2^24, or a strip that is not its row range");
        c->ids = ctx->featIds.ptr;
        const rtd::TraceParams& b = ctx->base;
        rtd::temporal_cam(b.cam_o, b.cam_x, b.cam_y, b.cam_oip, c->cam);
        c->fetch = fetch;
    }
    c->hdr = ctx->hdr.ptr;
    c->sq = spatialRadius != 0 ? nullptr : ctx->sq.ptr;
    c->feat = ctx->feat.ptr;
    c->n = ctx->seq.accumulated;
    c->m = ctx->featCount;
    c->spatialRadius = spatialRadius;
    c->committed = spatialRadius != 0 ? CommittedWord(ctx) : nullptr;
    return RT_OK;
}

// The gathered parts of a row-sharded picture; only the denoiser's own strips of the context (and the history) are touched.  With the
// temporal step the caller passes its frame and no parts: the frame's parts are then the parts, and it brings what DescribePicture takes
// from the context -- the ids, the image's height, the camera; the history is keyed with the parts' row set, shard 0: a contiguous call's
// key where nshards == 1.  (Neither: "null argument", the refusal of both checks for a missing record.)
// (spatialRadius: 0, or the radius of the spatial source, under which parts->sq is not looked at and n >= 1 is enough; the parts are a
// snapshot with their own n, so there is no committed word)
static int DescribeParts(rt_ctx* ctx, const char* who, const rt_shard_parts* parts, const rt_shard_frame* frame, const rt_denoise_params* params,
                         uint32_t spatialRadius, const rt_temporal_params* tparams, uint32_t fetch, DenoiseCall* c) {
    if (!ctx) return Fail(RT_ERR_INVALID_ARG, std::string(who) + ": null ctx");
    *c = DenoiseCall{};
    const bool spatial = spatialRadius != 0;
    const int rc = frame ? rtdn::CheckShardFrame(who, frame, params, tparams, fetch, true, &c->P, &c->T, &c->geom, spatial)
                         : rtdn::CheckShardParts(who, parts, params, true, &c->P, spatial);
    if (rc != RT_OK) return rc;
    RT_HIP(hipSetDevice(ctx->device));
    if (frame) {
        parts = &frame->parts;
        c->temporal = true;
        c->pic = rtseq::PictureKey{parts->W, frame->H, parts->rs};
        c->pic.rs.shard = 0;
        c->ids = static_cast<const uint32_t*>(frame->ids);
        c->cam = rtdn::CamOf(frame->camera);
        c->fetch = fetch;
    }
    c->W = parts->W;
    c->rows = parts->rs.num_rows;
    c->hdr = static_cast<const float*>(parts->hdr);
    c->sq = spatial ? nullptr : static_cast<const float*>(parts->sq);
    c->feat = static_cast<const float*>(parts->feat);
    c->n = parts->n;
    c->m = parts->m;
    c->spatialRadius = spatialRadius;
    c->layout = rtdn::ShardLayout{parts->rows_max, parts->rs.block_rows, parts->rs.nshards};
    return RT_OK;
}

// The entry behind the five of the context's own picture.
static int DenoisePicture(rt_ctx* ctx, const char* who, const rt_denoise_params* params, uint32_t spatialRadius, bool temporal,
                          const rt_temporal_params* tparams, uint32_t fetch, double* out_ms) {
    DenoiseCall c;
    const int rc = DescribePicture(ctx, who, params, spatialRadius, temporal, tparams, fetch, &c);
    return rc != RT_OK ? rc : DenoiseRun(ctx, who, c, out_ms);
}

int rt_denoise(rt_ctx* ctx, const rt_denoise_params* params, double* out_ms) { return DenoisePicture(ctx, "rt_denoise", params, 0, false, nullptr, 0, out_ms); }

// rt_denoise with the variance source chosen: the moments source is rt_denoise.
int rt_denoise_variance(rt_ctx* ctx, const rt_denoise_params* params, const rt_variance_params* vparams, double* out_ms) {
    const char* who = "rt_denoise_variance";
    if (!ctx) return Fail(RT_ERR_INVALID_ARG, std::string(who) + ": null ctx");
    rtd::VarianceParams V{};
    const int rc = rtdn::CheckVarianceParams(who, vparams, &V);
    if (rc != RT_OK) return rc;
    if (V.source == rtd::kVarianceMoments) return rt_denoise(ctx, params, out_ms);
    return DenoisePicture(ctx, who, params, V.radius, false, nullptr, 0, out_ms);
}

int rt_denoise_shards(rt_ctx* ctx, const rt_shard_parts* parts, const rt_denoise_params* params, double* out_ms) {
    DenoiseCall c;
    const int rc = DescribeParts(ctx, "rt_denoise_shards", parts, nullptr, params, 0, nullptr, 0, &c);
    return rc != RT_OK ? rc : DenoiseRun(ctx, "rt_denoise_shards", c, out_ms);
}

// rt_denoise_shards with the variance source chosen: the moments source is rt_denoise_shards.
int rt_denoise_shards_variance(rt_ctx* ctx, const rt_shard_parts* parts, const rt_denoise_params* params, const rt_variance_params* vparams, double* out_ms) {
    const char* who = "rt_denoise_shards_variance";
    if (!ctx) return Fail(RT_ERR_INVALID_ARG, std::string(who) + ": null ctx");
    rtd::VarianceParams V{};
    int rc = rtdn::CheckVarianceParams(who, vparams, &V);
    if (rc != RT_OK) return rc;
    if (V.source == rtd::kVarianceMoments) return rt_denoise_shards(ctx, parts, params, out_ms);
    DenoiseCall c;
    rc = DescribeParts(ctx, who, parts, nullptr, params, V.radius, nullptr, 0, &c);
    return rc != RT_OK ? rc : DenoiseRun(ctx, who, c, out_ms);
}

// rt_denoise with the temporal step in its prepare pass (rt_temporal.h) ...
int rt_denoise_temporal(rt_ctx* ctx, const rt_denoise_params* params, const rt_temporal_params* tparams, double* out_ms) {
    return DenoisePicture(ctx, "rt_denoise_temporal", params, 0, true, tparams, RT_TEMPORAL_FETCH_NEAREST, out_ms);
}

// ... with the way the history is fetched chosen: 1 runs the nearest kernel, 4 the bilinear one; the history is one state ...
int rt_denoise_temporal_fetch(rt_ctx* ctx, const rt_denoise_params* params, const rt_temporal_params* tparams, uint32_t fetch, double* out_ms) {
    return DenoisePicture(ctx, "rt_denoise_temporal_fetch", params, 0, true, tparams, fetch, out_ms);
}

// ... and with the variance source chosen: the moments source is the entry above.
int rt_denoise_temporal_variance(rt_ctx* ctx, const rt_denoise_params* params, const rt_temporal_params* tparams, uint32_t fetch,
                                 const rt_variance_params* vparams, double* out_ms) {
    const char* who = "rt_denoise_temporal_variance";
    if (!ctx) return Fail(RT_ERR_INVALID_ARG, std::string(who) + ": null ctx");
    rtd::VarianceParams V{};
    const int rc = rtdn::CheckVarianceParams(who, vparams, &V);
    if (rc != RT_OK) return rc;
    if (V.source == rtd::kVarianceMoments) return rt_denoise_temporal_fetch(ctx, params, tparams, fetch, out_ms);
    return DenoisePicture(ctx, who, params, V.radius, true, tparams, fetch, out_ms);
}

int rt_denoise_shards_temporal(rt_ctx* ctx, const rt_shard_frame* frame, const rt_denoise_params* params, const rt_temporal_params* tparams, uint32_t fetch,
                               double* out_ms) {
    DenoiseCall c;
    const int rc = DescribeParts(ctx, "rt_denoise_shards_temporal", nullptr, frame, params, 0, tparams, fetch, &c);
    return rc != RT_OK ? rc : DenoiseRun(ctx, "rt_denoise_shards_temporal", c, out_ms);
}

// ... and with the variance source chosen: the moments source is the entry above.
int rt_denoise_shards_temporal_variance(rt_ctx* ctx, const rt_shard_frame* frame, const rt_denoise_params* params, const rt_temporal_params* tparams,
                                        uint32_t fetch, const rt_variance_params* vparams, double* out_ms) {
    const char* who = "rt_denoise_shards_temporal_variance";
    if (!ctx) return Fail(RT_ERR_INVALID_ARG, std::string(who) + ": null ctx");
    rtd::VarianceParams V{};
    int rc = rtdn::CheckVarianceParams(who, vparams, &V);
    if (rc != RT_OK) return rc;
    if (V.source == rtd::kVarianceMoments) return rt_denoise_shards_temporal(ctx, frame, params, tparams, fetch, out_ms);
    DenoiseCall c;
    rc = DescribeParts(ctx, who, nullptr, frame, params, V.radius, tparams, fetch, &c);
    return rc != RT_OK ? rc : DenoiseRun(ctx, who, c, out_ms);
}

int rt_temporal_reset(rt_ctx* ctx) {
    if (!ctx) return Fail(RT_ERR_INVALID_ARG, "rt_temporal_reset: null ctx");
    ctx->tmpValid = false;
    return RT_OK;
}

// Empties the history of the pixels that hold one of the ids (rt_edit.hip, ../rt_forget.h): stream-ordered, no host wait but the
// staging's, and that only for more than kForgetInlineIds ids.  Needs no scene: ids are then bounded by what a scene can hold.
int rt_temporal_forget(rt_ctx* ctx, const uint32_t* ids, uint32_t n_ids) {
    if (!ctx || (!ids && n_ids != 0)) return Fail(RT_ERR_INVALID_ARG, "rt_temporal_forget: null argument");
    if (n_ids == 0 || !ctx->tmpValid) return RT_OK;
    const uint32_t nSpheres = ctx->seq.hasScene ? ctx->scene.n : rtscene::kForgetMaxIds;
    rtedit::ForgetPlan P = rtedit::PlanForget(ids, n_ids, nSpheres < rtscene::kForgetMaxIds ? nSpheres : rtscene::kForgetMaxIds);
    if (P.nothing) return RT_OK;
    RT_HIP(hipSetDevice(ctx->device));
    const size_t npix = (size_t)ctx->tmpPic.W * ctx->tmpPic.rs.num_rows;
    if (npix > 0x7fffffffull) return Fail(RT_ERR_INVALID_ARG, "rt_temporal_forget: a history of more than 2^31 pixels");
    if (!P.table.empty()) {
        if (const int rc = StageCopy(ctx, rtscene::PlanForgetStage(P.table, DestOf(ctx->forgetBits)))) return rc;
        P.set.bits = ctx->forgetBits.ptr;
    }
    const rt_ctx::TemporalSet& t = ctx->tmpSet[ctx->tmpCur & 1u];
    RT_HIP((hipError_t)rtedit::LaunchTemporalForget(ctx->stream, t.len.ptr, t.ids.ptr, (uint32_t)npix, P.set));
    return RT_OK;
}

int rt_download_temporal(rt_ctx* ctx, float* state4, uint32_t* len, uint32_t* target) {
    if (!ctx) return Fail(RT_ERR_INVALID_ARG, "rt_download_temporal: null ctx");
    if (!ctx->tmpValid) return Fail(RT_ERR_SEQUENCE, "rt_download_temporal: the history is empty");
    RT_HIP(hipSetDevice(ctx->device));
    const size_t npix = (size_t)ctx->tmpPic.W * ctx->tmpPic.rs.num_rows;
    const rt_ctx::TemporalSet& t = ctx->tmpSet[ctx->tmpCur & 1u];
    return CopyStrips(ctx, false, {{state4, t.state.ptr, npix * 4 * sizeof(float)}, {len, t.len.ptr, npix * sizeof(uint32_t)},
                                   {target, ctx->tmpTarget.ptr, npix * sizeof(uint32_t)}});
}

static int ReadDenoised(rt_ctx* ctx, const char* who, bool toDevice, void* rgb, void* var, void* ldr) {
    if (!ctx) return Fail(RT_ERR_INVALID_ARG, std::string(who) + ": null ctx");
    if (!ctx->denValid) return Fail(RT_ERR_SEQUENCE, std::string(who) + ": nothing denoised");
    RT_HIP(hipSetDevice(ctx->device));
    const size_t npix = (size_t)ctx->denW * ctx->denRows;
    return CopyStrips(ctx, toDevice, {{rgb, ctx->den.ptr, npix * 3 * sizeof(float)}, {var, ctx->denVar.ptr, npix * sizeof(float)}, {ldr, ctx->denLdr.ptr, npix * 3}});
}
int rt_download_denoised(rt_ctx* ctx, float* rgb, float* var, uint8_t* ldr) { return ReadDenoised(ctx, "rt_download_denoised", false, rgb, var, ldr); }
int rt_copy_denoised_to_device(rt_ctx* ctx, void* dev_rgb, void* dev_var, void* dev_ldr) {
    return ReadDenoised(ctx, "rt_copy_denoised_to_device", true, dev_rgb, dev_var, dev_ldr);
}

int rt_unit_denoise_forms(rt_ctx* ctx, uint32_t out[5]) {
    if (!ctx || !out) return Fail(RT_ERR_INVALID_ARG, "rt_unit_denoise_forms: null argument");
    for (uint32_t l = 0; l < rtd::kDenoiseMaxLevels; ++l) out[l] = ctx->denValid ? ctx->denForms[l] : 0u;
    return RT_OK;
}

int rt_synchronize(rt_ctx* ctx) {
    if (!ctx) return Fail(RT_ERR_INVALID_ARG, "rt_synchronize: null ctx");
    RT_HIP(hipSetDevice(ctx->device));
    int rcf = BatchFlush(ctx);  // pending frames are rendered,
    if (rcf != RT_OK) return rcf;
    rcf = PipelineFlush(ctx);  // frames in flight are finished and committed first
    if (rcf != RT_OK) return rcf;
    RT_HIP(hipStreamSynchronize(ctx->stream));
    return RT_OK;
}

// ------------------------------------------------------------------------ unit entries
int rt_unit_halton(rt_ctx* ctx, const uint32_t* index, uint32_t base, uint32_t n, float* out) {
    if (!ctx || !index || !out || base < 2) return Fail(RT_ERR_INVALID_ARG, "rt_unit_halton: invalid argument");
    if (n == 0) return RT_OK;
    RT_HIP(hipSetDevice(ctx->device));
    DevBuf<uint32_t> dIdx;
    DevBuf<float> dOut;
    int rc;
    if ((rc = dIdx.UploadFrom(index, n)) != RT_OK || (rc = dOut.Reserve(n)) != RT_OK) return rc;
    hipLaunchKernelGGL(rtd::k_unit_halton, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, dIdx.ptr, base, n, dOut.ptr);
    RT_HIP(hipGetLastError());
    return dOut.DownloadTo(out, n, ctx->stream);
}

int rt_unit_math(rt_ctx* ctx, uint32_t op, const float* x, const float* y, uint32_t n, float* out) {
    if (!ctx || !x || !out || op > 9) return Fail(RT_ERR_INVALID_ARG, "rt_unit_math: invalid argument");
    if (n == 0) return RT_OK;
    RT_HIP(hipSetDevice(ctx->device));
    DevBuf<float> dX, dY, dOut;
    int rc;
    if ((rc = dX.UploadFrom(x, n)) != RT_OK || (rc = y ? dY.UploadFrom(y, n) : dY.Reserve(n)) != RT_OK || (rc = dOut.Reserve(n)) != RT_OK) return rc;
    if (!y) RT_HIP(hipMemset(dY.ptr, 0, n * sizeof(float)));
    hipLaunchKernelGGL(rtd::k_unit_math, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, op, dX.ptr, dY.ptr, n, dOut.ptr);
    RT_HIP(hipGetLastError());
    return dOut.DownloadTo(out, n, ctx->stream);
}

int rt_unit_primary_rays(rt_ctx* ctx, uint32_t W, uint32_t H, const uint32_t* ijs, uint32_t n, float* out_rays) {
    if (!ctx || !ijs || !out_rays || W == 0 || H == 0) return Fail(RT_ERR_INVALID_ARG, "rt_unit_primary_rays: invalid argument");
    if (!ctx->seq.hasScene) return Fail(RT_ERR_NO_SCENE, "rt_unit_primary_rays: no scene uploaded");
    if (n == 0) return RT_OK;
    RT_HIP(hipSetDevice(ctx->device));
    DevBuf<uint32_t> dIjs;
    DevBuf<float> dOut;
    int rc;
    if ((rc = dIjs.UploadFrom(ijs, (size_t)n * 3)) != RT_OK || (rc = dOut.Reserve((size_t)n * 6)) != RT_OK) return rc;
    rtd::TraceParams tp = ctx->base;
    tp.W = W;
    tp.H = H;
    tp.sampler = ctx->sampler;
    hipLaunchKernelGGL(rtd::k_unit_primary, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, tp, dIjs.ptr, n, dOut.ptr);
    RT_HIP(hipGetLastError());
    return dOut.DownloadTo(out_rays, (size_t)n * 6, ctx->stream);
}

int rt_unit_closest_hit(rt_ctx* ctx, const float* rays, uint32_t n, float* out_hits) {
    if (!ctx || !rays || !out_hits) return Fail(RT_ERR_INVALID_ARG, "rt_unit_closest_hit: invalid argument");
    if (!ctx->seq.hasScene) return Fail(RT_ERR_NO_SCENE, "rt_unit_closest_hit: no scene uploaded");
    if (n == 0) return RT_OK;
    RT_HIP(hipSetDevice(ctx->device));
    DevBuf<float> dRays, dOut;
    int rc;
    if ((rc = dRays.UploadFrom(rays, (size_t)n * 6)) != RT_OK || (rc = dOut.Reserve((size_t)n * 10)) != RT_OK) return rc;
    if ((rc = LaunchClosest(ctx, dRays.ptr, n, dOut.ptr)) != RT_OK) return rc;
    return dOut.DownloadTo(out_hits, (size_t)n * 10, ctx->stream);
}

int rt_unit_trace(rt_ctx* ctx, uint32_t W, uint32_t H, const uint32_t* ijs, uint32_t n, uint32_t max_depth, uint64_t seed,
                  float* out_rgb, uint32_t* out_traversals) {
    if (!ctx || !ijs || !out_rgb || W == 0 || H == 0) return Fail(RT_ERR_INVALID_ARG, "rt_unit_trace: invalid argument");
    if (!ctx->seq.hasScene) return Fail(RT_ERR_NO_SCENE, "rt_unit_trace: no scene uploaded");
    if (n == 0) return RT_OK;
    RT_HIP(hipSetDevice(ctx->device));
    DevBuf<uint32_t> dIjs, dTrav;
    DevBuf<float> dOut;
    int rc;
    if ((rc = dIjs.UploadFrom(ijs, (size_t)n * 3)) != RT_OK || (rc = dTrav.Reserve(n)) != RT_OK || (rc = dOut.Reserve((size_t)n * 3)) != RT_OK) return rc;
    RT_HIP(hipMemsetAsync(ctx->counters.ptr, 0, 6 * sizeof(unsigned long long), ctx->stream));
    // the n listed paths as a "picture" of n pixels and one sample, over the whole image's rows
    rtd::TraceParams tp = PassParams(ctx, rtseq::PictureKey{W, H, rt_rowset{0, H, H, 0, 1}}, 1, 1, n, max_depth, seed);
    tp.path_list = dIjs.ptr;
    tp.samples = dOut.ptr;
    tp.trav_out = dTrav.ptr;
    if ((rc = LaunchTrace(ctx, tp)) != RT_OK) return rc;
    if ((rc = dOut.DownloadTo(out_rgb, (size_t)n * 3, ctx->stream)) != RT_OK) return rc;
    return out_traversals ? dTrav.DownloadTo(out_traversals, n, ctx->stream) : RT_OK;
}

int rt_unit_camera_rays(rt_ctx* ctx, const rt_camera* camera, const float* uv_offset, uint32_t n, float* out_rays) {
    if (!ctx || !camera || !uv_offset || !out_rays) return Fail(RT_ERR_INVALID_ARG, "rt_unit_camera_rays: invalid argument");
    if (n == 0) return RT_OK;
    RT_HIP(hipSetDevice(ctx->device));
    DevBuf<float> dIn, dOut;
    int rc;
    if ((rc = dIn.UploadFrom(uv_offset, (size_t)n * 4)) != RT_OK || (rc = dOut.Reserve((size_t)n * 6)) != RT_OK) return rc;
    rtd::TraceParams tp{};
    SetCamera(tp, *camera);
    hipLaunchKernelGGL(rtd::k_unit_camera, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, tp, dIn.ptr, n, dOut.ptr);
    RT_HIP(hipGetLastError());
    return dOut.DownloadTo(out_rays, (size_t)n * 6, ctx->stream);
}

int rt_unit_scatter(rt_ctx* ctx, const rt_material* material, const rt_light* sun, const float view_origin[3], const float* in,
                    uint32_t n, float* out) {
    if (!ctx || !material || !sun || !view_origin || !in || !out) return Fail(RT_ERR_INVALID_ARG, "rt_unit_scatter: invalid argument");
    if (const char* field = rtprep::MaterialFault(*material)) return Fail(RT_ERR_INVALID_ARG, rtprep::MaterialFaultMessage("rt_unit_scatter", "the record", *material, field));
    if (n == 0) return RT_OK;
    RT_HIP(hipSetDevice(ctx->device));
    DevBuf<float> dIn, dOut;
    DevBuf<rt_material> dMat;
    int rc;
    if ((rc = dIn.UploadFrom(in, (size_t)n * 12)) != RT_OK || (rc = dMat.UploadFrom(material, 1)) != RT_OK || (rc = dOut.Reserve((size_t)n * 11)) != RT_OK) return rc;
    rtd::TraceParams tp{};
    for (int k = 0; k < 3; ++k) tp.cam_o[k] = view_origin[k];
    SetLight(tp, *sun);
    tp.sampler = ctx->sampler;
    hipLaunchKernelGGL(rtd::k_unit_scatter, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, tp, dMat.ptr, dIn.ptr, n, dOut.ptr);
    RT_HIP(hipGetLastError());
    return dOut.DownloadTo(out, (size_t)n * 11, ctx->stream);
}

int rt_unit_tonemap(rt_ctx* ctx, const float* hdr_rgb, uint32_t n, uint32_t n_samples, uint8_t* out_rgb) {
    if (!ctx || !hdr_rgb || !out_rgb || n_samples == 0) return Fail(RT_ERR_INVALID_ARG, "rt_unit_tonemap: invalid argument");
    if (n == 0) return RT_OK;
    RT_HIP(hipSetDevice(ctx->device));
    DevBuf<float> dIn;
    DevBuf<uint8_t> dOut;
    int rc;
    if ((rc = dIn.UploadFrom(hdr_rgb, (size_t)n * 3)) != RT_OK || (rc = dOut.Reserve((size_t)n * 3)) != RT_OK) return rc;
    hipLaunchKernelGGL(rtd::k_unit_tonemap, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, dIn.ptr, n, n_samples, dOut.ptr);
    RT_HIP(hipGetLastError());
    return dOut.DownloadTo(out_rgb, (size_t)n * 3, ctx->stream);
}

// Host-only: the grid walk's row computation, the SAME functions the kernels call (rt_scan.h; RT_DEV is __host__ __device__).
int rt_unit_grid_rows(const float* segments, const int32_t* iu, uint32_t n, int32_t nv, int32_t* out_rows, float* out_s_enter) {
    if (!segments || !iu || !out_rows || nv <= 0) return Fail(RT_ERR_INVALID_ARG, "rt_unit_grid_rows: invalid argument");
    for (uint32_t k = 0; k < n; ++k) {
        const float* q = segments + 5 * (size_t)k;
        float slope, invAbsDu, sEnter;
        rtd::grid_segment_slope(q[0], q[1], q[2], q[3], slope, invAbsDu);
        int r0, r1;
        rtd::grid_slab_rows(q[0], q[1], q[2], q[3], q[4], slope, invAbsDu, (int)iu[k], (int)nv, r0, r1, sEnter);
        out_rows[2 * k] = r0;
        out_rows[2 * k + 1] = r1;
        if (out_s_enter) out_s_enter[k] = sEnter;
    }
    return RT_OK;
}

// Host-only: the scene as rt_scene_upload prepares it under the environment of the moment (materials play no part in the index).
static int PrepareForShadow(const char* who, const rt_sphere* spheres, uint32_t n, const rt_light* lights, uint32_t n_lights, uint32_t light,
                            rtprep::PreparedScene& P) {
    if (!spheres || n == 0 || !lights || n_lights == 0 || n_lights > RT_MAX_LIGHTS || light >= n_lights)
        return Fail(RT_ERR_INVALID_ARG, std::string(who) + ": invalid argument");
    if (!rtprep::AllFinite(spheres, n, nullptr)) return Fail(RT_ERR_INVALID_ARG, std::string(who) + ": a sphere's centre or radius is not finite");
    const std::vector<rt_material> mats(n, rt_material{});
    P = rtprep::PrepareScene(spheres, mats.data(), n, lights, n_lights, rtprep::PrepOptions::FromEnv());
    if (P.layout.scan.size() >= 65536) return Fail(RT_ERR_INVALID_ARG, std::string(who) + ": scenes beyond 65,535 scan entries are not supported");
    return RT_OK;
}

int rt_unit_launch_plan(const uint32_t* cases, uint32_t n, uint32_t* plans) {
    if ((!cases || !plans) && n != 0) return Fail(RT_ERR_INVALID_ARG, "rt_unit_launch_plan: invalid argument");
    for (uint32_t k = 0; k < n; ++k)
        if (rtplan::PlanPacked(cases + (size_t)k * rtplan::kCaseWords, plans + (size_t)k * rtplan::kPlanWords) != RT_OK)
            return Fail(RT_ERR_INVALID_ARG, "rt_unit_launch_plan: case " + std::to_string(k) + " describes no context or scene there can be");
    return RT_OK;
}

int rt_unit_last_trace_launch(rt_ctx* ctx, uint32_t case_words[28], uint32_t plan_words[28], uint32_t* launches) {
    static_assert(rtplan::kCaseWords == 28 && rtplan::kPlanWords == 28, "the words of rt_unit_launch_plan");
    if (!ctx) return Fail(RT_ERR_INVALID_ARG, "rt_unit_last_trace_launch: invalid argument");
    if (launches) *launches = ctx->traceLaunches;
    if (ctx->traceLaunches == 0) return Fail(RT_ERR_SEQUENCE, "rt_unit_last_trace_launch: this context has launched no trace kernel");
    if (case_words) std::memcpy(case_words, ctx->lastCaseWords, sizeof(ctx->lastCaseWords));
    if (plan_words) std::memcpy(plan_words, ctx->lastPlanWords, sizeof(ctx->lastPlanWords));
    return RT_OK;
}

int rt_unit_trace_variants(uint32_t* kernel_words, uint32_t cap, uint32_t* n) {
    if (!n || (!kernel_words && cap != 0)) return Fail(RT_ERR_INVALID_ARG, "rt_unit_trace_variants: invalid argument");
    *n = (uint32_t)rtplan::kTraceVariantCount;
    if (cap == 0) return RT_OK;
    if (cap < *n) return Fail(RT_ERR_INVALID_ARG, "rt_unit_trace_variants: capacity too small");
    for (int r = 0; r < rtplan::kTraceVariantCount; ++r) kernel_words[r] = rtplan::KernelWord(rtplan::kTraceVariants[r]);
    return RT_OK;
}

int rt_unit_last_trace_far_state(rt_ctx* ctx, uint32_t* lean) {
    if (!ctx || !lean) return Fail(RT_ERR_INVALID_ARG, "rt_unit_last_trace_far_state: invalid argument");
    if (ctx->traceLaunches == 0) return Fail(RT_ERR_SEQUENCE, "rt_unit_last_trace_far_state: this context has launched no trace kernel");
    *lean = ctx->lastTraceLean ? 1u : 0u;
    return RT_OK;
}

int rt_unit_trace_lean_variants(uint32_t* kernel_words, uint32_t cap, uint32_t* n) {
    if (!n || (!kernel_words && cap != 0)) return Fail(RT_ERR_INVALID_ARG, "rt_unit_trace_lean_variants: invalid argument");
    *n = (uint32_t)rtplan::kTraceLeanVariantCount;
    if (cap == 0) return RT_OK;
    if (cap < *n) return Fail(RT_ERR_INVALID_ARG, "rt_unit_trace_lean_variants: capacity too small");
    for (int r = 0; r < rtplan::kTraceLeanVariantCount; ++r) kernel_words[r] = rtplan::KernelWord(rtplan::kTraceLeanVariants[r]);
    return RT_OK;
}

int rt_unit_far_state_plan(const uint32_t* case_words, uint32_t path_list, uint32_t trav_out, uint32_t shadow_grid, uint32_t force_full, uint32_t* lean) {
    if (!case_words || !lean) return Fail(RT_ERR_INVALID_ARG, "rt_unit_far_state_plan: invalid argument");
    uint32_t plan[rtplan::kPlanWords];
    if (rtplan::PlanPacked(case_words, plan) != RT_OK) return Fail(RT_ERR_INVALID_ARG, "rt_unit_far_state_plan: the case describes no context or scene there can be");
    rtplan::FarStateAsk F;
    F.pathList = path_list != 0u, F.travOut = trav_out != 0u, F.shadowGrid = shadow_grid != 0u, F.forceFull = force_full != 0u;
    *lean = rtplan::FarStateLeanPacked(case_words, F) ? 1u : 0u;
    return RT_OK;
}

// which of light `light`'s indices: tier 1 = the index of rt_unit_shadow_index_host, tier 2 = light 0's second index
static const rtprep::ShadowGrid* ShadowTier(const char* who, const rtprep::PreparedScene& P, uint32_t light, uint32_t tier) {
    if (tier == 1u) return light == 0u ? &P.shadow : &P.extraShadow[light - 1u];
    if (tier == 2u && light == 0u) return &P.shadowFar;
    Fail(RT_ERR_INVALID_ARG, std::string(who) + ": tier 2 exists for light 0 only; tiers are 1 and 2");
    return nullptr;
}

int rt_unit_shadow_index_host(const rt_sphere* spheres, uint32_t n, const rt_light* lights, uint32_t n_lights, uint32_t light, uint32_t out_u[8],
                              float out_f[10], uint32_t cap_cells, uint16_t* cell_start, uint32_t cap_entries, uint16_t* entries,
                              uint32_t cap_global, uint16_t* global, uint32_t cap_orig, uint32_t* orig) {
    return rt_unit_shadow_index_host_tier(spheres, n, lights, n_lights, light, 1u, out_u, out_f, cap_cells, cell_start, cap_entries, entries, cap_global,
                                          global, cap_orig, orig);
}

int rt_unit_shadow_index_host_tier(const rt_sphere* spheres, uint32_t n, const rt_light* lights, uint32_t n_lights, uint32_t light, uint32_t tier,
                                   uint32_t out_u[8], float out_f[10], uint32_t cap_cells, uint16_t* cell_start, uint32_t cap_entries, uint16_t* entries,
                                   uint32_t cap_global, uint16_t* global, uint32_t cap_orig, uint32_t* orig) {
    if (!out_u || !out_f) return Fail(RT_ERR_INVALID_ARG, "rt_unit_shadow_index_host: invalid argument");
    rtprep::PreparedScene P;
    if (const int rc = PrepareForShadow("rt_unit_shadow_index_host", spheres, n, lights, n_lights, light, P)) return rc;
    const rtprep::ShadowGrid* Gp = ShadowTier("rt_unit_shadow_index_host_tier", P, light, tier);
    if (!Gp) return RT_ERR_INVALID_ARG;
    const rtprep::ShadowGrid& G = *Gp;
    const std::vector<uint32_t>& O = P.layout.orig;
    out_u[0] = G.enabled ? 1u : 0u;
    out_u[1] = G.nx; out_u[2] = G.ny;
    out_u[3] = (uint32_t)G.cellStart.size(); out_u[4] = (uint32_t)G.entries.size(); out_u[5] = (uint32_t)G.global.size();
    out_u[6] = (uint32_t)O.size();
    out_u[7] = P.layout.InGlobalMemory() ? 1u : 0u;
    for (int k = 0; k < 3; ++k) {
        out_f[k] = G.e1[k];
        out_f[3 + k] = G.e2[k];
    }
    out_f[6] = G.u0; out_f[7] = G.v0; out_f[8] = G.invCell; out_f[9] = G.p0sq;
    if ((cell_start && cap_cells < G.cellStart.size()) || (entries && cap_entries < G.entries.size()) || (global && cap_global < G.global.size()) ||
        (orig && cap_orig < O.size()))
        return Fail(RT_ERR_INVALID_ARG, "rt_unit_shadow_index_host: capacity too small");
    if (cell_start && !G.cellStart.empty()) std::memcpy(cell_start, G.cellStart.data(), G.cellStart.size() * sizeof(uint16_t));
    if (entries && !G.entries.empty()) std::memcpy(entries, G.entries.data(), G.entries.size() * sizeof(uint16_t));
    if (global && !G.global.empty()) std::memcpy(global, G.global.data(), G.global.size() * sizeof(uint16_t));
    if (orig && !O.empty()) std::memcpy(orig, O.data(), O.size() * sizeof(uint32_t));
    return RT_OK;
}

// Host-only: rt_shade.h's shadow_query and any_hit_all themselves (RT_DEV is __host__ __device__), asked as rt_kernels.h's hit
// processing asks them -- light 0 through the scene constants fill_consts makes of the launch parameters, lights 1 .. through
// their LightRec -- over the prepared tables where they lie on the host.
int rt_unit_shadow_query_host(const rt_sphere* spheres, uint32_t n, const rt_light* lights, uint32_t n_lights, uint32_t light,
                              const float* points, uint32_t n_points, uint8_t* out) {
    return rt_unit_shadow_query_host_tier(spheres, n, lights, n_lights, light, 1u, points, n_points, out);
}

// tier 2 (light 0): the question as the kernels without far-hit state ask it (rt_kernels.h farShadow): a point beyond the first index
// is answered by the second one within its radius (bit 2 set, bit 1 clear), else by the any-hit over every entry
int rt_unit_shadow_query_host_tier(const rt_sphere* spheres, uint32_t n, const rt_light* lights, uint32_t n_lights, uint32_t light, uint32_t tier,
                                   const float* points, uint32_t n_points, uint8_t* out) {
    if ((!points || !out) && n_points != 0) return Fail(RT_ERR_INVALID_ARG, "rt_unit_shadow_query_host: invalid argument");
    rtprep::PreparedScene P;
    if (const int rc = PrepareForShadow("rt_unit_shadow_query_host", spheres, n, lights, n_lights, light, P)) return rc;
    if (!ShadowTier("rt_unit_shadow_query_host_tier", P, light, tier)) return RT_ERR_INVALID_ARG;
    const rtprep::ShadowGrid& FG = P.shadowFar;
    rtd::LightRec FR{};
    if (tier == 2u && FG.enabled) {
        SetShadowGrid(FR, FG);
        FR.cell_start = FG.cellStart.data();
        FR.entries = FG.entries.empty() ? FG.cellStart.data() : FG.entries.data();  // (an empty list is never read: any address)
        FR.global = FG.global.empty() ? FG.cellStart.data() : FG.global.data();
    }
    const rtprep::ShadowGrid& G = light == 0u ? P.shadow : P.extraShadow[light - 1u];
    const float4* scanTab = reinterpret_cast<const float4*>(P.layout.scan.data());
    const uint32_t nPad = (uint32_t)P.layout.scan.size();
    const uint16_t none = 0;  // an empty list still has an address (UploadShadowGrid)
    const uint16_t* cells = G.cellStart.empty() ? &none : G.cellStart.data();
    const uint16_t* ents = G.entries.empty() ? &none : G.entries.data();
    const uint16_t* glob = G.global.empty() ? &none : G.global.data();
    rtd::TraceParams tp{};
    rtd::LightRec R{};
    SetLight(tp, lights[light]), SetLight(R, lights[light]);
    SetShadowGrid(tp, G), SetShadowGrid(R, G);  // (both forms, filled as rt_scene_upload fills them)
    R.cell_start = cells; R.entries = ents; R.global = glob;
    rtd::SceneConsts K;
    rtd::fill_consts(tp, K);
    const float4* entrySph = (light == 0u && !P.sgSph.empty()) ? reinterpret_cast<const float4*>(P.sgSph.data()) : nullptr;
    for (uint32_t k = 0; k < n_points; ++k) {
        const rtd::V3 pos = rtd::v3(points[3 * (size_t)k], points[3 * (size_t)k + 1], points[3 * (size_t)k + 2]);
        const float pp = rtd::dot3(pos, pos);
        bool useIndex, occ, useFar = false;
        if (light == 0u) {
            const rtd::V3 sunDir = rtd::v3(K.sun_dir[0], K.sun_dir[1], K.sun_dir[2]);
            const float aSun = rtd::dot3(sunDir, sunDir);
            useIndex = K.sg_enabled && pp <= K.sg_p0sq;
            useFar = !useIndex && FR.sg_enabled != 0u && pp <= FR.sg_p0sq;
            occ = useIndex ? rtd::shadow_query(K, scanTab, cells, ents, glob, false, (const float4*)nullptr, (const uint16_t*)nullptr, entrySph, pos, sunDir, aSun)
                  : useFar ? rtd::shadow_query(FR, scanTab, FR.cell_start, FR.entries, FR.global, false, (const float4*)nullptr, (const uint16_t*)nullptr,
                                               (const float4*)nullptr, pos, sunDir, aSun)
                           : rtd::any_hit_all(scanTab, nPad, pos, sunDir, aSun);
        } else {
            const rtd::LightRec& Lk = R;
            const rtd::V3 dirK = rtd::v3(Lk.sun_dir[0], Lk.sun_dir[1], Lk.sun_dir[2]);
            const float aK = rtd::dot3(dirK, dirK);
            useIndex = Lk.sg_enabled && pp <= Lk.sg_p0sq;
            occ = useIndex ? rtd::shadow_query(Lk, scanTab, Lk.cell_start, Lk.entries, Lk.global, false, (const float4*)nullptr, (const uint16_t*)nullptr,
                                               (const float4*)nullptr, pos, dirK, aK)
                           : rtd::any_hit_all(scanTab, nPad, pos, dirK, aK);
        }
        out[k] = (uint8_t)((occ ? 1u : 0u) | ((useIndex || useFar) ? 0u : 2u) | (useFar ? 4u : 0u));
    }
    return RT_OK;
}

int rt_unit_shadow(rt_ctx* ctx, uint32_t light, const float* points, uint32_t n, uint32_t glob_in_lds, uint8_t* out) {
    return rt_unit_shadow_tier(ctx, light, 1u, points, n, glob_in_lds, out);
}

int rt_unit_shadow_tier(rt_ctx* ctx, uint32_t light, uint32_t tier, const float* points, uint32_t n, uint32_t glob_in_lds, uint8_t* out) {
    if (!ctx || !points || !out) return Fail(RT_ERR_INVALID_ARG, "rt_unit_shadow: invalid argument");
    if (tier != 1u && !(tier == 2u && light == 0u)) return Fail(RT_ERR_INVALID_ARG, "rt_unit_shadow_tier: tier 2 exists for light 0 only; tiers are 1 and 2");
    if (!ctx->seq.hasScene) return Fail(RT_ERR_NO_SCENE, "rt_unit_shadow: no scene uploaded");
    if (light >= std::max(1u, ctx->base.n_lights)) return Fail(RT_ERR_INVALID_ARG, "rt_unit_shadow: the scene has no such light");
    if (n == 0) return RT_OK;
    RT_HIP(hipSetDevice(ctx->device));
    DevBuf<float> dIn;
    DevBuf<uint8_t> dOut;
    int rc;
    if ((rc = dIn.UploadFrom(points, (size_t)n * 3)) != RT_OK || (rc = dOut.Reserve(n)) != RT_OK) return rc;
    const size_t lds = (size_t)rtd::sg_glob_slots(64u) * 16;  // a global list has 64 entries at most (BuildShadowGrid)
    hipLaunchKernelGGL(rtd::k_unit_shadow, dim3((n + 255) / 256), dim3(256), lds, ctx->stream, ctx->base, light, glob_in_lds, dIn.ptr, n, dOut.ptr, tier);
    RT_HIP(hipGetLastError());
    return dOut.DownloadTo(out, n, ctx->stream);
}

int rt_unit_tile_masks(rt_ctx* ctx, uint32_t W, uint32_t H, rt_rowset rs, uint32_t cap_tiles, uint32_t* n_tiles, uint32_t* words,
                       uint32_t cap_spheres, uint32_t* group_of_sphere, uint64_t scans[2]) {
    if (!ctx || !n_tiles || W == 0 || H == 0) return Fail(RT_ERR_INVALID_ARG, "rt_unit_tile_masks: invalid argument");
    if (!ctx->seq.hasScene) return Fail(RT_ERR_NO_SCENE, "rt_unit_tile_masks: no scene uploaded");
    const uint32_t rows = rtprep::UnitStripRows(rs, W, H);
    if (rows == 0) return Fail(RT_ERR_INVALID_ARG, "rt_unit_tile_masks: bad row set");
    RT_HIP(hipSetDevice(ctx->device));
    int rc;
    if ((rc = BuildTileMasks(ctx, rtseq::PictureKey{W, H, rs}, W * rows, TileKnobsFromEnv())) != RT_OK) return rc;
    *n_tiles = rttile::MaskTiles(ctx->tiles);
    RT_HIP(hipStreamSynchronize(ctx->stream));
    if (words && *n_tiles != 0u) {
        if (cap_tiles < *n_tiles) return Fail(RT_ERR_INVALID_ARG, "rt_unit_tile_masks: capacity too small");
        RT_HIP(hipMemcpy(words, ctx->tileMasks.ptr, (size_t)*n_tiles * rtd::kTileMaskWords * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    if (group_of_sphere) {
        if (cap_spheres < ctx->scene.n) return Fail(RT_ERR_INVALID_ARG, "rt_unit_tile_masks: sphere capacity too small");
        std::vector<uint32_t> orig(ctx->base.n_padded);
        RT_HIP(hipMemcpy(orig.data(), ctx->orig.ptr, orig.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        rtprep::EntryOfSphere(orig.data(), orig.size(), ctx->scene.n, 2, group_of_sphere);  // flat scan: scan entry = 4 * group + member
    }
    if (scans) {
        unsigned long long c[4] = {0, 0, 0, 0};
        RT_HIP(hipMemcpy(c, ctx->counters.ptr, sizeof(c), hipMemcpyDeviceToHost));
        scans[0] = ctx->tileAcct.freshScans;  // host arithmetic: every block of 64 fresh paths of the last rt_render that launched
        scans[1] = c[3];
    }
    return RT_OK;
}

int rt_unit_tile_spheres(rt_ctx* ctx, uint32_t W, uint32_t H, rt_rowset rs, uint32_t cap_tiles, uint32_t* n_tiles, uint16_t* lists, uint64_t scans[3]) {
    if (!ctx || !n_tiles || W == 0 || H == 0) return Fail(RT_ERR_INVALID_ARG, "rt_unit_tile_spheres: invalid argument");
    if (!ctx->seq.hasScene) return Fail(RT_ERR_NO_SCENE, "rt_unit_tile_spheres: no scene uploaded");
    const uint32_t rows = rtprep::UnitStripRows(rs, W, H);
    if (rows == 0) return Fail(RT_ERR_INVALID_ARG, "rt_unit_tile_spheres: bad row set");
    RT_HIP(hipSetDevice(ctx->device));
    int rc;
    if ((rc = BuildTileMasks(ctx, rtseq::PictureKey{W, H, rs}, W * rows, TileKnobsFromEnv())) != RT_OK) return rc;
    *n_tiles = rttile::ListTiles(ctx->tiles);
    RT_HIP(hipStreamSynchronize(ctx->stream));
    if (lists && *n_tiles != 0u) {
        if (cap_tiles < *n_tiles) return Fail(RT_ERR_INVALID_ARG, "rt_unit_tile_spheres: capacity too small");
        RT_HIP(hipMemcpy(lists, ctx->tileSpheres.ptr, (size_t)*n_tiles * rtd::kTileSphereHalfs * sizeof(uint16_t), hipMemcpyDeviceToHost));
    }
    if (scans) {
        unsigned long long c[5] = {0, 0, 0, 0, 0};
        RT_HIP(hipMemcpy(c, ctx->counters.ptr, sizeof(c), hipMemcpyDeviceToHost));
        scans[0] = ctx->tileAcct.freshScans;
        scans[1] = c[3];
        scans[2] = c[4];
    }
    return RT_OK;
}

int rt_unit_tile_order_sort(rt_ctx* ctx, const uint8_t* classes, uint32_t n_tiles, uint32_t* order_out) {
    if (!ctx || !classes || !order_out || n_tiles == 0) return Fail(RT_ERR_INVALID_ARG, "rt_unit_tile_order_sort: invalid argument");
    for (uint32_t t = 0; t < n_tiles; ++t)
        if (classes[t] >= rtd::kTileClasses) return Fail(RT_ERR_INVALID_ARG, "rt_unit_tile_order_sort: tile " + std::to_string(t) + " has a class above 4");
    RT_HIP(hipSetDevice(ctx->device));
    constexpr size_t kGuard = 64;
    DevBuf<uint8_t> dCls;
    DevBuf<uint32_t> dOrder;
    int rc;
    if ((rc = dCls.UploadFrom(classes, n_tiles)) != RT_OK || (rc = dOrder.Reserve((size_t)n_tiles + kGuard)) != RT_OK) return rc;
    RT_HIP(hipMemsetAsync(dOrder.ptr, 0xff, ((size_t)n_tiles + kGuard) * sizeof(uint32_t), ctx->stream));
    hipLaunchKernelGGL(rtd::rt_tile_order_kernel, dim3(1), dim3(1024), 0, ctx->stream, dCls.ptr, n_tiles, dOrder.ptr);  // as LaunchTileOrder
    RT_HIP(hipGetLastError());
    return dOrder.DownloadTo(order_out, (size_t)n_tiles + kGuard, ctx->stream);
}

int rt_unit_tile_order(rt_ctx* ctx, uint32_t W, uint32_t H, rt_rowset rs, uint32_t source, uint32_t cap_tiles, uint32_t* n_tiles, float* pilot_rays,
                       uint8_t* classes, uint8_t* flags, uint32_t* order, uint32_t info[4]) {
    if (!ctx || !n_tiles || W == 0 || H == 0) return Fail(RT_ERR_INVALID_ARG, "rt_unit_tile_order: invalid argument");
    if (source > 1u) return Fail(RT_ERR_INVALID_ARG, "rt_unit_tile_order: source is 0 (build afresh) or 1 (the running accumulation's)");
    if (!ctx->seq.hasScene) return Fail(RT_ERR_NO_SCENE, "rt_unit_tile_order: no scene uploaded");
    const uint32_t rows = rtprep::UnitStripRows(rs, W, H);
    if (rows == 0) return Fail(RT_ERR_INVALID_ARG, "rt_unit_tile_order: bad row set");
    const rtseq::PictureKey pic{W, H, rs};
    const uint32_t nFull = (W * rows) >> 6, nPilot = nFull * rtd::kPilotsPerTile;
    const bool wanted = pilot_rays || classes || flags || order;
    RT_HIP(hipSetDevice(ctx->device));
    int rc;
    if (source == 1u) {
        const rttile::State::Order& o = ctx->tiles.order;
        const bool held = o.keyValid && o.orderValid && o.pic == pic && nFull != 0u;
        *n_tiles = held ? nFull : 0u;
        RT_HIP(hipStreamSynchronize(ctx->stream));
        if (!held) return RT_OK;
        if (wanted && cap_tiles < nFull) return Fail(RT_ERR_INVALID_ARG, "rt_unit_tile_order: capacity too small");
        if (pilot_rays) RT_HIP(hipMemcpy(pilot_rays, ctx->pilotRays.ptr, (size_t)nPilot * 6 * sizeof(float), hipMemcpyDeviceToHost));
        if (classes) RT_HIP(hipMemcpy(classes, ctx->tileClass.ptr, nFull, hipMemcpyDeviceToHost));
        if (order) RT_HIP(hipMemcpy(order, ctx->tileOrder.ptr, (size_t)nFull * sizeof(uint32_t), hipMemcpyDeviceToHost));
        if (flags) {
            if (o.flagsValid) RT_HIP(hipMemcpy(flags, ctx->skyFlags.ptr, nFull, hipMemcpyDeviceToHost));
            else std::memset(flags, 0, nFull);
        }
        if (info) {
            if (o.flagsValid) RT_HIP(hipMemcpy(info, ctx->skyInfo.ptr, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost));
            else std::memset(info, 0, 4 * sizeof(uint32_t));
        }
        return RT_OK;
    }
    // source 0: masks and lists as rt_unit_tile_spheres obtains them (the mask tables may be rebuilt for this picture), everything
    // else in buffers of this call's own: the kept order, flags and count, and rttile's account of them, are not touched.
    const rttile::Knobs knobs = TileKnobsFromEnv();
    if ((rc = BuildTileMasks(ctx, pic, W * rows, knobs)) != RT_OK) return rc;
    *n_tiles = nFull;
    if (nFull == 0u) {
        RT_HIP(hipStreamSynchronize(ctx->stream));
        return RT_OK;
    }
    if (wanted && cap_tiles < nFull) return Fail(RT_ERR_INVALID_ARG, "rt_unit_tile_order: capacity too small");
    const bool withFlags = rttile::ListTiles(ctx->tiles) != 0u && knobs.skipSky && knobs.excludeSky;
    DevBuf<float> dRays, dHits;
    DevBuf<uint8_t> dCls, dFlags;
    DevBuf<uint32_t> dOrder, dInfo;
    if ((rc = dRays.Reserve((size_t)nPilot * 6)) != RT_OK || (rc = dHits.Reserve((size_t)nPilot * 10)) != RT_OK || (rc = dCls.Reserve(nFull)) != RT_OK ||
        (rc = dOrder.Reserve(nFull)) != RT_OK || (rc = dFlags.Reserve(nFull)) != RT_OK || (rc = dInfo.Reserve(4)) != RT_OK)
        return rc;
    if (!withFlags) {  // no flags: the outputs read 0
        RT_HIP(hipMemsetAsync(dFlags.ptr, 0, nFull, ctx->stream));
        RT_HIP(hipMemsetAsync(dInfo.ptr, 0, 4 * sizeof(uint32_t), ctx->stream));
    }
    TileOrderDest dst;
    dst.pilotRays = dRays.ptr, dst.pilotHits = dHits.ptr, dst.cls = dCls.ptr, dst.order = dOrder.ptr, dst.flags = dFlags.ptr, dst.info = dInfo.ptr;
    rc = LaunchTileOrder(ctx, pic, nFull, withFlags, true, ctx->tileSpheres.ptr, dst);
    RT_HIP(hipStreamSynchronize(ctx->stream));  // (also after a failed launch: the buffers are freed at the return)
    if (rc != RT_OK) return rc;
    if (pilot_rays) RT_HIP(hipMemcpy(pilot_rays, dRays.ptr, (size_t)nPilot * 6 * sizeof(float), hipMemcpyDeviceToHost));
    if (classes) RT_HIP(hipMemcpy(classes, dCls.ptr, nFull, hipMemcpyDeviceToHost));
    if (flags) RT_HIP(hipMemcpy(flags, dFlags.ptr, nFull, hipMemcpyDeviceToHost));
    if (order) RT_HIP(hipMemcpy(order, dOrder.ptr, (size_t)nFull * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (info) RT_HIP(hipMemcpy(info, dInfo.ptr, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_unit_sky_planes(rt_ctx* ctx, uint64_t* planes) {
    if (!ctx || !planes) return Fail(RT_ERR_INVALID_ARG, "rt_unit_sky_planes: invalid argument");
    RT_HIP(hipSetDevice(ctx->device));
    RT_HIP(hipStreamSynchronize(ctx->stream));
    unsigned long long c[6] = {0, 0, 0, 0, 0, 0};
    RT_HIP(hipMemcpy(c, ctx->counters.ptr, sizeof(c), hipMemcpyDeviceToHost));
    *planes = c[5];
    return RT_OK;
}

int rt_unit_sky_excluded(rt_ctx* ctx, uint32_t* tiles) {
    if (!ctx || !tiles) return Fail(RT_ERR_INVALID_ARG, "rt_unit_sky_excluded: invalid argument");
    *tiles = ctx->tileAcct.skyExcluded;
    return RT_OK;
}

#ifdef RT_TIMELINE
// Diagnostic build only: wall-clock landmarks (100 MHz ticks) of the trace kernels since the last call; then reset.
int rt_debug_timeline(rt_ctx* ctx, unsigned long long out[16]) {
    if (!ctx || !out) return Fail(RT_ERR_INVALID_ARG, "rt_debug_timeline: invalid argument");
    RT_HIP(hipSetDevice(ctx->device));
    RT_HIP(hipStreamSynchronize(ctx->stream));
    RT_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(rtd::g_tl), 16 * sizeof(unsigned long long)));
    unsigned long long z[16] = {~0ull, 0, 0, 0, 0, 0, ~0ull, ~0ull, 0, 0, 0, 0, 0, 0, ~0ull, 0};
    RT_HIP(hipMemcpyToSymbol(HIP_SYMBOL(rtd::g_tl), z, sizeof(z)));
    return RT_OK;
}
int rt_debug_timeline_waves(rt_ctx* ctx, unsigned long long out[4096 * 8]) {
    if (!ctx || !out) return Fail(RT_ERR_INVALID_ARG, "rt_debug_timeline_waves: invalid argument");
    RT_HIP(hipSetDevice(ctx->device));
    RT_HIP(hipStreamSynchronize(ctx->stream));
    RT_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(rtd::g_tlWave), 4096 * 8 * sizeof(unsigned long long)));
    return RT_OK;
}
int rt_debug_timeline_ring(rt_ctx* ctx, unsigned long long out[4096 * 16]) {
    if (!ctx || !out) return Fail(RT_ERR_INVALID_ARG, "rt_debug_timeline_ring: invalid argument");
    RT_HIP(hipSetDevice(ctx->device));
    RT_HIP(hipStreamSynchronize(ctx->stream));
    RT_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(rtd::g_tlRing), 4096 * 16 * sizeof(unsigned long long)));
    return RT_OK;
}
int rt_debug_timeline_last(rt_ctx* ctx, unsigned int out[4096 * 4]) {
    if (!ctx || !out) return Fail(RT_ERR_INVALID_ARG, "rt_debug_timeline_last: invalid argument");
    RT_HIP(hipSetDevice(ctx->device));
    RT_HIP(hipStreamSynchronize(ctx->stream));
    RT_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(rtd::g_tlLast), 4096 * 4 * sizeof(unsigned int)));
    return RT_OK;
}
int rt_debug_timeline_hist(rt_ctx* ctx, unsigned int out[1024]) {
    if (!ctx || !out) return Fail(RT_ERR_INVALID_ARG, "rt_debug_timeline_hist: invalid argument");
    RT_HIP(hipSetDevice(ctx->device));
    RT_HIP(hipStreamSynchronize(ctx->stream));
    RT_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(rtd::g_tlHist), 1024 * sizeof(unsigned int)));
    static unsigned int zero[1024];
    RT_HIP(hipMemcpyToSymbol(HIP_SYMBOL(rtd::g_tlHist), zero, sizeof(zero)));
    return RT_OK;
}
#endif

#ifdef RT_STAMPS
// Diagnostic build only: read and clear the section clocks (see rt_params.h g_dbg).
int rt_debug_stamps(rt_ctx* ctx, unsigned long long out[20]) {
    if (!ctx || !out) return Fail(RT_ERR_INVALID_ARG, "rt_debug_stamps: invalid argument");
    RT_HIP(hipSetDevice(ctx->device));
    RT_HIP(hipStreamSynchronize(ctx->stream));
    RT_HIP(hipMemcpyFromSymbol(out, HIP_SYMBOL(rtd::g_dbg), 20 * sizeof(unsigned long long)));
    unsigned long long z[20] = {0};
    RT_HIP(hipMemcpyToSymbol(HIP_SYMBOL(rtd::g_dbg), z, sizeof(z)));
    return RT_OK;
}
#endif

#ifdef RT_PHASES
// Diagnostic build only (tools/phase_budget.py): read and clear the region counters (rt_params.h g_sites); out[2 * site] = wave
// visits, out[2 * site + 1] = active lanes.  names: the sites' names, comma separated, in id order.
int rt_debug_sites(rt_ctx* ctx, unsigned long long* out, uint32_t cap, const char** names) {
    static const char* kNames =
#define RT_SITE_NAME(n) #n ","
        RT_SITE_LIST(RT_SITE_NAME)
#undef RT_SITE_NAME
        ;
    if (names) *names = kNames;
    if (!ctx || !out || cap < 2u * rtd::SITE_COUNT) return Fail(RT_ERR_INVALID_ARG, "rt_debug_sites: invalid argument");
    RT_HIP(hipSetDevice(ctx->device));
    RT_HIP(hipStreamSynchronize(ctx->stream));
    static unsigned long long raw[rtd::SITE_COUNT * 16];
    RT_HIP(hipMemcpyFromSymbol(raw, HIP_SYMBOL(rtd::g_sites), sizeof(raw)));
    for (uint32_t k = 0; k < rtd::SITE_COUNT; ++k) {
        out[2 * k] = raw[16 * k];
        out[2 * k + 1] = raw[16 * k + 1];
    }
    std::memset(raw, 0, sizeof(raw));
    RT_HIP(hipMemcpyToSymbol(HIP_SYMBOL(rtd::g_sites), raw, sizeof(raw)));
    return RT_OK;
}
#endif

}  // extern "C"
