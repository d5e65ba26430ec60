// rt_sequence.h -- how rt_render calls are sequenced, decided without a device: which of the four progressive modes a call takes
// (plain, batched, render-ahead, pipelined), whether it starts, continues or breaks the accumulation, what every outside event
// voids, and how a sample range is cut into passes.  Plain C++ with no HIP header, no environment and no allocation, under the
// contract of rt_launch_plan.h: rt_capi.hip owns one State, asks for the steps of a call, carries them out on the device and reports
// each one done; host/sequence_selftest.cpp runs the same functions against a model of the device with no GPU.  DESIGN.md 4.2.
#pragma once

#include <stdint.h>

#include "../../../include/rt_api.h"

namespace rtseq {

// "The same picture": image size and row set.  (rt_rowset is five uint32_t with no padding: field by field equals a memcmp.)
struct PictureKey {
    uint32_t W = 0, H = 0;
    rt_rowset rs{};
};
inline bool operator==(const PictureKey& a, const PictureKey& b) {
    return a.W == b.W && a.H == b.H && a.rs.first_row == b.rs.first_row && a.rs.num_rows == b.rs.num_rows && a.rs.block_rows == b.rs.block_rows &&
           a.rs.nshards == b.rs.nshards && a.rs.shard == b.rs.shard;
}
inline bool operator!=(const PictureKey& a, const PictureKey& b) { return !(a == b); }

// One rt_render call.  rows: the local rows of pic.rs inside pic.H (rtprep::RowsetRowsWithin; 0: a bad row set) -- a function of
// the key, carried along so that this unit needs nothing of the scene preparation.
struct Call {
    PictureKey pic;
    uint32_t rows = 0;
    uint32_t s0 = 0, s1 = 0, max_depth = 0;
    uint64_t seed = 0;
    bool wants_stats = false;
};

struct State {
    bool hasScene = false;
    bool noise = false;          // rt_set_noise_estimate: the next / running accumulation keeps second moments
    uint32_t pipeDepth = 0;      // rt_set_frame_pipelining: calls a path may be carried across (0 = off)
    uint32_t batchFrames = 1;    // rt_set_frame_batch: sample planes that wait for one launch (1 = off)
    uint32_t lookahead = 1;      // rt_set_frame_lookahead: planes one launch traces (1 = off)
    // the running accumulation: its picture, local rows, and the samples accumulated so far (the next s0 must be accumulated + 1;
    // with frames in flight some of them are not in the strip yet -- the frame pipeline's commit logic knows which)
    PictureKey pic;
    uint32_t rows = 0;
    uint32_t accumulated = 0;
    // frame batching: the stats-less calls [s0, s1) recorded and not yet rendered
    struct Pending {
        bool on = false;
        PictureKey pic;
        uint32_t rows = 0, s0 = 0, s1 = 0, max_depth = 0;
        uint64_t seed = 0;
    } pend;
    // render-ahead: sample planes [base, base + spp) of the running accumulation sit in the sample buffer, traced by ONE launch;
    // planes below `next` have been added to the strip
    struct Ahead {
        bool valid = false;
        PictureKey pic;
        uint32_t base = 0, spp = 0, next = 0, max_depth = 0;
        uint64_t seed = 0;
    } ahead;
};

// ---- what an event voids or asks to be settled first.  The bits of State's own parts are applied by the event's function; the
// others name state of rt_capi.hip (device-side bookkeeping and tables) that the caller drops on being told.
enum : uint32_t {
    kPending = 1u << 0,       // the recorded batch
    kAhead = 1u << 1,         // the planes traced ahead
    kAccumulation = 1u << 2,  // the strip: the next rt_render must start at s0 == 1
    kInFlight = 1u << 3,      // carried paths and uncommitted regions of the frame pipeline
    kTileOrder = 1u << 4,     // work order and empty-list flags of the tiles
    kFeatures = 1u << 5,      // the feature strips
    kDenoised = 1u << 6,      // the denoised picture
};

// Rendered (kPending) or flushed (kInFlight) BEFORE the event takes effect, in this order.  An error there refuses a new scene or
// stream; the two settings are stored all the same (nothing is pending or in flight any more), as they always were.
constexpr uint32_t kSettleBeforeScene = kPending;               // pending frames were asked of the scene that is being replaced
constexpr uint32_t kSettleBeforeCamera = kPending;              // ... or of the camera that is being replaced
constexpr uint32_t kSettleBeforeStream = kPending | kInFlight;  // pending frames and frames in flight belong to the old stream
constexpr uint32_t kSettleBeforeBatchSetting = kPending;
// (rt_set_frame_pipelining settles kPending, then kInFlight, and stores the depth unless the BATCH failed; rt_set_frame_lookahead
// settles nothing)
constexpr uint32_t kSettleAtSynchronize = kPending | kInFlight;  // pending frames are rendered, frames in flight finished and committed

// One function per outside event.  Each applies the event to the state and returns everything it voided.
uint32_t SceneReplaced(State& st);              // rt_scene_upload, once the new tables are in place
uint32_t CameraChanged(State& st);              // rt_set_camera with another record than before (the caller requires hasScene): what
                                                // SceneReplaced voids -- every picture is a function of the camera -- with no scene set
uint32_t StreamReplaced(State& st);             // rt_set_stream
uint32_t SamplerChanged(State& st);             // rt_set_sampler with other flags than before
uint32_t NoiseToggled(State& st, bool on);      // rt_set_noise_estimate; voids only where `on` differs from the state
uint32_t Cleared(State& st);                    // rt_clear
uint32_t StepFailed(State& st);                 // a render step failed after it may have touched the strip
uint32_t TileTablesDropped(State& st);          // the tiles' order and flags were dropped or are about to be rebuilt
uint32_t BatchSettingChanged(State& st, uint32_t frames);
uint32_t LookaheadSettingChanged(State& st, uint32_t frames);
uint32_t PipeliningSettingChanged(State& st, uint32_t depth);
// A new accumulation starts -- in two moments, as rt_render meets them: Starting says what a call that starts one abandons (nothing
// where the call continues), before anything of the old strip is touched; Started makes the call's picture the running accumulation,
// once its strips are reserved and zeroed.
uint32_t AccumulationStarting(const State& st, const Call& c);
void AccumulationStarted(State& st, const Call& c);

// ---- the steps of one rt_render call, for the caller to carry out in order; the first that fails ends the call with its error.
enum class StepKind : uint32_t {
    AddAhead,       // add planes [first, first + count) of the buffer traced ahead to the strip
    Record,         // record the call into the pending batch
    RenderPending,  // render the pending batch with one launch (no statistics)
    RenderNow,      // render the call now; aheadEnd != 0: trace [s0, aheadEnd) with it and keep the planes from s1 on
    Refuse,         // refuse the call with this error: what CheckCall below finds, met where rt_render would meet it
};
struct Refusal {
    int status = RT_OK;  // RT_OK: not refused
    const char* message = "";
};
struct Step {
    StepKind kind = StepKind::RenderNow;
    uint32_t first = 0, count = 0;  // AddAhead
    uint32_t aheadEnd = 0;          // RenderNow
    Refusal refusal;                // Refuse
};
struct Steps {
    Step v[3];  // at most: render the batch this call does not continue, record the call, render the batch it completed
    uint32_t n = 0;
};
Steps PlanRender(const State& st, const Call& c);

// The state advances only through these, as the caller reports a step done.
void AheadAdded(State& st, const Step& s);
void Recorded(State& st, const Call& c);
Call PendingTaken(State& st);  // RenderPending begins: the batch as ONE call, no longer pending whatever becomes of it
// The readers (rt_resolve, rt_download, rt_copy_to_device, the noise entries) hand out the COMMITTED strip while a batch that
// continues it is pending.  A pending batch that does not continue it -- nothing is committed yet, or its first call had s0 == 1 and
// so starts a new accumulation, possibly of another size: the caller's picture is the new one -- is rendered first.
bool PendingMustRender(const State& st);

// ---- one render-now step (a call's own, or the pending batch's), in the order rt_render makes its checks.
void RenderBegins(State& st);  // whatever was traced ahead belongs to the calls before this one
Refusal CheckCall(const State& st, const Call& c);  // no scene; empty image or range; bad row set; image too large
// Frame pipelining: only calls that ask for no statistics may leave work in flight, and none while second moments are kept (the
// carrying kernel's commit adds none); the ring of pipeDepth + 2 regions stays below 2^31 samples.  True: the call pipelines where
// the launch plan has a carrying kernel for the scene (rtplan::TracePlan::pipelines), which the caller asks next.
bool MayPipeline(const State& st, const Call& c);
enum class Admission : uint32_t { Starts, Continues, Refused };
Admission Admit(const State& st, const Call& c, Refusal* why);  // start / continue / RT_ERR_SEQUENCE
void Rendered(State& st, const Call& c, uint32_t aheadEnd, uint32_t sppTrace);  // aheadEnd: the split's effective one

// ---- the pass split: [s0, s1) -- with planes traced ahead, [s0, aheadEnd) -- in passes whose sample buffer fits the workspace limit.
struct PassSplit {
    Refusal refused;     // RT_ERR_OUT_OF_MEMORY: the limit is below one sample per pixel
    uint32_t s0 = 0, s1 = 0;
    uint32_t aheadEnd = 0;  // effective: 0 where the planes traced ahead could not share one pass
    uint32_t sppTrace = 0;  // planes traced in all
    uint32_t sppPass = 0;   // planes per pass: the sample buffer holds npix * sppPass * 3 floats
};
PassSplit SplitPasses(uint32_t npix, uint32_t s0, uint32_t s1, uint32_t aheadEnd, uint64_t workspaceLimit);
// The sample buffer of sppPass planes could not be allocated: halve the pass (a smaller buffer only means more passes, bit-identical).
// A call that was tracing ahead and no longer fits one pass gives that up and renders its own planes in ordinary passes.
// False: the pass is one plane already, the call fails with the allocation's error.
bool ShrinkPass(PassSplit& p);
struct Pass {
    uint32_t s = 0, spp = 0;                // trace planes [s, s + spp) into the buffer's planes [0, spp)
    uint32_t add_first = 0, add_count = 0;  // then add the buffer's planes [add_first, add_first + add_count) to the strip
};
Pass FirstPass(const PassSplit& p);                  // spp == 0: no pass (left)
Pass NextPass(const PassSplit& p, const Pass& cur);

}  // namespace rtseq
