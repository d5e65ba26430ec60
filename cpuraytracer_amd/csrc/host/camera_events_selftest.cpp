// camera_events_selftest.cpp -- what a camera move voids (rtseq::CameraChanged, rttile::CameraChanged) against what a scene upload
// voids (the two SceneReplaced), with no device and no library.  A model stands in for rt_capi.hip as far as the two states go: it
// carries out the sequencer's steps and the tile tables' plans in rt_capi.hip's order (Render, RenderNow, BuildTables, SkyCountPoll,
// SetCamera and SceneUpload below are its twins), and the copy of the flagged tiles' count is a queue of words on their way to one
// pinned word behind one event that completes with its LATEST record.  Two parts: scenarios written from the contract of
// rt_set_camera in include/rt_api.h, and seeded random scripts of calls and events; after every step of every script the camera event
// and the scene event are applied to copies of the two states, which must then be equal field by field, with the same void mask.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <deque>
#include <string>

#include "rt_tile_tables.h"

namespace {

using rtseq::PictureKey;

int g_failures = 0;
std::string g_where;
#define CHECK(cond)                                                                                      \
    do {                                                                                                 \
        if (!(cond)) {                                                                                   \
            if (++g_failures <= 20) fprintf(stderr, "FAIL %s: %s (line %d)\n", g_where.c_str(), #cond, __LINE__); \
        }                                                                                                \
    } while (0)

struct Rng {
    uint64_t s;
    uint32_t next() {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)(s >> 33);
    }
    uint32_t below(uint32_t n) { return next() % n; }
    bool one_in(uint32_t n) { return below(n) == 0; }
};

PictureKey Pic(uint32_t W, uint32_t H) {
    PictureKey p;
    p.W = W, p.H = H;
    p.rs.first_row = 0, p.rs.num_rows = H, p.rs.block_rows = H, p.rs.nshards = 1, p.rs.shard = 0;
    return p;
}

// ---- field by field
bool Same(const rtseq::State& a, const rtseq::State& b) {
    const rtseq::State::Pending &p = a.pend, &q = b.pend;
    const rtseq::State::Ahead &x = a.ahead, &y = b.ahead;
    return a.hasScene == b.hasScene && a.noise == b.noise && a.pipeDepth == b.pipeDepth && a.batchFrames == b.batchFrames && a.lookahead == b.lookahead &&
           a.pic == b.pic && a.rows == b.rows && a.accumulated == b.accumulated &&  //
           p.on == q.on && p.pic == q.pic && p.rows == q.rows && p.s0 == q.s0 && p.s1 == q.s1 && p.max_depth == q.max_depth && p.seed == q.seed &&
           x.valid == y.valid && x.pic == y.pic && x.base == y.base && x.spp == y.spp && x.next == y.next && x.max_depth == y.max_depth && x.seed == y.seed;
}
bool Same(const rttile::State& a, const rttile::State& b) {
    return a.orderWanted == b.orderWanted &&  //
           a.masks.valid == b.masks.valid && a.masks.pic == b.masks.pic && a.masks.limit == b.masks.limit && a.masks.spheres == b.masks.spheres &&
           a.masks.tiles == b.masks.tiles &&  //
           a.order.keyValid == b.order.keyValid && a.order.orderValid == b.order.orderValid && a.order.flagsValid == b.order.flagsValid &&
           a.order.pic == b.order.pic && a.order.listLimit == b.order.listLimit && a.order.listSpheres == b.order.listSpheres &&  //
           a.count.pending == b.count.pending && a.count.known == b.count.known && a.count.value == b.count.value &&  //
           a.skySkip == b.skySkip && a.skyExclude == b.skyExclude;
}

// what the run reached
enum { kWithPending, kWithAhead, kWithInFlight, kWithMasks, kWithOrder, kWithCountPending, kWithCountKnown, kNoScene, kStaleInFlight, kSameRecord, kReachedCount };
const char* const kReachedName[kReachedCount] = {"pending-batch",  "planes-ahead", "frames-in-flight", "masks-valid",       "order-valid",
                                                 "count-pending",  "count-known",  "no-scene",         "stale-copy-in-flight", "same-record"};
uint64_t g_reached[kReachedCount], g_compared, g_moves;

struct Model {
    rtseq::State seq;
    rttile::State tiles;
    uint32_t cuCount = 4;  // the order exists from 8 full tiles on
    rttile::Knobs knobs;
    uint32_t camera = 0, cameraEpoch = 0;  // the current record (a label) and the generation of what was built from it
    uint32_t inFlight = 0;                 // frames of the pipeline not yet in the strip (dropped with kInFlight)
    bool features = false, denoised = false;
    uint32_t rendersOfBatch = 0;  // launches that settled a batch, and the camera generation each ran under
    uint32_t lastBatchEpoch = 0;
    // the count's way to the host: copies queued on the stream, one pinned word, one event whose state is its latest record's
    struct Copy {
        uint32_t value, epoch;
    };
    std::deque<Copy> copies;  // on their way, oldest first; the event is complete when none is left
    uint32_t pinned = 0, pinnedEpoch = 0;

    Model() { knobs.primarySpheres = 12; }  // (lists, and so flags and their count)
    uint32_t CountOf(const PictureKey& pic) const { return (cameraEpoch * 2654435761u ^ pic.W * 40503u) % ((pic.W * pic.rs.num_rows >> 6) + 1u); }
    void StreamAdvances(uint32_t n) {  // the device gets on with n of the queued copies
        for (; n != 0 && !copies.empty(); --n) {
            pinned = copies.front().value, pinnedEpoch = copies.front().epoch;
            copies.pop_front();
        }
    }
    void SkyCountPoll() {
        if (!rttile::CountToAwait(tiles)) return;
        if (!copies.empty()) return;  // hipErrorNotReady
        rttile::CountArrived(tiles, pinned);
        // the word that is taken is the one this camera's build copied: never a stale one's
        CHECK(tiles.count.known && pinnedEpoch == cameraEpoch && tiles.count.value == CountOf(tiles.order.pic));
    }
    void DropVoided(uint32_t voids) {
        if (voids & rtseq::kInFlight) inFlight = 0;
        if (voids & rtseq::kTileOrder) {
            rttile::Dropped(tiles);
            (void)rtseq::TileTablesDropped(seq);
        }
        if (voids & rtseq::kFeatures) features = false;
        if (voids & rtseq::kDenoised) denoised = false;
    }
    void BuildTables(const PictureKey& pic, uint32_t npix) {
        const rttile::MaskPlan mp = rttile::PlanMasks(tiles, pic, npix, knobs, true);
        if (mp.answer == rttile::MaskAnswer::Build) rttile::MasksBuilt(tiles, pic, mp);
        const rttile::OrderPlan op = rttile::PlanOrder(tiles, pic, npix, cuCount);
        if (!op.rebuild) return;
        (void)rtseq::TileTablesDropped(seq);
        if (op.count) copies.push_back(Copy{CountOf(pic), cameraEpoch});  // the copy, then the event recorded again behind it
        rttile::OrderBuilt(tiles, pic, op);
    }
    int RenderNow(const rtseq::Call& call, uint32_t aheadEnd) {
        rtseq::RenderBegins(seq);
        const rtseq::Refusal bad = rtseq::CheckCall(seq, call);
        if (bad.status != RT_OK) return bad.status;
        const uint32_t npix = call.pic.W * call.rows;
        SkyCountPoll();
        const bool pipelined = rtseq::MayPipeline(seq, call);
        const uint32_t abandoned = rtseq::AccumulationStarting(seq, call);
        DropVoided(abandoned);
        if (!abandoned && !pipelined) inFlight = 0;  // (flushed into the strip)
        rtseq::Refusal why;
        switch (rtseq::Admit(seq, call, &why)) {
            case rtseq::Admission::Refused: return why.status;
            case rtseq::Admission::Continues: break;
            case rtseq::Admission::Starts:
                rtseq::AccumulationStarted(seq, call);
                rttile::AccumulationStarts(tiles, knobs);
                BuildTables(call.pic, npix);
        }
        // every table a launch takes was built from the current camera
        const rttile::Use use = rttile::UseFor(tiles, call.pic, npix);
        if (use.nSky != 0) CHECK(tiles.count.value == CountOf(call.pic));
        if (pipelined) {
            inFlight = inFlight < seq.pipeDepth ? inFlight + 1 : seq.pipeDepth;
            rtseq::Rendered(seq, call, 0, 0);
            return RT_OK;
        }
        const rtseq::PassSplit split = rtseq::SplitPasses(npix, call.s0, call.s1, aheadEnd, 8ull << 30);
        rtseq::Rendered(seq, call, split.aheadEnd, split.sppTrace);
        return RT_OK;
    }
    int BatchFlush() {
        if (!seq.pend.on) return RT_OK;
        ++rendersOfBatch;
        lastBatchEpoch = cameraEpoch;
        return RenderNow(rtseq::PendingTaken(seq), 0);
    }
    int Settle(uint32_t what) {
        const int rc = (what & rtseq::kPending) ? BatchFlush() : RT_OK;
        if (rc == RT_OK && (what & rtseq::kInFlight)) inFlight = 0;
        return rc;
    }
    int Render(const PictureKey& pic, uint32_t s0, uint32_t s1, bool stats = false) {
        rtseq::Call call;
        call.pic = pic, call.rows = pic.rs.num_rows, call.s0 = s0, call.s1 = s1, call.max_depth = 8, call.seed = 1, call.wants_stats = stats;
        const rtseq::Steps steps = rtseq::PlanRender(seq, call);
        for (uint32_t k = 0; k < steps.n; ++k) {
            const rtseq::Step& step = steps.v[k];
            int rc = RT_OK;
            switch (step.kind) {
                case rtseq::StepKind::AddAhead: rtseq::AheadAdded(seq, step); break;
                case rtseq::StepKind::Record: rtseq::Recorded(seq, call); break;
                case rtseq::StepKind::RenderPending: rc = BatchFlush(); break;
                case rtseq::StepKind::RenderNow: rc = RenderNow(call, step.aheadEnd); break;
                case rtseq::StepKind::Refuse:
                    rtseq::RenderBegins(seq);
                    rc = step.refusal.status;
                    break;
            }
            if (rc != RT_OK) return rc;
        }
        return RT_OK;
    }
    int SceneUpload(uint32_t cam) {
        const int rc = Settle(rtseq::kSettleBeforeScene);
        if (rc != RT_OK) return rc;
        StreamAdvances(~0u);  // (the upload waits for the stream)
        camera = cam, ++cameraEpoch;
        rttile::SceneReplaced(tiles);
        (void)rtseq::TileTablesDropped(seq);
        DropVoided(rtseq::SceneReplaced(seq));
        return RT_OK;
    }
    // rt_set_camera.  *event: whether the call was an event at all.
    int SetCamera(uint32_t cam, bool* event = nullptr) {
        if (event) *event = false;
        if (!seq.hasScene) return RT_ERR_NO_SCENE;
        if (cam == camera) return RT_OK;  // the same record
        const int rc = Settle(rtseq::kSettleBeforeCamera);
        if (rc != RT_OK) return rc;
        if (!copies.empty()) ++g_reached[kStaleInFlight];  // (no wait: an old copy may still be on its way)
        camera = cam, ++cameraEpoch;
        rttile::CameraChanged(tiles);
        (void)rtseq::TileTablesDropped(seq);
        DropVoided(rtseq::CameraChanged(seq));
        if (event) *event = true;
        ++g_moves;
        return RT_OK;
    }
    void Features() { features = seq.hasScene; }
    void Denoise() { denoised = features && seq.accumulated != 0; }

    // From this state: the camera event against the scene event, on copies.
    void CompareEvents() {
        if (seq.pend.on) ++g_reached[kWithPending];
        if (seq.ahead.valid) ++g_reached[kWithAhead];
        if (inFlight) ++g_reached[kWithInFlight];
        if (tiles.masks.valid) ++g_reached[kWithMasks];
        if (tiles.order.orderValid) ++g_reached[kWithOrder];
        if (tiles.count.pending) ++g_reached[kWithCountPending];
        if (tiles.count.known) ++g_reached[kWithCountKnown];
        if (!seq.hasScene) {
            ++g_reached[kNoScene];  // (the camera event requires a scene: rt_set_camera refuses, and nothing moves)
            Model c = *this;
            CHECK(c.SetCamera(camera + 1) == RT_ERR_NO_SCENE && Same(c.seq, seq) && Same(c.tiles, tiles) && c.cameraEpoch == cameraEpoch);
            return;
        }
        CHECK(rtseq::kSettleBeforeCamera == rtseq::kSettleBeforeScene);
        // (both entries settle the same bits first; the events then meet the same state)
        rtseq::State s1 = seq, s2 = seq;
        rttile::State t1 = tiles, t2 = tiles;
        const uint32_t v1 = rtseq::CameraChanged(s1), v2 = rtseq::SceneReplaced(s2);
        rttile::CameraChanged(t1);
        rttile::SceneReplaced(t2);
        CHECK(v1 == v2 && v1 == (rtseq::kAhead | rtseq::kAccumulation | rtseq::kInFlight | rtseq::kFeatures | rtseq::kDenoised));
        CHECK(Same(s1, s2) && Same(t1, t2));
        CHECK(s1.hasScene && !s1.ahead.valid && s1.accumulated == 0);
        CHECK(s1.noise == seq.noise && s1.pipeDepth == seq.pipeDepth && s1.batchFrames == seq.batchFrames && s1.lookahead == seq.lookahead);  // kept
        CHECK(!t1.masks.valid && !t1.order.keyValid && !t1.order.orderValid && !t1.order.flagsValid && !t1.count.pending && !t1.count.known);
        CHECK(rttile::MaskTiles(t1) == 0 && rttile::ListTiles(t1) == 0 && !rttile::AccumulateByFlags(t1) && !rttile::CountToAwait(t1));
        ++g_compared;
    }
};

// ------------------------------------------------------------------------------------------------------------- scenarios
const PictureKey A = Pic(64, 32), B = Pic(72, 30);

Model Fresh() {
    Model m;
    CHECK(m.SceneUpload(1) == RT_OK);
    return m;
}

void ScenarioPendingBatchIsSettledFirst() {
    Model m = Fresh();
    rtseq::BatchSettingChanged(m.seq, 8);
    for (uint32_t f = 1; f <= 3; ++f) CHECK(m.Render(A, f, f + 1) == RT_OK);
    CHECK(m.seq.pend.on && m.seq.accumulated == 0 && m.rendersOfBatch == 0);
    CHECK((rtseq::kSettleBeforeCamera & rtseq::kPending) != 0 && (rtseq::kSettleBeforeCamera & rtseq::kInFlight) == 0);  // reported as to-be-settled first
    const uint32_t epoch = m.cameraEpoch;
    bool event = false;
    CHECK(m.SetCamera(2, &event) == RT_OK && event);
    CHECK(m.rendersOfBatch == 1 && m.lastBatchEpoch == epoch);  // rendered, under the camera it was asked of
    CHECK(!m.seq.pend.on && m.seq.accumulated == 0);
    CHECK(m.Render(A, 4, 5) == RT_ERR_SEQUENCE);
    CHECK(m.Render(A, 1, 2) == RT_OK);
}
void ScenarioAheadPlanesBecomeInvalid() {
    Model m = Fresh();
    rtseq::LookaheadSettingChanged(m.seq, 16);
    CHECK(m.Render(A, 1, 2) == RT_OK && m.Render(A, 2, 3) == RT_OK);
    CHECK(m.seq.ahead.valid && m.seq.ahead.spp == 16 && m.seq.accumulated == 2);
    CHECK(m.SetCamera(2) == RT_OK);
    CHECK(!m.seq.ahead.valid && m.seq.accumulated == 0 && m.seq.lookahead == 16);
    CHECK(m.Render(A, 3, 4) == RT_ERR_SEQUENCE);  // a continuing call
    const rtseq::Call c{A, 32, 1, 2, 8, 1, false};
    const rtseq::Steps s = rtseq::PlanRender(m.seq, c);
    CHECK(s.n == 1 && s.v[0].kind == rtseq::StepKind::RenderNow);  // a render that starts over traces anew: no plane is picked up
    CHECK(m.Render(A, 1, 2) == RT_OK && m.seq.ahead.valid && m.seq.ahead.base == 1);
}
void ScenarioFramesInFlightAreDropped() {
    Model m = Fresh();
    rtseq::PipeliningSettingChanged(m.seq, 4);
    for (uint32_t f = 1; f <= 3; ++f) CHECK(m.Render(A, f, f + 1) == RT_OK);
    CHECK(m.inFlight == 3 && m.seq.accumulated == 3);
    CHECK(m.SetCamera(2) == RT_OK && m.inFlight == 0 && m.seq.accumulated == 0 && m.seq.pipeDepth == 4);
    CHECK(m.Render(A, 4, 5) == RT_ERR_SEQUENCE && m.Render(A, 1, 2) == RT_OK);
}
void ScenarioCountIsNeitherPendingNorKnown() {
    for (int arrived = 0; arrived < 2; ++arrived) {
        Model m = Fresh();
        CHECK(m.Render(A, 1, 2) == RT_OK);
        CHECK(m.tiles.count.pending && !m.tiles.count.known && m.copies.size() == 1);
        if (arrived) {
            m.StreamAdvances(1);
            CHECK(m.Render(A, 2, 3) == RT_OK && m.tiles.count.known && !m.tiles.count.pending);
        }
        CHECK(m.SetCamera(2) == RT_OK);
        CHECK(!m.tiles.count.pending && !m.tiles.count.known && !m.tiles.masks.valid && !m.tiles.order.keyValid);
        // the old copy is still on its way when the new camera's tables are built: the poll finds the event not ready until the
        // newer copy has landed, and then takes the newer word
        CHECK(m.Render(A, 1, 2) == RT_OK && m.tiles.count.pending && m.copies.size() == (arrived ? 1u : 2u));
        if (!arrived) {
            m.StreamAdvances(1);  // the stale word lands
            CHECK(m.pinnedEpoch + 1 == m.cameraEpoch);
            CHECK(m.Render(A, 2, 3) == RT_OK && !m.tiles.count.known);  // not taken
        }
        m.StreamAdvances(1);
        CHECK(m.Render(A, 3 - arrived, 4 - arrived) == RT_OK && m.tiles.count.known && m.tiles.count.value == m.CountOf(A));
    }
}
void ScenarioSameRecordIsNoEvent() {
    Model m = Fresh();
    rtseq::BatchSettingChanged(m.seq, 4);
    CHECK(m.Render(A, 1, 5) == RT_OK && m.Render(A, 5, 6) == RT_OK);
    m.Features();
    m.Denoise();
    CHECK(m.seq.pend.on && m.seq.accumulated == 4 && m.features && m.denoised);
    const rtseq::State s = m.seq;
    const rttile::State t = m.tiles;
    const uint32_t epoch = m.cameraEpoch, moves = (uint32_t)g_moves, batches = m.rendersOfBatch;
    bool event = true;
    CHECK(m.SetCamera(m.camera, &event) == RT_OK && !event);
    CHECK(Same(m.seq, s) && Same(m.tiles, t) && m.cameraEpoch == epoch && (uint32_t)g_moves == moves && m.features && m.denoised && m.rendersOfBatch == batches);
    CHECK(m.Render(A, 6, 7) == RT_OK);  // the accumulation continues, the batch is still pending
    ++g_reached[kSameRecord];
    CHECK(m.SetCamera(2, &event) == RT_OK && event && !m.features && !m.denoised);
}
void ScenarioNoScene() {
    Model m;
    CHECK(m.SetCamera(2) == RT_ERR_NO_SCENE && !m.seq.hasScene && m.cameraEpoch == 0);
}

const struct {
    const char* name;
    void (*run)();
} kScenarios[] = {
    {"a pending batch is settled first", ScenarioPendingBatchIsSettledFirst},
    {"planes traced ahead become invalid", ScenarioAheadPlanesBecomeInvalid},
    {"frames in flight are dropped", ScenarioFramesInFlightAreDropped},
    {"the count is neither pending nor known", ScenarioCountIsNeitherPendingNorKnown},
    {"the same record is no event", ScenarioSameRecordIsNoEvent},
    {"no scene", ScenarioNoScene},
};

// ------------------------------------------------------------------------------------------------------------ model check
void RunScript(uint64_t seed, uint32_t steps) {
    Rng R{seed * 0x9e3779b97f4a7c15ull + 1};
    Model m;
    const PictureKey pics[3] = {A, B, Pic(16, 8)};  // (the last: too few tiles for an order)
    PictureKey pic = pics[R.below(3)];
    if (!R.one_in(8)) CHECK(m.SceneUpload(1) == RT_OK);
    for (uint32_t k = 0; k < steps; ++k) {
        g_where = "script " + std::to_string(seed) + " step " + std::to_string(k);
        const uint32_t op = R.below(100);
        if (op < 55) {
            const uint32_t promised = m.seq.pend.on ? m.seq.pend.s1 - 1 : m.seq.accumulated;
            const uint32_t kind = R.below(12);
            if (kind == 0) pic = pics[R.below(3)];
            const uint32_t s0 = (kind <= 1 || promised == 0) ? 1u : promised + 1u;
            (void)m.Render(pic, s0, s0 + (R.one_in(4) ? 1 + R.below(5) : 1), R.one_in(10));
        } else if (op < 63) {
            m.StreamAdvances(1 + R.below(2));
        } else if (op < 68) {
            (void)m.Settle(rtseq::kSettleBeforeBatchSetting);
            m.DropVoided(rtseq::BatchSettingChanged(m.seq, R.one_in(3) ? 1 : 2 + R.below(5)));
        } else if (op < 73) {
            m.DropVoided(rtseq::LookaheadSettingChanged(m.seq, R.one_in(3) ? 1 : 2 + R.below(7)));
        } else if (op < 78) {
            (void)m.Settle(rtseq::kPending);
            (void)m.Settle(rtseq::kInFlight);
            m.DropVoided(rtseq::PipeliningSettingChanged(m.seq, R.one_in(3) ? 0 : 1 + R.below(3)));
        } else if (op < 81) {
            (void)m.SceneUpload(1 + R.below(3));
        } else if (op < 89) {
            bool event = false;
            const uint32_t cam = 1 + R.below(3);
            const bool same = cam == m.camera, scene = m.seq.hasScene;
            const rtseq::State s = m.seq;
            const rttile::State t = m.tiles;
            const int rc = m.SetCamera(cam, &event);
            CHECK(rc == (scene ? RT_OK : RT_ERR_NO_SCENE) && event == (scene && !same));
            if (!event) CHECK(Same(m.seq, s) && Same(m.tiles, t));
            if (scene && same) ++g_reached[kSameRecord];
            if (event) CHECK(!m.seq.pend.on && !m.seq.ahead.valid && m.seq.accumulated == 0 && m.inFlight == 0 && !m.features && !m.denoised &&
                             !m.tiles.masks.valid && !m.tiles.count.pending && !m.tiles.count.known);
        } else if (op < 91) {
            m.DropVoided(rtseq::SamplerChanged(m.seq));
        } else if (op < 93) {
            m.DropVoided(rtseq::NoiseToggled(m.seq, R.one_in(2)));
        } else if (op < 94) {
            m.DropVoided(rtseq::Cleared(m.seq));
        } else if (op < 96) {
            m.knobs.primarySpheres = R.one_in(3) ? 0u : 12u;
            m.knobs.skipSky = !R.one_in(4);
            m.knobs.excludeSky = !R.one_in(4);
        } else if (op < 98) {
            m.Features();
        } else {
            m.Denoise();
        }
        m.CompareEvents();
        if (g_failures) return;
    }
}

}  // namespace

int main(int argc, char** argv) {
    const uint32_t scripts = argc > 1 ? (uint32_t)atoi(argv[1]) : 100000u, steps = 60;
    g_where = "scenarios";
    for (const auto& s : kScenarios) {
        const int before = g_failures;
        s.run();
        if (g_failures != before) fprintf(stderr, "scenario failed: %s\n", s.name);
    }
    const uint32_t nScenarios = (uint32_t)(sizeof(kScenarios) / sizeof(kScenarios[0]));
    for (uint32_t k = 0; k < scripts && g_failures == 0; ++k) RunScript(k, steps);
    printf("states compared %llu, camera moves %llu\nreached:", (unsigned long long)g_compared, (unsigned long long)g_moves);
    bool allReached = true;
    for (int k = 0; k < kReachedCount; ++k) printf(" %s %llu", kReachedName[k], (unsigned long long)g_reached[k]), allReached = allReached && g_reached[k] != 0;
    printf("\n");
    if (!allReached) fprintf(stderr, "FAIL: a kind of state was never reached\n");
    if (g_failures != 0 || !allReached) {
        printf("camera_events_selftest: FAILED (%d checks)\n", g_failures);
        return 1;
    }
    printf("%u scenarios, %u scripts of %u steps\ncamera_events_selftest: ok\n", nScenarios, scripts, steps);
    return 0;
}
