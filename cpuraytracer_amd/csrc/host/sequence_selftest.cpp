// sequence_selftest.cpp -- the sequencer (rt_sequence.h) alone, with no device and no library.  A model of the device stands in for
// rt_capi.hip: the sample buffer is an array of plane labels, the strip the list of labels added, the frame pipeline a queue of
// regions; the model carries out the sequencer's steps exactly as rt_capi.hip does (Render, RenderNow, Settle, DropVoided below are
// its twins).  Two parts: scenarios written from the contract of include/rt_api.h (rt_render, rt_set_frame_pipelining,
// rt_set_frame_batch, rt_set_frame_lookahead), and seeded random scripts of calls and events with "allocation failed" injected
// into the shrink loop, checked after every step.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <deque>
#include <string>
#include <vector>

#include "rt_sequence.h"

namespace {

using namespace rtseq;

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

PictureKey Pic(uint32_t W, uint32_t H, uint32_t first = 0, uint32_t num = 0) {
    PictureKey p;
    p.W = W, p.H = H;
    p.rs.first_row = first, p.rs.num_rows = num ? num : H - first, p.rs.block_rows = p.rs.num_rows, p.rs.nshards = 1, p.rs.shard = 0;
    return p;
}
uint32_t RowsOf(const PictureKey& p) { return (uint64_t)p.rs.first_row + p.rs.num_rows > p.H ? 0u : p.rs.num_rows; }  // (contiguous row sets only)

// counters of what the run reached
enum { kEvScene, kEvStream, kEvSampler, kEvNoise, kEvClear, kEvFailed, kEvStarted, kEvBatch, kEvLookahead, kEvPipelining, kEvTiles, kEvCount };
const char* const kEvName[kEvCount] = {"scene", "stream", "sampler", "noise", "clear", "step-failed", "started", "batch", "lookahead", "pipelining", "tiles-dropped"};
const char* const kStepName[5] = {"add-ahead", "record", "render-pending", "render-now", "refuse"};
uint64_t g_steps[5], g_events[kEvCount], g_shrinkWhileAhead, g_shrinks, g_multiPass, g_pipelined;

struct Plane {
    uint32_t s = 0;       // the sample index traced
    uint64_t tag = 0;     // scene, sampler, picture, depth and seed it was traced with
    uint32_t launch = 0;  // the launch that wrote it
};

struct Model {
    State seq;
    uint64_t workspaceLimit = 8ull << 30;
    bool kernelCarries = true;
    uint32_t sceneEpoch = 0, samplerEpoch = 0;
    // device
    std::vector<Plane> strip, buffer;
    std::deque<std::vector<Plane>> regions;  // frame pipeline: the newest calls' planes, not yet in the strip
    uint32_t launches = 0, aheadLaunch = 0;
    uint32_t allocFailures = 0;  // injected into the next Reserve loop
    int lastStatus = RT_OK;
    std::string lastMessage;
    uint32_t lastPasses = 0;

    uint64_t Tag(const Call& c) const {
        uint64_t h = 1469598103934665603ull;
        const uint64_t v[] = {sceneEpoch, samplerEpoch, c.pic.W, c.pic.H, c.pic.rs.first_row, c.pic.rs.num_rows, c.max_depth, c.seed};
        for (uint64_t x : v) h = (h ^ x) * 1099511628211ull;
        return h;
    }
    uint32_t InFlight() const {
        uint32_t n = 0;
        for (const auto& r : regions) n += (uint32_t)r.size();
        return n;
    }
    int Fail(int status, const char* msg) {
        lastStatus = status, lastMessage = msg;
        return status;
    }
    // the accumulate kernels: planes [first, first + count) of the buffer, which must be the launch's that the caller means
    void Add(const std::vector<Plane>& from, uint32_t first, uint32_t count, uint64_t tag, uint32_t launch) {
        CHECK((uint64_t)first + count <= from.size());
        for (uint32_t k = first; k < first + count && k < from.size(); ++k) {
            CHECK(from[k].s == strip.size() + 1);  // in sample order, nothing twice, nothing nobody asked for
            CHECK(from[k].tag == tag);
            CHECK(from[k].launch == launch);
            strip.push_back(from[k]);
        }
    }
    void PipelineFlush() {
        while (!regions.empty()) {
            const std::vector<Plane> r = regions.front();
            regions.pop_front();
            if (!r.empty()) Add(r, 0, (uint32_t)r.size(), r[0].tag, r[0].launch);
        }
    }
    void DropVoided(uint32_t voids) {
        if (voids & kInFlight) regions.clear();
        if (voids & kTileOrder) {
            ++g_events[kEvTiles];
            CHECK(TileTablesDropped(seq) == kAhead && !seq.ahead.valid);
        }
    }
    int BatchFlush() {
        if (!seq.pend.on) return RT_OK;
        return RenderNow(PendingTaken(seq), 0);
    }
    int Settle(uint32_t what) {
        int rc = (what & kPending) ? BatchFlush() : RT_OK;
        if (rc == RT_OK && (what & kInFlight)) PipelineFlush();
        return rc;
    }

    int RenderNow(const Call& call, uint32_t aheadEnd) {
        RenderBegins(seq);
        const Refusal bad = CheckCall(seq, call);
        if (bad.status != RT_OK) return Fail(bad.status, bad.message);
        const uint32_t npix = call.pic.W * call.rows;
        const bool pipelined = MayPipeline(seq, call) && kernelCarries;
        const uint32_t abandoned = AccumulationStarting(seq, call);
        DropVoided(abandoned);
        if (!abandoned && !pipelined) PipelineFlush();
        Refusal why;
        switch (Admit(seq, call, &why)) {
            case Admission::Refused: return Fail(why.status, why.message);
            case Admission::Continues: break;
            case Admission::Starts:
                strip.clear();
                AccumulationStarted(seq, call);
                ++g_events[kEvStarted];
        }
        const uint64_t tag = Tag(call);
        if (pipelined) {
            ++g_pipelined;
            std::vector<Plane> r;
            ++launches;
            for (uint32_t s = call.s0; s < call.s1; ++s) r.push_back(Plane{s, tag, launches});
            regions.push_back(r);
            while (regions.size() > seq.pipeDepth) {  // up to pipeDepth of the newest calls stay in flight
                const std::vector<Plane> old = regions.front();
                regions.pop_front();
                Add(old, 0, (uint32_t)old.size(), old[0].tag, old[0].launch);
            }
            Rendered(seq, call, 0, 0);
            return RT_OK;
        }
        PassSplit split = SplitPasses(npix, call.s0, call.s1, aheadEnd, workspaceLimit);
        if (split.refused.status != RT_OK) return Fail(split.refused.status, split.refused.message);
        const bool wasAhead = split.aheadEnd != 0;
        while (allocFailures != 0) {
            --allocFailures;
            ++g_shrinks;
            if (!ShrinkPass(split)) return Fail(RT_ERR_OUT_OF_MEMORY, "hipMalloc: out of memory");
        }
        if (wasAhead && split.aheadEnd == 0) ++g_shrinkWhileAhead;
        lastPasses = 0;
        for (Pass p = FirstPass(split); p.spp != 0; p = NextPass(split, p)) {
            CHECK(p.spp <= split.sppPass && (uint64_t)npix * p.spp < (1ull << 31) && (uint64_t)npix * split.sppPass * 12 <= workspaceLimit);
            ++launches;
            buffer.clear();
            for (uint32_t k = 0; k < p.spp; ++k) buffer.push_back(Plane{p.s + k, tag, launches});
            Add(buffer, p.add_first, p.add_count, tag, launches);
            ++lastPasses;
        }
        if (lastPasses > 1) ++g_multiPass;
        Rendered(seq, call, split.aheadEnd, split.sppTrace);
        if (split.aheadEnd) aheadLaunch = launches;
        return RT_OK;
    }

    // rt_render
    int Render(const PictureKey& pic, uint32_t s0, uint32_t s1, uint32_t depth, uint64_t seed, bool stats, std::vector<StepKind>* trace = nullptr) {
        lastStatus = RT_OK, lastMessage.clear();
        Call call;
        call.pic = pic, call.rows = RowsOf(pic), call.s0 = s0, call.s1 = s1, call.max_depth = depth, call.seed = seed, call.wants_stats = stats;
        const Steps steps = PlanRender(seq, call);
        CHECK(steps.n >= 1 && steps.n <= 3);
        for (uint32_t k = 0; k < steps.n; ++k) {
            const Step& step = steps.v[k];
            ++g_steps[(uint32_t)step.kind];
            if (trace) trace->push_back(step.kind);
            int rc = RT_OK;
            switch (step.kind) {
                case StepKind::AddAhead:
                    CHECK(seq.ahead.valid && buffer.size() == seq.ahead.spp);
                    Add(buffer, step.first, step.count, Tag(call), aheadLaunch);
                    AheadAdded(seq, step);
                    break;
                case StepKind::Record: Recorded(seq, call); break;
                case StepKind::RenderPending: rc = BatchFlush(); break;
                case StepKind::RenderNow: rc = RenderNow(call, step.aheadEnd); break;
                case StepKind::Refuse:
                    RenderBegins(seq);
                    rc = Fail(step.refusal.status, step.refusal.message);
                    break;
            }
            if (rc != RT_OK) return rc;
        }
        return RT_OK;
    }

    // the outside events, as rt_capi.hip's entries raise them; `expect`: what the contract says the event voids
    void Event(int which, uint32_t got, uint32_t expect) {
        ++g_events[which];
        CHECK(got == expect);
        if (got & kPending) CHECK(!seq.pend.on);
        if (got & kAhead) CHECK(!seq.ahead.valid);
        if (got & kAccumulation) CHECK(seq.accumulated == 0);
        DropVoided(got);
        if (got & kAccumulation) strip.clear();  // (nobody may read it any more: forget it, so that a read would show)
    }
    int SceneUpload() {
        const int rc = Settle(kSettleBeforeScene);
        if (rc != RT_OK) return rc;
        ++sceneEpoch;
        DropVoided(kTileOrder);  // (the tiles' tables go as soon as the scene's are overwritten)
        Event(kEvScene, SceneReplaced(seq), kAhead | kAccumulation | kInFlight | kFeatures | kDenoised);
        CHECK(seq.hasScene && !seq.pend.on);
        return RT_OK;
    }
    int SetStream() {
        const int rc = Settle(kSettleBeforeStream);
        if (rc != RT_OK) return rc;
        Event(kEvStream, StreamReplaced(seq), kAhead | kTileOrder);
        CHECK(!seq.pend.on && regions.empty());
        return RT_OK;
    }
    void SetSampler() {
        ++samplerEpoch;
        Event(kEvSampler, SamplerChanged(seq), kPending | kAhead | kAccumulation | kInFlight | kTileOrder | kFeatures);
    }
    void SetNoise(bool on) {
        const bool differs = on != seq.noise;
        Event(kEvNoise, NoiseToggled(seq, on), differs ? (kPending | kAhead | kAccumulation | kInFlight) : 0u);
        CHECK(seq.noise == on);
    }
    void Clear() { Event(kEvClear, Cleared(seq), kPending | kAhead | kAccumulation | kInFlight); }
    int SetBatch(uint32_t frames) {
        const int rc = Settle(kSettleBeforeBatchSetting);
        Event(kEvBatch, BatchSettingChanged(seq, frames), 0);
        CHECK(!seq.pend.on && seq.batchFrames == frames);
        return rc;
    }
    void SetLookahead(uint32_t frames) {
        Event(kEvLookahead, LookaheadSettingChanged(seq, frames), kAhead);
        CHECK(seq.lookahead == frames);
    }
    int SetPipelining(uint32_t depth) {
        int rc = Settle(kPending);
        if (rc != RT_OK) return rc;
        rc = Settle(kInFlight);
        Event(kEvPipelining, PipeliningSettingChanged(seq, depth), 0);
        CHECK(regions.empty() && seq.pipeDepth == depth);
        return rc;
    }
    int Synchronize() { return Settle(kSettleAtSynchronize); }
    // a reader: renders a pending batch that must be rendered, then hands out the committed strip; returns its sample count
    int Read(uint32_t* committed) {
        if (PendingMustRender(seq)) {
            const int rc = BatchFlush();
            if (rc != RT_OK) return rc;
        }
        if (seq.accumulated == 0) return RT_ERR_SEQUENCE;
        *committed = (uint32_t)strip.size();
        return RT_OK;
    }

    // what holds after every step of every script
    void Invariants() {
        CHECK(strip.size() + InFlight() == seq.accumulated);
        for (size_t k = 0; k < strip.size(); ++k) CHECK(strip[k].s == k + 1);
        if (seq.pipeDepth == 0) CHECK(regions.empty());
        CHECK(regions.size() <= seq.pipeDepth);
        if (seq.ahead.valid) {
            const State::Ahead& a = seq.ahead;
            CHECK(buffer.size() == a.spp && a.next == seq.accumulated + 1 && a.next > a.base && a.next <= a.base + a.spp && a.pic == seq.pic);
            for (size_t k = 0; k < buffer.size(); ++k) CHECK(buffer[k].s == a.base + k && buffer[k].launch == aheadLaunch);
            CHECK(regions.empty());  // (a batch may be pending beside it, after rt_set_frame_batch: rendering the batch drops it)
        }
        if (seq.pend.on) {
            const State::Pending& p = seq.pend;
            CHECK(p.s1 > p.s0 && p.s1 - p.s0 < seq.batchFrames && p.rows != 0);
            CHECK(p.s0 == 1 || (seq.accumulated != 0 && p.s0 == seq.accumulated + 1 && p.pic == seq.pic));
            CHECK(regions.empty());
        }
    }
};

// ------------------------------------------------------------------------------------------------------------- scenarios
// Written from the contract in include/rt_api.h; each starts from a context with a scene.
const PictureKey A = Pic(64, 32), B = Pic(72, 30);
typedef std::vector<StepKind> Trace;
const StepKind ADD = StepKind::AddAhead, REC = StepKind::Record, PEND = StepKind::RenderPending, NOW = StepKind::RenderNow, REF = StepKind::Refuse;

Model Fresh() {
    Model m;
    CHECK(m.SceneUpload() == RT_OK);
    return m;
}
// call f of a progressive sequence: sample plane f alone
int Frame(Model& m, uint32_t f, Trace* t = nullptr, const PictureKey& pic = A, uint32_t depth = 8, uint64_t seed = 1, bool stats = false) {
    return m.Render(pic, f, f + 1, depth, seed, stats, t);
}
uint32_t Committed(Model& m) {
    uint32_t n = 0xffffffffu;
    CHECK(m.Read(&n) == RT_OK);
    return n;
}

void ScenarioBatchOfFour() {
    Model m = Fresh();
    CHECK(m.SetBatch(4) == RT_OK);
    for (uint32_t f = 1; f <= 6; ++f) CHECK(Frame(m, f) == RT_OK);
    CHECK(m.strip.size() == 4 && m.seq.pend.on && m.seq.pend.s1 - m.seq.pend.s0 == 2);  // committed 4 with 2 pending
    CHECK(Committed(m) == 4 && m.seq.pend.on);                                            // a reader leaves them pending
    CHECK(m.Synchronize() == RT_OK && m.strip.size() == 6 && !m.seq.pend.on);             // rt_synchronize commits 6
    CHECK(m.launches == 2);
}
void ScenarioReaderRendersAStartingBatch() {
    Model m = Fresh();
    CHECK(m.SetBatch(4) == RT_OK);
    CHECK(Frame(m, 1) == RT_OK && Frame(m, 2) == RT_OK && m.strip.empty());
    CHECK(Committed(m) == 2 && !m.seq.pend.on);  // nothing committed yet: rendered first
    CHECK(Frame(m, 3) == RT_OK);
    CHECK(Frame(m, 1, nullptr, B) == RT_OK);     // a restart at another size: flushes frame 3, then waits
    CHECK(m.seq.pend.on && m.seq.pend.s0 == 1 && m.strip.size() == 3);
    CHECK(Committed(m) == 1 && m.seq.pic == B);  // the caller's picture is the new one
}
void ScenarioStatsSettleTheBatch() {
    Model m = Fresh();
    CHECK(m.SetBatch(4) == RT_OK);
    CHECK(Frame(m, 1) == RT_OK && Frame(m, 2) == RT_OK);
    Trace t;
    CHECK(Frame(m, 3, &t, A, 8, 1, true) == RT_OK);
    CHECK((t == Trace{PEND, NOW}) && m.strip.size() == 3 && !m.seq.pend.on);
}
void ScenarioOtherSettingsSettleAndStartTheirOwn() {
    for (int what = 0; what < 3; ++what) {
        Model m = Fresh();
        CHECK(m.SetBatch(4) == RT_OK);
        CHECK(Frame(m, 1) == RT_OK && Frame(m, 2) == RT_OK);
        Trace t;
        if (what == 0) CHECK(Frame(m, 3, &t, A, 8, 2) == RT_OK);   // another seed
        if (what == 1) CHECK(Frame(m, 3, &t, A, 9, 1) == RT_OK);   // another depth
        if (what == 2) CHECK(Frame(m, 1, &t, B, 8, 1) == RT_OK);   // another size (which can only start over)
        CHECK((t == Trace{PEND, REC}) && m.strip.size() == 2 && m.seq.pend.on && m.seq.pend.s1 - m.seq.pend.s0 == 1);
        CHECK(m.Synchronize() == RT_OK && m.strip.size() == (what == 2 ? 1u : 3u));
    }
}
void ScenarioLookaheadOfFour() {
    Model m = Fresh();
    m.SetLookahead(4);
    for (uint32_t f = 1; f <= 5; ++f) {
        Trace t;
        CHECK(Frame(m, f, &t) == RT_OK);
        CHECK(t == Trace{(f == 1 || f == 5) ? NOW : ADD});  // calls 2..4 only add
        CHECK(m.strip.size() == f && Committed(m) == f);    // display lag 0
        if (f == 1) CHECK(m.buffer.size() == 4 && m.buffer[0].s == 1 && m.buffer[3].s == 4);  // call 1 traces [1, 5)
        if (f == 5) CHECK(m.buffer.size() == 4 && m.buffer[0].s == 5 && m.buffer[3].s == 8);  // call 5 traces [5, 9)
    }
    CHECK(m.launches == 2);
}
void ScenarioLookaheadLongCall() {
    Model m = Fresh();
    m.SetLookahead(4);
    CHECK(m.Render(A, 1, 7, 8, 1, false) == RT_OK);
    CHECK(m.launches == 1 && m.buffer.size() == 6 && m.strip.size() == 6 && !m.seq.ahead.valid);  // 6 planes traced, none ahead
}
void ScenarioLookaheadDropsWhatDoesNotContinue() {
    Model m = Fresh();
    m.SetLookahead(4);
    CHECK(Frame(m, 1) == RT_OK && Frame(m, 2) == RT_OK && m.seq.ahead.valid);
    Trace t;
    CHECK(Frame(m, 3, &t, A, 8, 2) == RT_OK);  // another seed: traced anew
    CHECK(t == Trace{NOW} && m.launches == 2 && m.buffer[0].s == 3 && m.strip.size() == 3);
    CHECK(Frame(m, 4, nullptr, A, 8, 2, true) == RT_OK && !m.seq.ahead.valid && m.launches == 3);  // a call with statistics drops it
    CHECK(Frame(m, 5, nullptr, A, 8, 2) == RT_OK && m.seq.ahead.valid);
    m.Clear();
    CHECK(!m.seq.ahead.valid);
    CHECK(Frame(m, 1) == RT_OK && Frame(m, 1) == RT_OK && m.strip.size() == 1 && m.launches == 6);  // a restart traces anew
}
void ScenarioPrecedence() {
    {   // lookahead is ignored while batching is on
        Model m = Fresh();
        m.SetLookahead(4);
        CHECK(m.SetBatch(2) == RT_OK);
        Trace t;
        CHECK(Frame(m, 1, &t) == RT_OK && Frame(m, 2, &t) == RT_OK);
        CHECK((t == Trace{REC, REC, PEND}) && m.buffer.size() == 2 && !m.seq.ahead.valid);
    }
    {   // lookahead and batching are ignored while pipelining is on
        Model m = Fresh();
        m.SetLookahead(4);
        CHECK(m.SetBatch(2) == RT_OK && m.SetPipelining(2) == RT_OK);
        Trace t;
        for (uint32_t f = 1; f <= 4; ++f) CHECK(Frame(m, f, &t) == RT_OK);
        CHECK((t == Trace{NOW, NOW, NOW, NOW}) && !m.seq.pend.on && !m.seq.ahead.valid);
        CHECK(m.strip.size() == 2 && m.regions.size() == 2 && m.seq.accumulated == 4);  // the newest two calls in flight
        CHECK(Committed(m) == 2);
        CHECK(Frame(m, 5, nullptr, A, 8, 1, true) == RT_OK && m.strip.size() == 5);     // a call with statistics settles everything first
        CHECK(Frame(m, 6) == RT_OK && m.Synchronize() == RT_OK && m.strip.size() == 6);
        m.SetNoise(true);                                                                 // second moments: every call unpipelined
        CHECK(Frame(m, 1) == RT_OK && m.regions.empty() && m.strip.size() == 1);
    }
}
void ScenarioSequenceErrors() {
    Model m;
    CHECK(Frame(m, 1) == RT_ERR_NO_SCENE && m.lastMessage == "rt_render: no scene uploaded");
    CHECK(m.SceneUpload() == RT_OK);
    for (int mode = 0; mode < 4; ++mode) {
        m.Clear();
        CHECK(m.SetBatch(mode == 1 ? 3 : 1) == RT_OK && m.SetPipelining(mode == 3 ? 2 : 0) == RT_OK);
        m.SetLookahead(mode == 2 ? 4 : 1);
        CHECK(Frame(m, 2) == RT_ERR_SEQUENCE && m.lastMessage == "rt_render: first call of an accumulation must start at s0 == 1");
        CHECK(m.Render(A, 0, 1, 8, 1, false) == RT_ERR_INVALID_ARG && m.lastMessage == "rt_render: empty image or sample range");
        CHECK(m.Render(Pic(64, 32, 16, 32), 1, 2, 8, 1, false) == RT_ERR_INVALID_ARG && m.lastMessage == "rt_render: bad row set");
        CHECK(Frame(m, 1) == RT_OK && Frame(m, 2) == RT_OK);
        CHECK(Frame(m, 4) == RT_ERR_SEQUENCE && m.lastMessage == "rt_render: sample range or row set does not continue the accumulation");
        CHECK(m.Synchronize() == RT_OK && m.strip.size() == 2);  // a refusal leaves the accumulation as it was
        CHECK(Frame(m, 3, nullptr, B) == RT_ERR_SEQUENCE && m.lastMessage == "rt_render: sample range or row set does not continue the accumulation");
        CHECK(Frame(m, 3) == RT_OK && m.Synchronize() == RT_OK && m.strip.size() == 3);
    }
}
// each outside event in each mode, arriving after three 1-spp calls: what is committed afterwards, and what the next call may be
void ScenarioEventsInEveryMode() {
    for (int mode = 0; mode < 4; ++mode)
        for (int ev = 0; ev < 9; ++ev) {
            g_where = "events mode " + std::to_string(mode) + " event " + std::to_string(ev);
            Model m = Fresh();
            CHECK(m.SetBatch(mode == 1 ? 4 : 1) == RT_OK && m.SetPipelining(mode == 3 ? 2 : 0) == RT_OK);
            m.SetLookahead(mode == 2 ? 4 : 1);
            for (uint32_t f = 1; f <= 3; ++f) CHECK(Frame(m, f) == RT_OK);
            CHECK(m.seq.pend.on == (mode == 1) && m.seq.ahead.valid == (mode == 2) && m.regions.size() == (mode == 3 ? 2u : 0u));
            bool voids = true;  // the accumulation is void afterwards: the next call must start at s0 == 1
            switch (ev) {
                case 0: CHECK(m.SceneUpload() == RT_OK); break;
                case 1: CHECK(m.SetStream() == RT_OK); voids = false; break;
                case 2: m.SetSampler(); break;
                case 3: m.SetNoise(true); break;
                case 4: m.Clear(); break;
                case 5: m.Event(kEvFailed, StepFailed(m.seq), kAhead | kAccumulation | kInFlight); CHECK(!m.seq.pend.on || mode == 1); m.seq.pend.on = false; break;
                case 6: CHECK(m.SetBatch(2) == RT_OK); voids = false; break;
                case 7: m.SetLookahead(2); voids = false; break;
                case 8: CHECK(m.SetPipelining(1) == RT_OK); voids = false; break;
            }
            CHECK(!m.seq.ahead.valid || ev == 6 || ev == 8);  // nothing traced ahead survives (the batch and pipelining setters leave it: it was not theirs)
            m.Invariants();
            if (voids) {
                CHECK(m.seq.accumulated == 0 && !m.seq.pend.on && m.regions.empty());
                CHECK(Frame(m, 4) == RT_ERR_SEQUENCE);
                CHECK(Frame(m, 1) == RT_OK && m.Synchronize() == RT_OK && m.strip.size() == 1);
            } else {
                // stream and pipelining settle everything first, the batch setter the batch; the lookahead setter touches neither
                if (ev == 1 || ev == 8 || (ev == 6 && mode != 3)) CHECK(m.strip.size() == 3 && !m.seq.pend.on && m.regions.empty());
                CHECK(Frame(m, 4) == RT_OK && m.Synchronize() == RT_OK && m.strip.size() == 4);
            }
        }
    g_where = "scenarios";
}
// the render-ahead fallback (first item): the buffer of [s0, aheadEnd) cannot be had, a smaller one can
void ScenarioShrinkWhileAhead() {
    Model m = Fresh();
    m.SetLookahead(16);
    m.allocFailures = 1;  // 16 planes fail, 8 would fit
    CHECK(Frame(m, 1) == RT_OK);
    CHECK(m.strip.size() == 1 && m.lastPasses == 1 && m.buffer.size() == 1 && !m.seq.ahead.valid);  // its own plane only, nothing kept
    CHECK(Frame(m, 2) == RT_OK && m.seq.ahead.valid && m.buffer.size() == 16);                      // the next call traces ahead again
    PassSplit p = SplitPasses(64 * 32, 5, 8, 5 + 16, 8ull << 30);
    CHECK(p.aheadEnd == 21 && p.sppTrace == 16 && p.sppPass == 16);
    CHECK(ShrinkPass(p) && p.aheadEnd == 0 && p.sppTrace == 3 && p.sppPass == 3);
    CHECK(ShrinkPass(p) && p.sppPass == 2 && ShrinkPass(p) && p.sppPass == 1 && !ShrinkPass(p));
}
void ScenarioPassSplit() {
    const uint32_t npix = 72 * 30;
    PassSplit p = SplitPasses(npix, 1, 101, 0, 1u << 20);  // 1 MiB / (2160 * 12) = 40 planes
    CHECK(p.refused.status == RT_OK && p.sppPass == 40 && p.sppTrace == 100 && p.aheadEnd == 0);
    uint32_t n = 0, next = 1;
    for (Pass q = FirstPass(p); q.spp != 0; q = NextPass(p, q), ++n) {
        CHECK(q.s == next && q.add_first == 0 && q.add_count == q.spp);
        next += q.spp;
    }
    CHECK(n == 3 && next == 101);
    CHECK(SplitPasses(npix, 1, 2, 50, 1u << 20).aheadEnd == 0);   // 49 planes traced ahead do not share one pass of 40
    CHECK(SplitPasses(npix, 1, 2, 41, 1u << 20).aheadEnd == 41);
    CHECK(SplitPasses(npix, 1, 3, 3, 1u << 20).aheadEnd == 0);    // nothing beyond the call's own
    CHECK(SplitPasses(1u << 20, 1, 2, 0, 1u << 20).refused.status == RT_ERR_OUT_OF_MEMORY);
    CHECK(SplitPasses(1u << 30, 1, 9, 0, ~0ull).sppPass == 1);    // total_paths stays below 2^31
}

const struct {
    const char* name;
    void (*run)();
} kScenarios[] = {
    {"batch of four", ScenarioBatchOfFour},
    {"a reader renders a batch that starts", ScenarioReaderRendersAStartingBatch},
    {"statistics settle the batch", ScenarioStatsSettleTheBatch},
    {"other seed, depth or size", ScenarioOtherSettingsSettleAndStartTheirOwn},
    {"lookahead of four", ScenarioLookaheadOfFour},
    {"lookahead, a call of six planes", ScenarioLookaheadLongCall},
    {"lookahead drops what does not continue", ScenarioLookaheadDropsWhatDoesNotContinue},
    {"precedence of the modes", ScenarioPrecedence},
    {"sequence errors", ScenarioSequenceErrors},
    {"events in every mode", ScenarioEventsInEveryMode},
    {"shrink while tracing ahead", ScenarioShrinkWhileAhead},
    {"pass split", ScenarioPassSplit},
};

// ------------------------------------------------------------------------------------------------------------ model check
// One random script.  Next to the model's own checks the script keeps, from the contract alone, how many samples the caller has
// been promised (`promised`: committed or pending) and of which picture, and so which status every call must have.
void RunScript(uint64_t seed, uint32_t steps) {
    Rng R{seed * 0x9e3779b97f4a7c15ull + 1};
    Model m;
    const PictureKey pics[3] = {A, B, Pic(64, 32, 8, 16)};
    uint32_t promised = 0, depth = 8;
    uint64_t rseed = 1;
    PictureKey pic = pics[R.below(3)];
    if (!R.one_in(8)) CHECK(m.SceneUpload() == RT_OK);
    // an entry that settles a batch first can meet the batch's error: the one the script provokes is a workspace limit set, after the
    // batch was recorded, below one plane of its picture -- then the entry has not happened, and the promise is what is left
    const auto settled = [&](int rc) {
        if (rc == RT_OK) return true;
        CHECK(rc == RT_ERR_OUT_OF_MEMORY && m.lastMessage == "rt_render: workspace limit below one sample per pixel");
        promised = m.seq.accumulated;
        if (promised != 0) pic = m.seq.pic;
        return false;
    };
    for (uint32_t k = 0; k < steps; ++k) {
        g_where = "script " + std::to_string(seed) + " step " + std::to_string(k);
        const uint32_t op = R.below(100);
        if (op < 70) {
            // a call: mostly the one that continues, sometimes a restart, another picture, a gap, an empty range, other settings
            const uint32_t kind = R.below(20);
            PictureKey p = pic;
            uint32_t s0 = promised + 1;
            if (kind == 0 || promised == 0) s0 = 1;
            if (kind == 1) s0 = promised + 2;
            if (kind == 2) p = pics[R.below(3)];
            if (kind == 3) depth = 4 + R.below(4);
            if (kind == 4) rseed = 1 + R.below(3);
            uint32_t s1 = s0 + (R.one_in(4) ? 1 + R.below(9) : 1);
            if (kind == 5) s1 = s0;
            const bool stats = R.one_in(10);
            if (R.one_in(6)) m.allocFailures = 1 + R.below(4);
            const uint32_t injected = m.allocFailures;
            const int rc = m.Render(p, s0, s1, depth, rseed, stats);
            m.allocFailures = 0;
            int want = RT_OK;
            if (!m.seq.hasScene) want = RT_ERR_NO_SCENE;
            else if (s1 <= s0) want = RT_ERR_INVALID_ARG;
            else if (s0 != 1 && (promised == 0 || s0 != promised + 1 || p != pic)) want = RT_ERR_SEQUENCE;
            if (rc == RT_ERR_OUT_OF_MEMORY) {
                // a buffer of one plane was refused (injected), or the limit is below one plane of this picture -- in this call or in the
                // batch it settled: the promise is what is left
                CHECK(injected != 0 || m.lastMessage == "rt_render: workspace limit below one sample per pixel");
                promised = m.seq.accumulated;
                if (promised != 0) pic = m.seq.pic;
            } else {
                CHECK(rc == want);
                if (rc == RT_OK) promised = s1 - 1, pic = p;
            }
        } else if (op < 76) {
            uint32_t n = 0;
            const int rc = m.Read(&n);
            if (rc != RT_ERR_SEQUENCE) settled(rc);
            else CHECK(promised == 0);
            if (rc == RT_OK) CHECK(promised != 0 && n == m.strip.size() && n + m.InFlight() == m.seq.accumulated && n <= promised && m.seq.pic == pic);
        } else if (op < 80) {
            if (settled(m.Synchronize())) CHECK(m.strip.size() == promised && !m.seq.pend.on && m.regions.empty());
        } else if (op < 83) {
            settled(m.SetBatch(R.one_in(3) ? 1 : 2 + R.below(5)));
        } else if (op < 86) {
            m.SetLookahead(R.one_in(3) ? 1 : 2 + R.below(7));
        } else if (op < 89) {
            settled(m.SetPipelining(R.one_in(3) ? 0 : 1 + R.below(3)));
        } else if (op < 91) {
            if (settled(m.SceneUpload())) promised = 0;
        } else if (op < 93) {
            if (settled(m.SetStream())) CHECK(m.strip.size() == promised);
        } else if (op < 94) {
            m.SetSampler();
            promised = 0;
        } else if (op < 96) {
            const bool on = R.one_in(2);
            if (on != m.seq.noise) promised = 0;
            m.SetNoise(on);
        } else if (op < 97) {
            m.Clear();
            promised = 0;
        } else if (op < 98) {
            if (settled(m.SceneUpload())) {  // another class of scene: one the carrying kernel does or does not exist for
                m.kernelCarries = !R.one_in(3);
                promised = 0;
            }
        } else {
            const uint64_t plane = (uint64_t)pic.W * RowsOf(pic) * 12;
            m.workspaceLimit = R.one_in(2) ? (8ull << 30) : plane * (1 + R.below(5));
        }
        CHECK(promised == (m.seq.pend.on ? m.seq.pend.s1 - 1 : m.seq.accumulated));
        m.Invariants();
        if (g_failures) return;
    }
    g_where = "script " + std::to_string(seed) + " end";
    if (settled(m.Synchronize())) CHECK(m.strip.size() == promised);
    m.Invariants();
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
    // (StepFailed is raised by rt_capi.hip where a launch fails, which the model's launches never do: the scenarios raise it)
    for (uint32_t k = 0; k < scripts && g_failures == 0; ++k) RunScript(k, steps);
    printf("steps:");
    bool allReached = true;
    for (int k = 0; k < 5; ++k) printf(" %s %llu", kStepName[k], (unsigned long long)g_steps[k]), allReached = allReached && g_steps[k] != 0;
    printf("\nevents:");
    for (int k = 0; k < kEvCount; ++k) printf(" %s %llu", kEvName[k], (unsigned long long)g_events[k]), allReached = allReached && g_events[k] != 0;
    printf("\nshrinks %llu, shrink-while-ahead %llu, calls of several passes %llu, pipelined calls %llu\n", (unsigned long long)g_shrinks,
           (unsigned long long)g_shrinkWhileAhead, (unsigned long long)g_multiPass, (unsigned long long)g_pipelined);
    allReached = allReached && g_shrinks != 0 && g_shrinkWhileAhead != 0 && g_multiPass != 0 && g_pipelined != 0;
    if (!allReached) fprintf(stderr, "FAIL: a kind of step, an event or the shrink-while-ahead case was never reached\n");
    if (g_failures != 0 || !allReached) {
        printf("sequence_selftest: FAILED (%d checks)\n", g_failures);
        return 1;
    }
    printf("%u scenarios, %u scripts of %u steps\nsequence_selftest: ok\n", nScenarios, scripts, steps);
    return 0;
}
