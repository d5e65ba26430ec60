// rt_sequence.cpp -- the sequencing of rt_render calls (rt_sequence.h): plain C++, no HIP header, no environment, no allocation.
#include "rt_sequence.h"

namespace rtseq {

namespace {

bool SameSettings(const Call& c, const PictureKey& pic, uint32_t max_depth, uint64_t seed) {
    return pic == c.pic && max_depth == c.max_depth && seed == c.seed;
}
// (what every mode but the plain one asks of a call before it looks at it: the plain path's checks would refuse the others)
bool Renderable(const State& st, const Call& c) { return st.hasScene && c.pic.W != 0 && c.pic.H != 0 && c.s0 != 0 && c.s1 > c.s0; }
bool StartsNew(const State& st, const Call& c) { return c.s0 == 1 || st.accumulated == 0; }

void Push(Steps& S, StepKind kind) {
    S.v[S.n] = Step{};
    S.v[S.n++].kind = kind;
}

}  // namespace

// ------------------------------------------------------------------------------------------------------------------ events
uint32_t SceneReplaced(State& st) {
    // (the batch was settled under the old scene, kSettleBeforeScene; the tiles' tables went as soon as theirs were overwritten)
    st.hasScene = true;
    st.ahead.valid = false;
    st.accumulated = 0;
    return kAhead | kAccumulation | kInFlight | kFeatures | kDenoised;  // the feature strips and the denoised picture belonged to the scene that was replaced
}

uint32_t CameraChanged(State& st) {
    // (the batch was settled under the old camera, kSettleBeforeCamera; hasScene is the caller's precondition and stays as it is)
    st.ahead.valid = false;  // planes traced ahead were traced through the old camera
    st.accumulated = 0;      // samples of two cameras do not mix: the next rt_render starts over
    return kAhead | kAccumulation | kInFlight | kFeatures | kDenoised;  // frames in flight, feature strips and snapshot were the old camera's too
}

uint32_t StreamReplaced(State& st) {
    st.ahead.valid = false;  // planes traced ahead were produced on the old stream
    return kAhead | kTileOrder;  // ... and so were the order, the flags and the copy of their count
}

uint32_t SamplerChanged(State& st) {
    st.pend.on = false;      // pending frames of the old mapping are dropped with the accumulation they belonged to
    st.ahead.valid = false;  // (and the planes traced ahead, which no call could reach any more: they need accumulated + 1 == s0 > 1)
    st.accumulated = 0;      // samples of two mappings do not mix: the next rt_render starts over
    return kPending | kAhead | kAccumulation | kInFlight | kTileOrder | kFeatures;  // the pilot rays and the feature pass's primary rays use the lens mapping
}

uint32_t NoiseToggled(State& st, bool on) {
    uint32_t voids = 0;
    if (on != st.noise) {
        st.pend.on = false;  // as SamplerChanged: pending frames go with the accumulation they belonged to
        st.ahead.valid = false;
        st.accumulated = 0;  // a strip of moments cannot start in the middle: the next rt_render starts over
        voids = kPending | kAhead | kAccumulation | kInFlight;
    }
    st.noise = on;
    return voids;
}

uint32_t Cleared(State& st) {
    st.pend.on = false;
    st.ahead.valid = false;
    st.accumulated = 0;
    return kPending | kAhead | kAccumulation | kInFlight;
}

uint32_t StepFailed(State& st) {
    // some planes may already have been added to the strip: the accumulation is void, the next call must restart at s0 == 1
    st.ahead.valid = false;
    st.accumulated = 0;
    return kAhead | kAccumulation | kInFlight;
}

uint32_t TileTablesDropped(State& st) {
    st.ahead.valid = false;  // planes traced ahead by a truncated launch are only complete together with the flags
    return kAhead;
}

uint32_t BatchSettingChanged(State& st, uint32_t frames) {
    st.batchFrames = frames;  // (the batch was settled first, kSettleBeforeBatchSetting)
    return 0;
}

uint32_t LookaheadSettingChanged(State& st, uint32_t frames) {
    st.lookahead = frames;
    st.ahead.valid = false;
    return kAhead;
}

uint32_t PipeliningSettingChanged(State& st, uint32_t depth) {
    st.pipeDepth = depth;  // (batch and frames in flight were settled first)
    return 0;
}

uint32_t AccumulationStarting(const State& st, const Call& c) {
    return StartsNew(st, c) ? kInFlight : 0u;  // a new accumulation abandons whatever was in flight
}

void AccumulationStarted(State& st, const Call& c) {
    st.pic = c.pic;
    st.rows = c.rows;
    st.accumulated = 0;
}

// ------------------------------------------------------------------------------------------------------------------- steps
void AheadAdded(State& st, const Step& s) {
    st.ahead.next += s.count;
    st.accumulated += s.count;
}

void Recorded(State& st, const Call& c) {
    State::Pending& p = st.pend;
    if (!p.on) {
        p.on = true;
        p.pic = c.pic, p.rows = c.rows, p.s0 = c.s0, p.max_depth = c.max_depth, p.seed = c.seed;
    }
    p.s1 = c.s1;
}

Call PendingTaken(State& st) {
    const State::Pending& p = st.pend;
    Call c;
    c.pic = p.pic, c.rows = p.rows, c.s0 = p.s0, c.s1 = p.s1, c.max_depth = p.max_depth, c.seed = p.seed;
    st.pend.on = false;
    return c;
}

bool PendingMustRender(const State& st) { return st.pend.on && (st.accumulated == 0 || st.pend.s0 == 1u); }

void RenderBegins(State& st) { st.ahead.valid = false; }

Refusal CheckCall(const State& st, const Call& c) {
    if (!st.hasScene) return {RT_ERR_NO_SCENE, "rt_render: no scene uploaded"};
    if (c.pic.W == 0 || c.pic.H == 0 || c.s0 == 0 || c.s1 <= c.s0) return {RT_ERR_INVALID_ARG, "rt_render: empty image or sample range"};
    if (c.rows == 0) return {RT_ERR_INVALID_ARG, "rt_render: bad row set"};
    if ((uint64_t)c.pic.W * c.rows > (1ull << 31) || (uint64_t)c.pic.W * c.pic.H > 0xffffffffull) return {RT_ERR_INVALID_ARG, "rt_render: image too large"};
    return {};
}

bool MayPipeline(const State& st, const Call& c) {
    return st.pipeDepth > 0 && !c.wants_stats && !st.noise && (uint64_t)c.pic.W * c.rows * (c.s1 - c.s0) * (st.pipeDepth + 2u) < (1ull << 31);
}

Admission Admit(const State& st, const Call& c, Refusal* why) {
    if (StartsNew(st, c)) {
        if (c.s0 == 1) return Admission::Starts;
        *why = {RT_ERR_SEQUENCE, "rt_render: first call of an accumulation must start at s0 == 1"};
        return Admission::Refused;
    }
    if (st.pic == c.pic && c.s0 == st.accumulated + 1) return Admission::Continues;
    *why = {RT_ERR_SEQUENCE, "rt_render: sample range or row set does not continue the accumulation"};
    return Admission::Refused;
}

void Rendered(State& st, const Call& c, uint32_t aheadEnd, uint32_t sppTrace) {
    st.accumulated += c.s1 - c.s0;
    if (aheadEnd) {  // the planes [s1, aheadEnd) wait in the sample buffer
        State::Ahead& a = st.ahead;
        a.valid = true;
        a.pic = c.pic, a.max_depth = c.max_depth, a.seed = c.seed;
        a.base = c.s0, a.spp = sppTrace, a.next = c.s1;
    }
}

Steps PlanRender(const State& st, const Call& c) {
    Steps S;
    const bool deferrable = !c.wants_stats && st.pipeDepth == 0 && Renderable(st, c);  // (pipelining takes precedence over both)
    if (st.lookahead > 1 && st.batchFrames <= 1 && deferrable) {
        // render-ahead: the planes of this call may have been traced by an earlier call's launch -- then they are only ADDED (in
        // sample order, as always); else this call's launch traces its own planes and the next `lookahead` ones with them
        const State::Ahead& a = st.ahead;
        if (a.valid && SameSettings(c, a.pic, a.max_depth, a.seed) && c.s0 == a.next && c.s1 <= a.base + a.spp && st.accumulated + 1 == c.s0) {
            Push(S, StepKind::AddAhead);
            S.v[0].first = c.s0 - a.base, S.v[0].count = c.s1 - c.s0;
            return S;
        }
        const uint32_t want = c.s1 - c.s0 > st.lookahead ? c.s1 - c.s0 : st.lookahead;
        Push(S, StepKind::RenderNow);
        S.v[0].aheadEnd = c.s0 + want;
        return S;
    }
    State sim = st;  // the steps planned so far, taken as done
    const auto renderPending = [&]() {
        Push(S, StepKind::RenderPending);
        const Call p = PendingTaken(sim);
        Refusal why;
        if (Admit(sim, p, &why) == Admission::Starts) AccumulationStarted(sim, p);
        Rendered(sim, p, 0, 0);
    };
    if (st.batchFrames > 1 && deferrable) {
        // a pending batch this call does not continue is rendered first, as the calls were made
        if (sim.pend.on && !(SameSettings(c, sim.pend.pic, sim.pend.max_depth, sim.pend.seed) && sim.pend.s1 == c.s0)) renderPending();
        // only a call that the plain path would accept as the start or the continuation of an accumulation is deferred
        Refusal why;
        if (sim.pend.on || (c.rows != 0 && Admit(sim, c, &why) != Admission::Refused)) {
            Push(S, StepKind::Record);
            Recorded(sim, c);
            if (sim.pend.s1 - sim.pend.s0 >= st.batchFrames) renderPending();
            return S;
        }
    }
    if (sim.pend.on) renderPending();  // a call with statistics (or one that cannot be deferred) settles the pending batch first
    const Refusal bad = CheckCall(st, c);
    Push(S, bad.status != RT_OK ? StepKind::Refuse : StepKind::RenderNow);
    S.v[S.n - 1].refusal = bad;
    return S;
}

// --------------------------------------------------------------------------------------------------------------- pass split
PassSplit SplitPasses(uint32_t npix, uint32_t s0, uint32_t s1, uint32_t aheadEnd, uint64_t workspaceLimit) {
    PassSplit p;
    p.s0 = s0, p.s1 = s1;
    const uint64_t bytesPerSpp = (uint64_t)npix * 12;
    uint64_t sppMax = workspaceLimit / bytesPerSpp;
    const uint64_t sppPathCap = ((1ull << 31) - 1) / npix;  // total_paths stays below 2^31
    if (sppMax > sppPathCap) sppMax = sppPathCap;
    if (sppMax == 0) {
        p.refused = {RT_ERR_OUT_OF_MEMORY, "rt_render: workspace limit below one sample per pixel"};
        return p;
    }
    if (aheadEnd <= s1 || (uint64_t)(aheadEnd - s0) > sppMax) aheadEnd = 0;  // the planes traced ahead must share one pass
    p.aheadEnd = aheadEnd;
    p.sppTrace = aheadEnd ? aheadEnd - s0 : s1 - s0;
    p.sppPass = (uint32_t)(sppMax < p.sppTrace ? sppMax : p.sppTrace);
    return p;
}

bool ShrinkPass(PassSplit& p) {
    if (p.sppPass <= 1u) return false;
    p.sppPass = (p.sppPass + 1u) / 2u;
    if (p.aheadEnd != 0 && p.sppPass < p.sppTrace) {
        // Several passes share the sample buffer, so no plane beyond this call's own could wait in it: give up tracing ahead and
        // render [s0, s1) in ordinary passes.  (Tracing on in several passes added planes nobody had asked for to the strip.)
        p.aheadEnd = 0;
        p.sppTrace = p.s1 - p.s0;
        if (p.sppPass > p.sppTrace) p.sppPass = p.sppTrace;
    }
    return true;
}

static Pass PassFrom(const PassSplit& p, uint32_t s) {
    const uint32_t end = p.aheadEnd ? p.aheadEnd : p.s1;
    Pass q;
    if (p.sppPass == 0 || s >= end) return q;
    q.s = s;
    q.spp = end - s < p.sppPass ? end - s : p.sppPass;
    // of the planes traced, the call's own: [s, s + spp) within [s0, s1)
    q.add_first = 0;
    q.add_count = s >= p.s1 ? 0u : (p.s1 - s < q.spp ? p.s1 - s : q.spp);
    return q;
}
Pass FirstPass(const PassSplit& p) { return PassFrom(p, p.s0); }
Pass NextPass(const PassSplit& p, const Pass& cur) { return PassFrom(p, cur.s + cur.spp); }

}  // namespace rtseq
