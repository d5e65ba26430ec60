// rt_tile_tables.cpp -- the bookkeeping of the per-tile tables (rt_tile_tables.h): plain C++, no HIP header, no environment, no allocation.
#include "rt_tile_tables.h"

namespace rttile {

// ------------------------------------------------------------------------------------------------------------------ events
void SceneReplaced(State& st) {
    Dropped(st);
    st.masks.valid = false;
}

void CameraChanged(State& st) {
    // No host wait separates the old camera's tables from the new one's: a copy of the old count may still be on its way.  It can
    // never be taken for the new picture's -- pending is false until the rebuild's own copy is recorded behind it on the same
    // stream, and the one event is recorded again after that copy, so it completes only once the newer word has landed
    // (DESIGN.md 4.3).
    Dropped(st);
    st.masks.valid = false;
}

void Dropped(State& st) {
    st.order.keyValid = st.order.orderValid = st.order.flagsValid = false;
    st.count.pending = st.count.known = false;  // (a copy on its way lands in the pinned word unread; a newer one follows it on the stream)
}

void AccumulationStarts(State& st, const Knobs& knobs) {
    st.skySkip = knobs.skipSky;
    st.skyExclude = knobs.excludeSky;
}

void CountArrived(State& st, uint32_t n) {
    if (!st.count.pending) return;  // dropped since the copy was recorded: not this build's number
    st.count.pending = false;
    st.count.known = true;
    st.count.value = n;
}

void CountFailed(State& st) { st.count.pending = false; }

// ------------------------------------------------------------------------------------------------------------------- masks
MaskPlan PlanMasks(State& st, const PictureKey& pic, uint32_t npix, const Knobs& knobs, bool sceneTakesMasks) {
    MaskPlan p;
    p.nFull = npix >> 6;
    p.limit = knobs.primaryMaskLimit;
    p.sphLimit = knobs.primarySpheres;
    State::Masks& m = st.masks;
    if (!(knobs.primaryMask && p.nFull != 0u && sceneTakesMasks)) {
        m.valid = false;
        p.answer = MaskAnswer::NotWanted;
    } else if (m.valid && m.pic == pic && m.limit == p.limit && m.spheres == p.sphLimit) {
        p.answer = MaskAnswer::Keep;
    } else {
        m.valid = false;
        p.answer = MaskAnswer::Build;
    }
    return p;
}

void MasksBuilt(State& st, const PictureKey& pic, const MaskPlan& p) {
    st.masks.valid = true;
    st.masks.pic = pic;
    st.masks.limit = p.limit;
    st.masks.spheres = p.sphLimit;
    st.masks.tiles = p.nFull;
}

uint32_t MaskTiles(const State& st) { return st.masks.valid ? st.masks.tiles : 0u; }
uint32_t ListTiles(const State& st) { return (st.masks.valid && st.masks.spheres != 0u) ? st.masks.tiles : 0u; }

// --------------------------------------------------------------------------------------------------------- order and flags
OrderPlan PlanOrder(State& st, const PictureKey& pic, uint32_t npix, uint32_t cuCount) {
    // order and flags are a function of the scene (camera included), the image size, the strip and the lists' limits: a new
    // accumulation of the same picture -- a progressive restart, the next frame of a turntable with an unchanged scene -- keeps them
    OrderPlan p;
    p.nFull = npix >> 6;
    const State::Masks& m = st.masks;
    const bool lists = m.valid && m.pic == pic && m.spheres != 0u && p.nFull != 0u;
    const bool wantFlags = lists && st.skySkip && st.skyExclude;
    p.listLimit = wantFlags ? m.limit : 0u;
    p.listSpheres = wantFlags ? m.spheres : 0u;
    const State::Order& o = st.order;
    if (o.keyValid && o.pic == pic && o.listLimit == p.listLimit && o.listSpheres == p.listSpheres) return p;
    Dropped(st);
    p.rebuild = true;
    p.flags = wantFlags;
    p.order = st.orderWanted && p.nFull >= 2u * cuCount;  // (else too little work for the order to matter)
    p.count = p.flags && p.order;
    return p;
}

void OrderBuilt(State& st, const PictureKey& pic, const OrderPlan& p) {
    st.order.keyValid = true;
    st.order.orderValid = p.order;
    st.order.flagsValid = p.flags;
    st.order.pic = pic;
    st.order.listLimit = p.listLimit;
    st.order.listSpheres = p.listSpheres;
    st.count.pending = p.count;
    st.count.known = false;
}

// --------------------------------------------------------------------------------------------------------------------- use
Use UseFor(const State& st, const PictureKey& pic, uint32_t npix) {
    Use u;
    const uint32_t nFull = npix >> 6;
    u.masks = st.masks.valid && st.masks.pic == pic;
    u.lists = u.masks && st.masks.spheres != 0u;
    const bool keyHere = st.order.keyValid && st.order.pic == pic;
    u.order = keyHere && st.order.orderValid;
    u.sky_skip = (u.lists && st.skySkip) ? 1u : 0u;
    const bool leaveOut = keyHere && st.order.flagsValid && st.count.known && u.order && u.sky_skip != 0u && (npix & 63u) == 0u && st.count.value < nFull;
    u.nSky = leaveOut ? st.count.value : 0u;
    return u;
}

}  // namespace rttile
