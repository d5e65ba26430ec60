// rt_tile_tables.h -- the bookkeeping of the per-tile tables, decided without a device: which of the candidate masks, sphere lists,
// work order, empty-list flags and the flagged tiles' count are built, kept and used, and what every outside event voids.  Plain C++
// with no HIP header, no environment and no allocation, under the contract of rt_sequence.h: rt_capi.hip owns one State, asks what
// to do, carries that out on the device and reports it done; host/tile_tables_selftest.cpp runs the same functions against a model
// of the device with no GPU.  No validity of a tile table is tested or set anywhere else.  DESIGN.md 4.3.
#pragma once

#include <stdint.h>

#include "rt_sequence.h"

namespace rttile {

using rtseq::PictureKey;

// The environment of the moment, read by the caller where it always was: the mask knobs where an accumulation starts and at the unit
// entries that rebuild the masks, the two sky knobs where an accumulation starts only.  (RT_TILE_ORDER is read once, at rt_create:
// State::orderWanted.)
struct Knobs {
    bool primaryMask = true;        // RT_PRIMARY_MASK
    uint32_t primaryMaskLimit = 0;  // RT_PRIMARY_MASK_LIMIT
    uint32_t primarySpheres = 0;    // RT_PRIMARY_SPHERES, clamped to the lists' capacity (0: no lists)
    bool skipSky = true;            // RT_SKY_SKIP
    bool excludeSky = true;         // RT_SKY_EXCLUDE
};

struct State {
    bool orderWanted = true;  // RT_TILE_ORDER=0 keeps the image order
    // Candidate masks and sphere lists (built together): a function of the scene (camera included), the picture and the two limits.
    struct Masks {
        bool valid = false;
        PictureKey pic;
        uint32_t limit = 0, spheres = 0;  // spheres == 0: no lists
        uint32_t tiles = 0;
    } masks;
    // Work order and empty-list flags: one key and one lifetime.  The key says what orderValid / flagsValid describe: the picture,
    // and the lists' limits the flags were taken under (0, 0: no flags).  With flags the order ends with exactly the flagged tiles.
    struct Order {
        bool keyValid = false, orderValid = false, flagsValid = false;
        PictureKey pic;
        uint32_t listLimit = 0, listSpheres = 0;
    } order;
    // The flagged tiles' number reaches the host through pinned memory behind an event that is only ever queried: until it has
    // completed the count is unknown and every launch queues all tiles.
    struct Count {
        bool pending = false, known = false;
        uint32_t value = 0;
    } count;
    // the running accumulation's knobs (no table depends on skySkip; the unit entries that rebuild tables leave both alone)
    bool skySkip = true, skyExclude = true;
};

// ---- events.  Each applies itself to the state; dropping order or flags also voids the planes traced ahead, which the caller
// reports to the sequencer (rtseq::TileTablesDropped) -- after Dropped, and after a PlanOrder that answers Rebuild.
void SceneReplaced(State& st);                           // rt_scene_upload, as soon as the old tables' inputs are overwritten: nothing is valid
void CameraChanged(State& st);                           // rt_set_camera with another record: every table is a function of the camera, nothing is valid
void Dropped(State& st);                                 // rtseq::kTileOrder: order, flags and count (the masks stay)
void AccumulationStarts(State& st, const Knobs& knobs);  // before the two plans of the call that starts it
void CountArrived(State& st, uint32_t n);                // the event behind the copy was found complete: n is the pinned word
void CountFailed(State& st);                             // the query failed: the count stays unknown
// A copy of the count is on its way: SkyCountPoll queries its event, rt_set_stream waits for it (it must not land in the pinned word
// after a newer one's).
inline bool CountToAwait(const State& st) { return st.count.pending; }

// ---- the masks (and lists) for a picture of npix local pixels.  sceneTakesMasks: only the flat matrix-core scan of a one-level
// scene of at most 128 groups reads them (rtplan::ChooseScan, asked by the caller).
enum class MaskAnswer : uint32_t {
    Keep,       // valid for this picture and these limits
    NotWanted,  // no masks for this picture: they are invalid from here on
    Build,      // invalid from here on; build for nFull tiles under limit / sphLimit, then report MasksBuilt
};
struct MaskPlan {
    MaskAnswer answer = MaskAnswer::NotWanted;
    uint32_t nFull = 0, limit = 0, sphLimit = 0;
};
MaskPlan PlanMasks(State& st, const PictureKey& pic, uint32_t npix, const Knobs& knobs, bool sceneTakesMasks);
void MasksBuilt(State& st, const PictureKey& pic, const MaskPlan& p);  // every reservation and the launch succeeded
uint32_t MaskTiles(const State& st);  // tiles the valid masks cover (0: none), whatever picture they are of: the unit entries' answer
uint32_t ListTiles(const State& st);  // ... and the valid lists

// ---- order and flags for the accumulation that starts, AFTER the masks' plan was carried out for the same picture.
struct OrderPlan {
    bool rebuild = false;  // false: keep.  True: everything was dropped; carry out the three bits in this order, then report OrderBuilt
    bool flags = false;    // flag the tiles whose list is empty
    bool order = false;    // build the work order (behind the flags where there are any)
    bool count = false;    // copy the flagged tiles' number to the pinned word and record the event (only with flags AND order: without
                           // the order no launch can leave the flagged tiles out, and nobody needs their number)
    uint32_t nFull = 0;
    uint32_t listLimit = 0, listSpheres = 0;  // the key the result is kept under
};
OrderPlan PlanOrder(State& st, const PictureKey& pic, uint32_t npix, uint32_t cuCount);
// Only after EVERY launch and reservation of the rebuild succeeded: a rebuild that fails half way leaves everything dropped.
void OrderBuilt(State& st, const PictureKey& pic, const OrderPlan& p);

// ---- what one render call's passes take.  Every table is checked against the call's picture: a unit entry may have rebuilt the
// masks for another picture in the middle of an accumulation, and only the caller of today guarantees the same of the order.
struct Use {
    bool masks = false, lists = false, order = false;
    uint32_t sky_skip = 0;  // TraceParams::sky_skip: empty-list tiles are finished without rays
    // Empty-list tiles left out of the queue (0: none): their number had arrived when the call began, they are the order's tail, the
    // kernel would finish them without rays anyway and no partial tile follows the full ones in path-index space.
    uint32_t nSky = 0;
};
Use UseFor(const State& st, const PictureKey& pic, uint32_t npix);
// The tile-aware accumulation: the flagged tiles' planes are the constant, whether the launch that traced the buffer wrote them
// (with the same bits) or left them out.  The flags are those of the running accumulation's picture: only PlanOrder, where an
// accumulation starts, ever builds them.
inline bool AccumulateByFlags(const State& st) { return st.order.keyValid && st.order.flagsValid; }

}  // namespace rttile
