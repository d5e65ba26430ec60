// tile_tables_selftest.cpp -- the bookkeeping of the per-tile tables (rt_tile_tables.h) alone, with no device and no library.  A model
// of the device stands in for rt_capi.hip: every buffer remembers which (scene generation, picture, limits) its content was built
// from, the event behind the copy of the count completes a number of polls after its latest record, and the model carries out
// the unit's plans exactly as rt_capi.hip does (BuildTileMasks, BuildTileOrder, SkyCountPoll, Render, UnitEntry, SetStream and
// SceneUpload below are its twins), with a failure injected at a chosen reservation or launch.  Two parts: scenarios written from
// the comments of rt_tile_tables.h and DESIGN.md 5.1 and 10, and seeded random scripts, checked after every step.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <string>

#include "rt_tile_tables.h"

namespace {

using namespace rttile;

int g_failures = 0, g_printed = 0;
std::string g_where;
#define CHECK(cond)                                                                                      \
    do {                                                                                                 \
        if (!(cond)) {                                                                                   \
            if (++g_failures, ++g_printed <= 10) fprintf(stderr, "FAIL %s: %s (line %d)\n", g_where.c_str(), #cond, __LINE__); \
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
uint32_t NpixOf(const PictureKey& p) { return p.W * p.rs.num_rows; }

// what the run reached
enum { kKeep, kNotWanted, kMaskBuild, kFlagBuild, kOrderBuild, kCountArrived, kExcludedLaunch, kOtherPicThenContinue, kInjectedFailure, kReachedCount };
const char* const kReachedName[kReachedCount] = {"keep", "not-wanted", "mask-build", "flag-build", "order-build", "count-arrived", "excluded-launch",
                                                 "other-picture-then-continue", "injected-failure"};
uint64_t g_reached[kReachedCount];

constexpr int kOk = 0, kErr = 1;

// The content of a device buffer: what it was built from.  serial: the build that wrote it (0: never written).
struct Content {
    uint32_t serial = 0, scene = 0;
    PictureKey pic;
    uint32_t limit = 0, spheres = 0;
    uint32_t fromSerial = 0;  // flags: the lists they were taken from; order: the flags it was built with (0: none)
    uint32_t count = 0;       // flags: the flagged tiles
};

struct Model {
    State st;
    uint32_t cuCount = 4;  // the order exists from 8 full tiles on
    uint32_t scene = 1;    // generation
    bool sceneTakesMasks = true;
    uint32_t serials = 0;
    Content masks, lists, flags, order;
    // the copy of the count: device word -> pinned word, behind the event
    uint32_t copyValue = 0, copySerial = 0, pollsLeft = 0;
    bool evDone = true;
    uint32_t pinned = 0, pinnedSerial = 0, arrivedSerial = 0;
    // the running accumulation
    bool accOn = false;
    PictureKey accPic;
    Knobs accKnobs;
    bool otherPicRebuilt = false;  // a unit entry rebuilt the masks for another picture since the accumulation's last call
    // control
    Rng* rng = nullptr;       // null (scenarios): pollsNext / countNext decide
    uint32_t pollsNext = 0;   // polls that find the next recorded event not ready
    int64_t countNext = -1;   // the next flag build's count (-1: a function of scene and picture)
    uint32_t failIn = 0;      // the failIn-th reservation or launch from here fails (0: none)
    bool droppedReported = false;  // rtseq::TileTablesDropped was called during this step

    bool Point() {  // a reservation, a launch or a runtime call that can fail
        if (failIn != 0 && --failIn == 0) {
            ++g_reached[kInjectedFailure];
            return false;
        }
        return true;
    }
    uint32_t EmptyCount(const PictureKey& pic) const {
        const uint32_t nFull = NpixOf(pic) >> 6;
        if (countNext >= 0) return (uint32_t)countNext;
        const uint32_t v = (scene * 2654435761u ^ pic.W * 40503u ^ pic.H * 9176u) % (nFull + 2u);  // (all tiles empty happens too)
        return v > nFull ? nFull : v;
    }
    bool Current(const Content& c, const PictureKey& pic) const { return c.serial != 0 && c.scene == scene && c.pic == pic; }

    void NothingOfTheOrderIsValid(const PictureKey& pic) {
        CHECK(!AccumulateByFlags(st) && !CountToAwait(st) && !st.count.known);
        const Use u = UseFor(st, pic, NpixOf(pic));
        CHECK(!u.order && u.nSky == 0);
    }

    int BuildTileMasks(const PictureKey& pic, uint32_t npix, const Knobs& knobs) {
        const MaskPlan plan = PlanMasks(st, pic, npix, knobs, sceneTakesMasks);
        const bool wanted = knobs.primaryMask && (npix >> 6) != 0 && sceneTakesMasks;
        if (plan.answer == MaskAnswer::Keep) {
            ++g_reached[kKeep];
            CHECK(wanted && Current(masks, pic) && masks.limit == knobs.primaryMaskLimit && masks.spheres == knobs.primarySpheres);
            CHECK(knobs.primarySpheres == 0 || lists.serial == masks.serial);
            return kOk;
        }
        CHECK(MaskTiles(st) == 0 && ListTiles(st) == 0);
        if (plan.answer == MaskAnswer::NotWanted) {
            ++g_reached[kNotWanted];
            CHECK(!wanted);
            return kOk;
        }
        ++g_reached[kMaskBuild];
        CHECK(wanted && plan.nFull == npix >> 6 && plan.limit == knobs.primaryMaskLimit && plan.sphLimit == knobs.primarySpheres);
        if (!Point()) return kErr;
        if (plan.sphLimit != 0 && !Point()) return kErr;
        masks = Content{++serials, scene, pic, plan.limit, plan.sphLimit, 0, 0};  // the kernel writes both tables
        if (plan.sphLimit != 0) lists = masks;
        if (!Point()) return kErr;
        MasksBuilt(st, pic, plan);
        CHECK(MaskTiles(st) == plan.nFull && ListTiles(st) == (plan.sphLimit != 0 ? plan.nFull : 0u));
        return kOk;
    }

    int BuildTileOrder(const PictureKey& pic, uint32_t npix) {
        const State before = st;
        const OrderPlan plan = PlanOrder(st, pic, npix, cuCount);
        if (!plan.rebuild) {
            ++g_reached[kKeep];
            CHECK(before.order.keyValid && st.order.keyValid && st.order.pic == pic);
            return kOk;
        }
        droppedReported = true;
        NothingOfTheOrderIsValid(pic);
        const bool listsHere = ListTiles(st) != 0 && Current(lists, pic) && lists.serial == masks.serial;
        CHECK(plan.flags == (listsHere && accKnobs.skipSky && accKnobs.excludeSky));
        CHECK(plan.order == (st.orderWanted && (npix >> 6) >= 2 * cuCount));
        CHECK(plan.count == (plan.flags && plan.order) && plan.nFull == npix >> 6);
        if (plan.flags) {
            ++g_reached[kFlagBuild];
            for (int k = 0; k < 5; ++k)  // event, pinned word, two reservations, the memset
                if (!Point()) return kErr;
            CHECK(Current(lists, pic));  // the kernel reads the lists: they must be this picture's, of this scene
            CHECK(plan.listLimit == lists.limit && plan.listSpheres == lists.spheres);
            flags = Content{++serials, scene, pic, lists.limit, lists.spheres, lists.serial, EmptyCount(pic)};
            if (!Point()) return kErr;
        } else {
            CHECK(plan.listLimit == 0 && plan.listSpheres == 0);
        }
        if (plan.order) {
            ++g_reached[kOrderBuild];
            for (int k = 0; k < 6; ++k)  // four reservations, the pilot rays, their scan
                if (!Point()) return kErr;
            order = Content{++serials, scene, pic, 0, 0, plan.flags ? flags.serial : 0u, 0};
            if (!Point()) return kErr;
        }
        if (plan.count) {
            if (!Point()) return kErr;
            copyValue = flags.count, copySerial = flags.serial;
            if (!Point()) return kErr;
            evDone = false;
            pollsLeft = rng ? rng->below(4) : pollsNext;
        }
        OrderBuilt(st, pic, plan);
        CHECK(AccumulateByFlags(st) == plan.flags && CountToAwait(st) == plan.count && !st.count.known);
        return kOk;
    }

    void EventCompletes() {
        evDone = true;
        pinned = copyValue, pinnedSerial = copySerial;
    }
    void SkyCountPoll() {
        if (!CountToAwait(st)) return;
        if (rng && rng->one_in(64)) {
            CountFailed(st);  // the query itself failed
            CHECK(!CountToAwait(st) && !st.count.known);
        } else if (pollsLeft == 0) {
            EventCompletes();
            CountArrived(st, pinned);
            arrivedSerial = pinnedSerial;
            ++g_reached[kCountArrived];
            CHECK(!CountToAwait(st) && st.count.known);
        } else {
            --pollsLeft;
        }
    }

    // What UseFor hands out was built from the current scene, the call's picture and the limits in force; nSky only under all its rules.
    void CheckUse(const Use& u, const PictureKey& pic, uint32_t npix) {
        const uint32_t nFull = npix >> 6;
        if (u.masks) CHECK(Current(masks, pic) && masks.limit == st.masks.limit && masks.spheres == st.masks.spheres && MaskTiles(st) == nFull);
        if (u.lists) CHECK(u.masks && Current(lists, pic) && lists.serial == masks.serial && lists.spheres != 0);
        if (u.order) CHECK(Current(order, pic) && order.fromSerial == (AccumulateByFlags(st) ? flags.serial : 0u));
        CHECK(u.sky_skip == ((u.lists && accKnobs.skipSky) ? 1u : 0u));
        if (u.nSky != 0) {
            CHECK(AccumulateByFlags(st));
            CHECK(Current(flags, pic));                                              // the flags are valid for that picture,
            CHECK(flags.limit == st.order.listLimit && flags.spheres == st.order.listSpheres);
            CHECK(u.lists && lists.pic == flags.pic && lists.scene == flags.scene);  // taken from lists of that picture,
            CHECK(u.order && order.fromSerial == flags.serial);                      // the order was built with those flags,
            CHECK(evDone && arrivedSerial == flags.serial && u.nSky == flags.count);  // the count is known and is that build's,
            CHECK(accKnobs.skipSky && accKnobs.excludeSky);                          // the sky knobs are on,
            CHECK((npix & 63u) == 0 && u.nSky < nFull);                              // no partial tile, and some tile is left
        }
    }

    // rt_render through RenderNow, plain mode: start (s0 == 1) or continue the accumulation.
    int Render(const PictureKey& pic, bool start, const Knobs& knobs, Use* out = nullptr) {
        const uint32_t npix = NpixOf(pic);
        SkyCountPoll();  // before any table is rebuilt: the call that builds the flags never sees their number
        if (start) {
            accOn = true, accPic = pic, accKnobs = knobs, otherPicRebuilt = false;
            AccumulationStarts(st, knobs);
            const uint32_t serialsBefore = serials;
            int rc = BuildTileMasks(pic, npix, knobs);
            if (rc != kOk) {
                CHECK(MaskTiles(st) == 0 && !UseFor(st, pic, npix).masks);
                accOn = false;
                return rc;
            }
            if ((rc = BuildTileOrder(pic, npix)) != kOk) {
                NothingOfTheOrderIsValid(pic);
                accOn = false;
                return rc;
            }
            if (flags.serial > serialsBefore) CHECK(UseFor(st, pic, npix).nSky == 0);  // built by this call: their number cannot be known
        }
        CHECK(accOn && pic == accPic);
        const Use u = UseFor(st, pic, npix);
        CheckUse(u, pic, npix);
        if (u.nSky != 0) ++g_reached[kExcludedLaunch];
        if (!start && otherPicRebuilt) {
            ++g_reached[kOtherPicThenContinue];
            CHECK(!u.masks && !u.lists && u.sky_skip == 0 && u.nSky == 0);
            otherPicRebuilt = false;
        }
        // LaunchAccumulate: the flags name the tiles whose planes are the constant -- those of the accumulation's picture
        if (AccumulateByFlags(st)) CHECK(Current(flags, accPic));
        if (out) *out = u;
        return kOk;
    }

    // rt_unit_tile_masks / rt_unit_tile_spheres: the masks for any picture, under the mask knobs of the moment
    int UnitEntry(const PictureKey& pic, const Knobs& knobs) {
        const uint32_t before = masks.serial;
        const bool hadMasks = MaskTiles(st) != 0;
        const int rc = BuildTileMasks(pic, NpixOf(pic), knobs);
        if (accOn && (masks.serial != before || (hadMasks && MaskTiles(st) == 0))) otherPicRebuilt = !(pic == accPic);  // (an entry for the accumulation's own picture brings them back)
        if (rc == kOk && MaskTiles(st) != 0) CHECK(Current(masks, pic) && st.masks.pic == pic);
        return rc;
    }
    void SetStream() {
        if (CountToAwait(st)) EventCompletes();  // hipEventSynchronize: the copy has landed before a newer one can be recorded
        Dropped(st);
        droppedReported = true;
        NothingOfTheOrderIsValid(accPic);
    }
    void TablesDropped() {  // rtseq::kTileOrder from rt_set_sampler: the accumulation ends with it
        Dropped(st);
        droppedReported = true;
        accOn = false;
        NothingOfTheOrderIsValid(accPic);
    }
    void SceneUpload(bool takesMasks) {
        ++scene;
        sceneTakesMasks = takesMasks;
        SceneReplaced(st);
        droppedReported = true;
        accOn = false;
        NothingIsValid();
    }
    void NothingIsValid() {
        CHECK(MaskTiles(st) == 0 && ListTiles(st) == 0);
        NothingOfTheOrderIsValid(accPic);
        const Use u = UseFor(st, accPic, NpixOf(accPic));
        CHECK(!u.masks && !u.lists && !u.order && u.sky_skip == 0 && u.nSky == 0);
    }

    // after every step
    void Invariants(const State& before) {
        if (st.count.known) CHECK(evDone && arrivedSerial == flags.serial && flags.scene == scene && st.count.value == flags.count && AccumulateByFlags(st));
        if (CountToAwait(st)) CHECK(AccumulateByFlags(st) && st.order.orderValid && copySerial == flags.serial);
        CHECK(!(st.count.known && st.count.pending));
        if (AccumulateByFlags(st)) CHECK(Current(flags, st.order.pic) && (!accOn || st.order.pic == accPic));
        if (st.order.keyValid && st.order.orderValid) CHECK(Current(order, st.order.pic));
        if (!st.order.keyValid) CHECK(!AccumulateByFlags(st) && !UseFor(st, st.order.pic, NpixOf(st.order.pic)).order);
        if (MaskTiles(st) != 0) CHECK(Current(masks, st.masks.pic) && masks.limit == st.masks.limit && masks.spheres == st.masks.spheres);
        if (before.order.keyValid && !st.order.keyValid) CHECK(droppedReported);  // the sequencer hears of every drop
        droppedReported = false;
    }
};

Knobs Defaults() {
    Knobs k;
    k.primaryMaskLimit = 12, k.primarySpheres = 16;
    return k;
}

// ---------------------------------------------------------------------------------------------------------------- scenarios
int g_scenarios = 0;
struct Scenario {
    explicit Scenario(const char* name) {
        g_where = std::string("scenario \"") + name + "\"";
        ++g_scenarios;
    }
};

void Scenarios() {
    const PictureKey A = Pic(64, 32), B = Pic(128, 16), Partial = Pic(70, 33), Small = Pic(32, 8);  // 32, 32, 36 + a partial one, 4 full tiles
    const Knobs D = Defaults();
    Use u;
    {
        Scenario s("the call that builds the tables never sees the count; a restart keeps them and leaves the flagged tiles out");
        Model m;
        m.countNext = 5, m.pollsNext = 0;
        CHECK(m.Render(A, true, D, &u) == kOk);
        CHECK(u.masks && u.lists && u.order && u.sky_skip == 1 && u.nSky == 0);
        CHECK(AccumulateByFlags(m.st) && CountToAwait(m.st));
        const uint32_t built = m.serials;
        CHECK(m.Render(A, false, D, &u) == kOk);  // the continuing call polls first: the number has arrived
        CHECK(u.nSky == 5 && !CountToAwait(m.st));
        CHECK(m.Render(A, true, D, &u) == kOk);
        CHECK(m.serials == built && u.nSky == 5 && u.order && u.lists);  // nothing was rebuilt
    }
    {
        Scenario s("the count is unknown until the event has completed, however many calls ask");
        Model m;
        m.countNext = 7, m.pollsNext = 2;
        CHECK(m.Render(A, true, D, &u) == kOk && u.nSky == 0);
        CHECK(m.Render(A, false, D, &u) == kOk && u.nSky == 0 && !m.st.count.known);
        CHECK(m.Render(A, false, D, &u) == kOk && u.nSky == 0 && !m.st.count.known);
        CHECK(m.Render(A, false, D, &u) == kOk && u.nSky == 7 && m.st.count.known);
    }
    {
        Scenario s("RT_SKY_EXCLUDE=0 and RT_SKY_SKIP=0: no flags, no count, the plain accumulation; the order is built all the same");
        for (int which = 0; which < 2; ++which) {
            Model m;
            Knobs k = D;
            (which ? k.skipSky : k.excludeSky) = false;
            CHECK(m.Render(A, true, k, &u) == kOk);
            CHECK(u.masks && u.lists && u.order && u.nSky == 0 && u.sky_skip == (which ? 0u : 1u));
            CHECK(!AccumulateByFlags(m.st) && !CountToAwait(m.st) && m.flags.serial == 0 && m.order.serial != 0);
            CHECK(m.Render(A, true, D, &u) == kOk);  // the knobs are back: another key, flags and order are rebuilt
            CHECK(AccumulateByFlags(m.st) && m.flags.serial != 0 && m.order.fromSerial == m.flags.serial);
        }
    }
    {
        Scenario s("RT_TILE_ORDER=0: flags without an order; no count is asked for and no tile is left out");
        Model m;
        m.st.orderWanted = false;
        CHECK(m.Render(A, true, D, &u) == kOk);
        CHECK(m.Render(A, true, D, &u) == kOk);
        CHECK(AccumulateByFlags(m.st) && !CountToAwait(m.st) && !m.st.count.known && !u.order && u.nSky == 0 && u.sky_skip == 1);
    }
    {
        Scenario s("too few tiles for an order (below two per compute unit): flags alone");
        Model m;
        CHECK(m.Render(Small, true, D, &u) == kOk);
        CHECK(AccumulateByFlags(m.st) && !CountToAwait(m.st) && !u.order && u.lists);
    }
    {
        Scenario s("a partial last tile, or every tile flagged: all tiles are queued although the count is known");
        Model m;
        m.countNext = 3;
        CHECK(m.Render(Partial, true, D) == kOk);
        CHECK(m.Render(Partial, true, D, &u) == kOk);
        CHECK(m.st.count.known && u.nSky == 0 && u.order && AccumulateByFlags(m.st));
        Model n;
        n.countNext = 32;
        CHECK(n.Render(A, true, D) == kOk);
        CHECK(n.Render(A, true, D, &u) == kOk);
        CHECK(n.st.count.known && n.st.count.value == 32 && u.nSky == 0);
    }
    {
        Scenario s("a unit entry rebuilds the masks for another picture inside an accumulation");
        Model m;
        m.countNext = 5;
        CHECK(m.Render(A, true, D) == kOk);
        CHECK(m.Render(A, false, D, &u) == kOk && u.nSky == 5);
        const uint32_t orderBuilt = m.order.serial, flagsBuilt = m.flags.serial;
        CHECK(m.UnitEntry(B, D) == kOk && MaskTiles(m.st) == 32 && m.masks.pic == B);
        CHECK(m.Render(A, false, D, &u) == kOk);
        CHECK(!u.masks && !u.lists && u.sky_skip == 0 && u.nSky == 0);  // nothing of another picture's tables
        CHECK(u.order && AccumulateByFlags(m.st));  // order and flags are still this picture's: the launch traces the flagged tiles, with the constant's bits
        CHECK(m.Render(A, true, D, &u) == kOk);     // started again: the masks are rebuilt, order, flags and count kept
        CHECK(m.masks.pic == A && m.order.serial == orderBuilt && m.flags.serial == flagsBuilt);
        CHECK(u.masks && u.lists && u.order && u.nSky == 5);
    }
    {
        Scenario s("a unit entry with other limits for the same picture: the next accumulation rebuilds masks, flags and order");
        Model m;
        CHECK(m.Render(A, true, D) == kOk);
        Knobs k = D;
        k.primarySpheres = 8;
        CHECK(m.UnitEntry(A, k) == kOk && m.masks.spheres == 8);
        CHECK(m.Render(A, false, D, &u) == kOk && u.masks && u.lists);  // this picture's, under the limits they now have
        const uint32_t flagsBuilt = m.flags.serial;
        CHECK(m.Render(A, true, D, &u) == kOk);
        CHECK(m.masks.spheres == 16 && m.flags.serial == flagsBuilt);  // back to the key the flags were taken under: kept
        CHECK(m.Render(A, true, k, &u) == kOk);
        CHECK(m.masks.spheres == 8 && m.flags.serial > flagsBuilt && m.st.order.listSpheres == 8 && u.nSky == 0);
    }
    {
        Scenario s("a scene that takes no masks, RT_PRIMARY_MASK=0, RT_PRIMARY_SPHERES=0: no lists, so no flags; the order alone");
        for (int which = 0; which < 3; ++which) {
            Model m;
            Knobs k = D;
            if (which == 0) m.sceneTakesMasks = false;
            if (which == 1) k.primaryMask = false;
            if (which == 2) k.primarySpheres = 0;
            CHECK(m.Render(A, true, k, &u) == kOk);
            CHECK(u.masks == (which == 2) && !u.lists && u.order && u.sky_skip == 0 && u.nSky == 0 && !AccumulateByFlags(m.st));
            CHECK(MaskTiles(m.st) == (which == 2 ? 32u : 0u) && ListTiles(m.st) == 0);
        }
    }
    {
        Scenario s("a new scene voids every table; a new stream awaits the count and drops order and flags, not the masks");
        Model m;
        m.countNext = 5, m.pollsNext = 9;
        CHECK(m.Render(A, true, D) == kOk && CountToAwait(m.st));
        m.SetStream();
        CHECK(m.evDone && MaskTiles(m.st) == 32 && !AccumulateByFlags(m.st));
        CHECK(m.Render(A, false, D, &u) == kOk && u.masks && u.lists && !u.order && u.nSky == 0);  // the accumulation goes on without them
        CHECK(m.Render(A, true, D, &u) == kOk && u.order && AccumulateByFlags(m.st));
        m.SceneUpload(true);
        CHECK(m.Render(A, true, D, &u) == kOk && m.masks.scene == m.scene && m.flags.scene == m.scene && u.nSky == 0);
    }
    {
        Scenario s("a rebuild of order and flags that fails half way leaves everything dropped");
        for (uint32_t at = 1; at <= 18; ++at) {
            Model m;
            m.countNext = 5;
            CHECK(m.Render(A, true, D) == kOk);
            CHECK(m.Render(A, false, D, &u) == kOk && u.nSky == 5);
            Knobs k = D;
            k.primaryMaskLimit = 8;  // another key: masks (three points), then flags, order and count (sixteen)
            m.failIn = at;
            const int rc = m.Render(A, true, k, &u);
            CHECK(rc == kErr && m.failIn == 0);
            u = UseFor(m.st, A, NpixOf(A));
            if (at <= 3) {  // the masks' build failed: they are invalid, and the order's plan was never asked -- the old key stands
                CHECK(MaskTiles(m.st) == 0 && !u.masks && !u.lists && u.nSky == 0 && m.st.order.keyValid && m.st.order.listLimit == 12);
            } else {
                CHECK(!AccumulateByFlags(m.st) && !CountToAwait(m.st) && !m.st.count.known && !m.st.order.keyValid);
                CHECK(u.masks && !u.order && u.nSky == 0);
            }
            CHECK(m.Render(A, true, k, &u) == kOk && AccumulateByFlags(m.st) && u.order && u.nSky == 0);  // the next start builds what is missing
        }
        Model m;
        m.failIn = 19;  // (one more than a start has points)
        CHECK(m.Render(A, true, D) == kOk && m.failIn == 1);
    }
    {
        Scenario s("a count copied before a drop is never taken for the next build's");
        Model m;
        m.countNext = 5, m.pollsNext = 3;
        CHECK(m.Render(A, true, D) == kOk && CountToAwait(m.st));
        m.TablesDropped();  // (rt_set_sampler) -- the copy is still on its way
        CountArrived(m.st, 5);  // nobody asks any more; were it reported all the same, it is not this state's
        CHECK(!m.st.count.known);
        m.countNext = 9;
        CHECK(m.Render(A, true, D, &u) == kOk && u.nSky == 0 && CountToAwait(m.st));
        for (int k = 0; k < 3; ++k) CHECK(m.Render(A, false, D, &u) == kOk && u.nSky == 0);
        CHECK(m.Render(A, false, D, &u) == kOk && u.nSky == 9);
    }
}

// ----------------------------------------------------------------------------------------------------------- random scripts
constexpr uint32_t kScripts = 100000, kStepsPerScript = 60;

void RandomScripts() {
    const PictureKey pics[] = {Pic(64, 32), Pic(128, 16), Pic(64, 64), Pic(70, 33), Pic(32, 8), Pic(8, 4)};
    const uint32_t nPics = sizeof(pics) / sizeof(pics[0]);
    const uint32_t limits[] = {8, 12}, sphereLimits[] = {0, 8, 16, 16};
    const int before0 = g_failures;
    for (uint32_t script = 0; script < kScripts; ++script) {
        Rng rng{0x9E3779B97F4A7C15ull * (script + 1)};
        Model m;
        m.rng = &rng;
        m.st.orderWanted = !rng.one_in(8);
        auto randomKnobs = [&]() {
            Knobs k;
            k.primaryMask = !rng.one_in(8);
            k.primaryMaskLimit = limits[rng.below(2)];
            k.primarySpheres = sphereLimits[rng.below(4)];
            k.skipSky = !rng.one_in(6);
            k.excludeSky = !rng.one_in(6);
            return k;
        };
        Knobs last = randomKnobs();
        for (uint32_t step = 0; step < kStepsPerScript; ++step) {
            char where[96];
            snprintf(where, sizeof where, "script %u, step %u", script, step);
            g_where = where;
            const State before = m.st;
            const uint32_t what = rng.below(20);
            if (what < 1) {
                m.SceneUpload(!rng.one_in(6));
            } else if (what < 7) {
                if (!rng.one_in(3)) last = randomKnobs();  // (a restart mostly comes with the knobs of the last)
                const PictureKey pic = (m.accOn && !rng.one_in(3)) ? m.accPic : pics[rng.below(nPics)];
                (void)m.Render(pic, true, last);
            } else if (what < 14) {
                if (m.accOn) (void)m.Render(m.accPic, false, last);
            } else if (what < 16) {
                Knobs k = rng.one_in(2) ? last : randomKnobs();
                (void)m.UnitEntry((m.accOn && rng.one_in(2)) ? m.accPic : pics[rng.below(nPics)], k);
            } else if (what < 17) {
                m.SkyCountPoll();
            } else if (what < 18) {
                m.SetStream();
            } else if (what < 19) {
                m.TablesDropped();
            } else {
                m.failIn = 1 + rng.below(19);
            }
            m.Invariants(before);
        }
        if (g_failures != before0) break;
    }
}

}  // namespace

int main() {
    Scenarios();
    g_printed = 0;  // (both parts always run: each shows its own first failures)
    RandomScripts();
    printf("tile_tables_selftest: %d scenarios, %u scripts of %u steps\n", g_scenarios, kScripts, kStepsPerScript);
    printf("reached:");
    for (int k = 0; k < kReachedCount; ++k) printf(" %s %llu", kReachedName[k], (unsigned long long)g_reached[k]);
    printf("\n");
    for (int k = 0; k < kReachedCount; ++k)
        if (g_reached[k] == 0) {
            fprintf(stderr, "FAIL: \"%s\" was never reached\n", kReachedName[k]);
            ++g_failures;
        }
    if (g_failures != 0) {
        fprintf(stderr, "tile_tables_selftest: %d failure(s)\n", g_failures);
        return 1;
    }
    printf("tile_tables_selftest: ok\n");
    return 0;
}
