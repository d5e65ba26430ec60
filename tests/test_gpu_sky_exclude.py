"""Empty-list tiles kept out of the trace queue (rt_capi.hip BuildTileOrder / RenderNow, rt_kernels.h rt_sky_tiles_kernel): where an
accumulation starts, the full tiles whose sphere list has length 0 are flagged on the device and sorted last in work order; once
their number has reached the host (copied asynchronously, never waited for) a launch queues only the other tiles, the host sets the
flagged tiles' share of the counters, and the tile-aware accumulation adds the constant sky sample for them without reading the
sample buffer.  Nothing observable may change: HDR and LDR bits, second moments and error map, the traversal and segment counters,
the three tile statistics and the count of ray-less planes equal those of RT_SKY_EXCLUDE=0 (the previous behaviour), of
RT_SKY_SKIP=0 where the knob does not itself define the number, and the oracle's.

Because the count arrives asynchronously, every case renders the picture once, synchronizes, and starts the accumulation again:
the SECOND render is the one that is compared, and rt_unit_sky_excluded must then equal the number of tiles with an empty device
list (and 0 where the case is a fallback), so that the file cannot pass with the new path dead.  The first render uses ANOTHER
seed (the tables do not depend on it), so the sample buffer it leaves holds other samples: were the order's tail not exactly the
flagged tiles, the shortened launch would leave a real tile's planes unwritten and the accumulation would add the other seed's
samples for it -- pixels would differ, not only counters.  That is how the five-class order is checked on the device: no unit entry
hands out the order itself.

Shapes: the tile order exists from 512 full tiles on (two per compute unit), so every picture has more -- the cover scene at
384x198 has 1,188 full tiles and no partial one -- and spp is at most 5."""
import ctypes as C

import numpy as np
import pytest

NONE = 0xFFFF
DEPTH, SEED = 50, 1
W0, H0, SPP0 = 384, 198, 4  # the cover picture most cases share


@pytest.fixture(scope="module")
def scenes_mod(built):
    from cpuraytracer_amd import scenes
    return scenes


@pytest.fixture()
def own(built):
    """A context of its own, for the settings that outlive a call (noise estimate, workspace limit, render-ahead)."""
    from cpuraytracer_amd import HipRenderer
    r = HipRenderer(0)
    yield r
    r.close()


def _knobs(monkeypatch, exclude=None, skip=None):
    for name, v in (("RT_SKY_EXCLUDE", exclude), ("RT_SKY_SKIP", skip)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, v)


SETTINGS = {"default": {}, "exclude-off": {"exclude": "0"}, "skip-off": {"skip": "0"}}


def _list_lengths(hip, W, H, rs):
    from cpuraytracer_amd import _capi
    L = _capi.load()
    cap = (W * L.rt_rowset_local_rows(rs)) >> 6
    lists = np.zeros((max(cap, 1), 64), dtype=np.uint16)
    n = C.c_uint32(0)
    _capi.check(L.rt_unit_tile_spheres(hip._h, W, H, rs, cap, C.byref(n), lists.ctypes.data, None))
    return lists[:n.value, 0].copy()


def _scans(hip, W, H, rs):
    from cpuraytracer_amd import _capi
    n = C.c_uint32(0)
    scans = np.zeros(3, dtype=np.uint64)
    _capi.check(_capi.load().rt_unit_tile_spheres(hip._h, W, H, rs, 0, C.byref(n), None, scans.ctypes.data))
    return int(scans[0]), int(scans[1]), int(scans[2])


def _sky_planes(hip):
    from cpuraytracer_amd import _capi
    n = C.c_uint64(0)
    _capi.check(_capi.load().rt_unit_sky_planes(hip._h, C.byref(n)))
    return int(n.value)


def _excluded(hip):
    from cpuraytracer_amd import _capi
    n = C.c_uint32(0)
    _capi.check(_capi.load().rt_unit_sky_excluded(hip._h, C.byref(n)))
    return int(n.value)


class Shot:
    """What one compared render left: pictures, counters, statistics."""

    def __init__(self, hip, W, H, rs, st, excluded):
        from cpuraytracer_amd import _capi
        rs = rs if rs is not None else _capi.whole_image(H)
        self.excluded = excluded
        self.counters = (st.traversals, st.segments)
        self.passes = st.passes
        self.scans = _scans(hip, W, H, rs)
        self.sky = _sky_planes(hip)
        hip.resolve()
        self.hdr, self.ldr = hip.download()
        self.lens = _list_lengths(hip, W, H, rs)
        self.empty = int((self.lens == 0).sum())


def _second_render(hip, sc, W, H, s0, s1, rs=None):
    """Upload, render [s0, s1) once, synchronize, start the accumulation again: the second render's Shot."""
    hip.upload(sc)
    hip.render(W, H, s0, s1, DEPTH, SEED + 1, rowset=rs)  # another seed: the buffer it leaves holds other samples (module docstring)
    assert _excluded(hip) == 0, "the tables were just built: the count cannot be known to the first render"
    hip.synchronize()
    st = hip.render(W, H, s0, s1, DEPTH, SEED, rowset=rs)
    return Shot(hip, W, H, rs, st, _excluded(hip))


def _same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape, what
    bad = a.view(np.uint32 if a.dtype == np.float32 else a.dtype) != b.view(np.uint32 if b.dtype == np.float32 else b.dtype)
    assert not bad.any(), "%s: %d of %d values differ, first at %s" % (what, int(bad.sum()), bad.size, np.argwhere(bad)[0])


def _same_shot(a, b, what, sky=True):
    _same(a.hdr, b.hdr, what + ": HDR")
    _same(a.ldr, b.ldr, what + ": LDR")
    assert a.counters == b.counters, "%s: traversal / segment counters %s vs %s" % (what, a.counters, b.counters)
    assert a.scans == b.scans, "%s: tile statistics %s vs %s" % (what, a.scans, b.scans)
    if sky:
        assert a.sky == b.sky, "%s: ray-less planes %d vs %d" % (what, a.sky, b.sky)


def _three_settings(hip, monkeypatch, sc, W, H, spp, label, rs=None, min_empty=1):
    """The second render under the default, RT_SKY_EXCLUDE=0 and RT_SKY_SKIP=0: equal in everything but the knobs' own observables."""
    got = {}
    for name, kn in SETTINGS.items():
        _knobs(monkeypatch, **kn)
        got[name] = _second_render(hip, sc, W, H, 1, 1 + spp, rs)
    _knobs(monkeypatch)
    d = got["default"]
    print("%s: %d full tiles, %d with an empty list; excluded %s; scans %s; ray-less planes %s"
          % (label, len(d.lens), d.empty, {k: v.excluded for k, v in got.items()}, d.scans, {k: v.sky for k, v in got.items()}))
    assert d.empty >= min_empty, "%s: %d tiles have an empty list, at least %d are needed" % (label, d.empty, min_empty)
    assert d.excluded == d.empty, "%s: %d tiles were kept out of the queue, %d have an empty list" % (label, d.excluded, d.empty)
    assert got["exclude-off"].excluded == 0 and got["skip-off"].excluded == 0
    assert d.sky == d.empty * spp and got["exclude-off"].sky == d.empty * spp and got["skip-off"].sky == 0
    _same_shot(d, got["exclude-off"], label + ", default vs RT_SKY_EXCLUDE=0")
    _same_shot(d, got["skip-off"], label + ", default vs RT_SKY_SKIP=0", sky=False)
    return got


@pytest.fixture(scope="module")
def cover(scenes_mod):
    return scenes_mod.build_scene("cover", 1, W0, H0)


@pytest.fixture(scope="module")
def cover_oracle(oracle, cover):
    """The oracle's picture of the shared shape, samples 1..4: computed once, read only."""
    orc = oracle.Oracle()
    orc.upload(cover)
    st = orc.render(W0, H0, 1, 1 + SPP0, DEPTH, SEED, threads=4)
    orc.resolve()
    h, l = orc.download()
    orc.close()
    h.setflags(write=False)
    l.setflags(write=False)
    return h, l, (st.traversals, st.segments)


@pytest.mark.gpu
def test_default_equals_the_reference_settings_and_the_oracle(hip, monkeypatch, cover, cover_oracle):
    got = _three_settings(hip, monkeypatch, cover, W0, H0, SPP0, "cover %dx%d" % (W0, H0))
    d = got["default"]
    assert len(d.lens) == 1188
    _same(d.hdr, cover_oracle[0], "HDR vs the oracle")
    _same(d.ldr, cover_oracle[1], "LDR vs the oracle")
    assert d.counters == cover_oracle[2], "traversal counters differ from the oracle's"


@pytest.mark.gpu
def test_noise_estimate_on(own, monkeypatch, cover):
    got = {}
    for name in ("default", "exclude-off"):
        _knobs(monkeypatch, **SETTINGS[name])
        own.upload(cover)
        own.set_noise_estimate(True)
        own.render(W0, H0, 1, 1 + SPP0, DEPTH, SEED + 1)
        own.synchronize()
        own.render(W0, H0, 1, 1 + SPP0, DEPTH, SEED)
        ex = _excluded(own)
        own.synchronize()
        got[name] = (own.download(ldr=False)[0], own.download_moments(), own.noise_map(), ex)
    from cpuraytracer_amd import _capi
    empty = int((_list_lengths(own, W0, H0, _capi.whole_image(H0)) == 0).sum())
    assert empty > 0 and got["default"][3] == empty and got["exclude-off"][3] == 0, (empty, got["default"][3], got["exclude-off"][3])
    assert (got["default"][1] > 0).any()
    _same(got["default"][0], got["exclude-off"][0], "HDR")
    _same(got["default"][1], got["exclude-off"][1], "second moments")
    _same(got["default"][2], got["exclude-off"][2], "error map")


@pytest.mark.gpu
def test_several_passes(own, monkeypatch, cover, cover_oracle):
    """A workspace of 1 MiB holds one sample plane of this picture (912,384 bytes): four passes, each with the shorter queue."""
    _knobs(monkeypatch)
    own.set_workspace_limit(1 << 20)
    shot = _second_render(own, cover, W0, H0, 1, 1 + SPP0)
    assert shot.passes == SPP0, shot.passes
    assert shot.empty > 0 and shot.excluded == shot.empty, (shot.excluded, shot.empty)
    assert shot.sky == shot.empty * SPP0 and shot.scans[0] == 1188 * SPP0
    _same(shot.hdr, cover_oracle[0], "HDR vs the oracle")
    _same(shot.ldr, cover_oracle[1], "LDR vs the oracle")
    assert shot.counters == cover_oracle[2]


@pytest.mark.gpu
def test_resumed_accumulation(hip, monkeypatch, cover, cover_oracle):
    """1..3 then 3..5 against the one-shot 1..5; both calls of the resumed accumulation run with the shorter queue."""
    _knobs(monkeypatch)
    one = _second_render(hip, cover, W0, H0, 1, 1 + SPP0)
    assert one.empty > 0 and one.excluded == one.empty
    st1 = hip.render(W0, H0, 1, 3, DEPTH, SEED)
    assert _excluded(hip) == one.empty
    st2 = hip.render(W0, H0, 3, 5, DEPTH, SEED)
    assert _excluded(hip) == one.empty and _sky_planes(hip) == one.empty * 2  # the second call's own launch
    hip.resolve()
    h, l = hip.download()
    _same(h, one.hdr, "resumed accumulation vs one shot (HDR)")
    _same(l, one.ldr, "resumed accumulation vs one shot (LDR)")
    _same(h, cover_oracle[0], "resumed accumulation vs the oracle (HDR)")
    assert (st1.traversals + st2.traversals, st1.segments + st2.segments) == one.counters == cover_oracle[2]


@pytest.mark.gpu
def test_tables_rebuilt_for_another_picture_inside_an_accumulation(hip, monkeypatch, cover, cover_oracle):
    """rt_unit_tile_spheres for 128x64 between the calls 1..3 and 3..5 rebuilds masks and lists for that picture and leaves order,
    flags and count alone.  The continuing call must then take no table that is not its own picture's: no masks, no lists, no
    shorter queue (0 tiles kept out) and no ray-less planes -- its launch traces every tile and writes the flagged tiles' planes with
    the bits of the constant that the tile-aware accumulation still adds for them.  An accumulation started again finds the masks
    rebuilt for its picture under the order's unchanged key, the count still known: the shorter queue from its first call on."""
    from cpuraytracer_amd import _capi
    _knobs(monkeypatch)
    one = _second_render(hip, cover, W0, H0, 1, 1 + SPP0)
    assert one.empty > 0 and one.excluded == one.empty
    hip.render(W0, H0, 1, 3, DEPTH, SEED)
    assert _excluded(hip) == one.empty
    other = _list_lengths(hip, 128, 64, _capi.whole_image(64))
    assert len(other) == 128 * 64 // 64
    hip.render(W0, H0, 3, 5, DEPTH, SEED)
    after4 = (_excluded(hip), _sky_planes(hip))
    print("continued after the rebuild: excluded, ray-less planes = %s" % (after4,))
    assert after4 == (0, 0)
    hip.resolve()
    h, l = hip.download()
    _same(h, one.hdr, "continued after the rebuild vs one shot (HDR)")
    _same(l, one.ldr, "continued after the rebuild vs one shot (LDR)")
    _same(h, cover_oracle[0], "continued after the rebuild vs the oracle (HDR)")
    _same(l, cover_oracle[1], "continued after the rebuild vs the oracle (LDR)")
    hip.render(W0, H0, 1, 1 + SPP0, DEPTH, SEED)
    after5 = (_excluded(hip), _sky_planes(hip))
    print("started again after the rebuild: excluded, ray-less planes = %s, %d tiles have an empty list" % (after5, one.empty))
    assert after5 == (one.empty, one.empty * SPP0)
    hip.resolve()
    h, l = hip.download()
    _same(h, one.hdr, "started again after the rebuild vs one shot (HDR)")
    _same(l, one.ldr, "started again after the rebuild vs one shot (LDR)")
    _same(h, cover_oracle[0], "started again after the rebuild vs the oracle (HDR)")
    _same(l, cover_oracle[1], "started again after the rebuild vs the oracle (LDR)")


@pytest.mark.gpu
def test_render_ahead(own, monkeypatch, cover, cover_oracle):
    """rt_set_frame_lookahead(4): the first 1-spp call traces four planes with one launch over the shorter queue, the next three
    calls only add their plane -- the flagged tiles' from the constant, which that launch never wrote."""
    _knobs(monkeypatch)
    one = _second_render(own, cover, W0, H0, 1, 1 + SPP0)
    assert one.empty > 0
    own.set_frame_lookahead(4)
    for s in range(1, 1 + SPP0):
        own.render(W0, H0, s, s + 1, DEPTH, SEED, stats=False)
        assert _excluded(own) == one.empty  # (the launch of the first call; the others launch no trace kernel)
    own.synchronize()
    assert _sky_planes(own) == one.empty * SPP0  # ONE launch traced all four planes
    own.resolve()
    h, l = own.download()
    _same(h, one.hdr, "render-ahead vs one shot (HDR)")
    _same(l, one.ldr, "render-ahead vs one shot (LDR)")
    _same(h, cover_oracle[0], "render-ahead vs the oracle (HDR)")


@pytest.mark.gpu
def test_row_shards(hip, monkeypatch, scenes_mod):
    """Every third row of 384x288 (576 full tiles in the shard) against the whole image's rows."""
    from cpuraytracer_amd import _capi
    W, H, spp = 384, 288, 2
    sc = scenes_mod.build_scene("cover", 1, W, H)
    _knobs(monkeypatch)
    whole = _second_render(hip, sc, W, H, 1, 1 + spp)
    rs = _capi.cyclic_rows(H, 1, 3)
    rows = [int(_capi.load().rt_rowset_global_row(rs, k)) for k in range(_capi.load().rt_rowset_local_rows(rs))]
    assert len(rows) == H // 3 and rows[:3] == [1, 4, 7]
    part = _second_render(hip, sc, W, H, 1, 1 + spp, rs)
    print("384x288: excluded %d of %d tiles of the image, %d of %d of the row shard" % (whole.excluded, len(whole.lens), part.excluded, len(part.lens)))
    assert len(part.lens) == 576 and part.empty > 0 and whole.empty > 0
    assert whole.excluded == whole.empty and part.excluded == part.empty
    assert part.sky == part.empty * spp
    _same(part.hdr, whole.hdr[rows], "row shard vs the image's rows (HDR)")
    _same(part.ldr, whole.ldr[rows], "row shard vs the image's rows (LDR)")
    _knobs(monkeypatch, exclude="0")
    off = _second_render(hip, sc, W, H, 1, 1 + spp, rs)
    assert off.excluded == 0
    _same_shot(part, off, "row shard, default vs RT_SKY_EXCLUDE=0")


def _two_small_spheres(scenes_mod, oracle, W, H, n_lights, glass=False):
    """The construction of test_gpu_sky_skip.py: two small spheres near the image centre of the C1 camera, no floor; the tiles of
    the middle rows list a sphere, the rest see only sky.  glass: the left sphere is made a transparent dielectric and moved under
    the pixel left of the image centre in the middle row, which is the last pixel of its tile and so one of the tile's pilots."""
    sc = scenes_mod.build_scene("three", 1, W, H)
    sph = sc.spheres[:2].copy()
    sph["cx"], sph["cy"], sph["cz"], sph["r"] = [-0.04, 0.05], [0.01, -0.01], [1.0, 1.04], [0.03, 0.035]
    mats = sc.materials[:2].copy()
    if glass:
        mats["type"][0], mats["ior"][0] = 2, 1.5  # RT_MAT_DIELECTRIC_TRANSPARENT
        sph["cx"], sph["cy"] = [-0.0052, 0.07], [0.0, -0.01]
    sc2 = oracle.Scene(sph, mats, sc.camera, sc.sun, sc.sky, sc.exposure_scale)
    sc2.lights = [] if n_lights == 0 else [sc.sun, oracle.make_light((-0.6, 0.7, 0.35), (0.35, 0.55, 1.0), 25000.0)][:n_lights]
    return sc2


def _oracle_shot(oracle, sc, W, H, spp):
    orc = oracle.Oracle()
    orc.upload(sc)
    st = orc.render(W, H, 1, 1 + spp, DEPTH, SEED, threads=4)
    orc.resolve()
    h, l = orc.download()
    orc.close()
    return h, l, (st.traversals, st.segments)


@pytest.mark.gpu
def test_two_lights(hip, oracle, scenes_mod, monkeypatch):
    """A light list of another length than 1 runs the _lights kernel over the shorter queue."""
    W, H, spp = 384, 192, 3
    sc = _two_small_spheres(scenes_mod, oracle, W, H, 2)
    got = _three_settings(hip, monkeypatch, sc, W, H, spp, "two spheres, two lights", min_empty=(W * H // 64) // 4)
    ho, lo, co = _oracle_shot(oracle, sc, W, H, spp)
    _same(got["default"].hdr, ho, "HDR vs the oracle")
    _same(got["default"].ldr, lo, "LDR vs the oracle")
    assert got["default"].counters == co


@pytest.mark.gpu
def test_odd_sky(hip, oracle, scenes_mod, monkeypatch):
    """A zero channel and a channel of -0 (0 + 1 * -0 = +0 before the exposure) at exposure 0.37: the constant formed by
    rt_sky_tiles_kernel has the bits the trace kernel stores and the bits the traced path gives.  (Not compared with the oracle: at
    an exposure that is no power of two the device's picture differs from the oracle's in the last bits under every setting.)"""
    from cpuraytracer_amd import _capi
    W, H, spp = 384, 192, 3
    sc = _two_small_spheres(scenes_mod, oracle, W, H, 0)
    sky = _capi.RtMaterial.from_buffer_copy(bytes(sc.sky))
    sky.luminance = 3.0
    sky.rgb0[0], sky.rgb0[1], sky.rgb0[2] = 0.0, 0.7, -0.0
    sc.sky, sc.exposure_scale = sky, 0.37
    got = _three_settings(hip, monkeypatch, sc, W, H, spp, "zero sky channel, exposure 0.37", min_empty=(W * H // 64) // 4)
    h = got["default"].hdr
    assert got["default"].lens[0] == 0  # the corner tile is one of the excluded
    assert h[0, 0, 0] == 0.0 and h[0, 0, 1] > 0.0 and h[0, 0, 2] == 0.0
    assert not np.signbit(h[0, 0]).any()  # +0 in both zero channels, as the traced path's 0 + 1 * -0


@pytest.mark.gpu
def test_fallback_image_order(oracle, scenes_mod, monkeypatch, cover, cover_oracle):
    """RT_TILE_ORDER=0 (read when the context is created): no order, so no tile is kept out; the tile-aware accumulation still runs."""
    from cpuraytracer_amd import HipRenderer
    monkeypatch.setenv("RT_TILE_ORDER", "0")
    r = HipRenderer(0)
    try:
        _knobs(monkeypatch)
        shot = _second_render(r, cover, W0, H0, 1, 1 + SPP0)
        assert shot.empty > 0 and shot.excluded == 0 and shot.sky == shot.empty * SPP0
        _same(shot.hdr, cover_oracle[0], "HDR vs the oracle")
        _same(shot.ldr, cover_oracle[1], "LDR vs the oracle")
        assert shot.counters == cover_oracle[2]
    finally:
        r.close()


@pytest.mark.gpu
def test_fallback_partial_last_tile(hip, scenes_mod, monkeypatch):
    """300x150: 703 full tiles and a last one of 8 pixels, whose paths follow the full tiles' in path-index space: every tile is queued."""
    W, H, spp = 300, 150, 2
    sc = scenes_mod.build_scene("cover", 1, W, H)
    got = {}
    for name in ("default", "exclude-off"):
        _knobs(monkeypatch, **SETTINGS[name])
        got[name] = _second_render(hip, sc, W, H, 1, 1 + spp)
    _knobs(monkeypatch)
    d = got["default"]
    print("300x150: %d full tiles, %d with an empty list" % (len(d.lens), d.empty))
    assert len(d.lens) == 703 and (W * H) % 64 == 8
    assert d.excluded == 0 and got["exclude-off"].excluded == 0
    _same_shot(d, got["exclude-off"], "300x150, default vs RT_SKY_EXCLUDE=0")


@pytest.mark.gpu
def test_flagged_tile_next_to_a_glass_tile(hip, oracle, scenes_mod, monkeypatch):
    """The neighbour rule of the work order raises a tile beside a glass tile to the glass class; a tile whose list is empty is
    flagged AFTER that rule -- the list is a proof, the pilots are a guess -- and must still be kept out, the picture unchanged.
    The rule fires only where a PILOT ray's first hit is glass (pixels 0, 32 and 63 of a tile at sample 1): the glass sphere sits
    under pixel 191 of row 96, the last pixel of tile (96, 2), which is asserted through the production scan on that very ray; the
    tile on its left, (96, 1), has an empty list.  Were the flag applied before the rule, that tile would be sorted with the glass
    and a real tile would take its place in the tail: the shortened launch would leave the real tile's planes to the other seed's
    samples (module docstring) and trace the flagged one twice over in the counters."""
    W, H, spp = 384, 192, 3
    sc = _two_small_spheres(scenes_mod, oracle, W, H, 1, glass=True)
    hip.upload(sc)
    pilot = hip.unit_primary_rays(W, H, [[191, 96, 1]])
    hit = hip.unit_closest_hit(pilot)
    assert int(hit[0, 1:2].view(np.int32)[0]) == 0 and int(sc.materials["type"][0]) == 2, "the pilot ray of pixel 191, row 96 does not hit the glass sphere first"
    got = _three_settings(hip, monkeypatch, sc, W, H, spp, "glass sphere", min_empty=(W * H // 64) // 4)
    d = got["default"]
    lens = d.lens.reshape(H, W // 64)
    assert lens[96, 2] not in (0, NONE), "the glass tile lists no sphere"
    assert lens[96, 1] == 0, "the tile left of the glass tile has no empty list"
    assert d.excluded == d.empty  # (asserted by _three_settings already: every empty-list tile, this neighbour among them)
    ho, lo, co = _oracle_shot(oracle, sc, W, H, spp)
    _same(d.hdr, ho, "HDR vs the oracle")
    _same(d.ldr, lo, "LDR vs the oracle")
    assert d.counters == co
