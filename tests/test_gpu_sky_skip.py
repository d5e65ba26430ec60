"""Empty-list tiles (rt_kernels.h, K_GEN of the flat hit-stash kernels): a full tile whose sphere list has length 0 can only see the
sky, so the wave stores the tile's 64 samples of a plane -- (0 + 1 * sky) * exposure, by the expressions of the miss transition and
finishPath -- without generating rays or scanning.  Nothing observable may change: HDR and LDR bits, the traversal and segment
counters, the per-path traversal counts, the tile statistics and the noise estimate equal those of RT_SKY_SKIP=0 and the oracle's.

The knob is read when an accumulation starts, like RT_PRIMARY_SPHERES.  A skipped plane counts as a directly resolved scan, as it
did before it was skipped.  That the early-out FIRES is the kernel's own count (rt_unit_sky_planes: planes finished without rays):
it must equal (tiles whose device list has length 0) x spp with the knob on and 0 with RT_SKY_SKIP=0, in every case below -- the one
observable the two settings differ in, so that the file cannot pass with the early-out dead.

Not reachable today: the store trav_out[slot] = 1 of a skipped path.  Only rt_unit_trace sets trav_out, and it launches with a path
list, which has no tile tables and never skips; rt_render passes no trav_out.  The per-path counts below therefore come from code the
knob does not touch; what they check is that the skipped paths' share of the render's traversal counter (nTrav) is right."""
import ctypes as C

import numpy as np
import pytest

NONE = 0xFFFF
DEPTH, SEED = 50, 1


@pytest.fixture(scope="module")
def scenes_mod(built):
    from cpuraytracer_amd import scenes
    return scenes


@pytest.fixture()
def nr(built):
    """A context of its own for the noise-estimate switch."""
    from cpuraytracer_amd import HipRenderer
    r = HipRenderer(0)
    yield r
    r.close()


def _knob(monkeypatch, v):
    if v is None:
        monkeypatch.delenv("RT_SKY_SKIP", raising=False)
    else:
        monkeypatch.setenv("RT_SKY_SKIP", v)


def _list_lengths(hip, W, H, rs):
    """First half-word of every full tile's sphere list as the device built it (NONE: no list)."""
    from cpuraytracer_amd import _capi
    L = _capi.load()
    cap = (W * L.rt_rowset_local_rows(rs)) >> 6
    lists = np.zeros((max(cap, 1), 64), dtype=np.uint16)
    n = C.c_uint32(0)
    _capi.check(L.rt_unit_tile_spheres(hip._h, W, H, rs, cap, C.byref(n), lists.ctypes.data, None))
    return lists[:n.value, 0].copy()


def _scans(hip, W, H, rs):
    """(scans of 64 fresh paths, those that took a tile's tables, those resolved from a sphere list) of the last render."""
    from cpuraytracer_amd import _capi
    L = _capi.load()
    n = C.c_uint32(0)
    scans = np.zeros(3, dtype=np.uint64)
    _capi.check(L.rt_unit_tile_spheres(hip._h, W, H, rs, 0, C.byref(n), None, scans.ctypes.data))
    return int(scans[0]), int(scans[1]), int(scans[2])


def _sky_planes(hip):
    """Planes of 64 paths the last render finished without rays (the kernel's own count)."""
    from cpuraytracer_amd import _capi
    n = C.c_uint64(0)
    _capi.check(_capi.load().rt_unit_sky_planes(hip._h, C.byref(n)))
    return int(n.value)


def _render(hip, sc, W, H, s0, s1, rs=None):
    """One accumulation [s0, s1) of a freshly uploaded scene: HDR, LDR, (traversals, segments), the kernel's scan statistics, and
    its count of planes finished without rays."""
    from cpuraytracer_amd import _capi
    hip.upload(sc)
    st = hip.render(W, H, s0, s1, DEPTH, SEED, rowset=rs)
    scans = _scans(hip, W, H, rs if rs is not None else _capi.whole_image(H))
    sky = _sky_planes(hip)
    hip.resolve()
    h, l = hip.download()
    return h, l, (st.traversals, st.segments), scans, sky


def _oracle(oracle, sc, W, H, s0, s1, rs=None):
    orc = oracle.Oracle()
    orc.upload(sc)
    st = orc.render(W, H, s0, s1, DEPTH, SEED, rowset=rs, threads=4)
    orc.resolve()
    h, l = orc.download()
    orc.close()
    return h, l, (st.traversals, st.segments)


def _same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape, what
    bad = a.view(np.uint32 if a.dtype == np.float32 else a.dtype) != b.view(np.uint32 if b.dtype == np.float32 else b.dtype)
    assert not bad.any(), "%s: %d of %d values differ, first at %s" % (what, int(bad.sum()), bad.size, np.argwhere(bad)[0])


def _on_off_oracle(hip, oracle, monkeypatch, sc, W, H, spp, label, rs=None, min_empty=1, check_oracle=True):
    """The render with the knob off, with the default, and the oracle's: equal bits and counters; the direct count is that of the
    tiles with a list (skipped planes included) under both settings, and at least `min_empty` tiles have an empty one (0 for the
    shapes the cases are defined at but where no tile gets a list: a tile is 64 pixels of one row, and at these widths its cone
    spans too much of the picture)."""
    from cpuraytracer_amd import _capi
    got = {}
    for v in ("0", None):
        _knob(monkeypatch, v)
        got[v] = _render(hip, sc, W, H, 1, 1 + spp, rs)
    lens = _list_lengths(hip, W, H, rs if rs is not None else _capi.whole_image(H))
    empty, listed = int((lens == 0).sum()), int((lens != NONE).sum())
    print("%s: %d full tiles, %d with a list, %d of them empty; scans (total, with tables, direct) off %s on %s; planes without rays off %d on %d"
          % (label, len(lens), listed, empty, got["0"][3], got[None][3], got["0"][4], got[None][4]))
    assert empty >= min_empty, "%s: %d tiles have an empty list, at least %d are needed for the early-out to be exercised" % (label, empty, min_empty)
    for v in ("0", None):
        total, masked, direct = got[v][3]
        assert direct == listed * spp and direct >= empty * spp, (label, v, total, masked, direct, listed, empty)
    _same(got[None][0], got["0"][0], "%s: HDR, knob on vs off" % label)
    _same(got[None][1], got["0"][1], "%s: LDR, knob on vs off" % label)
    assert got[None][2] == got["0"][2], "%s: traversal counters differ between knob on and off" % label
    assert got[None][3] == got["0"][3], "%s: tile statistics differ between knob on and off" % label
    assert got["0"][4] == 0, "%s: %d planes were finished without rays with RT_SKY_SKIP=0" % (label, got["0"][4])
    assert got[None][4] == empty * spp, "%s: %d planes finished without rays, %d tiles x %d samples have an empty list" % (label, got[None][4], empty, spp)
    if not check_oracle:
        return got
    ho, lo, co = _oracle(oracle, sc, W, H, 1, 1 + spp, rs)
    _same(got[None][0], ho, "%s: HDR vs the oracle" % label)
    _same(got[None][1], lo, "%s: LDR vs the oracle" % label)
    assert got[None][2] == co, "%s: traversal counters differ from the oracle's" % label
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("aperture", [-1.0, 2.0], ids=["default-camera", "aperture-2"])
def test_cover_equals_the_knob_off_render_and_the_oracle(hip, oracle, scenes_mod, monkeypatch, aperture):
    """(a), (b): sky, horizon and ground tiles in one picture; at aperture 2.0 the lens widens what a tile can see."""
    W, H, spp = 256, 128, 4
    sc = scenes_mod.build_scene("cover", 1, W, H, aperture=aperture)
    got = _on_off_oracle(hip, oracle, monkeypatch, sc, W, H, spp, "cover %dx%d aperture %g" % (W, H, aperture))
    # per-path traversal counts from an explicit path list (a launch that never skips, with either knob: see the module's docstring);
    # their sum against the SKIPPING render's counter checks the traversals that render counted for the paths it did not trace
    jj, ii = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    ijs = np.concatenate([np.stack([ii.ravel(), jj.ravel(), np.full(ii.size, s)], axis=1) for s in range(1, 1 + spp)]).astype(np.uint32)
    trav = {}
    for v in ("0", None):
        _knob(monkeypatch, v)
        hip.upload(sc)
        trav[v] = hip.unit_trace(W, H, ijs, DEPTH, SEED)
    _same(trav[None][0], trav["0"][0], "per-path radiance, knob on vs off")
    assert np.array_equal(trav[None][1], trav["0"][1]), "per-path traversal counts differ between knob on and off"
    assert int(trav[None][1].astype(np.uint64).sum()) == got[None][2][0], "per-path traversal counts do not add up to the render's counter"
    assert int((trav[None][1] == 1).sum()) > 0  # paths that end on their first scan: the sky


def _two_small_spheres(scenes_mod, oracle, W, H, n_lights):
    """Two small spheres near the image centre of the C1 camera (origin, looking along +z, focused at distance 1), no floor.  They
    sit about the plane of focus, so the lens hardly widens them.  A tile is 64 pixels of one row, half a row here, and the cone
    about it reaches 32 rows up and down, so the tiles of the middle rows list a sphere; the rest (over a third) see only sky."""
    sc = scenes_mod.build_scene("three", 1, W, H)
    sph = sc.spheres[:2].copy()
    sph["cx"], sph["cy"], sph["cz"], sph["r"] = [-0.04, 0.05], [0.01, -0.01], [1.0, 1.04], [0.03, 0.035]
    sc2 = oracle.Scene(sph, sc.materials[:2].copy(), sc.camera, sc.sun, sc.sky, sc.exposure_scale)
    sc2.lights = [] if n_lights == 0 else [sc.sun, oracle.make_light((-0.6, 0.7, 0.35), (0.35, 0.55, 1.0), 25000.0)][:n_lights]
    return sc2


@pytest.mark.gpu
@pytest.mark.parametrize("n_lights", [0, 2], ids=["no-lights", "two-lights"])
def test_two_small_spheres_whole_blocks_are_skipped(hip, oracle, scenes_mod, monkeypatch, n_lights):
    """(c): with the sky tiles last in work order, whole queue blocks are skipped back to back; a light list of another length than 1
    runs the _lights kernel."""
    W, H, spp = 128, 64, 3
    sc = _two_small_spheres(scenes_mod, oracle, W, H, n_lights)
    _on_off_oracle(hip, oracle, monkeypatch, sc, W, H, spp, "two spheres, %d lights" % n_lights, min_empty=(W * H // 64) // 4)


@pytest.mark.gpu
@pytest.mark.parametrize("tile_order", ["1", "0"], ids=["sky-last", "image-order"])
@pytest.mark.parametrize("shape", [(192, 64), (256, 128)], ids=["192x64", "256x128"])
def test_queue_ending_on_skipped_tiles_drains_the_stash(oracle, scenes_mod, monkeypatch, tile_order, shape):
    """(d): with the tile order on, sky tiles come last in work order, so a wave's queue ends on skipped planes while hits of earlier
    tiles wait in its stash; they must still be popped and finished.  RT_TILE_ORDER is read when the context is created.  At 192x64
    no tile of the cover scene gets a list, so that shape pins the picture and a count of 0 skipped planes (asserted); at 256x128 44
    tiles are empty.  That records wait in a stash at the moment a queue ends is not observable from outside the kernel: a lost record
    would show as a pixel or a counter that differs from the oracle's."""
    from cpuraytracer_amd import HipRenderer
    (W, H), spp = shape, 2
    monkeypatch.setenv("RT_TILE_ORDER", tile_order)
    r = HipRenderer(0)
    try:
        sc = scenes_mod.build_scene("cover", 1, W, H)
        _on_off_oracle(r, oracle, monkeypatch, sc, W, H, spp, "cover %dx%d RT_TILE_ORDER=%s" % (W, H, tile_order), min_empty=0 if W == 192 else 8)
    finally:
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(128, 66), (384, 198)], ids=["128x66", "384x198"])
def test_row_shards_and_resumed_accumulation(hip, oracle, scenes_mod, monkeypatch, shape):
    """(e): every third row against the one-shot image's rows; s0 = 1..3 then 3..5 against the one-shot 1..5.  At 128x66 no tile of
    the row shard has an empty list; the larger shape is there for the early-out to fire in both layouts."""
    from cpuraytracer_amd import _capi
    W, H = shape
    sc = scenes_mod.build_scene("cover", 1, W, H)
    _knob(monkeypatch, None)
    whole, whole_l, _, wscans, wsky = _render(hip, sc, W, H, 1, 5)
    wlens = _list_lengths(hip, W, H, _capi.whole_image(H))
    rs = _capi.cyclic_rows(H, 1, 3)
    rows = [int(_capi.load().rt_rowset_global_row(rs, k)) for k in range(_capi.load().rt_rowset_local_rows(rs))]
    assert len(rows) == H // 3 and rows[:3] == [1, 4, 7]
    part, part_l, _, scans, sky = _render(hip, sc, W, H, 1, 5, rs)
    lens = _list_lengths(hip, W, H, rs)
    print("%dx%d: empty lists in %d of %d tiles of the image, %d of %d of the row shard" % (W, H, (wlens == 0).sum(), len(wlens), (lens == 0).sum(), len(lens)))
    assert ((wlens == 0).any() and (lens == 0).any()) == (W > 128), "empty lists are expected at the larger shape only"
    assert wsky == int((wlens == 0).sum()) * 4 and sky == int((lens == 0).sum()) * 4, (wsky, sky)
    assert wscans[2] == int((wlens != NONE).sum()) * 4 and scans[2] == int((lens != NONE).sum()) * 4
    _same(part, whole[rows], "row shard vs the one-shot image's rows (HDR)")
    _same(part_l, whole_l[rows], "row shard vs the one-shot image's rows (LDR)")
    _knob(monkeypatch, "0")
    off, off_l, _, _, off_sky = _render(hip, sc, W, H, 1, 5, rs)
    assert off_sky == 0
    _same(part, off, "row shard, knob on vs off")
    _knob(monkeypatch, None)
    hip.upload(sc)
    st1 = hip.render(W, H, 1, 3, DEPTH, SEED)
    st2 = hip.render(W, H, 3, 5, DEPTH, SEED)
    assert _sky_planes(hip) == int((wlens == 0).sum()) * 2  # the second call's own launch
    hip.resolve()
    h, l = hip.download()
    _same(h, whole, "resumed accumulation vs one shot (HDR)")
    _same(l, whole_l, "resumed accumulation vs one shot (LDR)")
    ho, lo, co = _oracle(oracle, sc, W, H, 1, 5)
    _same(whole, ho, "one shot vs the oracle")
    assert (st1.traversals + st2.traversals, st1.segments + st2.segments) == co


@pytest.mark.gpu
def test_noise_estimate_equals_the_knob_off_one(nr, scenes_mod, monkeypatch):
    """(f): the second moments are formed from the sample buffer, which holds the same samples."""
    W, H, spp = 256, 128, 4
    sc = scenes_mod.build_scene("cover", 1, W, H)
    got = {}
    for v in ("0", None):
        _knob(monkeypatch, v)
        nr.upload(sc)
        nr.set_noise_estimate(True)
        nr.render(W, H, 1, 1 + spp, DEPTH, SEED)
        nr.synchronize()
        got[v] = (nr.download(ldr=False)[0], nr.download_moments(), nr.noise_map())
    assert (got[None][1] > 0).any()
    _same(got[None][0], got["0"][0], "HDR")
    _same(got[None][1], got["0"][1], "second moments")
    _same(got[None][2], got["0"][2], "error map")


@pytest.mark.gpu
def test_sky_with_a_zero_channel_and_another_exposure(hip, oracle, scenes_mod, monkeypatch):
    """(g): the scene's sky material and exposure scale are plain inputs of rt_scene_upload.  A zero channel and a channel of -0
    (0 + 1 * -0 = +0 before the exposure): the stored bits are those of the knob-off render.  (Not compared with the oracle: at an
    exposure that is no power of two the device's picture differs from the oracle's in the last bits with the knob off as well --
    the stock scenes' 2^-15 makes every product with it exact.)"""
    from cpuraytracer_amd import _capi
    W, H, spp = 128, 64, 3
    sc = _two_small_spheres(scenes_mod, oracle, W, H, 0)
    sky = _capi.RtMaterial.from_buffer_copy(bytes(sc.sky))
    sky.luminance = 3.0
    sky.rgb0[0], sky.rgb0[1], sky.rgb0[2] = 0.0, 0.7, -0.0
    sc.sky, sc.exposure_scale = sky, 0.37
    got = _on_off_oracle(hip, oracle, monkeypatch, sc, W, H, spp, "zero sky channel, exposure 0.37", min_empty=(W * H // 64) // 4,
                         check_oracle=False)
    h = got[None][0]
    assert (h[0, 0] == h[0, 0]).all() and h[0, 0, 0] == 0.0 and h[0, 0, 1] > 0.0  # the corner pixel is sky
