"""The tiles' work order on the device (csrc/rt_kernels.h rt_pilot_rays_kernel, rt_tile_class_kernel, rt_tile_order_kernel;
csrc/rt_capi.hip LaunchTileOrder) against the numpy model of its contract (tests/work_order_cases.py; include/rt_api.h,
rt_unit_tile_order).  No picture, sample or counter depends on the order, so no other test can see it: an ascending sort, a neighbour
rule that never fires, classes from the wrong pilot or an order kept across a material edit leave every other test green.

Everything is exact equality: the pilots' rays and first hits are bit-equal to the oracle's, the rest is integers."""
import ctypes as C

import numpy as np
import pytest
import torch  # before the library is loaded, as in bench.py and tests/test_streams.py: the two then share one HIP runtime

import work_order_cases as wc

SKY_KNOBS = ("RT_SKY_EXCLUDE", "RT_SKY_SKIP")
MASK_KNOBS = ("RT_PRIMARY_MASK", "RT_PRIMARY_MASK_LIMIT", "RT_PRIMARY_SPHERES")


def _defaults(monkeypatch):
    for name in SKY_KNOBS + MASK_KNOBS + ("RT_TILE_ORDER",):
        monkeypatch.delenv(name, raising=False)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _first_difference(a, b):
    bad = np.argwhere(np.asarray(a) != np.asarray(b))
    return "%d of %d differ, first at %s: %s vs %s" % (len(bad), np.asarray(a).size, bad[0], np.asarray(a)[tuple(bad[0])], np.asarray(b)[tuple(bad[0])])


def _assert_equals_model(got, m, what, rays=True):
    assert got is not None and len(got["classes"]) == m["n"], "%s: %s tiles, the model has %d" % (what, None if got is None else len(got["classes"]), m["n"])
    if rays:
        assert np.array_equal(_bits(got["pilot_rays"]), _bits(m["pilot_rays"])), "%s: pilot rays: %s" % (what, _first_difference(_bits(got["pilot_rays"]), _bits(m["pilot_rays"])))
    assert np.array_equal(got["flags"], m["flags"]), "%s: flags: %s" % (what, _first_difference(got["flags"], m["flags"]))
    assert np.array_equal(got["classes"], m["classes"]), "%s: classes: %s" % (what, _first_difference(got["classes"], m["classes"]))
    assert int(got["info"][0]) == int(m["flags"].sum()), "%s: info[0] = %d, %d tiles are flagged" % (what, got["info"][0], m["flags"].sum())
    if m["sky"] is not None:
        assert np.array_equal(got["info"][1:], _bits(m["sky"])), "%s: the constant sample %s, the oracle's sky sample %s" % (what, got["info"][1:], _bits(m["sky"]))
    assert np.array_equal(got["order"], m["order"]), "%s: order: %s" % (what, _first_difference(got["order"], m["order"]))


# ------------------------------------------------------------------------------------------------------------------ the sort
@pytest.mark.gpu
def test_sort_equals_the_stable_descending_argsort_at_every_tile_count(hip):
    """rt_unit_tile_order_sort -- the production kernel, one workgroup of 1024 threads -- over every case of work_order_cases.sort_cases():
    n from 1 to 2^20 around the edges of per = ceil(n / 1024), the waves' prefix sums and the sixteen waves' totals.  The order equals
    numpy's stable argsort by descending class and the 64 guard words behind it are intact."""
    failures, cases = [], 0
    for label, classes in wc.sort_cases():
        order, guards = hip.unit_tile_order_sort(classes)
        cases += 1
        if not (guards == 0xFFFFFFFF).all():
            failures.append("%s: %d guard words overwritten" % (label, int((guards != 0xFFFFFFFF).sum())))
        want = wc.stable_descending(classes)
        if not np.array_equal(order, want):
            failures.append("%s: %s" % (label, _first_difference(order, want)))
    print("%d sort cases, %d failures" % (cases, len(failures)))
    assert not failures, failures[:20]


# ------------------------------------------------------------------------------------------------------------------ pilots, classes, flags, order
@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(wc.CASES)))
def test_fresh_build_equals_the_model(hip, oracle, monkeypatch, k):
    """source 0 on every scene case: the pilot rays equal the oracle's primary rays of pixels 0, 32 and 63 of every tile at sample 1 bit
    for bit (which pixels and which sample, under each row set, aperture and sampler); classes and flags equal the model's; info[0]
    is the number of flagged tiles and info[1..3] the sky sample the oracle traces; the order is the model's.  With RT_SKY_EXCLUDE=0, and
    again with RT_SKY_SKIP=0, no class 0 occurs and the other classes are unchanged."""
    _defaults(monkeypatch)
    c, m, m0 = wc.case(oracle, k), wc.case_model(oracle, k), wc.case_model(oracle, k, False)
    hip.upload(c.sc)
    hip.set_sampler(c.sampler)
    try:
        _assert_equals_model(hip.unit_tile_order(c.W, c.H, c.rs), m, c.label)
        for knob in SKY_KNOBS:
            _defaults(monkeypatch)
            monkeypatch.setenv(knob, "0")
            got = hip.unit_tile_order(c.W, c.H, c.rs)
            _assert_equals_model(got, m0, "%s, %s=0" % (c.label, knob))
            assert (got["classes"] >= 1).all() and not got["flags"].any() and not got["info"].any()
            keep = m["flags"] == 0
            assert np.array_equal(got["classes"][keep], m["classes"][keep])
    finally:
        hip.set_sampler(0)


# ------------------------------------------------------------------------------------------------------------------ production
def _threshold_heights():
    """Heights of a picture 256 wide (4 tiles a row) just above the work order's threshold of 2 x compute units full tiles, and one
    tile row short of it."""
    cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
    above, below = (2 * cus) // 4 + 1, (2 * cus + 3) // 4 - 1
    assert 4 * above >= 2 * cus > 4 * below > 0
    return cus, above, below


def _whole(H):
    from cpuraytracer_amd import _capi
    return _capi.whole_image(H)


def _cover(W, H):
    from cpuraytracer_amd import scenes
    return scenes.build_scene("cover", 1, W, H)


@pytest.fixture()
def own(built):
    from cpuraytracer_amd import HipRenderer
    r = HipRenderer(0)
    yield r
    r.close()


@pytest.mark.gpu
def test_render_keeps_and_uses_the_models_order(own, oracle, monkeypatch):
    """A cover picture with just over 2 x compute-units full tiles: after one rt_render of one sample at depth 2, source 1 -- what the
    context keeps for the accumulation -- equals source 0 and the model.  One tile row fewer: no order is kept."""
    _defaults(monkeypatch)
    cus, above, below = _threshold_heights()
    W = 256
    sc = _cover(W, above)
    m = wc.model(oracle, sc, W, above, _whole(above), 0)
    own.upload(sc)
    assert own.unit_tile_order(W, above, source=1) is None, "an order is kept before anything was rendered"
    own.render(W, above, 1, 2, 2, 1)
    kept = own.unit_tile_order(W, above, source=1)
    print("%d compute units: 256x%d has %d full tiles, 256x%d has %d" % (cus, above, m["n"], below, 4 * below))
    _assert_equals_model(kept, m, "kept after rt_render")
    _assert_equals_model(own.unit_tile_order(W, above, source=0), m, "fresh")
    assert own.unit_tile_order(W, above + 1, source=1) is None, "source 1 answers for another picture"
    lo = _cover(W, below)
    own.upload(lo)
    own.render(W, below, 1, 2, 2, 1)
    assert own.unit_tile_order(W, below, source=1) is None, "%d full tiles are below the threshold of %d" % (4 * below, 2 * cus)
    assert own.unit_tile_order(W, below, source=0) is not None  # (the unit entry builds for any tile count)


@pytest.mark.gpu
def test_no_order_is_kept_under_rt_tile_order_0(oracle, monkeypatch):
    from cpuraytracer_amd import HipRenderer
    _defaults(monkeypatch)
    _, above, _ = _threshold_heights()
    monkeypatch.setenv("RT_TILE_ORDER", "0")  # read when the context is created
    r = HipRenderer(0)
    try:
        sc = _cover(256, above)
        r.upload(sc)
        r.render(256, above, 1, 2, 2, 1)
        assert r.unit_tile_order(256, above, source=1) is None
        _assert_equals_model(r.unit_tile_order(256, above, source=0), wc.model(oracle, sc, 256, above, _whole(above), 0), "fresh under RT_TILE_ORDER=0")
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------------------------ edits
class _Edited:
    """A scene with some of its records replaced (the tables of rt_api.h, as HipRenderer.upload and the oracle read them)."""

    def __init__(self, sc, materials=None, camera=None):
        self.spheres, self.materials = sc.spheres, sc.materials if materials is None else materials
        self.camera, self.sun, self.sky, self.exposure_scale = sc.camera if camera is None else camera, sc.sun, sc.sky, sc.exposure_scale
        self.n = sc.n


@pytest.mark.gpu
def test_kept_order_follows_material_and_camera_edits(own, oracle, monkeypatch):
    """rt_set_materials swaps the records of the diffuse and of the glass sphere that most pilots hit first; after the next rt_render
    the kept order is that of the NEW types -- equal to a fresh build and to the model of the edited scene -- and differs from the
    old one.  The same after rt_set_camera.  A stale order here is a finding."""
    from cpuraytracer_amd import scenes
    _defaults(monkeypatch)
    _, H, _ = _threshold_heights()
    W = 256
    sc = _cover(W, H)
    rs = _whole(H)
    m = wc.model(oracle, sc, W, H, rs, 0)
    own.upload(sc)
    own.render(W, H, 1, 2, 2, 1)
    _assert_equals_model(own.unit_tile_order(W, H, source=1), m, "before the edits")
    hit = m["pilot_sphere"][m["pilot_sphere"] >= 0]
    ty, small = np.asarray(sc.materials["type"]), np.abs(np.asarray(sc.spheres["r"])) < 100.0
    count = np.bincount(hit, minlength=sc.n)
    diffuse = int(np.argmax(np.where((ty == 0) & small, count, -1)))
    glass = int(np.argmax(np.where((ty == wc.GLASS) & small, count, -1)))
    assert count[diffuse] > 0 and count[glass] > 0 and ty[diffuse] == 0 and ty[glass] == wc.GLASS
    mats = sc.materials.copy()
    mats[[diffuse, glass]] = mats[[glass, diffuse]]
    own.set_materials(mats, forget=False)
    assert own.unit_tile_order(W, H, source=1) is None, "the old order outlived rt_set_materials"
    own.render(W, H, 1, 2, 2, 1)
    edited = _Edited(sc, materials=mats)
    m1 = wc.model(oracle, edited, W, H, rs, 0)
    assert not np.array_equal(m1["classes"], m["classes"]), "the edit does not change a class: it tests nothing"
    _assert_equals_model(own.unit_tile_order(W, H, source=1), m1, "kept after rt_set_materials")
    _assert_equals_model(own.unit_tile_order(W, H, source=0), m1, "fresh after rt_set_materials")
    cam = scenes.orbit_camera(sc.camera, 9.0)
    own.set_camera(cam)
    assert own.unit_tile_order(W, H, source=1) is None, "the old order outlived rt_set_camera"
    own.render(W, H, 1, 2, 2, 1)
    m2 = wc.model(oracle, _Edited(sc, materials=mats, camera=cam), W, H, rs, 0)
    assert not np.array_equal(m2["classes"], m1["classes"])
    _assert_equals_model(own.unit_tile_order(W, H, source=1), m2, "kept after rt_set_camera")
    _assert_equals_model(own.unit_tile_order(W, H, source=0), m2, "fresh after rt_set_camera")


# ------------------------------------------------------------------------------------------------------------------ refusals
@pytest.mark.gpu
def test_refusals(own, oracle, monkeypatch):
    from cpuraytracer_amd import _capi
    _defaults(monkeypatch)
    L = _capi.load()
    INVALID, NO_SCENE = 2, 3
    n = C.c_uint32(77)
    out = np.zeros(64 + 8, dtype=np.uint32)
    good = np.array([0, 4, 2, 1, 3, 3, 0, 4], dtype=np.uint8)
    # the sort: needs no scene
    assert L.rt_unit_tile_order_sort(own._h, good.ctypes.data, 8, out.ctypes.data) == 0
    assert np.array_equal(out[:8], wc.stable_descending(good)) and (out[8:] == 0xFFFFFFFF).all()
    for bad in (5, 6, 255):
        a = good.copy()
        a[5] = bad
        assert L.rt_unit_tile_order_sort(own._h, a.ctypes.data, 8, out.ctypes.data) == INVALID and b"class" in L.rt_last_error()
    assert L.rt_unit_tile_order_sort(own._h, good.ctypes.data, 0, out.ctypes.data) == INVALID
    assert L.rt_unit_tile_order_sort(own._h, None, 8, out.ctypes.data) == INVALID
    assert L.rt_unit_tile_order_sort(own._h, good.ctypes.data, 8, None) == INVALID
    assert L.rt_unit_tile_order_sort(None, good.ctypes.data, 8, out.ctypes.data) == INVALID
    # the order
    c = wc.case(oracle, 9)
    args = (c.W, c.H, c.rs)
    assert L.rt_unit_tile_order(own._h, *args, 0, 0, C.byref(n), None, None, None, None, None) == NO_SCENE and b"no scene" in L.rt_last_error()
    own.upload(c.sc)
    assert L.rt_unit_tile_order(None, *args, 0, 0, C.byref(n), None, None, None, None, None) == INVALID
    assert L.rt_unit_tile_order(own._h, *args, 0, 0, None, None, None, None, None, None) == INVALID
    assert L.rt_unit_tile_order(own._h, 0, c.H, c.rs, 0, 0, C.byref(n), None, None, None, None, None) == INVALID
    assert L.rt_unit_tile_order(own._h, c.W, 0, c.rs, 0, 0, C.byref(n), None, None, None, None, None) == INVALID
    assert L.rt_unit_tile_order(own._h, *args, 2, 0, C.byref(n), None, None, None, None, None) == INVALID and b"source" in L.rt_last_error()
    beyond = _capi.RtRowset(10, c.H, c.H, 0, 1)  # rows 10 .. H + 9 of an image of H rows
    assert L.rt_unit_tile_order(own._h, c.W, c.H, beyond, 0, 0, C.byref(n), None, None, None, None, None) == INVALID and b"bad row set" in L.rt_last_error()
    # every output pointer null: only the count
    n.value = 77
    assert L.rt_unit_tile_order(own._h, *args, 0, 0, C.byref(n), None, None, None, None, None) == 0 and n.value == (c.W * c.H) >> 6
    cls = np.zeros(n.value, dtype=np.uint8)
    assert L.rt_unit_tile_order(own._h, *args, 0, n.value - 1, C.byref(n), None, cls.ctypes.data, None, None, None) == INVALID
    assert b"capacity too small" in L.rt_last_error() and n.value == (c.W * c.H) >> 6
    assert L.rt_unit_tile_order(own._h, *args, 0, n.value, C.byref(n), None, cls.ctypes.data, None, None, None) == 0
    assert np.array_equal(cls, wc.case_model(oracle, 9)["classes"])
    # a strip without a full tile: no order, no error
    assert L.rt_unit_tile_order(own._h, 9, 7, _capi.whole_image(7), 0, 0, C.byref(n), None, None, None, None, None) == 0 and n.value == 0
    assert L.rt_unit_tile_order(own._h, *args, 1, 0, C.byref(n), None, None, None, None, None) == 0 and n.value == 0  # nothing rendered


@pytest.mark.gpu
def test_entries_leave_a_running_accumulation_alone(own, oracle, monkeypatch):
    """Samples [1, 3), then both entries -- the sort, a fresh build for this picture and one for another picture -- then [3, 5): the
    strip equals the one-shot [1, 5), and what the context keeps for the accumulation is what it kept before the calls."""
    _defaults(monkeypatch)
    _, H, _ = _threshold_heights()
    W, depth, seed = 256, 8, 5
    sc = _cover(W, H)
    own.upload(sc)
    own.render(W, H, 1, 5, depth, seed)
    one, _ = own.download(ldr=False)
    own.upload(sc)
    own.render(W, H, 1, 3, depth, seed)
    before = own.unit_tile_order(W, H, source=1)
    assert before is not None
    own.unit_tile_order_sort(np.arange(3000) % 5)
    fresh = own.unit_tile_order(W, H, source=0)
    other = own.unit_tile_order(wc.CAP_W, wc.CAP_H, source=0)
    assert other is not None and len(other["classes"]) == (wc.CAP_W * wc.CAP_H) >> 6
    after = own.unit_tile_order(W, H, source=1)
    for name in ("pilot_rays", "classes", "flags", "order", "info"):
        assert np.array_equal(_bits(before[name]) if name == "pilot_rays" else before[name], _bits(after[name]) if name == "pilot_rays" else after[name]), name
        assert np.array_equal(_bits(before[name]) if name == "pilot_rays" else before[name], _bits(fresh[name]) if name == "pilot_rays" else fresh[name]), name
    own.render(W, H, 3, 5, depth, seed)
    two, _ = own.download(ldr=False)
    assert np.array_equal(_bits(one), _bits(two)), "the strip after [1, 3) + entries + [3, 5) differs from the one-shot [1, 5)"
