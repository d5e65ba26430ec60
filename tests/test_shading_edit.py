"""rt_set_materials, rt_set_lights, rt_set_exposure and rt_temporal_forget on the device: shading edits without a scene upload.  The core
comparison takes two contexts: B uploads scene S1, renders something and edits it to S2; A uploads S2.  From there both run the same
calls, and everything they hand out is compared bit for bit (tests/test_set_camera.py's `everything`, plus rt_denoise_variance and a
three-frame rt_denoise_temporal_variance chain)."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch  # before the library is loaded, as in tests/test_streams.py: a torch stream's handle is then a stream of the library's runtime

from temporal_common import NO_TARGET, TDEFAULTS, history_of
from test_denoise_cpu import DEFAULTS
from test_noise_estimate_cpu import assert_same_bits
from test_set_camera import assert_same_everything, code_of, everything, one_shot, rowset_of, three_lights_glossy

pytestmark = pytest.mark.gpu

RT_ERR_INVALID_ARG, RT_ERR_NO_SCENE, RT_ERR_SEQUENCE = 2, 3, 6
SKY = 0xFFFFFFFF
SHAPES = {"96x64": (96, 64), "70x41": (70, 41)}
GLASS, METAL, DIFFUSE, EMISSIVE = 2, 1, 0, 3


@pytest.fixture(scope="module")
def scenes(built):
    from cpuraytracer_amd import scenes
    return scenes


@pytest.fixture()
def ctxs(built):
    """Contexts of the test's own, closed afterwards."""
    from cpuraytracer_amd import HipRenderer
    made = []

    def make():
        made.append(HipRenderer(0))
        return made[-1]
    yield make
    for r in made:
        r.close()


def byte(k):
    return np.float32(k) * np.float32(1.0 / 255.0)


def edited(sc, materials=None, sky=None, lights=None, exposure=None):
    out = copy.copy(sc)
    if materials is not None:
        out.materials = materials
    if sky is not None:
        out.sky = sky
    if lights is not None:
        out.lights = list(lights)
    if exposure is not None:
        out.exposure_scale = float(exposure)
    return out


def lights_of(sc):
    ls = getattr(sc, "lights", None)
    return [sc.sun] if ls is None else list(ls)


def apply_edit(r, s1, s2, forget=False):
    """The calls that take a context holding S1 to S2 (same spheres, camera and light directions)."""
    if s2.materials is not s1.materials or s2.sky is not s1.sky:
        r.set_materials(s2.materials, s2.sky, forget=forget)
    if getattr(s2, "lights", None) is not getattr(s1, "lights", None):
        r.set_lights(lights_of(s2))
    if s2.exposure_scale != s1.exposure_scale:
        r.set_exposure(s2.exposure_scale)


def recoloured(sc, every=3):
    """Every `every`-th opaque or metal sphere gets another byte colour (the table still packs into 16 bytes)."""
    m = sc.materials.copy()
    pick = np.nonzero((m["type"] == DIFFUSE) | (m["type"] == METAL))[0][::every]
    assert pick.size > 0
    for k in pick:
        m["rgb0"][k] = [byte((37 * k + 11) % 256), byte((91 * k + 5) % 256), byte((53 * k + 200) % 256)]
    assert not np.array_equal(m["rgb0"], sc.materials["rgb0"])
    return m, [int(k) for k in pick]


def all_of(r, W, H, spp, depth, seed=1):
    """`everything` of tests/test_set_camera.py, then what this issue adds: rt_denoise_variance, and three frames of the
    rt_denoise_temporal_variance chain (one sample each, seeds seed + f, bilinear fetch, spatial variance) on an empty history."""
    from cpuraytracer_amd import _capi
    out = everything(r, W, H, None, spp, depth, seed, tables=True, temporal=False)
    V = _capi.variance_params(source=1)
    r.denoise(variance=V)
    for k, a in r.download_denoised().items():
        out["vden_" + k] = a
    r.temporal_reset()
    for f in range(3):
        r.render(W, H, 1, 2, depth, seed + f)
        r.render_features(W, H, 1, 2)
        r.denoise_temporal(fetch=4, variance=V)
        for k, a in dict(r.download_denoised(), **r.download_temporal()).items():
            out["chain%d_%s" % (f, k)] = a
    assert (out["chain2_len"] > 1).any() and (out["chain2_target"] != NO_TARGET).any()
    return out


def edit_against_upload(ctxs, s1, s2, W, H, spp, depth=50, forget=False):
    """Context B: upload S1, run everything once (tables, features, snapshot are there to be voided), edit to S2.  Context A: upload S2."""
    a, b = ctxs(), ctxs()
    b.upload(s1)
    b.set_noise_estimate(True)
    before = everything(b, W, H, None, 2, depth, 1, temporal=False)
    apply_edit(b, s1, s2, forget)
    a.upload(s2)
    a.set_noise_estimate(True)
    got, want = all_of(b, W, H, spp, depth), all_of(a, W, H, spp, depth)
    assert_same_everything(got, want, "edit against upload")
    return a, b, before, got


# ------------------------------------------------------------------------------------------------------------------ equivalence
@pytest.mark.parametrize("shape", list(SHAPES))
def test_recolour_only(ctxs, scenes, shape):
    W, H = SHAPES[shape]
    s1 = scenes.build_scene("cover", 1, W, H)
    m2, _ = recoloured(s1)
    a, b, before, got = edit_against_upload(ctxs, s1, edited(s1, materials=m2), W, H, 3)
    assert not np.array_equal(got["hdr"], one_shot(ctxs, s1, W, H, 3)[0])  # the edit shows
    assert got["launch"].case_words[4] & 8, "the recoloured cover scene still packs"


def packed_records_from_global_memory(monkeypatch):
    """RT_MATS16 is 0 by default and the small cover scene keeps its 48-byte records in LDS: the packed table is then never read.
    Under these two knobs every hit reads its material from global memory, the 16-byte record where the scene packs (mats16_mode 1)."""
    monkeypatch.setenv("RT_MATS16", "1")
    monkeypatch.setenv("RT_MATS_LDS", "0")


def test_recolour_reads_the_packed_table(ctxs, scenes, monkeypatch):
    packed_records_from_global_memory(monkeypatch)
    W, H = 70, 41
    s1 = scenes.build_scene("cover", 1, W, H)
    m2, _ = recoloured(s1)
    a, b, before, got = edit_against_upload(ctxs, s1, edited(s1, materials=m2), W, H, 3)
    assert before["launch"].plan_words[12] == 1 and got["launch"].plan_words[12] == 1  # mats16_mode: the edit's copy of mats16 is what is read


def test_recolour_three_spheres_depth_8(ctxs, scenes):
    W, H = 70, 41
    s1 = scenes.build_scene("three", 1, W, H)
    m2 = s1.materials.copy()
    m2["rgb0"][0] = [byte(200), byte(10), byte(90)]
    edit_against_upload(ctxs, s1, edited(s1, materials=m2), W, H, 2, depth=8)


def sky_of(sc, rgb, luminance):
    from cpuraytracer_amd import _capi
    sky = _capi.RtMaterial.from_buffer_copy(bytes(sc.sky))
    for c in range(3):
        sky.rgb0[c] = rgb[c]
    sky.luminance = luminance
    return sky


def excluded(r):
    from cpuraytracer_amd import _capi
    n = C.c_uint32(0)
    _capi.check(_capi.load().rt_unit_sky_excluded(r._h, C.byref(n)))
    return int(n.value)


def test_sky_colour_and_luminance(ctxs, scenes):
    """The sky is three launch parameters, a host record (the feature pass's miss albedo) and the constant sample of the empty-list
    tiles, which is rebuilt with the per-tile tables.  The small picture for everything; then 384 x 198 (1,188 full tiles: the tile
    order exists from 512 on), where the second render keeps the sky tiles out of the queue and adds the constant for them."""
    W, H = 96, 64
    s1 = scenes.build_scene("cover", 1, W, H)
    s2 = edited(s1, sky=sky_of(s1, (byte(250), byte(120), byte(30)), s1.sky.luminance * 0.5 + 1.0))
    a, b, before, got = edit_against_upload(ctxs, s1, s2, W, H, 2)
    assert not np.array_equal(before["feat_albedo"], got["feat_albedo"])  # the miss albedo moved
    W, H = 384, 198
    s1 = scenes.build_scene("cover", 1, W, H)
    s2 = edited(s1, sky=sky_of(s1, (byte(250), byte(120), byte(30)), s1.sky.luminance * 0.5 + 1.0))
    a, b = ctxs(), ctxs()
    b.upload(s1)
    b.render(W, H, 1, 3, 50, 2)
    b.synchronize()
    b.render(W, H, 1, 3, 50, 1)
    assert excluded(b) > 0  # the old sky's constant is in use
    old = b.download(ldr=False)[0]
    b.set_materials(s2.materials, s2.sky)
    a.upload(s2)
    shots = []
    for r in (b, a):
        r.render(W, H, 1, 3, 50, 2)  # another seed: the buffer it leaves holds other samples
        assert excluded(r) == 0, "the tables were just rebuilt: the count cannot be known to the first render"
        r.synchronize()
        st = r.render(W, H, 1, 3, 50, 1)
        n = excluded(r)
        r.resolve()
        shots.append((st, n) + r.download())
    (sb, nb, hb, lb), (sa, na, ha, la) = shots
    assert nb == na and nb > 0
    assert_same_bits(hb, ha, "second render after the sky edit: HDR")
    assert np.array_equal(lb, la) and (sb.traversals, sb.segments) == (sa.traversals, sa.segments)
    assert not np.array_equal(old, hb)


def test_type_changes_with_checker_textures(ctxs, scenes):
    """diffuse -> glass, metal -> diffuse, an emissive sphere's luminance; checker textures among them (the work order reads matType)."""
    W, H = 96, 64
    s1 = scenes.build_scene("cover", 1, W, H)
    m1 = s1.materials.copy()
    small = np.nonzero(s1.spheres["r"] < 100.0)[0]
    diffuse = [k for k in small if m1["type"][k] == DIFFUSE]
    metal = [k for k in small if m1["type"][k] == METAL]
    assert len(diffuse) > 8 and len(metal) > 4
    for k in diffuse[:4]:  # S1 already carries checkers and an emissive sphere, so both directions are edits
        m1["tex_type"][k], m1["tiling"][k], m1["rgb1"][k] = 1, 6.0, [byte(20), byte(220), byte(120)]
    m1["type"][diffuse[4]], m1["luminance"][diffuse[4]] = EMISSIVE, 4.0
    s1 = edited(s1, materials=m1)
    m2 = m1.copy()
    for k in diffuse[0:8:2]:
        m2["type"][k], m2["ior"][k], m2["smoothness"][k] = GLASS, 1.5, 1.0
    for k in metal[:4]:
        m2["type"][k] = DIFFUSE
    m2["tex_type"][metal[0]], m2["tiling"][metal[0]], m2["rgb1"][metal[0]] = 1, 3.0, [byte(0), byte(0), byte(255)]
    m2["tex_type"][0], m2["tiling"][0], m2["rgb1"][0] = 1 - m2["tex_type"][0], 2.0, [byte(40), byte(40), byte(40)]  # the floor
    m2["luminance"][diffuse[4]] = 9.0
    a, b, before, got = edit_against_upload(ctxs, s1, edited(s1, materials=m2), W, H, 3)
    assert not np.array_equal(before["hdr"], one_shot(ctxs, edited(s1, materials=m2), W, H, 2)[0])


@pytest.mark.parametrize("direction", ["packable-to-not", "not-to-packable"])
def test_an_edit_that_flips_mats16(ctxs, scenes, monkeypatch, direction):
    """A colour off the byte grid takes the 48-byte records; back on it, the packed ones.  The launch plan must see the flip: its
    case word 4 (bit 3: the scene packs) and the plan's mats16_mode are the upload's, and differ from the ones before the edit."""
    packed_records_from_global_memory(monkeypatch)
    W, H = 96, 64
    packed = scenes.build_scene("cover", 1, W, H)
    m = packed.materials.copy()
    k = int(np.nonzero((m["type"] == DIFFUSE) & (packed.spheres["r"] < 100.0))[0][0])
    m["rgb0"][k] = [0.123456, 0.5, 0.25]
    loose = edited(packed, materials=m)
    s1, s2 = (packed, loose) if direction == "packable-to-not" else (loose, packed)
    a, b, before, got = edit_against_upload(ctxs, s1, s2, W, H, 2)
    want_bit = 0 if direction == "packable-to-not" else 8
    assert before["launch"].case_words[4] & 8 == 8 - want_bit and got["launch"].case_words[4] & 8 == want_bit
    la = a.last_trace_launch()
    print("mats16_mode (plan word 12): before %d, after %d, upload %d" % (before["launch"].plan_words[12], got["launch"].plan_words[12], la.plan_words[12]))
    assert got["launch"].plan_words[12] != before["launch"].plan_words[12], "the reported variant did not change"
    assert got["launch"].plan_words[12] == (1 if want_bit else 0)
    assert got["kernel"] == tuple((f, getattr(la, f)) for f in la._fields if f in ("row", "lights") or f.startswith("k"))
    assert got["launch"].plan_words[12] == la.plan_words[12] and got["launch"].case_words[4] == la.case_words[4]


@pytest.mark.parametrize("mode", ["plain", "batch", "lookahead", "pipelining"])
def test_progressive_modes(ctxs, scenes, mode):
    W, H, depth, seed = 96, 64, 50, 1
    s1 = scenes.build_scene("cover", 1, W, H)
    m2, _ = recoloured(s1)
    s2 = edited(s1, materials=m2, exposure=s1.exposure_scale * 0.75)
    a, b = ctxs(), ctxs()

    def setting(r):
        if mode == "batch":
            r.set_frame_batch(8)
        elif mode == "lookahead":
            r.set_frame_lookahead(16)
        elif mode == "pipelining":
            r.set_frame_pipelining(4)
    b.upload(s1)
    setting(b)
    frames = 2 if mode == "lookahead" else 3
    for f in range(1, 1 + frames):
        b.render(W, H, f, f + 1, depth, seed, stats=False)
    apply_edit(b, s1, s2)
    code, msg = code_of(b.render, W, H, frames + 1, frames + 2, depth, seed, stats=False)
    assert code == RT_ERR_SEQUENCE, msg
    a.upload(s2)
    setting(a)
    pics = []
    for r in (b, a):
        for f in range(1, 9):
            r.render(W, H, f, f + 1, depth, seed, stats=False)
        r.synchronize()
        assert r.committed_samples() == 8
        r.resolve()
        pics.append(r.download())
    assert_same_bits(pics[0][0], pics[1][0], "%s: eight frames after the edit: HDR" % mode)
    assert np.array_equal(pics[0][1], pics[1][1])
    one = ctxs()  # ... and equal the one-shot render (no plane of the old materials was picked up)
    one.upload(s2)
    one.render(W, H, 1, 9, depth, seed)
    assert_same_bits(pics[0][0], one.download(ldr=False)[0], "%s: eight frames after the edit against one call" % mode)


def relit(oracle, lights):
    """Other colours and luminances, the directions bit for bit."""
    from cpuraytracer_amd import _capi
    out = []
    for k, l in enumerate(lights):
        n = _capi.RtLight.from_buffer_copy(bytes(l))
        n.color[0], n.color[1], n.color[2] = byte(255 - 60 * k), byte(90 + 50 * k), byte(30 + 100 * k)
        n.luminance = l.luminance * (0.5 + 0.4 * k)
        out.append(n)
    return out


@pytest.mark.parametrize("n_lights", [1, 3])
def test_lights_with_glossy_materials(ctxs, scenes, oracle, n_lights):
    """Light 0's radiance is a launch parameter; lights 1 and 2 keep theirs in their records in device memory, patched on the stream
    by rt_light_radiance_kernel.  Also against the oracle's render of S2."""
    W, H, spp = 96, 64, 3
    s1 = three_lights_glossy(scenes, oracle, W, H)
    s1.lights = s1.lights[:n_lights]
    s2 = edited(s1, lights=relit(oracle, s1.lights))
    a, b, before, got = edit_against_upload(ctxs, s1, s2, W, H, spp)
    assert bool(got["launch"].lights) == (n_lights > 1)
    assert not np.array_equal(before["hdr"], one_shot(ctxs, s2, W, H, 2)[0])
    orc = oracle.Oracle()
    orc.upload(s2)
    so = orc.render(W, H, 1, 1 + spp, 50, 1, threads=8)
    orc.resolve()
    ho, lo = orc.download()
    orc.close()
    assert_same_bits(got["hdr"], ho, "%d lights after set_lights: HDR against the oracle" % n_lights)
    assert np.array_equal(got["ldr"], lo)
    assert (int(got["stats"][1]), int(got["stats"][2])) == (so.traversals, so.segments)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_exposure(ctxs, scenes, shape):
    W, H = SHAPES[shape]
    s1 = scenes.build_scene("cover", 1, W, H)
    a, b, before, got = edit_against_upload(ctxs, s1, edited(s1, exposure=s1.exposure_scale * 2.5), W, H, 2)
    assert not np.array_equal(before["ldr"], one_shot(ctxs, edited(s1, exposure=s1.exposure_scale * 2.5), W, H, 2)[1])


# ------------------------------------------------------------------------------------------------------------------ void and keep
@pytest.mark.parametrize("what", ["materials", "sky", "lights", "exposure"])
def test_an_edit_voids_pictures_and_keeps_the_history(ctxs, scenes, what):
    W, H = 96, 64
    s1 = scenes.build_scene("cover", 1, W, H)
    r = ctxs()
    r.upload(s1)
    r.set_noise_estimate(True)
    everything(r, W, H, None, 2, 50, 1)  # (its temporal call leaves a history)
    r.download_features(), r.download_denoised()
    hist = r.download_temporal()
    if what == "materials":
        r.set_materials(recoloured(s1)[0], forget=False)
    elif what == "sky":
        r.set_materials(s1.materials, sky_of(s1, (byte(1), byte(2), byte(3)), 2.0), forget=False)
    elif what == "lights":
        r.set_lights(relit(None, [s1.sun]))
    else:
        r.set_exposure(s1.exposure_scale * 3.0)
    assert code_of(r.download_features)[0] == RT_ERR_SEQUENCE
    assert code_of(r.download_denoised)[0] == RT_ERR_SEQUENCE
    assert code_of(r.download)[0] == RT_ERR_SEQUENCE
    assert code_of(r.render, W, H, 3, 4, 50, 1)[0] == RT_ERR_SEQUENCE
    kept = r.download_temporal()  # the history is kept, every word of it
    assert_same_bits(kept["state"], hist["state"], "history state across the edit")
    assert np.array_equal(kept["len"], hist["len"]) and np.array_equal(kept["target"], hist["target"])
    r.render(W, H, 1, 3, 50, 2)
    r.render_features(W, H, 1, 3)
    r.denoise_temporal(fetch=4)
    assert (r.download_temporal()["len"] > 1).any()  # ... and the next temporal call blends with it


def test_the_same_records_change_nothing(ctxs, scenes):
    W, H = 96, 64
    s1 = scenes.build_scene("cover", 1, W, H)
    r = ctxs()
    r.upload(s1)
    r.set_noise_estimate(True)
    r.render(W, H, 1, 3, 50, 1)
    r.render_features(W, H, 1, 3)
    r.denoise()
    feat, den = r.download_features(), r.download_denoised()
    assert r.set_materials(s1.materials.copy(), s1.sky) == []
    r.set_lights([s1.sun])
    r.set_exposure(s1.exposure_scale)
    for k, a in r.download_features().items():  # still served
        assert np.array_equal(a.view(np.uint32), feat[k].view(np.uint32)), k
    for k, a in r.download_denoised().items():
        assert np.array_equal(a.view(np.uint8), den[k].view(np.uint8)), k
    r.render(W, H, 3, 5, 50, 1)  # continues
    r.resolve()
    want = one_shot(ctxs, s1, W, H, 4)
    assert_same_bits(r.download()[0], want[0], "continued across the same records: HDR")
    assert np.array_equal(r.download()[1], want[1])
    assert_same_bits(r.download_moments(), want[2], "continued across the same records: moments")
    r.set_frame_batch(8)  # a pending batch stays pending
    r.render(W, H, 5, 6, 50, 1, stats=False)
    r.set_materials(s1.materials, s1.sky), r.set_lights([s1.sun]), r.set_exposure(s1.exposure_scale)
    assert r.committed_samples() == 4
    r.synchronize()
    assert r.committed_samples() == 5


def test_refusals_come_before_any_side_effect(ctxs, scenes, oracle):
    from cpuraytracer_amd import _capi
    L = _capi.load()
    W, H = 96, 64
    s1 = three_lights_glossy(scenes, oracle, W, H)
    m2, _ = recoloured(s1)
    r = ctxs()
    assert code_of(r.set_lights, s1.lights)[0] == RT_ERR_NO_SCENE and code_of(r.set_exposure, 1.0)[0] == RT_ERR_NO_SCENE
    sky = _capi.RtMaterial.from_buffer_copy(bytes(s1.sky))
    assert L.rt_set_materials(r._h, m2.ctypes.data, m2.shape[0], C.byref(sky)) == RT_ERR_NO_SCENE
    r.upload(s1)
    r.set_noise_estimate(True)
    r.render(W, H, 1, 2, 50, 1)
    s = 2

    def mats(change):
        m = m2.copy()
        change(m)
        return m

    def light(k, change):
        ls = relit(oracle, s1.lights)
        change(ls[k])
        return ls

    def put(rec, field, k, v):
        getattr(rec, field)[k] = v
    nan, inf = float("nan"), float("inf")
    refused = [
        ("null materials", lambda: _capi.check(L.rt_set_materials(r._h, None, m2.shape[0], C.byref(sky))), "null"),
        ("null sky", lambda: _capi.check(L.rt_set_materials(r._h, m2.ctypes.data, m2.shape[0], None)), "null"),
        ("another count", lambda: r.set_materials(m2[:-1]), "records for a scene of"),
        ("type 4", lambda: r.set_materials(mats(lambda m: m["type"].__setitem__(7, 4))), "sphere 7"),
        ("NaN smoothness", lambda: r.set_materials(mats(lambda m: m["smoothness"].__setitem__(3, nan))), "sphere 3"),
        ("sky outside the domain", lambda: r.set_materials(m2, sky_of(s1, (nan, 0.0, 0.0), 1.0)), "the sky"),
        ("null lights", lambda: _capi.check(L.rt_set_lights(r._h, None, 3)), "null"),
        ("another light count", lambda: r.set_lights(s1.lights[:2]), "lights for a scene uploaded with 3"),
        ("a turned light", lambda: r.set_lights(light(1, lambda l: put(l, "direction", 0, l.direction[0] + 0.01))), "needs an rt_scene_upload"),
        ("a turned light 0", lambda: r.set_lights(light(0, lambda l: put(l, "direction", 2, -l.direction[2]))), "needs an rt_scene_upload"),
        ("NaN colour", lambda: r.set_lights(light(2, lambda l: put(l, "color", 1, nan))), "not finite"),
        ("infinite luminance", lambda: r.set_lights(light(0, lambda l: setattr(l, "luminance", inf))), "not finite"),
        ("NaN exposure", lambda: r.set_exposure(nan), "not finite"),
        ("infinite exposure", lambda: r.set_exposure(-inf), "not finite"),
    ]
    for what, call, text in refused:
        code, msg = code_of(call)
        assert code == RT_ERR_INVALID_ARG and text in msg, (what, code, msg)
        r.render(W, H, s, s + 1, 50, 1, stats=False)  # the running accumulation continues
        s += 1
    r.resolve()
    want = one_shot(ctxs, s1, W, H, s - 1)
    assert_same_bits(r.download()[0], want[0], "continued across the refusals: HDR")
    assert np.array_equal(r.download()[1], want[1])
    assert_same_bits(r.download_moments(), want[2], "continued across the refusals: moments")
    # forget's own: a null context, null ids with a count; and what it accepts without a history or a scene
    one = (C.c_uint32 * 1)(0)
    assert L.rt_temporal_forget(None, one, 1) == RT_ERR_INVALID_ARG and L.rt_temporal_forget(r._h, None, 1) == RT_ERR_INVALID_ARG
    assert L.rt_temporal_forget(r._h, None, 0) == 0 and L.rt_temporal_forget(r._h, one, 1) == 0
    bare = ctxs()
    assert L.rt_temporal_forget(bare._h, one, 1) == 0


# ------------------------------------------------------------------------------------------------------------------ asynchrony
TARGET_MS = 40.0  # as tests/test_streams.py: it only has to outlast a few host-side enqueues, and the query() assertion decides


def test_edits_queue_behind_running_work_without_a_host_wait(ctxs, scenes):
    """On a caller stream with a 40 ms delay queued: render under M1, set_materials(M2), set_materials(M3), render.  The first picture is
    M1's and the second M3's although every table copy was ordered while the M1 render had not started -- M2's staging is not
    overwritten by M3's (two sets in turn) -- and an event behind the delay is still pending when the edit calls have returned."""
    torch.cuda.init()
    torch.cuda.set_device(0)
    W, H, spp, depth = 96, 64, 2, 8
    s1 = scenes.build_scene("cover", 1, W, H)
    m1 = s1.materials
    m2, _ = recoloured(s1, every=2)
    m3 = m2.copy()
    k = int(np.nonzero((m3["type"] == DIFFUSE) & (s1.spheres["r"] < 100.0))[0][0])
    m3["rgb0"][k] = [0.123456, 0.5, 0.25]  # M3 does not pack: mats16Ok flips under queued work as well
    m3["type"][np.nonzero(m3["type"] == METAL)[0][:3]] = GLASS
    m3["ior"][m3["type"] == GLASS] = 1.5
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):  # one timed delay gives the cycles of 40 ms
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(1000)
        e0.record(stream)
        torch.cuda._sleep(10**6)
        e1.record(stream)
    e1.synchronize()
    cycles = int(1e6 / e0.elapsed_time(e1) * TARGET_MS)
    first = torch.empty((H, W, 3), dtype=torch.float32, device="cuda:0")
    r = ctxs()
    r.set_stream(stream.cuda_stream)
    r.upload(s1)
    r.render(W, H, 1, 1 + spp, depth, 1, stats=False)  # (everything a first launch loads, before the delay)
    r.synchronize()
    behind = torch.cuda.Event()
    with torch.cuda.stream(stream):
        torch.cuda._sleep(cycles)
        behind.record(stream)
    r.render(W, H, 1, 1 + spp, depth, 1, stats=False)
    r.copy_to_device(dev_hdr_ptr=first.data_ptr())
    r.set_materials(m2, forget=False)
    r.set_materials(m3, forget=False)
    assert not behind.query(), "the delay had ended when the edit calls had returned: nothing was shown to be asynchronous"
    r.render(W, H, 1, 1 + spp, depth, 1, stats=False)
    r.synchronize()
    second = r.download(ldr=False)[0]
    want1 = one_shot(ctxs, s1, W, H, spp, depth)[0]
    want3 = one_shot(ctxs, edited(s1, materials=m3), W, H, spp, depth)[0]
    assert_same_bits(first.cpu().numpy(), want1, "the render queued before the edits: M1's picture")
    assert_same_bits(second, want3, "the render after the two edits: M3's picture")
    assert not np.array_equal(want1, want3) and not np.array_equal(one_shot(ctxs, edited(s1, materials=m2), W, H, spp, depth)[0], want3)
    assert m1 is s1.materials


# ------------------------------------------------------------------------------------------------------------------ forget
def strips(r):
    hdr, _ = r.download(ldr=False)
    d = r.download_features()
    feat = np.concatenate([d["albedo"], d["normal"], d["depth"][..., None], d["coverage"][..., None]], axis=-1)
    return hdr, r.download_moments(), np.ascontiguousarray(feat), d["id"]


def frame(r, W, H, seed, spp=2):
    r.render(W, H, 1, 1 + spp, 50, seed)
    r.render_features(W, H, 1, 1 + spp)
    return strips(r)


def twin_step(S, Q, feat, ids, W, H, cam, hist, fetch, T):
    from cpuraytracer_amd import _capi
    return _capi.unit_temporal_host(S, Q, 2, feat, 2, ids, W, H, cam, history=hist, params=_capi.denoise_params(**DEFAULTS),
                                    tparams=_capi.temporal_params(**dict(TDEFAULTS, **T)), fetch=fetch)


@pytest.mark.parametrize("fetch", [1, 4])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_forget_empties_the_named_pixels_and_nothing_else(ctxs, scenes, shape, fetch):
    """Two temporal frames from one camera; forget a large sphere, then the sky.  len equals the twin's, the rest of the history is
    untouched, and the next temporal call -- the device's against the host twin's on the twin-forgotten history -- treats the named
    pixels as pixels with no history."""
    from cpuraytracer_amd import _capi
    W, H = SHAPES[shape]
    T = dict(max_history=8)
    tp = _capi.temporal_params(**dict(TDEFAULTS, **T))
    sc = scenes.build_scene("cover", 1, W, H)
    r = ctxs()
    r.upload(sc)
    r.set_noise_estimate(True)
    hist = None
    for f in range(2):
        S, Q, feat, ids = frame(r, W, H, 1 + f)
        r.denoise_temporal(None, tp, fetch=fetch)
        hist = history_of(twin_step(S, Q, feat, ids, W, H, sc.camera, hist, fetch, T))
    before = r.download_temporal()
    assert np.array_equal(before["len"], hist["len"]) and (before["len"] == 2).any()
    counts = np.bincount(ids[ids != SKY].ravel(), minlength=sc.n)
    counts[0] = 0  # (not the floor)
    big = int(np.argmax(counts))
    assert counts[big] >= 16 and (ids == SKY).sum() >= 16
    for forget in ([big], [SKY, sc.n, sc.n + 77]):  # (ids at or above the count are accepted and match nothing)
        r.temporal_forget(forget)
        hist["len"] = _capi.unit_temporal_forget_host(hist["len"], hist["ids"], sc.n, forget)
        after = r.download_temporal()
        assert np.array_equal(after["len"], hist["len"])
        assert_same_bits(after["state"], before["state"], "state after forget")
        assert np.array_equal(after["target"], before["target"])
    named = (ids == big) | (ids == SKY)
    assert np.array_equal(hist["len"] == 0, named | (before["len"] == 0)) and np.array_equal(hist["len"][~named], before["len"][~named])
    r.temporal_forget([])  # nothing
    assert np.array_equal(r.download_temporal()["len"], hist["len"])
    # the next temporal call: the same camera, so every pixel reprojects onto itself, and only the named ones are rejected
    S, Q, feat, ids3 = frame(r, W, H, 3)
    r.denoise_temporal(None, tp, fetch=fetch)
    got = dict(r.download_denoised(), **r.download_temporal())
    want = twin_step(S, Q, feat, ids3, W, H, sc.camera, hist, fetch, T)
    assert_same_bits(got["state"], want["state"], "after forget: state")
    assert np.array_equal(got["len"], want["len"]) and np.array_equal(got["target"], want["target"])
    assert_same_bits(got["rgb"], want["rgb"], "after forget: den")
    assert_same_bits(got["var"], want["var"], "after forget: den_var")
    assert np.array_equal(ids3, ids)
    assert (got["len"][named] == 1).all() and (got["target"][named] == NO_TARGET).all()
    own = twin_step(S, Q, feat, ids3, W, H, sc.camera, None, fetch, T)["state"]  # the frame's own prepared (c, v)
    assert np.array_equal(got["state"][named].view(np.uint32), own[named].view(np.uint32))
    inner = ~named
    assert (got["len"][inner] >= 2).any() and (got["target"][inner] != NO_TARGET).any()


def test_forget_takes_more_ids_than_travel_by_value(ctxs, scenes):
    """More than 16 ids go through the table form: the device against the twin, and against forgetting the same ids one by one."""
    from cpuraytracer_amd import _capi
    W, H = 96, 64
    sc = scenes.build_scene("cover", 1, W, H)
    a, b = ctxs(), ctxs()
    lens = []
    many = [int(k) for k in range(1, sc.n, 3)] + [SKY, sc.n + 5]
    assert len(many) > 100
    for r, chunks in ((a, [many]), (b, [many[i:i + 7] for i in range(0, len(many), 7)])):
        r.upload(sc)
        r.set_noise_estimate(True)
        ids = frame(r, W, H, 1)[3]
        r.denoise_temporal()
        for c in chunks:
            r.temporal_forget(c)
        lens.append(r.download_temporal()["len"])
    want = _capi.unit_temporal_forget_host(np.ones((H, W), np.uint32), ids, sc.n, many)
    assert np.array_equal(lens[0], want) and np.array_equal(lens[1], want)
    assert (want == 0).any() and (want == 1).any()


def test_set_materials_forgets_exactly_the_changed_spheres(ctxs, scenes):
    W, H = 96, 64
    sc = scenes.build_scene("cover", 1, W, H)
    m2, picked = recoloured(sc, every=5)
    r = ctxs()
    r.upload(sc)
    r.set_noise_estimate(True)
    ids = frame(r, W, H, 1)[3]
    r.denoise_temporal()
    assert r.set_materials(m2) == picked
    ln = r.download_temporal()["len"]
    assert np.array_equal(ln == 0, np.isin(ids, picked)) and (ln == 0).any()
    assert r.set_materials(m2, sky_of(sc, (byte(9), byte(9), byte(9)), 1.0)) == [SKY]
    ln = r.download_temporal()["len"]
    assert np.array_equal(ln == 0, np.isin(ids, picked + [SKY]))
    assert r.set_materials(sc.materials, forget=False) == []
    assert np.array_equal(r.download_temporal()["len"], ln)
