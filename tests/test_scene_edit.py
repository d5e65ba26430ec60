"""The edits' one copier on the device (csrc/rt_capi.hip StageCopy over host/rt_scene_edit.h's plans): edits of different kinds -- the
material tables, the shadow indices' tables, the forget table -- queued back to back take the two pinned staging slots in turn, each
with tables of another size.  Context B queues them without a synchronise in between; context A gets the same final scene by an upload,
or makes the same calls with a synchronise after each.  Everything handed out is compared bit for bit."""
import numpy as np
import pytest
import torch  # noqa: F401  before the library is loaded, as in tests/test_streams.py

from test_light_turn import TURNS, light_of, lights_bytes, same_launch
from test_noise_estimate_cpu import assert_same_bits
from test_set_camera import cam_bytes, turned, with_camera
from test_shading_edit import SKY, byte, edited, frame, lights_of, sky_of

pytestmark = pytest.mark.gpu

SPP, DEPTH, SEED = 2, 8, 1
GLASS = 2


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


def recolour(sc, salt):
    """Another byte colour for every sphere that has a colour (the table still packs into 16 bytes)."""
    m = sc.materials.copy()
    pick = np.nonzero(m["type"] != GLASS)[0]
    assert pick.size > 0
    for k in pick:
        m["rgb0"][k] = [byte((37 * k + 11 * salt) % 256), byte((91 * k + 5 + salt) % 256), byte((53 * k + 200 * salt) % 256)]
    return m


def relit(light, k):
    return light_of(light, color=(byte(255 - 60 * k), byte(90 + 50 * k), byte(30 + 100 * k)), luminance=light.luminance * (0.5 + 0.4 * k))


def picture(r, W, H):
    """One accumulation with statistics and the launcher's account of it, its resolve and the moments."""
    out = {}
    st = r.render(W, H, 1, 1 + SPP, DEPTH, SEED)
    out["stats"] = (st.samples, st.traversals, st.segments, st.local_rows, st.passes)
    launch = r.last_trace_launch()
    out["launch"] = launch
    out["kernel"] = tuple((f, getattr(launch, f)) for f in launch._fields if f in ("row", "lights") or f.startswith("k"))
    out["far_state"] = r.last_trace_far_state()
    r.resolve()
    out["hdr"], out["ldr"] = r.download()
    out["sq"] = r.download_moments()
    return out


@pytest.mark.parametrize("name,W,H", [("three", 64, 32), ("cover", 96, 64)])
def test_queued_edits_of_every_kind_against_an_upload(ctxs, scenes, name, W, H):
    s1 = scenes.build_scene(name, 1, W, H)
    sun = lights_of(s1)[0]
    m2, m3 = recolour(s1, 1), recolour(s1, 2)
    assert not np.array_equal(m2["rgb0"], s1.materials["rgb0"]) and not np.array_equal(m3["rgb0"], m2["rgb0"])
    sky2 = sky_of(s1, (byte(40), byte(90), byte(200)), 0.75)
    reshaped = light_of(sun, TURNS["reshaping"])
    recoloured = relit(reshaped, 1)
    last = light_of(recoloured, TURNS["x-dominant"])
    exposure2 = 0.5 * s1.exposure_scale
    cam2 = turned(scenes, s1.camera, 5.0)
    final = with_camera(edited(s1, materials=m3, sky=sky2, lights=[last], exposure=exposure2), cam2)
    assert bytes(sky2) != bytes(s1.sky) and lights_bytes([last]) != lights_bytes([sun]) and cam_bytes(cam2) != cam_bytes(s1.camera)

    a, b = ctxs(), ctxs()
    b.upload(s1)
    b.set_noise_estimate(True)
    first = picture(b, W, H)
    # seven edits, nothing synchronised in between: the material tables and the indices' tables take the two slots in turn
    b.set_materials(m2, sky2, forget=False)
    b.turn_lights([reshaped], forget=False)
    b.set_lights([recoloured])
    b.set_exposure(exposure2)
    b.set_camera(cam2)
    b.set_materials(m3, sky2, forget=False)
    b.turn_lights([last], forget=False)
    got = picture(b, W, H)

    a.upload(final)
    a.set_noise_estimate(True)
    want = picture(a, W, H)
    what = "%s: seven queued edits against the upload" % name
    assert_same_bits(got["hdr"], want["hdr"], what + ": HDR")
    assert np.array_equal(got["ldr"], want["ldr"]), what + ": LDR"
    assert_same_bits(got["sq"], want["sq"], what + ": moments")
    assert got["stats"] == want["stats"], what
    same_launch(got, want, what)
    assert cam_bytes(b.get_camera()) == cam_bytes(cam2) == cam_bytes(a.get_camera())
    assert lights_bytes(b.get_lights()) == lights_bytes([last]) == lights_bytes(a.get_lights())
    assert not np.array_equal(got["hdr"], first["hdr"])  # the edits show


def test_a_forget_table_between_two_edits_that_stage(ctxs, scenes):
    """The history case: two temporal frames, then set_materials -- rt_temporal_forget with more ids than travel by value (the table
    form, which takes a slot) -- turn_lights, then one more temporal frame.  A synchronises after every call, B after none."""
    W, H = 96, 64
    sc = scenes.build_scene("cover", 1, W, H)
    m2 = recolour(sc, 1)
    many = [int(k) for k in range(1, sc.n, 3)] + [SKY]
    assert len(many) > 100  # (kForgetInlineIds is 16)
    lights2 = [light_of(lights_of(sc)[0], TURNS["reshaping"])]
    results = []
    for r, settle in ((ctxs(), True), (ctxs(), False)):
        def done():
            if settle:
                r.synchronize()
        r.upload(sc)
        r.set_noise_estimate(True)
        for f in range(2):
            ids = frame(r, W, H, 1 + f)[3]
            r.denoise_temporal(fetch=4)
        done()
        r.set_materials(m2, forget=False)
        done()
        r.temporal_forget(many)
        done()
        r.turn_lights(lights2, forget=False)
        done()
        r.render(W, H, 1, 1 + SPP, 50, 3, stats=False)
        done()
        r.render_features(W, H, 1, 1 + SPP)
        done()
        r.denoise_temporal(fetch=4)
        done()
        results.append((dict(r.download_denoised(), **r.download_temporal()), ids))
    (want, ids), (got, _) = results
    assert set(got) == set(want)
    for k in want:
        if want[k].dtype.kind == "f":
            assert_same_bits(got[k], want[k], "queued against settled: " + k)
        else:
            assert np.array_equal(got[k], want[k]), k
    # the forget took effect and the history behind it did not vanish: forgotten pixels start over, others blend on
    named = np.isin(ids, many)
    assert named.any() and (~named).any() and (want["len"][named] == 1).all() and (want["len"] > 1).any()
