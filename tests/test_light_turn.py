"""rt_turn_lights and rt_get_lights on the device: the lights turn without a scene upload.  The core comparison is the one of
tests/test_shading_edit.py: context B uploads scene S1, renders everything once and turns its lights to S2's; context A uploads S2.
From there both run the same calls (`all_of`) and everything they hand out is compared bit for bit -- with the launcher's own account
of the variant and the LDS image (rt_unit_last_trace_launch), which follow the index's size, and rt_unit_last_trace_far_state."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch  # before the library is loaded, as in tests/test_streams.py: a torch stream's handle is then a stream of the library's runtime

import far_shadow_cases as fsc
import trace_variant_cases as tvc
from test_noise_estimate_cpu import assert_same_bits
from test_set_camera import assert_same_everything, code_of, everything, one_shot, three_lights_glossy
from test_shading_edit import all_of, lights_of

pytestmark = pytest.mark.gpu

RT_ERR_INVALID_ARG, RT_ERR_NO_SCENE, RT_ERR_SEQUENCE = 2, 3, 6
F = np.float32
# plan words that follow the flagged tiles' count, which arrives when it arrives (tests/test_set_camera.py assert_same_everything):
# blocks, queue_block, static_blocks, dyn_begin, dyn_blocks
PLAN_WORDS_OF_THE_COUNT = (2, 21, 22, 23, 24)


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


def light_of(light, direction=None, color=None, luminance=None, length=1.0):
    """A copy of the record; direction: normalised in binary64, scaled to `length`, rounded once."""
    from cpuraytracer_amd import _capi
    out = _capi.RtLight.from_buffer_copy(bytes(light))
    if direction is not None:
        d = np.asarray(direction, dtype=np.float64)
        d = d / np.sqrt(np.dot(d, d)) * length
        for c in range(3):
            out.direction[c] = F(d[c])
    if color is not None:
        for c in range(3):
            out.color[c] = F(color[c])
    if luminance is not None:
        out.luminance = F(luminance)
    return out


def with_lights(sc, lights):
    out = copy.copy(sc)
    out.lights = list(lights)
    out.sun = out.lights[0]
    return out


def direction_of(light):
    return np.array([light.direction[0], light.direction[1], light.direction[2]], dtype=np.float64)


def index_of(sc, tier=1):
    """Light 0's index as the host builds it under the environment of the moment (no device): enabled, nx, ny, entries."""
    probe = with_lights(sc, lights_of(sc))
    return fsc.host_index_tier(probe, tier)


def same_launch(got, want, what):
    """The launcher's account of the first trace launch of `everything`: the packed case (the scene's shape with the index's sizes
    among it) and the plan (LDS image, variant) but the words that follow the flagged tiles' count."""
    a, b = got["launch"], want["launch"]
    assert np.array_equal(a.case_words, b.case_words), "%s: case words %s != %s" % (what, a.case_words, b.case_words)
    keep = [k for k in range(28) if k not in PLAN_WORDS_OF_THE_COUNT]
    assert np.array_equal(a.plan_words[keep], b.plan_words[keep]), "%s: plan words %s != %s" % (what, a.plan_words, b.plan_words)
    assert got["kernel"] == want["kernel"] and got["far_state"] == want["far_state"], what


def lights_bytes(ls):
    return [bytes(l) for l in ls]


def turn_against_upload(ctxs, s1, s2, W, H, spp, depth=50, what="turn against upload"):
    """Context B: upload S1, run everything once (tables, features, snapshot are there to be voided), turn to S2.  Context A: upload S2."""
    a, b = ctxs(), ctxs()
    b.upload(s1)
    b.set_noise_estimate(True)
    before = everything(b, W, H, None, 2, depth, 1, temporal=False)
    b.turn_lights(lights_of(s2), forget=False)
    a.upload(s2)
    a.set_noise_estimate(True)
    got, want = all_of(b, W, H, spp, depth), all_of(a, W, H, spp, depth)
    assert_same_everything(got, want, what)
    same_launch(got, want, what)
    assert lights_bytes(b.get_lights()) == lights_bytes(lights_of(s2)) == lights_bytes(a.get_lights())
    return a, b, before, got


# ------------------------------------------------------------------------------------------------------------------ equivalence
# The turns of every scene, as directions of light 0.  None: half a degree about the vertical from SMALL_FROM -- the scenes' own sun,
# (1, 1, 1) / sqrt 3, sits on the builder's basis switch (|Lx| against |Ly| and |Lz|), where the smallest turn reshapes the grid.
TURNS = {"small": None, "reshaping": (0.15, 0.35, -0.9), "down": (0.0, 1.0, 0.0), "grazing": (1.0, 0.05, 0.0), "x-dominant": (0.9, 0.3, 0.25)}
SMALL_FROM = (-0.2, 0.9, 0.4)


def turn_pair(scenes, sc, turn):
    """The uploaded scene and the turned one."""
    sun = lights_of(sc)[0]
    if TURNS[turn] is None:
        s1 = with_lights(sc, [light_of(sun, SMALL_FROM)] + lights_of(sc)[1:])
        return s1, with_lights(sc, [scenes.turn_light(lights_of(s1)[0], 0.5)] + lights_of(sc)[1:])
    return sc, with_lights(sc, [light_of(sun, TURNS[turn])] + lights_of(sc)[1:])


def turned_scene(scenes, s1, turn):
    return turn_pair(scenes, s1, turn)[1]


def check_the_turn_is_the_turn(s1, s2, turn):
    """On the CPU: the small turn leaves the grid's shape alone, the reshaping one changes nx, ny and the entry count, the x-dominant
    one switches the basis where the uploaded light did not."""
    d1, d2 = direction_of(lights_of(s1)[0]), direction_of(lights_of(s2)[0])
    assert not np.array_equal(d1, d2)
    g1, g2 = index_of(s1), index_of(s2)
    assert g1.enabled and g2.enabled
    if turn == "small":
        assert (g1.nx, g1.ny) == (g2.nx, g2.ny)
    if turn == "reshaping":  # (an index in global memory may sit at the limit of 256 cells along one axis before and after)
        assert (g1.nx != g2.nx or g1.ny != g2.ny) and len(g1.cell_start) != len(g2.cell_start) and len(g1.entries) != len(g2.entries), \
            (g1.nx, g1.ny, len(g1.entries), g2.nx, g2.ny, len(g2.entries))
    if turn == "x-dominant":
        assert not (abs(d1[0]) > abs(d1[1]) and abs(d1[0]) > abs(d1[2])) and abs(d2[0]) > abs(d2[1]) and abs(d2[0]) > abs(d2[2])
    return g2


@pytest.mark.parametrize("turn,shape", [(t, "96x64") for t in TURNS] + [("reshaping", "70x41"), ("grazing", "70x41")])
def test_cover_flat_scan_index_in_lds_and_far_tier(ctxs, scenes, turn, shape):
    W, H = {"96x64": (96, 64), "70x41": (70, 41)}[shape]
    s1, s2 = turn_pair(scenes, scenes.build_scene("cover", 1, W, H), turn)
    g2 = check_the_turn_is_the_turn(s1, s2, turn)
    assert not g2.in_global_memory and index_of(s2, 2).enabled  # the index staged into LDS, and the far tier
    a, b, before, got = turn_against_upload(ctxs, s1, s2, W, H, 3, what="cover, " + turn)
    assert got["launch"].kScan == 1 and got["launch"].kLds
    assert not np.array_equal(got["hdr"], one_shot(ctxs, s1, W, H, 3)[0])  # the turn shows


@pytest.mark.parametrize("turn", list(TURNS))
@pytest.mark.parametrize("grid", ["cells", "hierarchy"])
def test_grid10k_index_in_global_memory(ctxs, scenes, monkeypatch, grid, turn):
    """Recipe rows 6 and 14 of trace_variant_cases: grid10k as it is (the cell grid) and under RT_GRID=0 (the hierarchy)."""
    if grid == "hierarchy":
        monkeypatch.setenv("RT_GRID", "0")
    else:
        monkeypatch.delenv("RT_GRID", raising=False)
    W, H = 70, 41
    s1, s2 = turn_pair(scenes, tvc.build_scene("grid10k", W, H), turn)
    if grid == "cells":  # (on the CPU the hierarchy of 10,004 spheres takes seconds to build, and the index's shape is the same under both)
        assert check_the_turn_is_the_turn(s1, s2, turn).in_global_memory
    a, b, before, got = turn_against_upload(ctxs, s1, s2, W, H, 2, what="grid10k %s, %s" % (grid, turn))
    assert got["launch"].kScan == (3 if grid == "cells" else 2)


def test_index_off_and_on(ctxs, scenes):
    """A direction of length 3 is no direction: no index, no far tier, shadow rays on the scan -- and back.  Both states equal the
    uploading contexts', the variant row included; the far-tier record disappears and reappears."""
    W, H = 96, 64
    s_on = scenes.build_scene("cover", 1, W, H)
    sun = lights_of(s_on)[0]
    s_off = with_lights(s_on, [light_of(sun, direction_of(sun), length=3.0)])
    s_back = with_lights(s_on, [light_of(sun, (0.3, 0.8, 0.5))])
    assert index_of(s_on).enabled and not index_of(s_off).enabled and not index_of(s_off, 2).enabled and index_of(s_back, 2).enabled
    a, b, before, off = turn_against_upload(ctxs, s_on, s_off, W, H, 2, what="index off")
    # the launch plan saw the index go: the packed case (index on, its sizes) and the LDS image differ from the ones before the turn
    assert before["launch"].case_words.tolist() != off["launch"].case_words.tolist()
    assert before["launch"].plan_words.tolist() != off["launch"].plan_words.tolist()
    b.turn_lights(lights_of(s_back), forget=False)
    c = ctxs()
    c.upload(s_back)
    c.set_noise_estimate(True)
    got, want = all_of(b, W, H, 2, 50), all_of(c, W, H, 2, 50)
    assert_same_everything(got, want, "index on again")
    same_launch(got, want, "index on again")
    assert got["launch"].row == before["launch"].row and got["launch"].case_words.tolist() != off["launch"].case_words.tolist()
    # ... and a context whose index was off AT THE UPLOAD has the buffers all the same
    d = ctxs()
    d.upload(s_off)
    d.set_noise_estimate(True)
    d.render(W, H, 1, 3, 50, 1)
    d.turn_lights(lights_of(s_back), forget=False)
    got = all_of(d, W, H, 2, 50)
    assert_same_everything(got, want, "index switched on after an upload without it")
    same_launch(got, want, "index switched on after an upload without it")


def row_of_spheres(sc):
    """The cover scene's small spheres in one row along x on the ground.  Lit from above the row's footprints span 217 units, the 64
    cells allowed are 3.4 wide and a footprint lies in one or two of them; lit almost along the row they span 25 units, the cells are
    a footprint wide and each footprint lies in four."""
    out = copy.copy(sc)
    sp = sc.spheres.copy()
    small = np.nonzero(np.abs(sp["r"]) < 0.3)[0]
    assert small.size > 400
    for q, k in enumerate(small):
        sp["cx"][k], sp["cy"][k], sp["cz"][k] = (q - small.size / 2) * 0.45, 0.2, 0.0
    out.spheres = sp
    return out


def test_a_larger_index_than_the_uploaded_one(ctxs, scenes):
    """Upload with the direction whose index is the smallest of the set, turn to the one whose index is the largest: the room is the
    reservation's, not the uploaded index's.  (The far tier goes the other way: on at the upload, off after the turn.)"""
    W, H = 96, 64
    s0 = row_of_spheres(scenes.build_scene("cover", 1, W, H))
    sun = lights_of(s0)[0]
    cands = [with_lights(s0, [light_of(sun, d)]) for d in [(0.0, 1.0, 0.3), (0.3, 0.8, 0.5), (1.0, 0.1, 0.05), (0.9, 0.3, 0.25)]]
    entries = [len(index_of(s).entries) for s in cands]
    print("entries per direction:", entries)
    assert all(index_of(s).enabled for s in cands)
    small, large = cands[int(np.argmin(entries))], cands[int(np.argmax(entries))]
    assert max(entries) >= 1.5 * min(entries), entries
    a, b, before, got = turn_against_upload(ctxs, small, large, W, H, 2, what="a larger index")
    assert before["launch"].case_words.tolist() != got["launch"].case_words.tolist()  # the launch plan saw the other size


# ------------------------------------------------------------------------------------------------------------------ light lists
def relit(l, k):
    return light_of(l, color=(F(255 - 60 * k) / F(255), F(90 + 50 * k) / F(255), F(30 + 100 * k) / F(255)), luminance=l.luminance * (0.5 + 0.4 * k))


OTHER_DIRECTIONS = [(0.4, 0.6, -0.7), (0.8, 0.5, 0.1), (-0.3, 0.9, -0.2)]


@pytest.mark.parametrize("case", ["light 0 only", "a light >= 1 only", "all together", "colour and direction in the same call"])
@pytest.mark.parametrize("n_lights", [2, 3])
def test_light_lists_with_glossy_materials(ctxs, scenes, oracle, n_lights, case):
    """Light 0 is launch parameters and its tables; lights 1 .. keep direction, radiance and index in their records in device memory,
    rewritten on the stream by rt_light_index_kernel.  (With that launch left out, "a light >= 1 only" fails: docs/EXPERIMENTS.md.)"""
    W, H, spp = 96, 64, 2
    s1 = three_lights_glossy(scenes, oracle, W, H)
    s1.lights = s1.lights[:n_lights]
    new = list(s1.lights)
    which = {"light 0 only": [0], "a light >= 1 only": [n_lights - 1]}.get(case, list(range(n_lights)))
    for k in which:
        new[k] = light_of(new[k], OTHER_DIRECTIONS[k])
        if case == "colour and direction in the same call":
            new[k] = relit(new[k], k)
    s2 = with_lights(s1, new)
    a, b, before, got = turn_against_upload(ctxs, s1, s2, W, H, spp, what="%d lights, %s" % (n_lights, case))
    assert got["launch"].lights
    assert not np.array_equal(got["hdr"], one_shot(ctxs, s1, W, H, spp)[0])


def test_three_lights_against_the_oracle(ctxs, scenes, oracle):
    W, H, spp = 70, 41, 2
    s1 = three_lights_glossy(scenes, oracle, W, H)
    s2 = with_lights(s1, [relit(light_of(l, OTHER_DIRECTIONS[k]), k) for k, l in enumerate(s1.lights)])
    r = ctxs()
    r.upload(s1)
    r.render(W, H, 1, 2, 50, 1)
    r.turn_lights(s2.lights)
    st = r.render(W, H, 1, 1 + spp, 50, 1)
    r.resolve()
    hg, lg = r.download()
    orc = oracle.Oracle()
    orc.upload(s2)
    so = orc.render(W, H, 1, 1 + spp, 50, 1, threads=8)
    orc.resolve()
    ho, lo = orc.download()
    orc.close()
    assert_same_bits(hg, ho, "three turned lights: HDR against the oracle")
    assert np.array_equal(lg, lo) and (st.traversals, st.segments) == (so.traversals, so.segments)


# ------------------------------------------------------------------------------------------------------------------ unit entries
def query_points(sc, rng, m=600):
    """Points near the field, points on the ground out to beyond the far tier's radius, and points above it."""
    g1, g2 = index_of(sc), index_of(sc, 2)
    P0, P2 = float(np.sqrt(g1.p0sq)), float(np.sqrt(g2.p0sq)) if g2.enabled else 4.0 * float(np.sqrt(g1.p0sq))
    near = rng.uniform(-12, 12, (m, 3)) * np.array([1.0, 0.1, 1.0]) + np.array([0.0, 0.6, 0.0])
    rad, th = rng.uniform(0.5 * P0, 1.3 * P2, m), rng.uniform(0, 2 * np.pi, m)
    R = fsc.FLOOR_R
    ground = np.stack([rad * np.cos(th), np.sqrt(np.maximum(R * R - rad * rad, 0.0)) - R, rad * np.sin(th)], 1)
    return np.concatenate([near, ground, ground + np.array([0.0, 0.3, 0.0])]).astype(F)


def test_unit_entries_after_a_turn(ctxs, scenes, oracle):
    W, H = 96, 64
    s1 = three_lights_glossy(scenes, oracle, W, H)
    s2 = with_lights(s1, [light_of(l, OTHER_DIRECTIONS[k]) for k, l in enumerate(s1.lights)])
    a, b = ctxs(), ctxs()
    b.upload(s1)
    b.render(W, H, 1, 2, 50, 1)
    pts = query_points(s2, np.random.default_rng(11))
    old = b.unit_shadow(0, pts)
    b.turn_lights(s2.lights)
    a.upload(s2)
    for light in range(3):
        for lds in (False, True):
            got, want = b.unit_shadow(light, pts, glob_in_lds=lds), a.unit_shadow(light, pts, glob_in_lds=lds)
            assert np.array_equal(got, want), (light, lds)
            assert (want & 1).any() and not (want & 1).all() and (want & 2).any() and not (want & 2).all()
    got, want = b.unit_shadow_tier(2, pts), a.unit_shadow_tier(2, pts)
    assert np.array_equal(got, want) and (want & 4).any() and (want & 2).any() and ((want & 6) == 0).any()
    probe = with_lights(s2, s2.lights)
    assert np.array_equal(want, fsc.host_query_tier(probe, 2, pts))  # ... and the host twin over a fresh preparation
    assert not np.array_equal(old, b.unit_shadow(0, pts))


# ------------------------------------------------------------------------------------------------------------------ progressive modes
@pytest.mark.parametrize("mode", ["plain", "batch", "lookahead", "pipelining"])
def test_progressive_modes(ctxs, scenes, mode):
    W, H, depth, seed = 96, 64, 50, 1
    s1 = scenes.build_scene("cover", 1, W, H)
    s2 = turned_scene(scenes, s1, "reshaping")
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
    before = b.committed_samples()
    b.turn_lights(lights_of(s2))
    if mode == "batch":
        assert before == 0 and b.committed_samples() == 0  # the pending batch was rendered under the old lights, then voided with them
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
    assert_same_bits(pics[0][0], pics[1][0], "%s: eight frames after the turn: HDR" % mode)
    assert np.array_equal(pics[0][1], pics[1][1])
    assert_same_bits(pics[0][0], one_shot(ctxs, s2, W, H, 8)[0], "%s: eight frames after the turn against one call" % mode)


def test_a_pending_batch_is_rendered_under_the_old_lights(ctxs, scenes):
    """The batch was asked of the old lights: the turn renders it first (one more trace launch, the samples committed) and then voids
    the picture with everything else."""
    W, H = 96, 64
    s1 = scenes.build_scene("cover", 1, W, H)
    s2 = turned_scene(scenes, s1, "down")
    r = ctxs()
    r.upload(s1)
    r.render(W, H, 1, 3, 50, 1, stats=False)
    r.set_frame_batch(8)
    r.render(W, H, 3, 4, 50, 1, stats=False)  # pending
    r.render(W, H, 4, 5, 50, 1, stats=False)
    launches = r.trace_launches()
    assert r.committed_samples() == 2
    r.turn_lights(lights_of(s2))
    assert r.trace_launches() == launches + 1  # the two pending planes, in one launch, under the old lights
    assert code_of(r.render, W, H, 5, 6, 50, 1, stats=False)[0] == RT_ERR_SEQUENCE
    r.set_frame_batch(1)
    assert_same_bits(one_shot_of(r, W, H, 3), one_shot(ctxs, s2, W, H, 3)[0], "after the settled batch and the turn: S2's picture")


# ------------------------------------------------------------------------------------------------------------------ void and keep
@pytest.mark.parametrize("forget", [False, True])
def test_a_turn_voids_pictures_and_keeps_or_forgets_the_history(ctxs, scenes, forget):
    W, H = 96, 64
    s1 = scenes.build_scene("cover", 1, W, H)
    s2 = turned_scene(scenes, s1, "reshaping")
    r = ctxs()
    r.upload(s1)
    r.set_noise_estimate(True)
    everything(r, W, H, None, 2, 50, 1)  # (its temporal call leaves a history)
    r.download_features(), r.download_denoised()
    hist = r.download_temporal()
    assert r.turn_lights(lights_of(s2), forget=forget) is forget
    assert code_of(r.download_features)[0] == RT_ERR_SEQUENCE
    assert code_of(r.download_denoised)[0] == RT_ERR_SEQUENCE
    assert code_of(r.download)[0] == RT_ERR_SEQUENCE
    assert code_of(r.render, W, H, 3, 4, 50, 1)[0] == RT_ERR_SEQUENCE
    if not forget:
        kept = r.download_temporal()  # the history is kept, every word of it
        assert_same_bits(kept["state"], hist["state"], "history state across the turn")
        assert np.array_equal(kept["len"], hist["len"]) and np.array_equal(kept["target"], hist["target"])
    r.render(W, H, 1, 3, 50, 2)
    r.render_features(W, H, 1, 3)
    r.denoise_temporal(fetch=4)
    ln = r.download_temporal()["len"]
    assert (ln == 1).all() if forget else (ln > 1).any()  # forgotten: every pixel starts over; kept: the next call blends with it


def test_colour_alone_through_turn_lights_forgets_nothing(ctxs, scenes):
    W, H = 96, 64
    s1 = scenes.build_scene("cover", 1, W, H)
    r = ctxs()
    r.upload(s1)
    r.set_noise_estimate(True)
    everything(r, W, H, None, 2, 50, 1)
    hist = r.download_temporal()
    assert r.turn_lights([relit(lights_of(s1)[0], 1)]) is False  # forget=True, and no direction changed
    assert np.array_equal(r.download_temporal()["len"], hist["len"])
    assert code_of(r.download)[0] == RT_ERR_SEQUENCE  # an event all the same
    got = one_shot_of(r, W, H, 2)
    a = ctxs()
    a.upload(with_lights(s1, [relit(lights_of(s1)[0], 1)]))
    assert_same_bits(got, one_shot_of(a, W, H, 2), "colour through turn_lights against the upload")


def one_shot_of(r, W, H, spp):
    r.render(W, H, 1, 1 + spp, 50, 1)
    return r.download(ldr=False)[0]


def test_the_same_records_change_nothing(ctxs, scenes):
    """Nothing is voided and nothing is enqueued: an event recorded on the context's stream before the call and one after it complete
    together (behind a delay that is still running when the call has returned)."""
    torch.cuda.init()
    torch.cuda.set_device(0)
    W, H = 96, 64
    s1 = scenes.build_scene("cover", 1, W, H)
    stream = torch.cuda.Stream()
    r = ctxs()
    r.set_stream(stream.cuda_stream)
    r.upload(s1)
    r.set_noise_estimate(True)
    r.render(W, H, 1, 3, 50, 1)
    r.render_features(W, H, 1, 3)
    r.denoise()
    feat, den = r.download_features(), r.download_denoised()
    launches = r.trace_launches()
    same = [light_of(l) for l in lights_of(s1)]
    e0, e1 = torch.cuda.Event(), torch.cuda.Event()
    with torch.cuda.stream(stream):
        torch.cuda._sleep(20_000_000)  # some milliseconds: it only has to outlast the call
        e0.record(stream)
    assert r.turn_lights(same) is False
    e1.record(stream)
    pending = not e0.query()
    e1.synchronize()
    assert e0.query()  # nothing stood between the two events
    assert pending, "the delay had ended when the call had returned: nothing was shown"
    assert r.trace_launches() == launches
    for k, a in r.download_features().items():  # still served
        assert np.array_equal(a.view(np.uint32), feat[k].view(np.uint32)), k
    for k, a in r.download_denoised().items():
        assert np.array_equal(a.view(np.uint8), den[k].view(np.uint8)), k
    r.render(W, H, 3, 5, 50, 1)  # continues
    r.resolve()
    want = one_shot(ctxs, s1, W, H, 4)
    assert_same_bits(r.download()[0], want[0], "continued across the same records: HDR")
    r.set_frame_batch(8)  # a pending batch stays pending
    r.render(W, H, 5, 6, 50, 1, stats=False)
    r.turn_lights(same)
    assert r.committed_samples() == 4
    r.synchronize()
    assert r.committed_samples() == 5


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_come_before_any_side_effect(ctxs, scenes, oracle):
    from cpuraytracer_amd import _capi
    L = _capi.load()
    W, H = 96, 64
    s1 = three_lights_glossy(scenes, oracle, W, H)
    r = ctxs()
    n = C.c_uint32(77)
    assert code_of(r.turn_lights, s1.lights)[0] == RT_ERR_NO_SCENE and code_of(r.get_lights)[0] == RT_ERR_NO_SCENE
    r.upload(s1)
    r.set_noise_estimate(True)
    r.render(W, H, 1, 2, 50, 1)
    s = 2
    nan, inf = float("nan"), float("inf")

    def changed(k, field, j, v):
        ls = [light_of(l, OTHER_DIRECTIONS[i]) for i, l in enumerate(s1.lights)]
        if j is None:
            setattr(ls[k], field, v)
        else:
            getattr(ls[k], field)[j] = v
        return ls
    arr = (_capi.RtLight * 3)(*[light_of(l, OTHER_DIRECTIONS[i]) for i, l in enumerate(s1.lights)])
    refused = [
        ("null context", lambda: _capi.check(L.rt_turn_lights(None, arr, 3)), "null"),
        ("null lights", lambda: _capi.check(L.rt_turn_lights(r._h, None, 3)), "null"),
        ("another count", lambda: r.turn_lights(s1.lights[:2]), "lights for a scene uploaded with 3"),
        ("no lights", lambda: _capi.check(L.rt_turn_lights(r._h, None, 0)), "lights for a scene uploaded with 3"),
        ("NaN direction", lambda: r.turn_lights(changed(1, "direction", 2, nan)), "light 1 has a direction that is not finite"),
        ("infinite direction", lambda: r.turn_lights(changed(0, "direction", 0, -inf)), "light 0 has a direction that is not finite"),
        ("NaN colour", lambda: r.turn_lights(changed(2, "color", 1, nan)), "light 2 has a colour or a luminance that is not finite"),
        ("infinite luminance", lambda: r.turn_lights(changed(0, "luminance", None, inf)), "not finite"),
        ("get_lights: null count", lambda: _capi.check(L.rt_get_lights(r._h, arr, 3, None)), "null"),
        ("get_lights: null out", lambda: _capi.check(L.rt_get_lights(r._h, None, 3, C.byref(n))), "null"),
        ("get_lights: capacity", lambda: _capi.check(L.rt_get_lights(r._h, arr, 2, C.byref(n))), "capacity too small"),
    ]
    for what, call, text in refused:
        code, msg = code_of(call)
        assert code == RT_ERR_INVALID_ARG and text in msg, (what, code, msg)
        assert lights_bytes(r.get_lights()) == lights_bytes(s1.lights), what
        r.render(W, H, s, s + 1, 50, 1, stats=False)  # the running accumulation continues
        s += 1
    assert L.rt_get_lights(r._h, None, 0, C.byref(n)) == 0 and n.value == 3  # the count alone
    r.resolve()
    want = one_shot(ctxs, s1, W, H, s - 1)
    assert_same_bits(r.download()[0], want[0], "continued across the refusals: HDR")
    assert np.array_equal(r.download()[1], want[1])
    assert_same_bits(r.download_moments(), want[2], "continued across the refusals: moments")


def test_set_lights_after_a_turn(ctxs, scenes, oracle):
    """rt_set_lights compares with the directions set last: it accepts the turned ones and still refuses others, in its old words."""
    W, H = 96, 64
    s1 = three_lights_glossy(scenes, oracle, W, H)
    turned = [light_of(l, OTHER_DIRECTIONS[k]) for k, l in enumerate(s1.lights)]
    r = ctxs()
    r.upload(s1)
    r.turn_lights(turned)
    code, msg = code_of(r.set_lights, s1.lights)  # the uploaded directions are no longer the current ones
    assert code == RT_ERR_INVALID_ARG and "has another direction than the uploaded one: a direction change needs an rt_scene_upload" in msg
    recoloured = [relit(l, k) for k, l in enumerate(turned)]
    r.set_lights(recoloured)
    assert lights_bytes(r.get_lights()) == lights_bytes(recoloured)
    a = ctxs()
    a.upload(with_lights(s1, recoloured))
    assert_same_bits(one_shot_of(r, W, H, 2), one_shot_of(a, W, H, 2), "set_lights after a turn against the upload")


# ------------------------------------------------------------------------------------------------------------------ asynchrony
TARGET_MS = 40.0  # as tests/test_streams.py: it only has to outlast a few host-side enqueues, and the query() assertion decides


def test_turns_queue_behind_running_work_without_a_host_wait(ctxs, scenes):
    """On a caller stream with a 40 ms delay queued: render under L1, turn_lights(L2), turn_lights(L3), render.  The first picture is
    L1's and the second L3's although every table copy was ordered while the L1 render had not started -- L2's staging is not
    overwritten by L3's (two slots in turn) -- and an event behind the delay is still pending when the turns have returned.  A third
    queued turn may wait for the first one's slot: only its picture is asserted."""
    torch.cuda.init()
    torch.cuda.set_device(0)
    W, H, spp, depth = 96, 64, 2, 8
    s1 = scenes.build_scene("cover", 1, W, H)
    s2, s3, s4 = (turned_scene(scenes, s1, t) for t in ("reshaping", "x-dominant", "down"))
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
    r.turn_lights(lights_of(s2), forget=False)
    r.turn_lights(lights_of(s3), forget=False)
    assert not behind.query(), "the delay had ended when the turns had returned: nothing was shown to be asynchronous"
    r.render(W, H, 1, 1 + spp, depth, 1, stats=False)
    r.synchronize()
    second = r.download(ldr=False)[0]
    want1 = one_shot(ctxs, s1, W, H, spp, depth)[0]
    want3 = one_shot(ctxs, s3, W, H, spp, depth)[0]
    assert_same_bits(first.cpu().numpy(), want1, "the render queued before the turns: L1's picture")
    assert_same_bits(second, want3, "the render after the two turns: L3's picture")
    assert not np.array_equal(want1, want3) and not np.array_equal(one_shot(ctxs, s2, W, H, spp, depth)[0], want3)
    for s in (s2, s1, s4):  # three more, queued back to back
        r.turn_lights(lights_of(s), forget=False)
    r.render(W, H, 1, 1 + spp, depth, 1, stats=False)
    assert_same_bits(r.download(ldr=False)[0], one_shot(ctxs, s4, W, H, spp, depth)[0], "after three more queued turns: L4's picture")
