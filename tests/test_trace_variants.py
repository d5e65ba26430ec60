"""The trace-kernel census on the device (-m gpu): every recipe of tests/trace_variant_cases.py on a fresh context -- the launcher must
report the recipe's kernel (rt_unit_last_trace_launch), and that kernel must render the oracle's bits at a shape that makes every wave
claim from the dynamic queue and steal from other shards, twice on the same context.  A closing test compares the kernels reported
over the module with the 110 the library instantiates.

The shape: 131 x 61 pixels (7,991: no multiple of 64, rows of no multiple of 64, so tiles wrap rows and the last tile is partial), depth
50, and as many samples per pixel as give the dynamic queue two blocks for every launched wave beyond the static block each wave starts
with: 3 x 128 paths per wave, about 1.6 M paths where a CU holds 16 waves, half and a quarter of that under the smaller settings.  The
conditions are asserted from the plan words the launcher reports, not from this arithmetic.  The oracle renders once per (scene, light
list), progressively through the samples-per-pixel counts its recipes need."""
import numpy as np
import pytest

import trace_variant_cases as T

pytestmark = pytest.mark.gpu


def assert_same(a, b, what):
    """The only difference allowed is 0."""
    assert a.shape == b.shape and a.dtype == b.dtype, what
    ba, bb = (np.ascontiguousarray(x).view(np.uint32) if x.dtype == np.float32 else x for x in (a, b))
    if not np.array_equal(ba, bb):
        d = np.nanmax(np.abs(a.astype(np.float64) - b.astype(np.float64)))
        raise AssertionError("%s: %d of %d values differ, max abs diff %g" % (what, int(np.count_nonzero(ba != bb)), a.size, d))


W, H, DEPTH, SEED = 131, 61, 50, 1
CARRY_W, CARRY_H, CARRY_FRAMES = 83, 47, 40  # 3,901 pixels: ragged too

# (row, lights) of every trace launch the launcher reported in this module, and the recipes that ran (the closing test reads both)
_REPORTED = set()
_RAN = []
_DEVICE_ERROR = []


def _spp_for(recipe, cu_count):
    """Samples per pixel that give every wave its static block and two dynamic ones: ceil(3 x waves x 128 / pixels)."""
    if recipe.mode != "ordinary":
        return CARRY_FRAMES
    waves = cu_count * T.waves_per_cu(recipe.env)
    spp = -(-3 * waves * 128 // (W * H))
    return spp + 1 if spp % 64 == 0 else spp  # (an odd pixel count times a multiple of 128 samples would end on a whole block)


@pytest.fixture(scope="module")
def cu_count(hip):
    """Compute units of device 0, as rt_create counts them: read off a launch of the shared context (case word [12])."""
    sc = T.build_scene("small300", 16, 8)
    hip.upload(sc)
    hip.render(16, 8, 1, 2, 2, SEED)
    return int(hip.last_trace_launch().case_words[12])


@pytest.fixture(scope="module")
def oracle_pictures(oracle, cu_count):
    """{(scene, n_lights, W, H, spp): (hdr, ldr, traversals, segments, samples)}: one oracle per (scene, light list, picture size),
    rendered progressively through the sorted sample counts its recipes ask for (the strip after [1, 1 + spp) is the one-shot strip:
    samples are added in order).  Read-only afterwards."""
    wanted = {}
    for r in T.RECIPES:
        size = (W, H) if r.mode == "ordinary" else (CARRY_W, CARRY_H)
        wanted.setdefault((r.scene, r.n_lights) + size, set()).add(_spp_for(r, cu_count))
    out = {}
    for (scene, n_lights, w, h), spps in sorted(wanted.items()):
        orc = oracle.Oracle()
        orc.upload(T.build_scene(scene, w, h, n_lights))
        done, trav, seg, smp = 0, 0, 0, 0
        for spp in sorted(spps):
            st = orc.render(w, h, 1 + done, 1 + spp, DEPTH, SEED, accel=oracle.ACCEL_PADDED_LIST, threads=16)
            done, trav, seg, smp = spp, trav + st.traversals, seg + st.segments, smp + st.samples
            orc.resolve()
            hdr, ldr = orc.download()
            hdr.setflags(write=False)
            ldr.setflags(write=False)
            out[(scene, n_lights, w, h, spp)] = (hdr, ldr, trav, seg, smp)
        orc.close()
    return out


RT_ERR_HIP = 4


@pytest.fixture(autouse=True)
def _device_errors_end_the_module():
    """Most of these kernels are run by nothing else.  When one leaves the device in error (a HIP call failed), no later recipe is
    started on it: the session ends there, with that recipe's name."""
    yield
    if _DEVICE_ERROR:
        pytest.exit("census stopped: %s left the device in error: %s" % (_DEVICE_ERROR[0], _DEVICE_ERROR[1]), returncode=3)


def _guard(recipe, fn):
    """Run fn(); a HIP error is recorded for the fixture above before it propagates."""
    from cpuraytracer_amd import _capi
    try:
        return fn()
    except _capi.RtError as e:
        if e.code == RT_ERR_HIP:
            _DEVICE_ERROR[:] = [recipe.name, str(e)]
        raise


def _fresh_context(monkeypatch, recipe):
    """A context created under the recipe's environment, which stays set until the test ends (rt_create reads the settings, the upload
    the layout's, every launch the knobs)."""
    from cpuraytracer_amd import HipRenderer
    for k, v in recipe.env.items():
        monkeypatch.setenv(k, v)
    return HipRenderer(0)


def _check_report(r, recipe, launches, exact=True):
    """The launcher's account after a render: the recipe's kernel, instantiated, and words that the plan reproduces."""
    from cpuraytracer_amd import _capi, renderer
    tl = r.last_trace_launch()
    _REPORTED.add((tl.row, tl.lights))
    k = renderer.decode_kernel_word(recipe.kernel)
    assert tl.kernel_word == recipe.kernel, "%s reached %s (row %d%s), not %s (row %d%s)" % (
        recipe.name, renderer.decode_kernel_word(tl.kernel_word), tl.row, ", twin" if tl.lights else "", k, recipe.row, ", twin" if k["lights"] else "")
    assert tl.kernel_word >> 31 == 1 and tl.row == recipe.row and tl.lights == (recipe.n_lights != 1)
    assert tl.launches == launches if exact else tl.launches >= launches
    # the CPU plan tests' entry answers the shape of this real upload with the plan that was applied, all 28 words
    again = np.zeros(28, dtype=np.uint32)
    _capi.check(_capi.load().rt_unit_launch_plan(tl.case_words.ctypes.data, 1, again.ctypes.data))
    assert np.array_equal(again, tl.plan_words), "rt_unit_launch_plan(case words) differs from the applied plan at words %s" % np.flatnonzero(again != tl.plan_words)
    assert tl.plan_words[0] == 0 and tl.case_words[11] == recipe.n_lights
    return tl


@pytest.mark.parametrize("recipe", [r for r in T.RECIPES if r.mode == "ordinary"], ids=lambda r: r.name)
def test_recipe_reaches_its_kernel_and_renders_the_oracles_bits(built, monkeypatch, oracle_pictures, cu_count, recipe):
    spp = _spp_for(recipe, cu_count)
    r = _fresh_context(monkeypatch, recipe)
    try:
        _RAN.append(recipe)
        _guard(recipe, lambda: _render_twice_and_compare(r, recipe, spp, oracle_pictures[(recipe.scene, recipe.n_lights, W, H, spp)]))
    finally:
        r.close()


def _render_twice_and_compare(r, recipe, spp, oracle_picture):
    hdr_o, ldr_o, trav_o, seg_o, smp_o = oracle_picture
    assert r.trace_launches() == 0
    r.upload(T.build_scene(recipe.scene, W, H, recipe.n_lights))
    # ---- one render over the whole sample range
    st = r.render(W, H, 1, 1 + spp, DEPTH, SEED)
    tl = _check_report(r, recipe, st.passes)
    # the shape, from the plan: ragged picture, depth 50, and a dynamic queue of at least two blocks per launched wave
    threads = int(tl.case_words[14])
    assert st.passes == 1 and tl.case_words[24] == W * H * spp and (W * H) % 64 != 0 and W % 64 != 0
    assert tl.case_words[25] == 50 and tl.case_words[26] == 0 and threads == tl.kThreads
    assert tl.blocks == tl.case_words[12] * tl.case_words[13], "fewer workgroups than the device holds: %d" % tl.blocks
    assert tl.queue_block % 64 == 0 and tl.static_blocks >= 1
    assert tl.dyn_blocks >= 2 * tl.blocks * (threads // 64), "dynamic queue of %d blocks for %d waves" % (tl.dyn_blocks, tl.blocks * (threads // 64))
    assert tl.dyn_begin == tl.blocks * (threads // 64) * tl.queue_block * tl.static_blocks
    assert (W * H * spp - tl.dyn_begin) % tl.queue_block != 0  # the short last block
    r.resolve()
    hdr, ldr = r.download()
    assert_same(hdr, hdr_o, "%s: HDR vs the oracle" % recipe.name)
    assert_same(ldr, ldr_o, "%s: LDR vs the oracle" % recipe.name)
    assert (st.traversals, st.segments, st.samples) == (trav_o, seg_o, smp_o)
    # ---- the same range again on the warm context, as three progressive calls of unequal size
    r.clear()
    a, b = 1 + max(1, spp // 7), 1 + max(2, spp // 7 + spp // 3)
    parts = [r.render(W, H, s0, s1, DEPTH, SEED) for s0, s1 in ((1, a), (a, b), (b, 1 + spp))]
    _check_report(r, recipe, st.passes + sum(p.passes for p in parts))
    r.resolve()
    hdr2, ldr2 = r.download()
    assert_same(hdr2, hdr, "%s: three progressive calls vs the one render" % recipe.name)
    assert_same(ldr2, ldr, "%s: three progressive calls vs the one render, LDR" % recipe.name)
    assert (sum(p.traversals for p in parts), sum(p.segments for p in parts), sum(p.samples for p in parts)) == (trav_o, seg_o, smp_o)


@pytest.mark.parametrize("recipe", [r for r in T.RECIPES if r.mode != "ordinary"], ids=lambda r: r.name)
def test_the_carrying_kernel_renders_the_oracles_bits(built, monkeypatch, oracle_pictures, cu_count, recipe):
    """Row 0, both twins: stats-less 1-spp frames under rt_set_frame_pipelining, whose kernels carry their unfinished paths into the next
    frame's kernel; after rt_synchronize the strip is the ORACLE's render of all the samples."""
    from cpuraytracer_amd import _capi
    w, h, frames = CARRY_W, CARRY_H, CARRY_FRAMES
    hdr_o, ldr_o, _, _, _ = oracle_pictures[(recipe.scene, recipe.n_lights, w, h, frames)]
    r = _fresh_context(monkeypatch, recipe)
    try:
        _RAN.append(recipe)
        _guard(recipe, lambda: _pipelined_frames_and_compare(r, recipe, w, h, frames, hdr_o, ldr_o))
    finally:
        r.close()


def _pipelined_frames_and_compare(r, recipe, w, h, frames, hdr_o, ldr_o):
    from cpuraytracer_amd import _capi
    # before any launch: the documented refusal, and a count of zero
    with pytest.raises(_capi.RtError) as e:
        r.last_trace_launch()
    assert e.value.code == _capi.RT_ERR_SEQUENCE and r.trace_launches() == 0
    r.upload(T.build_scene(recipe.scene, w, h, recipe.n_lights))
    with pytest.raises(_capi.RtError) as e:
        r.last_trace_launch()
    assert e.value.code == _capi.RT_ERR_SEQUENCE
    assert (w * h) % 64 != 0 and w % 64 != 0
    r.set_frame_pipelining(recipe.mode[1])
    for f in range(frames):
        r.render(w, h, 1 + f, 2 + f, DEPTH, SEED, stats=False)
        if f in (0, frames // 2):
            tl = _check_report(r, recipe, f + 1, exact=False)
            assert tl.kCarry and tl.case_words[26] == 1 and tl.plan_words[10] & 128
            assert (tl.queue_block, tl.static_blocks, tl.dyn_begin, tl.dyn_blocks) == (0, 0, 0, 0)  # the pipelined path cuts its own queue
    r.synchronize()
    assert r.committed_samples() == frames
    tl = _check_report(r, recipe, r.trace_launches())  # (the flush launches the same kernel over the carried paths)
    assert tl.launches > frames and tl.kCarry
    r.resolve()
    hdr, ldr = r.download()
    assert_same(hdr, hdr_o, "%s: pipelined frames vs the oracle" % recipe.name)
    assert_same(ldr, ldr_o, "%s: pipelined frames vs the oracle, LDR" % recipe.name)


def test_every_kernel_of_the_library_was_reported(built):
    """The closing test: the (row, twin) pairs the launcher reported over this module are those of the recipes that ran -- all 110 minus
    NOT_RUN when the whole module ran.  (Under a -k selection only the selected recipes are checked.)"""
    from cpuraytracer_amd import renderer
    assert _RAN, "no recipe ran before the closing test"
    rows = renderer.trace_variants()
    want = {(r.row, r.n_lights != 1) for r in _RAN}
    assert want <= _REPORTED, "kernels never reported: %s" % sorted(want - _REPORTED)
    assert _REPORTED <= want, "kernels reported that no recipe that ran expects: %s" % sorted(_REPORTED - want)
    if len(_RAN) == len(T.RECIPES):
        not_run = {(row, lights) for row, _ in T.NOT_RUN for lights in (False, True)}
        every = {(row, lights) for row in range(len(rows)) for lights in (False, True)}
        assert len(every) == 110 and len(not_run) <= 2 * T.MAX_NOT_RUN
        assert _REPORTED == every - not_run, "of %d kernels %d were reported; missing %s" % (len(every), len(_REPORTED), sorted(every - not_run - _REPORTED))
        print("trace-kernel census: %d of %d (row, twin) pairs reported, NOT_RUN %d rows" % (len(_REPORTED), len(every), len(T.NOT_RUN)))
