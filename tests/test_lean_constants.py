"""The launch constants of the trace kernels without far-hit state, read back from LDS (-m gpu; rt_params.h fill_lean_consts,
DESIGN.md §5.1 "launch constants in LDS").  Those kernels keep in LDS what the persistent loop reads of the kernel arguments -- the
tile tables and their divisors, the sample region, the queue's window and cursors, the sample buffer, depth limit, stash policy,
material form, the scene's light records and entry count, the counters -- and every case below moves some of them away from the
value a wrong read would still get right:

  second call     cover 256 x 128, spp 4: 512 full tiles, so the second call takes the short queue of RT_SKY_EXCLUDE (total_paths,
                  dyn_begin, dyn_blocks, static_blocks differ from the first call's);
  partial tile    70 x 41, spp 3: npix_local is no multiple of 64, W is no power of two, spp_pass is odd;
  rank 1 of 2     the cyclic rows of the second of two ranks (rs.shard, rs.nshards, fd_rows, the lens table's k0);
  continued       a second render with s0 = 5 (s0 and the jitter table's base are not 1);
  depth           max_depth 1, 2 and 50;
  seed            two render seeds (both halves of the 64-bit seed's low word change the streams);
  stash           RT_STASH_CAP=20 with RT_STASH_PROCESS=7: the smallest chunks of LDS the constants can get, and another policy;
  RT_SKY_SKIP=0, RT_TILE_ORDER=0 (tile_order is null), RT_MATS16=1 (the packed materials through the pointer kept in LDS);
  far             the scene of tests/far_shadow_cases.py, where a fifth of the shadow rays read the second index's record.

For each: HDR bits, traversals and segments equal the oracle's over its plain list, and the same call under RT_FAR_STATE=1 (the
kernels that read the kernel arguments); rt_unit_last_trace_far_state says which kernel ran."""
import numpy as np
import pytest

import far_shadow_cases as FS

pytestmark = pytest.mark.gpu

W0, H0, SPP0 = 256, 128, 4


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# name: (scene, W, H, [(s0, s1), ...] calls of one accumulation, depth, seed, rows, environment, context knobs)
CASES = {
    "second_call": ("cover", W0, H0, [(1, 1 + SPP0)], 50, 1, "whole", {}),
    "partial_tile": ("cover", 70, 41, [(1, 4)], 50, 1, "whole", {}),
    "rank1of2": ("cover", W0, H0, [(1, 1 + SPP0)], 50, 1, "rank1of2", {}),
    "continued": ("cover", W0, H0, [(1, 5), (5, 8)], 50, 1, "whole", {}),
    "depth1": ("cover", W0, H0, [(1, 3)], 1, 1, "whole", {}),
    "depth2": ("cover", W0, H0, [(1, 3)], 2, 1, "whole", {}),
    "seed": ("cover", W0, H0, [(1, 3)], 50, 0x9E3779B9, "whole", {}),
    "stash_policy": ("cover", W0, H0, [(1, 1 + SPP0)], 50, 1, "whole", {"RT_STASH_CAP": "20", "RT_STASH_PROCESS": "7"}),
    "sky_skip_off": ("cover", W0, H0, [(1, 1 + SPP0)], 50, 1, "whole", {"RT_SKY_SKIP": "0"}),
    "tile_order_off": ("cover", W0, H0, [(1, 1 + SPP0)], 50, 1, "whole", {"RT_TILE_ORDER": "0"}),
    "mats16_global": ("cover", W0, H0, [(1, 1 + SPP0)], 50, 1, "whole", {"RT_MATS16": "1"}),
    "far": ("far", 128, 64, [(1, 5)], 6, 7, "whole", {}),
    "far_rank1of2_stash_policy": ("far", 128, 64, [(1, 4)], 6, 7, "rank1of2", {"RT_STASH_CAP": "16", "RT_STASH_PROCESS": "3"}),
    "far_mats16_global": ("far", 128, 64, [(1, 5)], 6, 7, "whole", {"RT_MATS16": "1"}),
}
KNOB_NAMES = ("RT_FAR_STATE", "RT_STASH_CAP", "RT_STASH_PROCESS", "RT_SKY_SKIP", "RT_TILE_ORDER", "RT_MATS16")


def _scene(oracle, name, W, H):
    if name == "far":
        sc = FS.far_scene(oracle, W, H)
        sun = sc.lights[0]
        del sc.lights  # the scene's one sun: the single-light kernels
        sc.sun = sun
        return sc
    from cpuraytracer_amd import scenes
    return scenes.build_scene("cover", 1, W, H)


def _rowset(oracle, rows, H):
    return None if rows == "whole" else oracle.RtRowset(0, H, 1, 1, 2)


@pytest.fixture(scope="module")
def oracle_pictures(oracle):
    """{(scene, W, H, calls, depth, seed, rows): (hdr, traversals and segments of the last call)} from the oracle's plain list: one
    render per distinct picture, shared by the cases that differ in knobs only.  Read-only afterwards."""
    out = {}
    for scene, W, H, calls, depth, seed, rows, _env in CASES.values():
        key = (scene, W, H, tuple(calls), depth, seed, rows)
        if key in out:
            continue
        orc = oracle.Oracle()
        orc.upload(_scene(oracle, scene, W, H))
        for s0, s1 in calls:
            st = orc.render(W, H, s0, s1, depth, seed, rowset=_rowset(oracle, rows, H), accel=oracle.ACCEL_LIST, threads=8)
        orc.resolve()
        hdr, _ = orc.download()
        hdr.setflags(write=False)
        out[key] = (hdr, st.traversals, st.segments)
        orc.close()
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_lean_kernels_read_their_launch_constants_from_lds(built, oracle, monkeypatch, oracle_pictures, name):
    from cpuraytracer_amd import HipRenderer
    scene, W, H, calls, depth, seed, rows, env = CASES[name]
    sc = _scene(oracle, scene, W, H)
    rs = _rowset(oracle, rows, H)
    hdr_o, trav_o, seg_o = oracle_pictures[(scene, W, H, tuple(calls), depth, seed, rows)]
    shots = {}
    for far_state in ("lean", "full"):
        for k in KNOB_NAMES:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        if far_state == "full":
            monkeypatch.setenv("RT_FAR_STATE", "1")
        r = HipRenderer(0)  # (RT_TILE_ORDER is read when the context is created)
        try:
            r.upload(sc)
            # the picture once with another seed, so that the compared accumulation finds the tile tables built, the count of
            # empty-list tiles on the host (the short queue) and other samples in the sample buffer
            r.render(W, H, calls[0][0], calls[0][1], depth, seed + 1, rowset=rs)
            r.synchronize()
            for s0, s1 in calls:
                st = r.render(W, H, s0, s1, depth, seed, rowset=rs)
                tl = r.last_trace_launch()
                assert tl.kLds and tl.kScan == 1 and tl.kStash and not tl.kCarry and not tl.lights, name
                assert r.last_trace_far_state() == far_state, name
            if name == "second_call":  # ... and the short queue really was taken (tests/test_gpu_sky_exclude.py)
                import ctypes as C
                from cpuraytracer_amd import _capi
                n = C.c_uint32(0)
                _capi.check(_capi.load().rt_unit_sky_excluded(r._h, C.byref(n)))
                assert n.value > 0, "the second call did not take the short queue"
            r.resolve()
            hdr, _ = r.download()
            shots[far_state] = (hdr, st.traversals, st.segments)
        finally:
            r.close()
        what = "%s, %s kernel" % (name, far_state)
        assert hdr.shape == hdr_o.shape, what
        diff = int(np.count_nonzero(_bits(hdr) != _bits(hdr_o)))
        assert diff == 0, "%s: %d of %d HDR values differ from the oracle's" % (what, diff, hdr.size)
        assert (st.traversals, st.segments) == (trav_o, seg_o), what
    assert np.array_equal(_bits(shots["lean"][0]), _bits(shots["full"][0])) and shots["lean"][1:] == shots["full"][1:], name
