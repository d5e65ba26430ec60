"""The kernels without far-hit state on the device (-m gpu; DESIGN.md §5.1 "far hit points"): a scene in which a fifth and more of the
shadow rays start beyond the first shadow index (tests/far_shadow_cases.py far_scene; tests/test_far_shadow_cpu.py asserts that from the
oracle alone), rendered at 128 x 64, spp 4, depth 6.  HDR bits, traversals and segments equal the oracle's over its plain list, and this
library's with the far-hit state forced (RT_FAR_STATE=1) and with every shadow ray on the scan (RT_SHADOW_GRID=0); over the whole image
and over the cyclic rows of two ranks; with the scene's one sun and with light lists of 0, 2 and 3 lights.  The launcher reports the
lean kernel by default and the one with far-hit state under each knob.  And the device's answers from the second index
(rt_unit_shadow_tier) equal the host twin's on the points of the CPU file."""
import numpy as np
import pytest

import far_shadow_cases as FS
from test_far_shadow_cpu import FAR_DEPTH, FAR_H, FAR_SEED, FAR_SPP, FAR_W

pytestmark = pytest.mark.gpu

EXTRA_LIGHTS = (((-0.6, 0.7, 0.35), (0.35, 0.55, 1.0), 25000.0), ((0.2, 0.25, -0.9), (1.0, 0.4, 0.3), 12000.0))
KNOBS = ({}, {"RT_FAR_STATE": "1"}, {"RT_SHADOW_GRID": "0"})


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _scene(oracle, n_lights):
    sc = FS.far_scene(oracle, FAR_W, FAR_H)
    sun = sc.lights[0]
    if n_lights == 0:
        sc.lights = []
    elif n_lights > 1:
        sc.lights = [sun] + [oracle.make_light(*l) for l in EXTRA_LIGHTS[:n_lights - 1]]
    else:
        del sc.lights  # the scene's one sun: the single-light kernels
        sc.sun = sun
    return sc


def _rowsets(oracle):
    return {"whole": None, "rank0of2": oracle.RtRowset(0, FAR_H, 1, 0, 2), "rank1of2": oracle.RtRowset(0, FAR_H, 1, 1, 2)}


@pytest.fixture(scope="module")
def oracle_pictures(oracle):
    """{(n_lights, rows): (hdr, traversals, segments)} from the oracle's plain list scan.  Read-only afterwards."""
    out = {}
    for n_lights in (1, 0, 2, 3):
        orc = oracle.Oracle()
        orc.upload(_scene(oracle, n_lights))
        for rows, rs in _rowsets(oracle).items():
            st = orc.render(FAR_W, FAR_H, 1, 1 + FAR_SPP, FAR_DEPTH, FAR_SEED, rowset=rs, accel=oracle.ACCEL_LIST, threads=8)
            orc.resolve()
            hdr, _ = orc.download()
            hdr.setflags(write=False)
            out[(n_lights, rows)] = (hdr, st.traversals, st.segments)
        orc.close()
    return out


@pytest.mark.parametrize("n_lights", (1, 0, 2, 3))
def test_far_scene_renders_the_oracles_bits_under_every_knob(built, oracle, monkeypatch, oracle_pictures, n_lights):
    from cpuraytracer_amd import HipRenderer
    sc = _scene(oracle, n_lights)
    for env in KNOBS:
        for k in ("RT_FAR_STATE", "RT_SHADOW_GRID"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        r = HipRenderer(0)  # (RT_SHADOW_GRID is read when the context is created)
        try:
            r.upload(sc)
            for rows, rs in _rowsets(oracle).items():
                r.clear()
                st = r.render(FAR_W, FAR_H, 1, 1 + FAR_SPP, FAR_DEPTH, FAR_SEED, rowset=rs)
                r.resolve()
                hdr, _ = r.download()
                tl = r.last_trace_launch()
                what = "%d lights, %s, %s" % (n_lights, rows, env or "default")
                # the flat LDS hit-stash family; lean by default wherever light 0 has an index, far-hit state under either knob
                assert tl.kLds and tl.kScan == 1 and tl.kStash and not tl.kCarry and tl.lights == (n_lights != 1), what
                assert r.last_trace_far_state() == ("lean" if not env and n_lights != 0 else "full"), what
                hdr_o, trav_o, seg_o = oracle_pictures[(n_lights, rows)]
                assert hdr.shape == hdr_o.shape
                diff = int(np.count_nonzero(_bits(hdr) != _bits(hdr_o)))
                assert diff == 0, "%s: %d of %d HDR values differ from the oracle's" % (what, diff, hdr.size)
                assert (st.traversals, st.segments) == (trav_o, seg_o), what
        finally:
            r.close()


def test_path_lists_keep_the_far_state_and_the_oracles_counts(built, oracle, monkeypatch):
    """rt_unit_trace on the same context: a path list with per-path traversal counts takes the kernel with far-hit state, and its
    radiance and counts are the oracle's -- for paths whose first hit lies beyond the first index as well."""
    from cpuraytracer_amd import HipRenderer
    for k in ("RT_FAR_STATE", "RT_SHADOW_GRID"):
        monkeypatch.delenv(k, raising=False)
    sc = _scene(oracle, 1)
    rng = np.random.default_rng(11)
    ijs = np.stack([rng.integers(0, FAR_W, 600), rng.integers(FAR_H // 2, FAR_H, 600), rng.integers(1, 40, 600)], 1).astype(np.uint32)
    orc = oracle.Oracle()
    orc.upload(sc)
    rgb_o, trav_o = orc.trace(FAR_W, FAR_H, ijs, FAR_DEPTH, FAR_SEED)
    orc.close()
    r = HipRenderer(0)
    try:
        r.upload(sc)
        r.render(FAR_W, FAR_H, 1, 2, FAR_DEPTH, FAR_SEED)
        assert r.last_trace_far_state() == "lean"
        rgb, trav = r.unit_trace(FAR_W, FAR_H, ijs, FAR_DEPTH, FAR_SEED)
        assert r.last_trace_far_state() == "full"
        assert np.array_equal(_bits(rgb), _bits(rgb_o)) and np.array_equal(trav, trav_o)
    finally:
        r.close()


@pytest.mark.parametrize("name", ("far_scene", "field_1000", "field_1000_low_sun", "halving"))
def test_device_answers_from_the_second_index_equal_the_host_twins(built, oracle, hip, name):
    """rt_unit_shadow_tier(tier 2) over the uploaded tables against rt_unit_shadow_query_host_tier on the CPU file's points of the case:
    the same byte per point (which is the oracle's any-hit and the two radii's verdict: tests/test_far_shadow_cpu.py), with the first
    index's global list walked from LDS and from global memory; and tier 1 is rt_unit_shadow."""
    c = FS.build_case(oracle, name)
    hip.upload(c.sc)
    want = FS.host_query_tier(c.sc, 2, c.pts)
    assert np.array_equal(want, c.want) and (want & 4).sum() >= 2000
    for glob_in_lds in (False, True):
        got = hip.unit_shadow_tier(2, c.pts, glob_in_lds=glob_in_lds)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, "%s: %d of %d device answers differ; first: point %r, device %d, host %d" % (
            name, bad.size, len(want), c.pts[bad[0]].tolist(), got[bad[0]], want[bad[0]])
    assert np.array_equal(hip.unit_shadow_tier(1, c.pts[:2000]), hip.unit_shadow(0, c.pts[:2000]))
