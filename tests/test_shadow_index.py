"""The shadow index on the device (-m gpu): `rt_unit_shadow` runs the production `shadow_query` / `any_hit_all` over the tables
`rt_scene_upload` put on the device, for the query points of tests/test_shadow_index_cpu.py; and the production kernels, with their
own staging of the index, render column scenes -- where most shadow questions overflow the query's register queue -- like the oracle."""
import numpy as np
import pytest

from test_primary_tables_fuzz import assert_same
from test_shadow_index_cpu import _columns, build_case, candidates, host_index, host_query, light_dir, make_light

# flat, hierarchy and grid; lights 0, 1 and 7; RT_SG_SPH=1, RT_SHADOW_CELLS=64; unnormalised lights, with the index and without
UNIT_CASES = ("flat5", "flat64_floor_big_light1", "flat150_floor_2big_light7", "flat150_negative", "flat150_sun*0.51", "flat150_sun*1.99_light7",
              "flat150_sun*0.49", "hierarchy1500_sg_sph", "tree_top_16_+x_light1", "grid3000", "grid3000_cells64", "columns_sun", "columns_sun*1.99",
              "offset_2e2_xy_light1", "flat480_tiny_light7")


@pytest.mark.gpu
@pytest.mark.parametrize("name", UNIT_CASES)
def test_device_answers_equal_the_host_twin_and_the_oracle(oracle, monkeypatch, name):
    """6,040 to 19,176 points per case, the global list read from its id list and from the LDS copy: the device's byte equals
    rt_unit_shadow_query_host's, and both equal the oracle's any-hit (bit 0) and the enabled flag and p0sq (bit 1)."""
    from cpuraytracer_amd import HipRenderer
    c = build_case(oracle, name)
    for key, value in c.env.items():
        monkeypatch.setenv(key, value)
    host = host_query(c.sc, c.k, c.pts)
    r = HipRenderer(0)  # the knobs are read when a context is created
    try:
        r.upload(c.sc)
        for lds in (False, True):
            got = r.unit_shadow(c.k, c.pts, glob_in_lds=lds)
            for what, want in (("the host twin", host), ("the oracle", c.want)):
                bad = np.nonzero(got != want)[0]
                assert bad.size == 0, "%s, global list %s: %d of %d answers differ from %s; first: point %r, device %d, expected %d" % (
                    name, "in LDS" if lds else "by id", bad.size, len(got), what, c.pts[bad[0]].tolist(), got[bad[0]], want[bad[0]])
    finally:
        r.close()


def _column_scene(oracle, light, length):
    d = light_dir(oracle, light)
    sc = _columns(oracle, d)
    sc.lights = [make_light(d * length)]
    return sc


def crowded_first_hits(oracle, sc, W, H, ijs):
    """Fraction of the first hits of the given samples whose shadow question has five or more listed spheres with a possible root."""
    orc = oracle.Oracle()
    try:
        orc.upload(sc)
        hits = orc.closest_hit(orc.primary_rays(W, H, ijs))
    finally:
        orc.close()
    hit = hits[:, 1].view(np.int32) >= 0
    n = candidates(sc, host_index(sc, 0), np.array(sc.lights[0].direction[:], dtype=np.float64), np.ascontiguousarray(hits[hit, 2:5]))
    return float((n >= 5).sum()) / len(ijs)


@pytest.mark.gpu
@pytest.mark.parametrize("length", (0.51, 1.0, 1.99))
@pytest.mark.parametrize("light", ("sun", "+y"))
def test_column_scenes_render_like_the_oracle_and_like_the_scan(oracle, monkeypatch, light, length):
    """The production kernels over the columns stacked along the stock sun and along +y, the light scaled to length 0.51, 1 and 1.99:
    3,000 traced samples at depth 0 and at depth 6 and a 160 x 100 image at 2 spp equal the oracle's bits and traversal counts, with
    the index and under RT_SHADOW_GRID=0.  At least 10 % of the first hits (25 % along the sun, 28 % along +y) ask a shadow question with five
    or more candidates."""
    from cpuraytracer_amd import HipRenderer
    sc = _column_scene(oracle, light, length)
    W, H, m = 160, 100, 3000
    rng = np.random.default_rng(11)
    ijs = np.stack([rng.integers(0, W, m), rng.integers(0, H, m), rng.integers(1, 600, m)], 1).astype(np.uint32)
    assert host_index(sc, 0).enabled and crowded_first_hits(oracle, sc, W, H, ijs) >= 0.10
    orc = oracle.Oracle()
    try:
        orc.upload(sc)
        want = [orc.trace(W, H, ijs, depth, 77, accel=oracle.ACCEL_PADDED_LIST) for depth in (0, 6)]
        so = orc.render(W, H, 1, 3, 6, 9, accel=oracle.ACCEL_PADDED_LIST, threads=8)
        ho, _ = orc.download()
    finally:
        orc.close()
    for grid in ("1", "0"):
        monkeypatch.setenv("RT_SHADOW_GRID", grid)
        r = HipRenderer(0)
        try:
            r.upload(sc)
            for depth, (ro, to) in zip((0, 6), want):
                rg, tg = r.unit_trace(W, H, ijs, depth, 77)
                assert_same(rg, ro, "RT_SHADOW_GRID=%s, depth %d: per-sample radiance" % (grid, depth))
                assert np.array_equal(tg, to), "RT_SHADOW_GRID=%s, depth %d: traversal counts" % (grid, depth)
            sg = r.render(W, H, 1, 3, 6, 9)
            hg, _ = r.download(ldr=False)
            assert_same(hg, ho, "RT_SHADOW_GRID=%s: whole image HDR" % grid)
            assert (sg.traversals, sg.segments) == (so.traversals, so.segments), grid
        finally:
            r.close()
