"""Light 0's second shadow index and the far-hit-state rule, without a GPU (DESIGN.md §5.1 "far hit points"; cases and point classes in
tests/far_shadow_cases.py).  The standard is tests/test_shadow_index_cpu.py's: no tolerance anywhere, equalities and inclusions against
the oracle's any-hit of the ray (p, L) over the plain sphere list.

Also here: the precondition of tests/test_far_shadow.py's scene, from the oracle alone; and the launch plan's rule for the kernels
without far-hit state (host/far_state_selftest.cpp, and rt_unit_far_state_plan over the recorded launch-plan cases)."""
import os
import subprocess

import numpy as np
import pytest

import far_shadow_cases as FS
import launch_plan_cases as G
import test_shadow_index_cpu as S
from conftest import ROOT
from test_primary_tables_fuzz import _accepted

F = np.float32
# at scale 1e-3 the floor has radius 1 and P0 is 1.01 (it does not shrink below 1): every point down-light of the field at that distance
# lies inside the floor or behind it, and the floor decides
FLOOR_DECIDES = ("field_1000_scale_1e-3",)


def test_second_index_exists_where_it_should(built, oracle):
    """Every case has a second index whose radius is four times the first's, or 1.01 times the farthest surface where that is nearer (the
    halving scene, and the scene at scale 1e-3, whose floor of radius 1 ends 2 units from the origin while P0 = 2 reach + 8 r + 1 cannot
    shrink below 1: both its indices hold all 59 spheres in their global lists); it lies in 16-bit tables like the first."""
    for name in FS.CASES:
        c = FS.build_case(oracle, name)
        P0, P2 = np.sqrt(np.float64(c.G1.p0sq)), np.sqrt(np.float64(c.G2.p0sq))
        print("%s: first index %d x %d, global %d, P0 %.6g; second %s %d x %d, entries %d, global %d, P2 %.6g" % (
            name, c.G1.nx, c.G1.ny, len(c.G1.glob), P0, "on" if c.G2.enabled else "OFF", c.G2.nx, c.G2.ny, len(c.G2.entries), len(c.G2.glob), P2))
        assert c.G2.enabled, name
        far = float((np.linalg.norm(np.stack([c.sc.spheres["cx"], c.sc.spheres["cy"], c.sc.spheres["cz"]], 1).astype(np.float64), axis=1)
                     + np.abs(c.sc.spheres["r"].astype(np.float64))).max())
        assert abs(P2 / min(4.0 * P0, 1.01 * far) - 1.0) < 1e-5, (name, P0, P2, far)
        assert len(c.G2.glob) <= 64 and len(c.G2.entries) < 65535
    h = FS.build_case(oracle, "halving")
    # the halving rule fired: the second index has 128 cells a side, half the 256 an index in global memory may have, and its cells are
    # wider than two median footprints (at most 2 x 0.931: radius 0.01, |c| <= 141.5, P2 = 304), which only the limit makes them
    print("halving: second index %d x %d cells of %.4f, %d entries" % (h.G2.nx, h.G2.ny, 1.0 / h.G2.inv, len(h.G2.entries)))
    assert max(h.G2.nx, h.G2.ny) == 128 and 1.0 / np.float64(h.G2.inv) > 2 * 0.931, (h.G2.nx, h.G2.ny, 1.0 / h.G2.inv)
    assert abs(np.sqrt(np.float64(h.G2.p0sq)) / (1.01 * 301.0) - 1.0) < 1e-3


@pytest.mark.parametrize("name", sorted(FS.CASES))
def test_host_answers_equal_the_oracles_any_hit(built, oracle, name):
    """All classes: bit 0 of rt_unit_shadow_query_host_tier(tier 2) equals the oracle's any-hit, bits 1 and 2 what the two radii say.
    Conditions on the inputs: at least 2,000 points per case are answered by the second index; among the grazing points at least 100
    are decided by a sphere that is not the floor (occluded over the scene without its floor, not occluded by the floor alone) unless
    the light shines from below (or FLOOR_DECIDES); both sides of both cuts occur."""
    c = FS.build_case(oracle, name)
    got = FS.host_query_tier(c.sc, 2, c.pts)
    a = c.slices["a"]
    decided = c.occluded_by_small[a] & ~c.occluded_by_floor[a] & c.second[a]
    print("%s: %d points, %d answered by the second index, %d by every entry; grazing: %d occluded, %d decided by a small sphere" % (
        name, len(c.pts), int(c.second.sum()), int((~c.first & ~c.second).sum()), int(c.occluded[a].sum()), int(decided.sum())))
    assert c.second.sum() >= 2000, name
    if c.ld[1] >= 0 and name not in FLOOR_DECIDES:
        assert decided.sum() >= 100, (name, int(decided.sum()))
    cut = c.slices["c"]
    assert c.first[cut].any() and c.second[cut].any() and (~c.first[cut] & ~c.second[cut]).any(), name
    for key, sl in c.slices.items():
        bad = np.nonzero(got[sl] != c.want[sl])[0]
        assert bad.size == 0, "%s, class (%s): %d of %d answers differ; first: point %r, got %d, want %d" % (
            name, key, bad.size, sl.stop - sl.start, c.pts[sl][bad[0]].tolist(), got[sl][bad[0]], c.want[sl][bad[0]])
    # tier 1 of the new entry is the old entry
    assert np.array_equal(FS.host_query_tier(c.sc, 1, c.pts[:500]), S.host_query(c.sc, 0, c.pts[:500]))


@pytest.mark.parametrize("name", sorted(FS.CASES))
def test_every_accepted_far_pair_is_listed(built, oracle, name):
    """Class (a): every (point, sphere) pair of the [aimed spheres x points] matrix that the oracle's Sphere::Intersect accepts, for a
    point the second index answers, has the sphere's scan entry in that index's global list or in the list of the cell the device
    arithmetic picks for the point.  At least 500 such pairs per case, unless the light shines from below."""
    c = FS.build_case(oracle, name)
    G2, sl = c.G2, c.slices["a"]
    pts = c.pts[sl]
    spheres = np.unique(c.aimed)
    sub = oracle.Scene(c.sc.spheres[spheres], c.sc.materials[spheres], c.sc.camera, c.sc.sun, c.sc.sky, c.sc.exposure_scale)
    rays = np.concatenate([pts, np.broadcast_to(c.ld.astype(F), pts.shape)], 1)
    acc = _accepted(oracle, sub, rays)
    inside = c.second[sl]
    cells, _, _ = S.device_cell(G2, pts)
    lists, _ = S.cell_lists(G2, cells)
    in_global = np.isin(G2.entry_of[spheres], G2.glob.astype(np.int64))
    checked = missing = 0
    for row, s in enumerate(spheres):
        hit = acc[row] & inside
        if not hit.any():
            continue
        checked += int(hit.sum())
        if not in_global[row]:
            missing += int((~(lists[hit] == G2.entry_of[s]).any(1)).sum())
    print("%s: %d accepted pairs checked, %d missing; second index %d x %d, global %d" % (name, checked, missing, G2.nx, G2.ny, len(G2.glob)))
    assert checked == int((acc & inside[None, :]).sum())
    if c.ld[1] >= 0:
        assert checked >= 500, (name, checked)
    assert missing == 0, "%s: %d accepted pairs are in no list walked for their point" % (name, missing)


# ------------------------------------------------------------------------------------------------ the GPU test's scene
FAR_W, FAR_H, FAR_SPP, FAR_DEPTH, FAR_SEED = 128, 64, 4, 6, 1


def far_scene_shadow_queries(oracle):
    """Every occlusion query of the oracle's render of the far scene: [n, 4] = origin, occluded."""
    sc = FS.far_scene(oracle, FAR_W, FAR_H)
    orc = oracle.Oracle()
    out = []
    try:
        orc.upload(sc)
        for j in range(FAR_H):
            for i in range(FAR_W):
                for s in range(1, 1 + FAR_SPP):
                    q, _ = orc.trace_path(FAR_W, FAR_H, i, j, s, FAR_DEPTH, FAR_SEED)
                    sh = q[q[:, 6] == 1.0]
                    if len(sh):
                        out.append(sh[:, [0, 1, 2, 7]])
    finally:
        orc.close()
    return sc, np.concatenate(out)


def test_far_scene_asks_far_shadow_questions(built, oracle):
    """The precondition of tests/test_far_shadow.py, from the oracle alone: of the shadow queries of its render (128 x 64, spp 4, depth
    6) at least 20 % start beyond the first index's radius, and at least 1 % of those are occluded by a sphere that is not the floor."""
    sc, q = far_scene_shadow_queries(oracle)
    G1 = FS.host_index_tier(sc, 1)
    pts = np.ascontiguousarray(q[:, :3], dtype=F)
    far = ~(S.dot3(pts, pts) <= G1.p0sq)
    ld = np.array(sc.lights[0].direction[:], dtype=F)
    orc = oracle.Oracle()
    try:
        orc.upload(oracle.Scene(sc.spheres[:-1], sc.materials[:-1], sc.camera, sc.sun, sc.sky, sc.exposure_scale))
        rays = np.concatenate([pts[far], np.broadcast_to(ld, pts[far].shape)], 1)
        by_small = orc.closest_hit(rays)[:, 1].view(np.int32) >= 0
    finally:
        orc.close()
    print("far scene: %d shadow queries, %d (%.1f %%) beyond P0 = %.4g, of those %d (%.1f %%) occluded by a sphere that is not the floor" % (
        len(q), int(far.sum()), 100.0 * far.mean(), np.sqrt(np.float64(G1.p0sq)), int(by_small.sum()), 100.0 * by_small.mean()))
    assert far.mean() >= 0.20 and by_small.mean() >= 0.01
    # ... and a few start beyond the second index as well (bounces that reach the floor farther out): the any-hit over every entry
    G2 = FS.host_index_tier(sc, 2)
    beyond = ~(S.dot3(pts, pts) <= G2.p0sq)
    print("far scene: %d shadow queries start beyond P2 = %.4g" % (int(beyond.sum()), np.sqrt(np.float64(G2.p0sq))))
    assert G2.enabled and 0 < beyond.sum() < 0.05 * len(pts)


# ------------------------------------------------------------------------------------------------ the launch plan's rule
def test_far_state_rule_passes_its_standalone_selftest(built):
    """host/far_state_selftest.cpp: lean for the stock scenes' shapes; far-hit state for a disabled index, a path list, per-path
    traversal counts and RT_FAR_STATE=1; and the rule's statement over 100,000 generated launches."""
    exe = os.path.join(ROOT, "cpuraytracer_amd", "lib", "far_state_selftest")
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "100000 generated cases" in p.stdout and "6 of 6 lean kernel functions chosen" in p.stdout and "far_state_selftest: ok" in p.stdout


def test_far_state_rule_over_the_recorded_launch_plan_cases(built):
    """rt_unit_far_state_plan over the cases of tests/launch_plan_cases.py, whose plans tests/golden/launch_plans.npz records: lean exactly
    when the recorded kernel is one of the lean list's, the launch is ordinary and the scene has a shadow index -- and never under a path
    list, traversal counts, RT_SHADOW_GRID=0 or RT_FAR_STATE=1.  The lean list is the flat LDS hit-stash rows of the variant list."""
    from cpuraytracer_amd import renderer
    lean_words = renderer.trace_lean_variants()
    rows = renderer.trace_variants()
    assert len(lean_words) == 3 and set(lean_words) <= set(rows)
    for w in rows:
        k = renderer.decode_kernel_word(w)
        assert (w in lean_words) == (k["kLds"] and k["kScan"] == 1 and k["kStash"] and not k["kCarry"]), k
    with np.load(os.path.join(ROOT, "tests", "golden", "launch_plans.npz")) as z:
        kernel, status = z["kernel"], z["status"]
    packed, _ = G.all_cases()
    assert len(packed) == len(kernel)
    idx = np.arange(0, len(packed), 7)
    n_lean = 0
    for i in idx:
        c = packed[i]
        family = status[i] == 0 and ((int(kernel[i]) & ~1) | (1 << 31)) in lean_words
        want = bool(family and c[G.W["mode"]] == 0 and (c[G.W["shape_flags"]] & G.SG))
        assert renderer.far_state_plan(c) == want, i
        n_lean += want
        if want:
            for kw in ({"path_list": True}, {"trav_out": True}, {"shadow_grid": False}, {"force_full": True}):
                assert not renderer.far_state_plan(c, **kw), (i, kw)
    assert n_lean >= 100, n_lean
    bad = G.pack([G.base_case(reserved=1)])[0]
    with pytest.raises(Exception):
        renderer.far_state_plan(bad)
