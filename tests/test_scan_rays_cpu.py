"""The generator of tests/test_scan_rays.py is honest (no GPU; the oracle and the layout queries alone): the directed rays of
tests/scan_cases.py reach what they are aimed at, counted per scene and printed.  A count that falls short is the generator's to fix,
never the threshold's."""
import functools

import numpy as np
import pytest

import scan_cases as G
from test_primary_tables_fuzz import bits

F = np.float32
SCENES = G.scene_names()
TIE_SCENES = [c.name for c in G.scene_cases() if c.spec["ties"] and not c.name.startswith("valu")]


@functools.lru_cache(maxsize=None)
def full_hits(oracle, name):
    """the oracle's list scan over every class of the scene, in class order (computed once, never written to)"""
    orc = oracle.Oracle()
    try:
        orc.upload(G.scene(oracle, name))
        out = orc.closest_hit(G.rays(oracle, name).all(), oracle.ACCEL_LIST)
    finally:
        orc.close()
    out.setflags(write=False)
    return out


def index_of(hits):
    return hits[:, 1].copy().view(np.int32)


def class_hits(oracle, name, label):
    return full_hits(oracle, name)[G.rays(oracle, name).slice_of(label)]


def test_the_cases_cover_the_sizes_knobs_and_scan_variants(oracle):
    cases = G.scene_cases()
    assert len(cases) == 12
    assert sorted(c.spec["n"] for c in cases if c.spec["layout"] == "box" and not c.name.startswith("valu")) == [5, 37, 64, 509, 512, 513]
    assert {c.variant for c in cases} == {(False, 3), (False, 2), (True, 1), (True, 0), (False, 0)}  # RT_SCAN_VARIANTS, all five
    assert sorted(c.spec["layout"] for c in cases if c.spec["ties"] and not c.name.startswith("valu")) == ["box", "layer", "soup"]
    for c in cases:
        sc = G.scene(oracle, c.name)
        assert sc.n == c.spec["n"]
        with G.environment(c.env):
            assert G.layout_info(sc.spheres)[0] == c.kind, "%s is not laid out for the scan it is meant for" % c.name
            scan, tree_in_lds, instantiated = G.planned_scan(sc, c.env)
            assert scan == c.variant and instantiated, "%s: the plan of the scan-only launch is %r" % (c.name, scan)
            assert tree_in_lds == (c.variant == (False, 2) and c.env.get("RT_TREE_LDS") != "0"), c.name
        if c.spec["negative"]:
            assert (sc.spheres["r"] < 0).sum() >= sc.n // 5
    r = G.radii(G.scene(oracle, "flat512_negative_scale_1e3"))
    assert r.max() / np.sort(r)[8] >= 500.0  # three decades (the bias spheres, absolute, lie far below)


@pytest.mark.parametrize("name", SCENES)
def test_every_ray_is_finite_and_no_class_is_empty(oracle, name):
    R = G.rays(oracle, name)
    sc = G.scene(oracle, name)
    want = {"grazers", "starters", "behind", "near", "degenerate", "crowded"} | ({"ties"} if sc.meta["dups"] else set())
    assert set(R.classes) == want
    sizes = {k: len(v) for k, v in R.classes.items()}
    rays, crowded_at = G.all_rays(oracle, name)
    print(name, sizes, "in all", len(rays))
    assert all(v >= 500 for v in sizes.values())
    assert np.isfinite(rays).all() and (np.abs(rays[:, 3:]).max(axis=1) > 0).all()
    assert 20000 <= len(rays) <= 40000 and len(rays) % 64 != 0 and crowded_at % 64 == 0
    # degenerate directions: every kind of origin, hits among them
    kinds = np.bincount(R.meta["degenerate"]["kind"], minlength=5)
    hit = index_of(class_hits(oracle, name, "degenerate")) >= 0
    print(name, "degenerate: origins outside / inside / on a face / on a cell border / one zero component", kinds.tolist(), "hits", int(hit.sum()))
    assert (kinds >= 100).all() and hit.sum() >= 300


@pytest.mark.parametrize("name", SCENES)
def test_behind_rule_rays_start_as_close_to_a_bound_as_its_members_allow(oracle, name):
    """The bounds of rt_unit_layout carry the filter's margin: the members of a group end mu Rf short of its surface (printed: the
    smallest mu of the 40 tightest groups is 1e-3 to 7e-3, and 0.99 at the 2e4 offset, where the margin K eps |C|^2 dwarfs the group).
    A ray whose normalised b = d.(o - C) / |o - C| is at most 1e-2 reaches only what lies within b^2 / 2 = 5e-5 of its own distance from
    C, so from (1 + delta) Rf it can hit a member only if delta <= -(mu - 5e-5): every ray with delta > -0.9 mu -- the shell rays at
    delta = +-[1e-7, 1e-2] with at least 50 per decade and side, origins outside heading away among them -- must NOT hit its group
    (asserted), and the inside decades 1e-7 .. 1e-3 of delta cannot hold a hit.  What can: the edge rays, which start a fraction e of
    the members' reach below that reach; per decade of e in [1e-7, 1e-2] at least 50 of them hit the aimed group, heading in and
    heading out at least 15 each -- down to the floor that the bias and binary32 set (computed below, printed)."""
    R = G.rays(oracle, name)
    m = R.meta["behind"]
    group_of = _groups(oracle, name)[0]
    idx = index_of(class_hits(oracle, name, "behind"))
    in_group = (idx >= 0) & (group_of[np.maximum(idx, 0)] == m["group"])
    beta, delta, mu, edge = m["beta"], m["delta"], m["mu"], m["edge"]
    print("%s behind: %d rays, mu of the aimed groups %.2e .. %.2e; hits in the aimed group: edge %d of %d, shell %d of %d" % (
        name, len(idx), mu.min(), mu.max(), (in_group & edge).sum(), edge.sum(), (in_group & ~edge).sum(), (~edge).sum()))
    assert (mu > 0).all()
    cannot = delta > -0.9 * mu
    assert (in_group & cannot).sum() == 0, "a ray this flat hit a member from beyond the members' reach"
    lg = np.log10(np.abs(delta))
    for side in (-1.0, 1.0):
        for lo in range(-7, -2):
            sel = ~edge & (np.sign(delta) == side) & (lg >= lo - 1e-3) & (lg < lo + 1 + 1e-3)
            print("%s behind shell delta %+d x [1e%d, 1e%d): %d rays, %d cannot hit" % (name, side, lo, lo + 1, sel.sum(), (sel & cannot).sum()))
            assert sel.sum() >= 50
    # how close can a hit start?  The root must exceed the bias, an absolute length: s >= 0.00033 (|d| = 0.3) along a tangent leaves
    # s^2 / (2 reach^2) of the reach behind; and binary32 holds the origin to an ulp of its coordinates (for the group of median reach).
    below = m["below"]
    rays = R.classes["behind"]
    typical = float(np.median(m["reach"]))
    floor = max(0.00033 ** 2 / (2.0 * typical ** 2), float(np.spacing(np.abs(rays[:, :3]).max())) / typical)
    with np.errstate(invalid="ignore", divide="ignore"):
        le = np.log10(below)
    asked = 0
    for lo in range(-7, -2):
        sel = edge & in_group & (below > 0) & (le >= lo) & (le < lo + 1)
        ask = 10.0 ** lo >= floor
        asked += ask
        print("%s behind edge, origin [1e%d, 1e%d) of the reach below it: %d hits in the aimed group (heading in %d, heading out %d)%s" % (
            name, lo, lo + 1, sel.sum(), (sel & (beta < 0)).sum(), (sel & (beta > 0)).sum(), "" if ask else " -- below the floor %.1e, not asked" % floor))
        if ask:
            assert sel.sum() >= 50 and (sel & (beta < 0)).sum() >= 15 and (sel & (beta > 0)).sum() >= 15
    assert (in_group & edge).sum() >= 300 and (in_group & edge & (beta > 0)).sum() >= 100
    assert asked >= 4 or name in ("flat37_negative_scale_1e-3", "flat64_offset_2e4"), "only the tiny scene and the far one have a floor above 1e-7"


@functools.lru_cache(maxsize=None)
def _groups(oracle, name):
    with G.environment(G.case(name).env):
        return G.group_bounds(G.scene(oracle, name))


@pytest.mark.parametrize("name", SCENES)
def test_grazers_fall_on_both_sides_of_the_silhouette(oracle, name):
    """Per decade of |delta| and per side, at least 100 rays whose root the oracle accepts for the grazed sphere and 100 it rejects
    (near origins decide by the side; from 300 and 3,000 extents away binary32 decides); within |delta| <= 1e-6 both outcomes at
    least 50 times; the grazed sphere is the scene's closest hit for at least half of the accepted rays."""
    R = G.rays(oracle, name)
    sc = G.scene(oracle, name)
    m = R.meta["grazers"]
    own = G.own_sphere_hits(oracle, sc, m["sphere"], R.classes["grazers"])
    acc = index_of(own) >= 0
    lg = np.log10(np.abs(m["delta"]))
    for side in (-1.0, 1.0):
        for lo in range(-8, -1):
            sel = (np.sign(m["delta"]) == side) & (lg >= lo) & (lg < lo + 1)
            a, r = int((sel & acc).sum()), int((sel & ~acc).sum())
            print("%s grazers delta %+d x [1e%d, 1e%d): accepted %d rejected %d" % (name, side, lo, lo + 1, a, r))
            assert a >= 100 and r >= 100
    tiny = np.abs(m["delta"]) <= 1e-6
    assert (tiny & acc).sum() >= 50 and (tiny & ~acc).sum() >= 50
    full = index_of(class_hits(oracle, name, "grazers"))
    closest = acc & (full == m["sphere"])
    print("%s grazers: %d accepted, the grazed sphere is the closest hit of %d" % (name, acc.sum(), closest.sum()))
    assert closest.sum() * 2 >= acc.sum()


def _roots64(sc, sphere, rays):
    """both roots of each ray against its sphere in binary64 (of the binary32 inputs); NaN without a real root"""
    c, r = G.centres(sc)[sphere], G.radii(sc)[sphere]
    o, d = rays[:, :3].astype(np.float64), rays[:, 3:].astype(np.float64)
    oc = o - c
    a, b, cq = (d * d).sum(1), (oc * d).sum(1), (oc * oc).sum(1) - r * r
    with np.errstate(invalid="ignore"):
        sq = np.sqrt(b * b - a * cq)
    return (-b - sq) / a, (-b + sq) / a


@pytest.mark.parametrize("name", SCENES)
def test_surface_starters_reach_the_bias_and_the_second_root(oracle, name):
    """At least 200 rays whose accepted root is the second one.  Where the scene has spheres of radius 5e-4 .. 4e-3 (every scene but
    flat5, whose five spheres are the pairs): the second root of the chords lies within 8 ulp of 0.001 -- measured in binary64 on the
    rounded ray -- and the oracle accepts it at least 50 times and rejects it at least 50 times."""
    R = G.rays(oracle, name)
    sc = G.scene(oracle, name)
    m = R.meta["starters"]
    rays = R.classes["starters"]
    own = G.own_sphere_hits(oracle, sc, m["sphere"], rays)
    acc = index_of(own) >= 0
    t1, t2 = _roots64(sc, m["sphere"], rays)
    t = own[:, 0].astype(np.float64)
    second = acc & (np.abs(t - t2) < np.abs(t - t1))
    ulp = float(np.spacing(G.BIAS))
    near_bias = np.zeros(len(rays), dtype=bool)
    near_bias[m["n_generic"]:] = np.abs(t2[m["n_generic"]:] - float(G.BIAS)) <= 8.0 * ulp
    below_bias = G.radii(sc)[m["sphere"]] * 2.0 < float(G.BIAS)
    print("%s starters: %d rays, second root taken %d; second root within 8 ulp of the bias: accepted %d rejected %d; on spheres with a diameter below the bias %d (accepted %d)" % (
        name, len(rays), second.sum(), (near_bias & acc).sum(), (near_bias & ~acc).sum(), below_bias.sum(), (below_bias & acc).sum()))
    assert second.sum() >= 200
    if name != "flat5":
        assert len(m["target"]) >= 500
        assert (near_bias & acc).sum() >= 50 and (near_bias & ~acc).sum() >= 50
        assert below_bias.sum() >= 50


@pytest.mark.parametrize("name", TIE_SCENES)
def test_ties_are_exact_and_go_to_the_lower_index(oracle, name):
    """At least 300 rays of the tie class have a second sphere at the closest hit's t, bit for bit: the oracle's closest hit over the
    scene MINUS the winner has the same t bits.  The winner is then the lower original index; the tie makers' two members lie in
    different groups (cells, for the grid) of the layout."""
    R = G.rays(oracle, name)
    sc = G.scene(oracle, name)
    rays = R.classes["ties"]
    m = R.meta["ties"]
    full = class_hits(oracle, name, "ties")
    win = index_of(full)
    ours = (win == m["first"]) | (win == m["second"])
    tied = np.zeros(len(rays), dtype=bool)
    other = np.full(len(rays), -1)
    orc = oracle.Oracle()
    try:
        for k in np.unique(win[ours]):
            sel = np.nonzero(ours & (win == k))[0]
            orc.upload(G.without(oracle, sc, int(k)))
            h = orc.closest_hit(rays[sel], oracle.ACCEL_LIST)
            i2 = index_of(h)
            i2 = np.where(i2 >= k, i2 + 1, i2)  # back to the whole scene's numbering
            same = (i2 >= 0) & (bits(h[:, 0]) == bits(full[sel, 0]))
            tied[sel], other[sel] = same, np.where(same, i2, -1)
    finally:
        orc.close()
    n_dup = sum(len(rays[m["first"] == a]) for a, _ in sc.meta["dups"])
    dup_ties, mirror_ties = int(tied[:n_dup].sum()), int(tied[n_dup:].sum())
    print("%s ties: %d rays, the tie maker wins %d, exact ties %d (duplicates %d, mirror pairs %d)" % (name, len(rays), ours.sum(), tied.sum(), dup_ties, mirror_ties))
    assert tied.sum() >= 300 and dup_ties >= 100 and mirror_ties >= 100
    assert (win[tied] < other[tied]).all(), "the list scan keeps the lower index on equal t"
    assert np.array_equal(np.minimum(win[tied], other[tied]), m["first"][tied]) and np.array_equal(np.maximum(win[tied], other[tied]), m["second"][tied])
    assert (m["second"] - m["first"]).min() >= min(sc.n // 2, 400), "the members of a tie lie far apart in the list"
    group_of = _groups(oracle, name)[0]
    with G.environment(G.case(name).env):
        g = G.grid_info(sc.spheres)
    where = g[7] if g is not None else group_of
    apart = sum(1 for a, b in sc.meta["dups"] if group_of[a] != group_of[b])  # (a copy lies where its original does: often one group)
    apart_mirror = sum(1 for a, b in sc.meta["mirrors"] if group_of[a] != group_of[b] and where[a] != where[b])
    print("%s ties: %d of %d duplicates and %d of %d mirror pairs span two groups%s" % (
        name, apart, len(sc.meta["dups"]), apart_mirror, len(sc.meta["mirrors"]), " and two cells" if g is not None else ""))
    assert apart_mirror * 2 >= len(sc.meta["mirrors"])


@pytest.mark.parametrize("name", SCENES)
def test_near_equal_roots_come_in_both_orders(oracle, name):
    """The rays sorted by the gap the oracle's own roots have, k = round(-log2 |t_B / t_A - 1|): for every k = 9 .. 24 (a gap of one
    ulp is k = 23 or 24) the scene's closest hit is the nearer of the pair with B nearer and with A nearer, and with the winner
    earlier in the list than the loser and later, at least 20 times each -- in every scene, the one at (2e4, -1e4, 1.5e4) and the one
    of scale 1e-3 included: the generator aims the DIRECTION (a free binary32 vector) from the origin as binary32 holds it, and keeps
    of its candidates what the oracle's roots measure."""
    R = G.rays(oracle, name)
    sc = G.scene(oracle, name)
    m = R.meta["near"]
    rays = R.classes["near"]
    ha, hb = G.own_sphere_hits(oracle, sc, m["a"], rays), G.own_sphere_hits(oracle, sc, m["b"], rays)
    both = (index_of(ha) >= 0) & (index_of(hb) >= 0)
    ta, tb = ha[:, 0].astype(np.float64), hb[:, 0].astype(np.float64)
    with np.errstate(all="ignore"):
        kk = np.where(both & (ta != tb), np.rint(-np.log2(np.abs(tb / ta - 1.0))), -1).astype(np.int64)
    win = index_of(class_hits(oracle, name, "near"))
    print("%s near: %d rays, both spheres hit %d, exact ties %d, gaps beyond 2^-9 %d" % (name, len(rays), both.sum(), (both & (ta == tb)).sum(), (both & (kk >= 0) & (kk < 9)).sum()))
    short = []
    for k in G.EPS_K:
        sel = kk == k
        row = []
        for b_nearer in (True, False):
            near_one, far_one = (m["b"], m["a"]) if b_nearer else (m["a"], m["b"])
            for early in (True, False):
                row.append(int((sel & ((tb < ta) == b_nearer) & (win == near_one) & ((near_one < far_one) == early)).sum()))
        print("%s near 2^-%d: %d rays aimed, %d measured; B nearer and (earlier, later) in the list %d %d, A nearer and (earlier, later) %d %d" % (
            name, k, (m["k"] == k).sum(), sel.sum(), row[0], row[1], row[2], row[3]))
        if min(row) < 20:
            short.append((k, row))
    assert not short, short


@pytest.mark.parametrize("name", SCENES)
def test_crowded_waves_overflow_the_group_pool(oracle, name):
    """Every scene in which a line can cross more than 10 bounds (all but the two smallest): at least 8 of the crowded waves cross more than 640 group bounds with their 64 rays together (the
    flat scan's pool of (ray, group) items per pass), counted on the bounds of rt_unit_layout in binary64; the waves after them miss
    everything but for their one crowded ray."""
    R = G.rays(oracle, name)
    rays = R.classes["crowded"]
    _, Cg, Rf, _ = _groups(oracle, name)
    o, d = rays[:, :3].astype(np.float64), rays[:, 3:].astype(np.float64)
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    oc = Cg[None, :, :] - o[:, None, :]
    s = np.maximum((oc * d[:, None, :]).sum(2), 0.0)  # the half-line's closest point
    dist2 = ((oc - s[:, :, None] * d[:, None, :]) ** 2).sum(2)
    crossed = (dist2 < (Rf * Rf)[None, :]).sum(1)
    starts = R.meta["crowded"]["crowded"]
    per_wave = np.array([crossed[a:a + 64].sum() for a in starts])
    idx = index_of(class_hits(oracle, name, "crowded"))
    lone = np.array([(idx[a + 128:a + 192] >= 0).sum() for a in starts])
    print("%s crowded: %d groups; bounds crossed per crowded wave %s; hits per crowded wave %s" % (
        name, len(Rf), per_wave.tolist(), [int((idx[a:a + 64] >= 0).sum()) for a in starts]))
    assert all((idx[a + 64:a + 128] < 0).all() for a in starts) and (lone <= 1).all()
    # can a wave of this scene overflow the pool at all?  Only if some line crosses more than 10 of its bounds: 4,000 random lines
    # through the scene (flat5 has 8 bounds; the 16 of the 37-sphere scene lie apart, no line crosses more than a few of them)
    sc = G.scene(oracle, name)
    rng = np.random.default_rng(5)
    p = sc.meta["centre"] + rng.uniform(-0.6, 0.6, (4000, 3)) * sc.meta["extent"]
    u = rng.normal(size=(4000, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    pc = Cg[None, :, :] - p[:, None, :]
    miss2 = (pc * pc).sum(2) - ((pc * u[:, None, :]).sum(2)) ** 2
    most = int((miss2 < (Rf * Rf)[None, :]).sum(1).max())
    print("%s crowded: the best of 4,000 random lines crosses %d bounds" % (name, most))
    if most > 10:
        assert (per_wave > 640).sum() >= 8
    else:
        assert name in ("flat5", "flat37_negative_scale_1e-3")
    if len(Rf) >= 100:  # the scenes with a row of spheres (or the layer): the one crowded ray of an idle wave hits it
        assert lone.sum() >= 6


@pytest.mark.parametrize("name", ["flat509_ties", "hierarchy1500_floor_ties"])
def test_list_scan_equals_the_bvh_traversal_on_every_ray(oracle, name):
    """The oracle's list scan against its BvhNode traversal on ALL rays of two scenes (neither has a negative radius: the reference's
    boxes take the radius as their extent), ties included, under the reference's tie rule (exact ties go to the right child).  Rays
    that differ by that rule alone -- the same t bits, another index -- are counted and must not exceed the tie class.

    What else differs is what tests/test_reference_code_cpu.py knows as a slab-test loss: from an origin hundreds of extents away the
    binary32 discriminant of the list scan exceeds r^2 and "hits" a sphere whose box the exact ray does not enter, and the tree
    rightly never visits it (its result is then a miss or a farther sphere).  Each such ray must pass that file's test of a loss
    (`classify_bvh`: the binary64 ray misses the winner's box shrunk by 1e-6 of the coordinates), and none may start within 20 extents
    of the scene: there the two scans are equal on every ray but the ties.  Measured, of 37,413 rays each: flat509_ties 611 ties and
    3,364 losses, hierarchy1500_floor_ties 873 ties and 5,783 losses (grazers from 300 and 3,000 extents away); 0 unexplained."""
    from test_reference_code_cpu import classify_bvh
    rays, _ = G.all_rays(oracle, name)
    sc = G.scene(oracle, name)
    orc = oracle.Oracle()
    try:
        orc.upload(sc)
        hl = orc.closest_hit(rays, oracle.ACCEL_LIST)
        hb = orc.closest_hit(rays, oracle.ACCEL_BVH)
    finally:
        orc.close()
    equal, tie, lost, unexplained = classify_bvh(hl, hb, rays, sc.spheres)
    far = np.linalg.norm(rays[:, :3].astype(np.float64) - sc.meta["centre"], axis=1) > 20.0 * sc.meta["extent"]
    n_tie_rays = len(G.rays(oracle, name).classes["ties"])
    print("%s: %d rays (%d from beyond 20 extents); BvhNode equals the list on %d, differs by the tie rule alone on %d (tie class: %d rays), "
          "slab-test losses %d (%d of them from within 20 extents), unexplained %d" % (
              name, len(rays), far.sum(), equal.sum(), tie.sum(), n_tie_rays, lost.sum(), (lost & ~far).sum(), unexplained.sum()))
    assert unexplained.sum() == 0
    assert (index_of(hl)[tie] < index_of(hb)[tie]).all(), "the list keeps the lower index"
    assert tie.sum() <= n_tie_rays
    assert (lost & ~far).sum() == 0
