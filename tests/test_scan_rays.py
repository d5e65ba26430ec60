"""The closest-hit scans as shipped (csrc/rt_scan.h through rt_unit_closest_hit, which launches the scan variant rt_render uses for the
uploaded scene) on the DIRECTED rays of tests/scan_cases.py: silhouette grazers, surface starters, the behind rule, near-equal
roots, exact ties, degenerate directions, crowded waves.  One test per scene case, a fresh context under the case's knobs; every
record equals the oracle's list scan bit for bit -- t, index, position, normal, uv of every ray, no tolerance -- in the order given,
in a seeded random order and reversed.  tests/test_scan_rays_cpu.py shows on the oracle alone that the rays reach what they aim at."""
import functools
import re

import numpy as np
import pytest

import scan_cases as G
from test_primary_tables_fuzz import assert_same, bits

pytestmark = pytest.mark.gpu

F = np.float32
CASES = [c.name for c in G.scene_cases()]
SCAN_NAMES = {(False, 3): "cell grid, tables in global memory", (False, 2): "hierarchy, tables in global memory", (True, 1): "flat scan in LDS",
              (True, 0): "VALU scan, tables in LDS", (False, 0): "VALU scan, tables in global memory"}
LAUNCH_LINE = re.compile(r"rt_trace launch: tree=(\d+) flat=(\d+) ldsTables=(\d+) blocks=\d+ threads=\d+ lds=\d+ B \(cand \d+, tables \d+, leaf \d+, ops \d+, sg \d+, tree (\d+),")


@functools.lru_cache(maxsize=None)
def reference(oracle, name):
    """(rays, index of the first crowded wave, the oracle's list scan of them) of a case's scene: computed once, never written to."""
    rays, crowded_at = G.all_rays(oracle, name)
    orc = oracle.Oracle()
    try:
        orc.upload(G.scene(oracle, name))
        want = orc.closest_hit(rays, oracle.ACCEL_LIST)
    finally:
        orc.close()
    rays.setflags(write=False)
    want.setflags(write=False)
    return rays, crowded_at, want


def scans_reported(stderr_text):
    """((kLds, kScan), bytes of the hierarchy's bounds in LDS) of every launch in the RT_VERBOSE lines: the launcher's own account of
    the scan it chose for the context's scene and settings (host/rt_launch_plan.cpp ChooseScan, which the scan-only launch of
    rt_unit_closest_hit asks as well: PlanScanOnly).  `flat` is flat + 2 grid + 4 grid with its tables in LDS."""
    out = []
    for mt in LAUNCH_LINE.finditer(stderr_text):
        tree, flat, lds_tables, tree_bytes = (int(mt.group(k)) for k in range(1, 5))
        if flat & 2:
            scan = (False, 3)
        elif tree:
            scan = (False, 2)
        else:
            scan = (bool(lds_tables), 1 if flat & 1 else 0)
        out.append((scan, tree_bytes))
    return out


def class_report(oracle, name, crowded_at, rays, got, want):
    """which classes the differing rays belong to, and the first of them: its six floats, both records"""
    bad = np.nonzero((bits(got) != bits(want)).any(axis=1))[0]
    R = G.rays(oracle, name)
    bounds, at = [], 0
    for label, v in R.classes.items():
        if label == "crowded":
            continue
        bounds.append((label, at, at + len(v)))
        at += len(v)
    bounds += [("padding", at, crowded_at), ("crowded", crowded_at, crowded_at + len(R.classes["crowded"])), ("random", crowded_at + len(R.classes["crowded"]), len(rays))]
    per = {label: int(((bad >= a) & (bad < b)).sum()) for label, a, b in bounds}
    k = int(bad[0])
    return "%d of %d rays differ %r; first: ray %d %r (hex %s): device %r, oracle %r" % (
        len(bad), len(rays), {k_: v for k_, v in per.items() if v}, k, rays[k].tolist(), [hex(x) for x in bits(rays[k])], got[k].tolist(), want[k].tolist())


def assert_records(oracle, name, crowded_at, rays, got, want, what):
    if not np.array_equal(bits(got), bits(want)):
        raise AssertionError("%s, %s: %s" % (name, what, class_report(oracle, name, crowded_at, rays, got, want)))


@pytest.mark.parametrize("name", CASES)
def test_directed_rays_through_the_production_scan(oracle, monkeypatch, capfd, name):
    """A fresh context under the case's knobs.  The plan of the scan-only launch (rt_unit_launch_plan word [26]) names the scan variant
    the case is meant for, and the context's launcher reports the same scan for its trace launch (a scene that takes another scan
    fails here, it is not skipped), with the hierarchy's bounds in LDS or, RT_TREE_LDS=0, not.  Then all ten floats of every ray
    against the oracle's list scan: as given (a count that is no multiple of 256 or 64: dead lanes, a partial block), in a seeded
    random order and reversed -- a ray's answer depends neither on its lane nor on its neighbours (pooled lists, ds_bpermute hand-offs,
    drains) --, and launches of 1, 63, 64 and 65 rays cut from the crowded waves."""
    from cpuraytracer_amd import HipRenderer
    c = G.case(name)
    sc = G.scene(oracle, name)
    rays, crowded_at, want = reference(oracle, name)
    assert len(rays) % 256 != 0 and len(rays) % 64 != 0
    for key, value in c.env.items():
        monkeypatch.setenv(key, value)
    monkeypatch.setenv("RT_VERBOSE", "1")
    assert G.layout_info(sc.spheres)[0] == c.kind, "%s is not laid out for the scan it is meant for" % name
    # the scan-only launch's own plan (rt_unit_launch_plan word [26]: PlanScanOnly, which LaunchClosest asks) ...
    scan, tree_in_lds, instantiated = G.planned_scan(sc, c.env)
    assert instantiated and scan == c.variant, "%s: the scan-only launch is planned as the %s, not the %s" % (name, SCAN_NAMES.get(scan, scan), SCAN_NAMES[c.variant])
    assert tree_in_lds == (c.variant == (False, 2) and c.env.get("RT_TREE_LDS") != "0"), name
    r = HipRenderer(0)  # the knobs are read when a context is created
    try:
        r.upload(sc)
        # ... and what the context itself, with its own reading of the knobs and of the uploaded scene, reports for a launch
        capfd.readouterr()
        r.unit_trace(16, 8, np.array([[3, 2, 1], [12, 5, 2]], dtype=np.uint32), 2, 5)
        taken = scans_reported(capfd.readouterr().err)
        assert taken, "the launcher did not report its launch"
        for scan, tree_bytes in taken:
            assert scan == c.variant, "%s took the %s, not the %s" % (name, SCAN_NAMES[scan], SCAN_NAMES[c.variant])
            if c.variant == (False, 2):
                assert (tree_bytes == 0) == (c.env.get("RT_TREE_LDS") == "0"), (name, tree_bytes)
        assert_records(oracle, name, crowded_at, rays, r.unit_closest_hit(rays), want, "rays as given")
        perm = np.random.default_rng(c.spec["seed"] + 7).permutation(len(rays))
        got = np.empty_like(want)
        got[perm] = r.unit_closest_hit(rays[perm])
        assert_records(oracle, name, crowded_at, rays, got, want, "rays in a random order")
        got = r.unit_closest_hit(rays[::-1])[::-1]
        assert_records(oracle, name, crowded_at, rays, got, want, "rays reversed")
        for count, start in ((1, crowded_at + 5), (63, crowded_at), (64, crowded_at), (65, crowded_at + 33)):
            assert_same(r.unit_closest_hit(rays[start:start + count]), want[start:start + count], "%s: a launch of %d rays" % (name, count))
    finally:
        r.close()
    hit = want[:, 1].copy().view(np.int32) >= 0
    print("%s: %d rays, %d hits, scan: %s" % (name, len(rays), hit.sum(), SCAN_NAMES[c.variant]))


@pytest.mark.parametrize("name", [c.name for c in G.scene_cases() if c.image])
def test_the_trace_kernels_agree_on_these_scenes(oracle, monkeypatch, name):
    """One flat, one hierarchy and one cell-grid scene through the production trace kernels, whose bounces are surface starters: 3,000
    traced samples at depth 6 and a 160 x 100 image at 2 spp, depth 6, equal the oracle's bits and traversal counts -- the unit entry
    and the megakernel agree on these scenes."""
    from cpuraytracer_amd import HipRenderer
    c = G.case(name)
    sc = G.scene(oracle, name)
    W, H, m = 160, 100, 3000
    rng = np.random.default_rng(c.spec["seed"] + 11)
    ijs = np.stack([rng.integers(0, W, m), rng.integers(0, H, m), rng.integers(1, 600, m)], 1).astype(np.uint32)
    orc = oracle.Oracle()
    try:
        orc.upload(sc)
        ro, to = orc.trace(W, H, ijs, 6, 77, accel=oracle.ACCEL_PADDED_LIST)
        so = orc.render(W, H, 1, 3, 6, 9, accel=oracle.ACCEL_PADDED_LIST, threads=8)
        ho, _ = orc.download()
    finally:
        orc.close()
    for key, value in c.env.items():
        monkeypatch.setenv(key, value)
    r = HipRenderer(0)
    try:
        r.upload(sc)
        rg, tg = r.unit_trace(W, H, ijs, 6, 77)
        assert_same(rg, ro, "%s: per-sample radiance, depth 6" % name)
        assert np.array_equal(tg, to), "%s: traversal counts" % name
        sg = r.render(W, H, 1, 3, 6, 9)
        hg, _ = r.download(ldr=False)
        assert_same(hg, ho, "%s: whole image HDR" % name)
        assert (sg.traversals, sg.segments) == (so.traversals, so.segments), name
    finally:
        r.close()
    print("%s: %d traversals over %d segments in the image, %.1f per sample in the traced samples" % (name, so.traversals, so.segments, float(to.mean())))
