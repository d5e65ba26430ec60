"""Sphere lists of the primary rays (csrc/rt_tile_mask.h, rt_scan.h scan_tile_spheres): the scan of a tile's 64 fresh paths tests
every ray directly against the spheres listed for the tile, in place of the candidate words and the pooled resolve.

A list may only be LOOSER than the truth: every sphere with an accepted root for any primary ray of the tile must be listed.  That is
checked against the oracle (its ray generation, its Sphere::Intersect) on the host twin of the construction; the kernel is then
checked to give the same bits and counters with and without the lists, to build the host twin's lists, and to take the direct path."""
import ctypes as C

import numpy as np
import pytest

MASK_LIMIT, SPHERE_LIMIT = 16, 24  # the library's defaults (rt_tile_mask.h)
NONE = 0xFFFF


@pytest.fixture(scope="module")
def scenes_mod(built):
    from cpuraytracer_amd import scenes
    return scenes


def _camera_cases(scenes_mod):
    # the cameras of tests/test_primary_mask.py: widths that are no multiple of 64, so that tiles wrap the row ends
    return [("cover aperture 0.4", scenes_mod.build_scene("cover", 1, 1210, 800), 1210, 800),
            ("cover aperture 2.0", scenes_mod.build_scene("cover", 1, 1210, 800, aperture=2.0), 1210, 800),
            ("cover aperture 0", scenes_mod.build_scene("cover", 1, 1210, 800, aperture=0.0), 1210, 800),
            ("three (C1 camera)", scenes_mod.build_scene("three", 1, 200, 100), 200, 100)]


def _host_lists(sc, W, H, rs, sphere_limit=SPHERE_LIMIT, mask_limit=MASK_LIMIT):
    from cpuraytracer_amd import _capi
    L = _capi.load()
    cap = (W * L.rt_rowset_local_rows(rs)) >> 6
    lists = np.zeros((max(cap, 1), 64), dtype=np.uint16)
    eos = np.zeros(sc.n, dtype=np.uint32)
    n = C.c_uint32(0)
    cam = _capi.RtCamera.from_buffer_copy(bytes(sc.camera))
    _capi.check(L.rt_unit_tile_spheres_host(np.ascontiguousarray(sc.spheres).ctypes.data, sc.n, C.byref(cam), W, H, rs, mask_limit, sphere_limit,
                                            cap, C.byref(n), lists.ctypes.data, eos.ctypes.data))
    return lists[:n.value], eos


def _listed(lists):
    """[nTiles, nEntries] bool: the entry is in the tile's list (no row is set for a tile without a list)."""
    has = lists[:, 0] != NONE
    cnt = np.where(has, lists[:, 0], 0).astype(np.int64)
    table = np.zeros((len(lists), int(lists[:, 1:].max()) + 2 if len(lists) else 1), dtype=bool)
    for k in range(63):
        rows = np.nonzero(cnt > k)[0]
        table[rows, lists[rows, 1 + k]] = True
    return has, cnt, table


def _random_pairs(rng, rs, W, n_full, n):
    """n random (i, j, s) inside the full tiles of the strip, and their tiles."""
    pl = rng.integers(0, n_full * 64, n)
    lr, i = pl // W, pl % W
    lb = lr // rs.block_rows
    j = rs.first_row + (lb * rs.nshards + rs.shard) * rs.block_rows + (lr - lb * rs.block_rows)
    s = rng.integers(1, 1025, n)
    return np.stack([i, j, s], axis=1).astype(np.uint32), (pl >> 6).astype(np.int64)


def _violations(oracle, sc, W, H, ijs, tiles, lists, entry_of_sphere):
    """(ray, sphere) pairs for which the oracle's Sphere::Intersect accepts a root (a one-sphere scene through its list scan) and the
    sphere's entry is missing from the list of the ray's tile.  Returns (violations, accepted pairs checked)."""
    orc = oracle.Oracle()
    orc.upload(sc)
    rays = orc.primary_rays(W, H, ijs)  # the oracle's own jitter and lens point for (i, j, s)
    orc.close()
    has, _, table = _listed(lists)
    bad = checked = 0
    one = oracle.Oracle()
    for k in range(sc.n):
        single = oracle.Scene(sc.spheres[k:k + 1], sc.materials[k:k + 1], sc.camera, sc.sun, sc.sky, sc.exposure_scale)
        one.upload(single)
        hit = one.closest_hit(rays)[:, 1].view(np.int32) >= 0
        hit &= has[tiles]
        if hit.any():
            e = int(entry_of_sphere[k])
            ok = table[tiles[hit], e] if e < table.shape[1] else np.zeros(int(hit.sum()), dtype=bool)
            bad += int((~ok).sum())
            checked += int(hit.sum())
    one.close()
    return bad, checked


def test_host_lists_are_sound_against_the_oracle(built, oracle, scenes_mod):
    """200,000 random primary rays per camera (the oracle's ray generation; random pixels, samples and so lens points): every sphere the
    oracle's Sphere::Intersect accepts a root for is in the list of the ray's tile, for every tile that has one.  No violation."""
    from cpuraytracer_amd import _capi
    rng = np.random.default_rng(23)
    cases = _camera_cases(scenes_mod)
    for (label, sc, W, H), rs in ((cases[0], _capi.cyclic_rows(800, 1, 3)), (cases[1], _capi.cyclic_rows(800, 1, 3)),
                                  (cases[2], _capi.whole_image(800)), (cases[3], _capi.cyclic_rows(100, 1, 3)),
                                  (cases[0], _capi.whole_image(800)), (cases[1], _capi.cyclic_rows(800, 1, 2, block_rows=4))):
        label = "%s, rows %d/%d x %d" % (label, rs.shard, rs.nshards, rs.block_rows)
        lists, eos = _host_lists(sc, W, H, rs)
        assert len(lists) > 0, label
        has, cnt, _ = _listed(lists)
        ijs, tiles = _random_pairs(rng, rs, W, len(lists), 200000)
        bad, checked = _violations(oracle, sc, W, H, ijs, tiles, lists, eos)
        print("%s: %d accepted (ray, sphere) pairs, %d violations, %.1f %% of the tiles with a list, %.2f spheres per list"
              % (label, checked, bad, 100.0 * has.mean(), cnt[has].mean() if has.any() else 0.0))
        assert checked > 0 and bad == 0, label


def test_lists_hold_real_entries_in_order_and_cover_the_headline_picture(built, scenes_mod):
    """Not vacuous: on the cover scene at 1200x800 (the headline picture) at least half of the full tiles have a list at the default
    limit.  Entries ascend, are real spheres (no padding entry), and a looser limit only adds lists."""
    from cpuraytracer_amd import _capi
    W, H = 1200, 800
    sc = scenes_mod.build_scene("cover", 1, W, H)
    rs = _capi.whole_image(H)
    lists, eos = _host_lists(sc, W, H, rs)
    assert len(lists) == W * H // 64
    has, cnt, _ = _listed(lists)
    print("cover 1200x800: %.1f %% of the tiles with a list, spheres per list mean %.2f, max %d; histogram %s"
          % (100.0 * has.mean(), cnt[has].mean(), cnt[has].max(), np.bincount(cnt[has]).tolist()))
    assert has.mean() >= 0.5
    real = set(int(e) for e in eos)
    for t in np.nonzero(has)[0][::97]:
        ent = lists[t, 1:1 + cnt[t]].astype(np.int64)
        assert (np.diff(ent) > 0).all() and all(int(e) in real for e in ent)
    assert cnt[has].max() <= SPHERE_LIMIT
    loose, _ = _host_lists(sc, W, H, rs, sphere_limit=63)
    lhas, lcnt, _ = _listed(loose)
    assert (lhas | ~has).all() and np.array_equal(loose[has], lists[has])
    off, _ = _host_lists(sc, W, H, rs, sphere_limit=0)
    assert len(off) == 0


def _device_lists(hip, W, H, rs):
    from cpuraytracer_amd import _capi
    L = _capi.load()
    cap = (W * L.rt_rowset_local_rows(rs)) >> 6
    lists = np.zeros((max(cap, 1), 64), dtype=np.uint16)
    n = C.c_uint32(0)
    _capi.check(L.rt_unit_tile_spheres(hip._h, W, H, rs, cap, C.byref(n), lists.ctypes.data, None))
    return lists[:n.value]


def _scans(hip, W, H, rs):
    from cpuraytracer_amd import _capi
    L = _capi.load()
    n = C.c_uint32(0)
    scans = np.zeros(3, dtype=np.uint64)
    _capi.check(L.rt_unit_tile_spheres(hip._h, W, H, rs, 0, C.byref(n), None, scans.ctypes.data))
    return int(scans[0]), int(scans[1]), int(scans[2])


def _same_lists(dev, host):
    """Equal counts and equal entries up to each count (the slots behind a count are unspecified on the device)."""
    if dev.shape != host.shape or not np.array_equal(dev[:, 0], host[:, 0]):
        return False
    cnt = np.where(host[:, 0] != NONE, host[:, 0], 0).astype(np.int64)
    live = np.arange(63)[None, :] < cnt[:, None]
    return bool(np.array_equal(np.where(live, dev[:, 1:], 0), np.where(live, host[:, 1:], 0)))


@pytest.mark.gpu
def test_device_lists_equal_the_host_twins(hip, scenes_mod, monkeypatch):
    from cpuraytracer_amd import _capi
    monkeypatch.delenv("RT_PRIMARY_SPHERES", raising=False)
    monkeypatch.delenv("RT_PRIMARY_MASK_LIMIT", raising=False)
    for label, sc, W, H in _camera_cases(scenes_mod):
        for rs in (_capi.cyclic_rows(H, 1, 3), _capi.whole_image(H)):
            hip.upload(sc)
            dev = _device_lists(hip, W, H, rs)
            host, _ = _host_lists(sc, W, H, rs)
            assert len(host) > 0 and _same_lists(dev, host), "%s: host and device lists differ" % label


def _render(hip, W, H, spp, rs=None, seed=1):
    st = hip.render(W, H, 1, 1 + spp, 50, seed, rowset=rs)
    hip.resolve()
    h, l = hip.download()
    return h.tobytes(), l.tobytes(), st.traversals, st.segments


def _with_exact_ties(oracle, sc):
    """The scene with every eighth sphere's geometry copied over its successor's (the materials stay: the scene keeps its size and its
    flat layout): equal roots, so the closest hit -- and with it the material -- is decided by the original index in the key."""
    sph = sc.spheres.copy()
    src = np.arange(4, sc.n - 1, 8)
    sph[src + 1] = sph[src]
    return oracle.Scene(sph, sc.materials, sc.camera, sc.sun, sc.sky, sc.exposure_scale)


@pytest.mark.gpu
def test_images_and_counters_are_the_same_with_and_without_lists(hip, oracle, scenes_mod, monkeypatch):
    """RT_PRIMARY_SPHERES=0 and the default (read when an accumulation starts): equal HDR and LDR bytes and equal traversal counters;
    the kernel's count of directly resolved scans is 0 with the knob off and > 0 with it on."""
    from cpuraytracer_amd import _capi
    cases = [("cover 1200x800 spp 8", dict(W=1200, H=800, spp=8)),
             ("cover aperture 2.0", dict(W=640, H=400, spp=4, aperture=2.0)),
             ("cyclic row set", dict(W=500, H=300, spp=3, rows3=True)),
             ("partial last tile", dict(W=333, H=101, spp=3)),
             ("exact ties", dict(W=640, H=400, spp=4, ties=True))]
    for label, c in cases:
        W, H = c["W"], c["H"]
        sc = scenes_mod.build_scene("cover", 1, W, H, aperture=c.get("aperture", -1.0))
        if c.get("ties"):
            sc = _with_exact_ties(oracle, sc)
        rs = _capi.cyclic_rows(H, 2, 3) if c.get("rows3") else None
        got = {}
        for m in ("0", None, "63"):
            if m is None:
                monkeypatch.delenv("RT_PRIMARY_SPHERES", raising=False)
            else:
                monkeypatch.setenv("RT_PRIMARY_SPHERES", m)
            hip.upload(sc)
            got[m] = _render(hip, W, H, c["spp"], rs)
            total, masked, direct = _scans(hip, W, H, rs if rs is not None else _capi.whole_image(H))
            print("%s, RT_PRIMARY_SPHERES=%s: %d scans of fresh paths, %d with a tile's tables, %d direct" % (label, m, total, masked, direct))
            assert (direct == 0) if m == "0" else (0 < direct <= masked), (label, m, total, masked, direct)
        for m in (None, "63"):
            assert got["0"][0] == got[m][0], "%s: HDR differs (%s)" % (label, m)
            assert got["0"][1] == got[m][1], "%s: LDR differs (%s)" % (label, m)
            assert got["0"][2:] == got[m][2:], "%s: traversal counters differ (%s)" % (label, m)


@pytest.mark.gpu
def test_c2_primary_scans_take_the_direct_path(hip, scenes_mod, monkeypatch):
    """The headline workload (cover, 1200x800, spp 128) by the kernel's own count: at least half of the scans of 64 fresh paths are
    resolved from a sphere list (the share of tiles that have one, see the host test), none with the knob off."""
    from cpuraytracer_amd import _capi
    W, H, spp = 1200, 800, 128
    sc = scenes_mod.build_scene("cover", 1, W, H)
    for m in ("0", None):
        if m is None:
            monkeypatch.delenv("RT_PRIMARY_SPHERES", raising=False)
        else:
            monkeypatch.setenv("RT_PRIMARY_SPHERES", m)
        hip.upload(sc)
        hip.render(W, H, 1, 1 + spp, 50, 1)
        total, masked, direct = _scans(hip, W, H, _capi.whole_image(H))
        print("c2, RT_PRIMARY_SPHERES=%s: %d scans of 64 fresh paths, %d with a tile's tables, %d direct (%.2f %%)"
              % (m, total, masked, direct, 100.0 * direct / max(1, total)))
        assert total == W * H * spp // 64
        assert (direct == 0) if m == "0" else (direct >= 0.5 * total)
