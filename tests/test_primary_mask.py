"""Tile masks of the primary rays (csrc/rt_tile_mask.h): the flat scan of a tile's 64 fresh paths takes its candidate groups from a
per-tile mask instead of running the matrix-core filter.

A mask may only be LOOSER than the truth: every group that holds a sphere with an accepted root for any primary ray of the tile must
have its bit set.  That is checked against the oracle (its ray generation, its Sphere::Intersect), not against the kernel; the
kernel is then checked to give the same bits with and without the masks, and to take the masked path at all."""
import ctypes as C

import numpy as np
import pytest

KBASE = (0, 64, 16, 80)  # rt_scan.h: bit N from the top of candidate word k is group KBASE[k] + N + (N & 16)


def _mask_has_group(words, tiles, groups):
    """words [nTiles, 8]; tiles, groups: arrays -> bool array: the group's bit is set in the tile's candidate words."""
    r = groups & 63
    q = r >> 4
    word = (groups >> 6) + 2 * (q & 1)
    n = (r & 15) + 16 * (q >> 1)
    return ((words[tiles, word] >> (31 - n).astype(np.uint32)) & 1) == 1


def test_word_layout_restated_here_is_the_scans():
    seen = set()
    for k in range(4):
        for n in range(32):
            g = KBASE[k] + n + (n & 16)
            w = np.zeros((1, 8), dtype=np.uint32)
            w[0, k] = np.uint32(0x80000000 >> n)
            assert _mask_has_group(w, np.array([0]), np.array([g]))[0]
            seen.add(g)
    assert seen == set(range(128))


def _camera_cases(scenes_mod):
    # (label, scene, W, H): widths that are no multiple of 64, so that tiles wrap the row ends
    return [("cover aperture 0.4", scenes_mod.build_scene("cover", 1, 1210, 800), 1210, 800),
            ("cover aperture 2.0", scenes_mod.build_scene("cover", 1, 1210, 800, aperture=2.0), 1210, 800),
            ("cover aperture 0", scenes_mod.build_scene("cover", 1, 1210, 800, aperture=0.0), 1210, 800),
            ("three (C1 camera)", scenes_mod.build_scene("three", 1, 200, 100), 200, 100)]


@pytest.fixture(scope="module")
def scenes_mod(built):
    from cpuraytracer_amd import scenes
    return scenes


def _random_pairs(rng, rs, W, n_full, n):
    """n random (i, j, s) inside the full tiles of the strip, and their tiles."""
    pl = rng.integers(0, n_full * 64, n)
    lr, i = pl // W, pl % W
    lb = lr // rs.block_rows
    j = rs.first_row + (lb * rs.nshards + rs.shard) * rs.block_rows + (lr - lb * rs.block_rows)
    s = rng.integers(1, 1025, n)
    return np.stack([i, j, s], axis=1).astype(np.uint32), (pl >> 6).astype(np.int64)


def _violations(oracle, sc, W, H, ijs, tiles, words, group_of_sphere):
    """Every (ray, sphere) pair for which the oracle's Sphere::Intersect accepts a root (a one-sphere scene through its list scan) whose
    group's bit is clear in a tile that has a mask.  Returns (violations, accepted pairs checked)."""
    orc = oracle.Oracle()
    orc.upload(sc)
    rays = orc.primary_rays(W, H, ijs)
    orc.close()
    has_mask = (words[tiles, 4] & 1) == 1
    bad = checked = 0
    one = oracle.Oracle()
    for k in range(sc.n):
        single = oracle.Scene(sc.spheres[k:k + 1], sc.materials[k:k + 1], sc.camera, sc.sun, sc.sky, sc.exposure_scale)
        one.upload(single)
        hit = one.closest_hit(rays)[:, 1].view(np.int32) >= 0
        hit &= has_mask
        if hit.any():
            g = np.full(int(hit.sum()), int(group_of_sphere[k]), dtype=np.int64)
            ok = _mask_has_group(words, tiles[hit], g)
            bad += int((~ok).sum())
            checked += int(hit.sum())
    one.close()
    return bad, checked


def _host_masks(sc, W, H, rs, limit=16):  # limit: the library's default (rt_tile_mask.h)
    from cpuraytracer_amd import _capi
    L = _capi.load()
    rows = L.rt_rowset_local_rows(rs)
    cap = (W * rows) >> 6
    words = np.zeros((max(cap, 1), 8), dtype=np.uint32)
    gos = np.zeros(sc.n, dtype=np.uint32)
    n = C.c_uint32(0)
    cam = _capi.RtCamera.from_buffer_copy(bytes(sc.camera))
    _capi.check(L.rt_unit_tile_masks_host(np.ascontiguousarray(sc.spheres).ctypes.data, sc.n, C.byref(cam), W, H, rs, limit, cap, C.byref(n),
                                          words.ctypes.data, gos.ctypes.data))
    return words[:n.value], gos


def test_cone_bound_covers_random_primary_rays(built, scenes_mod):
    """The bound the masks rest on: every point (1 - l) O + l F of a primary ray of a pixel run lies within |1 - l| rhoL + l rhoF of the
    axis point camO + l (Fc - camO), for random pixels of the run, jitter in [0, 1)^2, lens points of the unit disc and l >= 0.
    Camera::GetRay restated in binary64 (camera.cpp:30-48)."""
    from cpuraytracer_amd import _capi
    L = _capi.load()
    rng = np.random.default_rng(7)
    for label, sc, W, H in _camera_cases(scenes_mod):
        cam = _capi.RtCamera.from_buffer_copy(bytes(sc.camera))
        o, mx, my, oip = (np.array(v[:3], dtype=np.float64) for v in (cam.origin, cam.x, cam.y, cam.origin_image_plane))
        for _ in range(40):
            i0 = int(rng.integers(0, W))
            i1 = min(W - 1, i0 + int(rng.integers(0, 64)))
            j = int(rng.integers(0, H))
            out = np.zeros(9, dtype=np.float64)
            _capi.check(L.rt_unit_tile_cone(C.byref(cam), W, H, i0, i1, j, out.ctypes.data))
            assert out[8] == 1.0, label
            D, rhoL, rhoF = out[3:6], out[6], out[7]
            n = 2000
            uvx = (rng.integers(i0, i1 + 1, n) + rng.random(n)) / W
            uvy = (j + rng.random(n)) / H
            th, rr = rng.random(n) * 2 * np.pi, np.sqrt(rng.random(n))
            rr[: n // 10] = 1.0  # the rim of the lens
            lens = np.stack([rr * np.cos(th), rr * np.sin(th)], axis=1)
            pp = oip + (2 * uvx - 1)[:, None] * mx + (-2 * uvy + 1)[:, None] * my
            v = pp - o
            F = o + cam.focal_length * v / np.linalg.norm(v, axis=1)[:, None]
            O = o + (0.5 * cam.aperture * lens[:, 0])[:, None] * mx + (0.5 * cam.aperture * lens[:, 1])[:, None] * my
            lam = np.concatenate([rng.random(n // 2) * 2.0, rng.random(n - n // 2) * 60.0])
            P = (1 - lam)[:, None] * O + lam[:, None] * F
            dist = np.linalg.norm(P - (o + lam[:, None] * D), axis=1)
            reach = np.abs(1 - lam) * rhoL + lam * rhoF
            assert (dist <= reach + 1e-9).all(), (label, i0, i1, j, float((dist - reach).max()))


def test_host_masks_are_sound_against_the_oracle(built, oracle, scenes_mod):
    """The masks as the host evaluates the shipped header, against the oracle, without a GPU (a smaller sample of the GPU test below)."""
    from cpuraytracer_amd import _capi
    rng = np.random.default_rng(11)
    cases = _camera_cases(scenes_mod)
    # 3-way cyclic single rows; the whole image (block_rows = H: what the benchmark renders); blocks of four rows, second of two shards
    for (label, sc, W, H), rs in ((cases[0], _capi.cyclic_rows(800, 1, 3)), (cases[1], _capi.cyclic_rows(800, 1, 3)),
                                  (cases[3], _capi.cyclic_rows(100, 1, 3)), (cases[0], _capi.whole_image(800)),
                                  (cases[1], _capi.cyclic_rows(800, 1, 2, block_rows=4))):
        label = "%s, rows %d/%d x %d" % (label, rs.shard, rs.nshards, rs.block_rows)
        words, gos = _host_masks(sc, W, H, rs)
        assert len(words) > 0, label
        ijs, tiles = _random_pairs(rng, rs, W, len(words), 20000)
        bad, checked = _violations(oracle, sc, W, H, ijs, tiles, words, gos)
        print("%s: %d accepted (ray, sphere) pairs, %d violations, %.1f candidate groups per tile, %.1f %% of the tiles without a mask"
              % (label, checked, bad, words[:, 5].mean(), 100.0 * ((words[:, 4] & 1) == 0).mean()))
        assert checked > 0 and bad == 0, label


def _device_masks(hip, W, H, rs):
    from cpuraytracer_amd import _capi
    L = _capi.load()
    rows = L.rt_rowset_local_rows(rs)
    cap = (W * rows) >> 6
    words = np.zeros((max(cap, 1), 8), dtype=np.uint32)
    n = C.c_uint32(0)
    gos = np.zeros(20000, dtype=np.uint32)
    _capi.check(L.rt_unit_tile_masks(hip._h, W, H, rs, cap, C.byref(n), words.ctypes.data, gos.shape[0], gos.ctypes.data, None))
    return words[:n.value], gos


def _mask_scans(hip, W, H, rs):
    from cpuraytracer_amd import _capi
    L = _capi.load()
    n = C.c_uint32(0)
    scans = np.zeros(2, dtype=np.uint64)
    _capi.check(L.rt_unit_tile_masks(hip._h, W, H, rs, 0, C.byref(n), None, 0, None, scans.ctypes.data))
    return int(scans[0]), int(scans[1])


@pytest.mark.gpu
def test_device_masks_are_sound_against_the_oracle(hip, oracle, scenes_mod):
    """At least 200,000 random (pixel, sample) pairs per camera: the oracle's primary ray, every sphere whose Sphere::Intersect
    accepts a root for it, and the bit of that sphere's group in the mask the DEVICE built for the pixel's tile.  No violation is
    allowed.  Width 1210 (tiles wrap rows), rows 1, 4, 7, ... of the image (a tile's rows are not adjacent).  Tiles without a mask
    keep the filter and are exempt; their share is reported, and bounded on the cover scene at its own aperture."""
    from cpuraytracer_amd import _capi
    rng = np.random.default_rng(5)
    for label, sc, W, H in _camera_cases(scenes_mod):
        rs = _capi.cyclic_rows(H, 1, 3)
        hip.upload(sc)
        words, gos = _device_masks(hip, W, H, rs)
        assert len(words) == (W * _capi.load().rt_rowset_local_rows(rs)) >> 6, label
        hw, hg = _host_masks(sc, W, H, rs)
        assert np.array_equal(hw[:, :6], words[:, :6]) and np.array_equal(hg, gos[:sc.n]), "%s: host and device masks differ" % label
        ijs, tiles = _random_pairs(rng, rs, W, len(words), 200000)
        bad, checked = _violations(oracle, sc, W, H, ijs, tiles, words, gos[:sc.n])
        no_mask = float(((words[:, 4] & 1) == 0).mean())
        print("%s: %d accepted (ray, sphere) pairs, %d violations, %.2f candidate groups per tile, %.2f %% of the tiles without a mask"
              % (label, checked, bad, words[:, 5].mean(), 100.0 * no_mask))
        assert checked > 0 and bad == 0, label
        if label == "cover aperture 0.4":
            assert no_mask < 0.5


def _render(hip, W, H, spp, rs=None, seed=1):
    st = hip.render(W, H, 1, 1 + spp, 50, seed, rowset=rs)
    hip.resolve()
    h, l = hip.download()
    return h.tobytes(), l.tobytes(), st.traversals, st.segments


@pytest.mark.gpu
def test_images_and_counters_are_the_same_with_and_without_masks(hip, oracle, scenes_mod, monkeypatch):
    """RT_PRIMARY_MASK=0 and =1 (read when an accumulation starts): equal HDR and LDR bytes and equal traversal counters."""
    from cpuraytracer_amd import _capi
    three_lights = None
    cases = [("cover 1200x800 spp 8", dict(W=1200, H=800, spp=8)),
             ("cover aperture 2.0", dict(W=640, H=400, spp=4, aperture=2.0)),
             ("partial last tile", dict(W=333, H=101, spp=3)),  # 333 * 101 = 64 * 525 + 33
             ("3-way row set", dict(W=500, H=300, spp=3, rows3=True)),
             ("three lights", dict(W=320, H=200, spp=3, lights=True))]
    for label, c in cases:
        W, H = c["W"], c["H"]
        sc = scenes_mod.build_scene("cover", 1, W, H, aperture=c.get("aperture", -1.0))
        if c.get("lights"):
            three_lights = [sc.sun, oracle.make_light((-0.6, 0.7, 0.35), (0.35, 0.55, 1.0), 25000.0),
                            oracle.make_light((0.0, 1.0, 0.0), (1.0, 1.0, 1.0), 5000.0)]
            sc.lights = three_lights
        rs = _capi.cyclic_rows(H, 2, 3) if c.get("rows3") else None
        got = {}
        for m in ("0", "1"):
            monkeypatch.setenv("RT_PRIMARY_MASK", m)
            hip.upload(sc)
            got[m] = _render(hip, W, H, c["spp"], rs)
            total, masked = _mask_scans(hip, W, H, rs if rs is not None else _capi.whole_image(H))
            assert (masked == 0) if m == "0" else (masked > 0), (label, m, total, masked)
        assert got["0"][0] == got["1"][0], "%s: HDR differs" % label
        assert got["0"][1] == got["1"][1], "%s: LDR differs" % label
        assert got["0"][2:] == got["1"][2:], "%s: traversal counters differ" % label
    # spp 1 per frame in the look-ahead mode
    sc = scenes_mod.build_scene("cover", 1, 320, 200)
    frames = {}
    try:
        for m in ("0", "1"):
            monkeypatch.setenv("RT_PRIMARY_MASK", m)
            hip.upload(sc)
            hip.set_frame_lookahead(4)
            for f in range(9):
                hip.render(320, 200, 1 + f, 2 + f, 50, 1, stats=False)
            hip.resolve()
            h, l = hip.download()
            frames[m] = (h.tobytes(), l.tobytes())
            total, masked = _mask_scans(hip, 320, 200, _capi.whole_image(200))  # of the last launch that traced ahead
            assert (masked == 0) if m == "0" else (masked > 0), ("look-ahead", m, total, masked)
    finally:
        hip.set_frame_lookahead(1)
    assert frames["0"] == frames["1"], "look-ahead frames differ"


@pytest.mark.gpu
def test_c2_primary_scans_take_the_masked_path(hip, scenes_mod, monkeypatch):
    """Without this a silent fall-back to the filter would pass everything above: at least 95 % of the scans of 64 fresh paths of
    the headline workload (cover, 1200x800, spp 128) must have taken a tile mask, by the kernel's own count."""
    from cpuraytracer_amd import _capi
    monkeypatch.delenv("RT_PRIMARY_MASK", raising=False)
    monkeypatch.delenv("RT_PRIMARY_MASK_LIMIT", raising=False)
    W, H, spp = 1200, 800, 128
    sc = scenes_mod.build_scene("cover", 1, W, H)
    hip.upload(sc)
    hip.render(W, H, 1, 1 + spp, 50, 1)
    total, masked = _mask_scans(hip, W, H, _capi.whole_image(H))
    print("c2: %d scans of 64 fresh paths, %d with a tile mask (%.2f %%)" % (total, masked, 100.0 * masked / max(1, total)))
    assert total == W * H * spp // 64
    assert masked >= 0.95 * total
