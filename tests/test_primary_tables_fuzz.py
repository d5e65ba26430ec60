"""Fuzz of the primary rays' per-tile tables (csrc/rt_tile_mask.h, rt_scan.h scan_tile_spheres) and of spheres of negative radius.

The tables are conservative culls: a mask bit or a list entry that is missing drops a hit without a trace.  tests/test_primary_mask.py
and tests/test_primary_spheres.py pin them at the two stock scenes' cameras; here seeded random scenes and cameras (inside spheres,
just above a surface, 5 to 150 degrees, lenses of either sign, focal planes off the look-at point, widths from 1 to 333, three kinds of
row set) are checked on the host twins of the construction against the oracle's Camera::GetRay and Sphere::Intersect, with rays aimed
at the tiles' extremes.  One third of the cases negate every third radius: r < 0 is legal input (the reference's Sphere::Intersect
tests r * r and divides the normal by r -- the hollow sphere), and every bound must enclose |r|.

The gpu-marked tests then check that the device builds the host twins' tables, that random cameras really take the masked and the
direct paths and render the oracle's image on each, and that negative radii render like the oracle's through every scan variant."""
import ctypes as C
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

NONE = 0xFFFF
N_CASES = 42
RAYS_PER_CASE = 40000
F = np.float32
ONE_BELOW = F(1.0 - 2.0 ** -24)  # the largest binary32 below 1: the far end of a jitter component
ROW_Y0 = 0.484  # _row_scene: the middle of the range of heights (0.480 .. 0.488) at which a tile holds exactly 63


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same(a, b, what):
    ba, bb = bits(a), bits(b)
    if not np.array_equal(ba, bb):
        bad = np.nonzero(ba.reshape(-1) != bb.reshape(-1))[0]
        raise AssertionError("%s: %d / %d values differ bitwise; first at %d: %r vs %r"
                             % (what, bad.size, ba.size, bad[0], np.asarray(a).reshape(-1)[bad[0]], np.asarray(b).reshape(-1)[bad[0]]))


# ------------------------------------------------------------------------------------------------ scenes
def _scene(oracle, centers, radii, types, cam_o, cam_l, vfov, aspect, focal, aperture, rng=None):
    """Flat scene from arrays; the camera is the oracle's Camera(origin, look-at, vfov, aspect, focal length, aperture)."""
    n = len(radii)
    sph = np.zeros(n, dtype=oracle.SPHERE_DTYPE)
    sph["cx"], sph["cy"], sph["cz"], sph["r"] = centers[:, 0], centers[:, 1], centers[:, 2], radii
    mat = np.zeros(n, dtype=oracle.MATERIAL_DTYPE)
    k255 = np.float32(1) / np.float32(255)
    types = np.asarray(types, dtype=np.uint32)
    mat["type"] = types
    mat["ior"] = 1.5
    mat["smoothness"] = np.where(types == 1, 0.0, 16.0)
    mat["rgb0"] = (np.array([200, 120, 60], dtype=np.float32) * k255)[None, :]
    if rng is not None:
        mat["tex_type"] = rng.integers(0, 2, n)
        mat["tiling"] = rng.choice([4.0, 50.0, 2500.0], n)
        mat["rgb0"] = rng.integers(0, 256, (n, 3)).astype(np.float32) * k255
        mat["rgb1"] = rng.integers(0, 256, (n, 3)).astype(np.float32) * k255
        mat["smoothness"] = np.where(types == 1, 0.0, rng.uniform(1.0, 64.0, n)).astype(np.float32)
        mat["ior"] = rng.uniform(1.1, 2.4, n).astype(np.float32)
    mat["luminance"] = np.where(types == 3, 3000.0, 0.0).astype(np.float32)
    ref = oracle.build_scene("three", 1, 1.5)  # its sun, sky and exposure
    cam = oracle.RtCamera()
    o, la = np.asarray(cam_o, dtype=np.float64), np.asarray(cam_l, dtype=np.float64)
    oracle.lib().orc_camera_make((C.c_float * 3)(*o), (C.c_float * 3)(*la), float(vfov), float(aspect), float(focal), float(aperture), C.byref(cam))
    return oracle.Scene(sph, mat, cam, ref.sun, ref.sky, ref.exposure_scale, "fuzz", 0)


def _unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


class Case:
    pass


@functools.lru_cache(maxsize=None)
def _case(oracle, k):
    """Case k of the seeded generator (the docstring of test_host_tables_are_sound_for_random_scenes_and_cameras lists the draws)."""
    from cpuraytracer_amd import _capi
    rng = np.random.default_rng(7100 + k)
    c = Case()
    c.k = k
    n = int(rng.choice([3, 20, 64, 200, 480]))
    extent = float(rng.choice([3.0, 12.0, 40.0]))
    centers = rng.uniform(-extent, extent, size=(n, 3))
    centers[:, 1] = np.abs(centers[:, 1]) * 0.25
    radii = np.exp(rng.uniform(np.log(0.02), np.log(2.0), n)) * extent / 12.0  # log-uniform over two decades
    if rng.random() < 0.4:  # a huge floor
        centers = np.concatenate([centers, [[0.0, -400.0 - radii.max(), 0.0]]])
        radii = np.concatenate([radii, [400.0]])
    n = len(radii)
    scale = float(rng.choice([1.0, 1e-2, 1e2]))
    offset = np.zeros(3) if rng.random() < 0.5 else _unit(rng) * 10.0 ** rng.uniform(1.0, 5.0)
    place = int(rng.integers(0, 3))  # camera outside the scene / inside a sphere / 1.01 r above a surface
    q = int(rng.integers(0, n))
    if place == 0:
        cam_o = rng.uniform(-1, 1, 3) * extent * 1.5 + [0.0, extent * 0.5, 0.0]
    elif place == 1:
        cam_o = centers[q] + 0.3 * radii[q] * _unit(rng)
    else:
        cam_o = centers[q] + 1.01 * radii[q] * _unit(rng)
    cam_l = rng.uniform(-0.3, 0.3, 3) * extent
    vfov = float(rng.choice([5.0, 20.0, 60.0, 100.0, 150.0]))
    aperture = float(rng.choice([0.0, 1.0, -1.0]) * rng.choice([0.02, 0.3]) * extent / 12.0)
    focal = float(np.linalg.norm(cam_o - cam_l)) if rng.random() < 0.5 else float(rng.uniform(0.2, 3.0) * extent)
    c.W, c.H = [(64, 40), (100, 37), (333, 50), (16, 64), (130, 33), (1, 128)][int(rng.integers(0, 6))]
    aspect = c.W / float(c.H) if rng.random() < 0.5 else 1.5
    kind = int(rng.integers(0, 3))
    c.rs = (_capi.whole_image(c.H), _capi.cyclic_rows(c.H, 1, 3), _capi.cyclic_rows(c.H, 0, 2, block_rows=4))[kind]
    c.negative = k % 3 == 1
    if c.negative:
        radii[::3] = -radii[::3]  # every third radius, the floor's turn included where it falls
    c.zero = k % 8 == 5
    if c.zero:
        radii[int(rng.integers(0, n))] = 0.0
    types = rng.choice([0, 0, 0, 1, 2, 3], n)
    c.sc = _scene(oracle, (centers * scale + offset).astype(np.float32), (radii * scale).astype(np.float32), types, cam_o * scale + offset,
                  cam_l * scale + offset, vfov, aspect, focal * scale, aperture * scale, rng)
    c.label = "case %d: n %d, scale %g, |offset| %.3g, camera %s, vfov %g, aperture %.3g, %dx%d, rows %d/%d x %d%s%s" % (
        k, n, scale, np.linalg.norm(offset), ("outside", "inside a sphere", "above a surface")[place], vfov, aperture * scale, c.W, c.H,
        c.rs.shard, c.rs.nshards, c.rs.block_rows, ", negative radii" if c.negative else "", ", one radius 0" if c.zero else "")
    return c


# ------------------------------------------------------------------------------------------------ the host twins
def _host_masks(sc, W, H, rs, limit):
    from cpuraytracer_amd import _capi
    L = _capi.load()
    cap = (W * L.rt_rowset_local_rows(rs)) >> 6
    words = np.zeros((max(cap, 1), 8), dtype=np.uint32)
    gos = np.zeros(sc.n, dtype=np.uint32)
    n = C.c_uint32(0)
    cam = _capi.RtCamera.from_buffer_copy(bytes(sc.camera))
    _capi.check(L.rt_unit_tile_masks_host(np.ascontiguousarray(sc.spheres).ctypes.data, sc.n, C.byref(cam), W, H, rs, limit, cap, C.byref(n),
                                          words.ctypes.data, gos.ctypes.data))
    return words[:n.value], gos


def _host_lists(sc, W, H, rs, mask_limit, sphere_limit):
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


def _mask_has_group(words, tiles, group):
    """rt_scan.h's candidate words (tests/test_primary_mask.py checks this layout against the scan's)."""
    r = group & 63
    q = r >> 4
    word = (group >> 6) + 2 * (q & 1)
    n = (r & 15) + 16 * (q >> 1)
    return ((words[tiles, word] >> np.uint32(31 - n)) & 1) == 1


def _listed(lists):
    """[nTiles, 65536 entries at most] bool: the entry is in the tile's list (no row is set for a tile without a list)."""
    has = lists[:, 0] != NONE
    cnt = np.where(has, lists[:, 0], 0).astype(np.int64)
    table = np.zeros((len(lists), int(lists[:, 1:].max()) + 2 if len(lists) else 1), dtype=bool)
    for k in range(63):
        rows = np.nonzero(cnt > k)[0]
        table[rows, lists[rows, 1 + k]] = True
    return has, cnt, table


# ------------------------------------------------------------------------------------------------ rays at the tiles' extremes
def _extreme_rays(oracle, c, n_full, n, rng):
    """n primary rays of the strip's full tiles through the oracle's Camera::GetRay, and their tiles.  40 % sit on the first or the last
    pixel of their tile; 30 % have both jitter components from {0, 1 - 2^-24}; half of the lens points lie on the unit circle, the
    rest are uniform in the disc.  uv is formed as the reference forms it (spheres-app.cpp:132-161): float(i + jitter) / float(W)."""
    W, H, rs = c.W, c.H, c.rs
    tiles = rng.integers(0, n_full, n)
    lane = rng.integers(0, 64, n)
    edge = rng.random(n) < 0.4
    lane[edge] = rng.choice([0, 63], int(edge.sum()))
    pl = tiles * 64 + lane
    lr, i = pl // W, pl % W
    lb = lr // rs.block_rows
    j = rs.first_row + (lb * rs.nshards + rs.shard) * rs.block_rows + (lr - lb * rs.block_rows)
    assert (j < H).all()
    jit = rng.random((n, 2), dtype=np.float32)
    corner = rng.random(n) < 0.3
    jit[corner] = rng.choice([F(0.0), ONE_BELOW], (int(corner.sum()), 2))
    u = (i.astype(np.float32) + jit[:, 0]) / F(W)
    v = (j.astype(np.float32) + jit[:, 1]) / F(H)
    theta = rng.uniform(0.0, 2.0 * np.pi, n)
    rad = np.where(rng.random(n) < 0.5, 1.0, np.sqrt(rng.random(n)))
    lx, ly = (rad * np.cos(theta)).astype(np.float32), (rad * np.sin(theta)).astype(np.float32)
    for _ in range(3):  # binary32 points of the CLOSED unit disc: a rounding that left it steps back towards the centre
        out = lx.astype(np.float64) ** 2 + ly.astype(np.float64) ** 2 > 1.0
        lx[out], ly[out] = np.nextafter(lx[out], F(0.0)), np.nextafter(ly[out], F(0.0))
    assert (lx.astype(np.float64) ** 2 + ly.astype(np.float64) ** 2 <= 1.0).all()
    rays = oracle.camera_rays(c.sc.camera, np.stack([u, v, lx, ly], 1).astype(np.float32))
    return rays, tiles.astype(np.int64)


def _accepted(oracle, sc, rays, workers=8):
    """[n spheres, n rays] bool: the oracle's Sphere::Intersect accepts a root -- a one-sphere scene through its list scan."""
    def some(ks):
        one = oracle.Oracle()
        out = []
        for k in ks:
            one.upload(oracle.Scene(sc.spheres[k:k + 1], sc.materials[k:k + 1], sc.camera, sc.sun, sc.sky, sc.exposure_scale))
            out.append(one.closest_hit(rays)[:, 1].view(np.int32) >= 0)
        one.close()
        return out
    parts = [list(range(w, sc.n, workers)) for w in range(workers)]
    with ThreadPoolExecutor(workers) as ex:
        got = list(ex.map(some, parts))
    acc = np.zeros((sc.n, len(rays)), dtype=bool)
    for ks, rows in zip(parts, got):
        for k, row in zip(ks, rows):
            acc[k] = row
    return acc


def _check_case(oracle, c, n_rays=RAYS_PER_CASE):
    """(accepted pairs checked against a mask, mask bits missing, accepted pairs checked against a list, list entries missing) of one
    case, with the loosest knobs (mask limit 128, sphere limit 63): every tile that can have a table has one, and the tables of the
    default knobs are a subset with the same bits and entries (tests/test_primary_spheres.py)."""
    sc, W, H, rs = c.sc, c.W, c.H, c.rs
    words, gos = _host_masks(sc, W, H, rs, 128)
    lists, eos = _host_lists(sc, W, H, rs, 128, 63)
    if len(words) == 0:
        return 0, 0, 0, 0
    assert len(lists) == len(words)
    rng = np.random.default_rng(9100 + c.k)
    rays, tiles = _extreme_rays(oracle, c, len(words), n_rays, rng)
    has_mask = (words[tiles, 4] & 1) == 1
    has_list, _, table = _listed(lists)
    acc = _accepted(oracle, sc, rays)
    m_checked = m_bad = l_checked = l_bad = 0
    for k in range(sc.n):
        hit = acc[k] & has_mask
        if hit.any():
            m_checked += int(hit.sum())
            m_bad += int((~_mask_has_group(words, tiles[hit], int(gos[k]))).sum())
        hit = acc[k] & has_list[tiles]
        if hit.any():
            e = int(eos[k])
            ok = table[tiles[hit], e] if e < table.shape[1] else np.zeros(int(hit.sum()), dtype=bool)
            l_checked += int(hit.sum())
            l_bad += int((~ok).sum())
    return m_checked, m_bad, l_checked, l_bad


def test_host_tables_are_sound_for_random_scenes_and_cameras(built, oracle):
    """42 seeded cases.  Each draws n from {3, 20, 64, 200, 480} plus an optional huge floor (<= 512 spheres: the flat layout, the one
    with tables), log-uniform radii over two decades, a scene scale from {1, 1e-2, 1e2} and an offset up to 1e5, the camera outside
    the scene, inside a random sphere or 1.01 r above a random surface, vfov from {5, 20, 60, 100, 150}, an aperture of 0 or of either
    sign, the focal length at the look-at distance or independent of it, (W, H) from {(64,40), (100,37), (333,50), (16,64), (130,33),
    (1,128)} at aspect W/H or 1.5, and the whole image, rows 1 of 3, or row blocks 0 of 2 of four rows.  Every third case negates every
    third radius; a few set one radius to 0.

    40,000 rays per case through the oracle's Camera::GetRay, aimed at the tiles' extremes (_extreme_rays).  For every sphere whose
    one-sphere oracle scene accepts a root, the group's bit is set in the tile's mask and the entry is in the tile's list, wherever the
    tile has one.  No violation.

    Against a vacuous pass: at least half of the cases have masks and at least one accepted pair; at least 400,000 accepted pairs in
    all; at least 5 of the negative-radius cases are non-vacuous."""
    live = live_negative = total = 0
    failures = []
    for k in range(N_CASES):
        c = _case(oracle, k)
        mc, mb, lc, lb = _check_case(oracle, c)
        print("%s: %d accepted pairs under a mask, %d bits missing; %d under a list, %d entries missing" % (c.label, mc, mb, lc, lb))
        total += mc
        live += mc > 0
        live_negative += c.negative and mc > 0
        if mb or lb:
            failures.append((c.label, mb, lb))
    print("%d of %d cases with masks and accepted pairs (%d with negative radii), %d accepted pairs" % (live, N_CASES, live_negative, total))
    assert not failures, failures
    assert 2 * live >= N_CASES and total >= 400000 and live_negative >= 5, (live, total, live_negative)


def test_non_finite_spheres_are_refused_by_the_host_entries(built, oracle):
    """No bound can be built from a NaN or an infinite centre or radius: the host twins refuse the scene with RT_ERR_INVALID_ARG and a
    message (rt_scene_upload does the same: test_error_codes in tests/test_gpu_parity.py)."""
    from cpuraytracer_amd import _capi
    L = _capi.load()
    c = _case(oracle, 0)
    for field, value in (("r", np.nan), ("r", np.inf), ("cx", -np.inf), ("cz", np.nan)):
        sph = c.sc.spheres.copy()
        sph[field][1] = value
        out = (C.c_uint32 * 5)()
        assert L.rt_unit_layout_info(sph.ctypes.data, len(sph), out) == 2 and b"not finite" in L.rt_last_error()
        n = C.c_uint32(0)
        assert L.rt_unit_layout(sph.ctypes.data, len(sph), 0, C.byref(n), None, None) == 2
        cam = _capi.RtCamera.from_buffer_copy(bytes(c.sc.camera))
        assert L.rt_unit_tile_masks_host(sph.ctypes.data, len(sph), C.byref(cam), c.W, c.H, c.rs, 16, 0, C.byref(n), None, None) == 2
        assert L.rt_unit_tile_spheres_host(sph.ctypes.data, len(sph), C.byref(cam), c.W, c.H, c.rs, 16, 24, 0, C.byref(n), None, None) == 2


def test_oracles_padded_list_equals_its_plain_list_on_mixed_sign_scenes(built, oracle):
    """The GPU tests below compare with the oracle's padded list tree (its fast, provably conservative route to the list scan's
    answer): with negative radii it must still give the plain list scan's closest hits, bit for bit -- its boxes enclose |r| too."""
    for name in sorted(VARIANTS):
        sc = VARIANTS[name][0](oracle)
        orc = oracle.Oracle()
        orc.upload(sc)
        rng = np.random.default_rng(5)
        ijs = np.stack([rng.integers(0, 300, 3000), rng.integers(0, 200, 3000), rng.integers(1, 600, 3000)], 1).astype(np.uint32)
        rays = orc.primary_rays(300, 200, ijs)
        assert_same(orc.closest_hit(rays, oracle.ACCEL_PADDED_LIST), orc.closest_hit(rays, oracle.ACCEL_LIST), "%s: padded list vs list" % name)
        rp, tp = orc.trace(300, 200, ijs[:600], 12, 77, accel=oracle.ACCEL_PADDED_LIST)
        rl, tl = orc.trace(300, 200, ijs[:600], 12, 77, accel=oracle.ACCEL_LIST)
        orc.close()
        assert_same(rp, rl, "%s: traced samples, padded list vs list" % name)
        assert np.array_equal(tp, tl)


# ------------------------------------------------------------------------------------------------ the 63 | 64 scene
def _row_scene(oracle, y0=ROW_Y0):
    """W = 64: a tile is an image row, and its cone is round -- as wide as the image.  A horizontal row of 121 small spheres above the
    image centre, seen through 20 degrees from close by (the tables' margins grow with the camera's distance from the origin): the cone of an image row reaches the spheres within half an image width of the row's
    centre, fewer from row to row down the image.  At this height of the row some tile reaches exactly 63 spheres -- a full list --
    and the tile above it more: no list."""
    from cpuraytracer_amd import _capi
    n = 121
    centers = np.stack([(np.arange(n) - 60.0) * 0.02, np.full(n, y0), np.zeros(n)], 1)
    radii = np.full(n, 0.008)
    radii[1::4] = -radii[1::4]
    c = Case()
    c.k, c.W, c.H = 1000, 64, 40
    c.negative, c.zero = True, False
    c.rs = _capi.whole_image(c.H)
    c.sc = _scene(oracle, centers.astype(np.float32), radii.astype(np.float32), np.tile([0, 1, 2, 0], 31)[:n], (0.0, 0.0, -4.0), (0.0, 0.0, 0.0), 20.0,
                  1.6, 4.0, 0.0)
    c.label = "row of 121 small spheres"
    return c


def test_row_scene_has_a_full_list_beside_a_tile_without_one(built, oracle):
    """The host twin's counts on the scene the GPU test renders: with the loosest knobs some tile's list holds exactly 63 entries (the
    most a record holds) and a neighbouring tile, masked as well, reaches 64 or more spheres and so has none."""
    c = _row_scene(oracle)
    words, _ = _host_masks(c.sc, c.W, c.H, c.rs, 128)
    lists, _ = _host_lists(c.sc, c.W, c.H, c.rs, 128, 63)
    assert len(lists) == c.W * c.H // 64 and ((words[:, 4] & 1) == 1).all()
    cnt = lists[:, 0].astype(np.int64)
    print("row scene, spheres per tile:", cnt.tolist())
    full = np.nonzero(cnt == 63)[0]
    assert len(full) > 0
    assert any((t > 0 and cnt[t - 1] == NONE) or (t + 1 < len(cnt) and cnt[t + 1] == NONE) for t in full)
    mc, mb, lc, lb = _check_case(oracle, c)
    assert mc > 0 and mb == 0 and lb == 0  # (the rows that see the spheres reach all of them: lc == 0, their tiles have no list)


# ------------------------------------------------------------------------------------------------ GPU
# Twelve of the cases above whose tiles have tables (the tests assert that they have); the second row negates every third radius.
GPU_CASES = (3, 5, 6, 8, 9, 21,
             10, 13, 16, 22, 25, 37)
FORCED = {"RT_PRIMARY_MASK_LIMIT": "128", "RT_PRIMARY_SPHERES": "63"}  # every maskable tile takes the direct path
KNOBS = (("mask off", {"RT_PRIMARY_MASK": "0"}), ("default", {}), ("forced", FORCED))


def _gpu_case(oracle, k):
    return _row_scene(oracle) if k == 1000 else _case(oracle, k)


def _oracle_rows(oracle, rs):
    return oracle.RtRowset(rs.first_row, rs.num_rows, rs.block_rows, rs.shard, rs.nshards)


def _set_knobs(monkeypatch, env):
    for name in ("RT_PRIMARY_MASK", "RT_PRIMARY_MASK_LIMIT", "RT_PRIMARY_SPHERES"):
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)


def _knob_limits(env):
    return int(env.get("RT_PRIMARY_MASK_LIMIT", 16)), int(env.get("RT_PRIMARY_SPHERES", 24))  # the library's defaults (rt_tile_mask.h)


def _device_masks(hip, n, W, H, rs):
    from cpuraytracer_amd import _capi
    L = _capi.load()
    cap = (W * L.rt_rowset_local_rows(rs)) >> 6
    words = np.zeros((max(cap, 1), 8), dtype=np.uint32)
    gos = np.zeros(n, dtype=np.uint32)
    cnt = C.c_uint32(0)
    _capi.check(L.rt_unit_tile_masks(hip._h, W, H, rs, cap, C.byref(cnt), words.ctypes.data, n, gos.ctypes.data, None))
    return words[:cnt.value], gos


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
@pytest.mark.parametrize("k", GPU_CASES + (1000,))
def test_device_tables_equal_the_host_twins(hip, oracle, monkeypatch, k):
    """Masks, group of every sphere and sphere lists as the device builds them, under the default knobs and the loosest ones."""
    c = _gpu_case(oracle, k)
    for env in ({}, FORCED):
        _set_knobs(monkeypatch, env)
        mask_limit, sphere_limit = _knob_limits(env)
        hip.upload(c.sc)
        words, gos = _device_masks(hip, c.sc.n, c.W, c.H, c.rs)
        hw, hg = _host_masks(c.sc, c.W, c.H, c.rs, mask_limit)
        assert len(hw) > 0, c.label
        assert np.array_equal(hw[:, :6], words[:, :6]) and np.array_equal(hg, gos), "%s: host and device masks differ (%s)" % (c.label, env)
        host, _ = _host_lists(c.sc, c.W, c.H, c.rs, mask_limit, sphere_limit)
        assert _same_lists(_device_lists(hip, c.W, c.H, c.rs), host), "%s: host and device lists differ (%s)" % (c.label, env)


@pytest.mark.gpu
@pytest.mark.parametrize("k", GPU_CASES + (1000,))
def test_random_cameras_take_the_masked_and_direct_paths_and_render_the_oracles_image(hip, oracle, monkeypatch, k):
    """RT_PRIMARY_MASK=0, the default knobs, and RT_PRIMARY_MASK_LIMIT=128 with RT_PRIMARY_SPHERES=63: each render equals the live
    oracle's bit for bit (HDR, traversal and segment totals).  Where the host twin says that tiles have masks or lists, the kernel's
    own counts of scans that used them are > 0; with the knob off they are 0."""
    c = _gpu_case(oracle, k)
    spp, depth, seed = 3, 10, 40 + k
    orc = oracle.Oracle()
    orc.upload(c.sc)
    so = orc.render(c.W, c.H, 1, 1 + spp, depth, seed, rowset=_oracle_rows(oracle, c.rs), accel=oracle.ACCEL_PADDED_LIST, threads=8)
    ho, _ = orc.download()
    orc.close()
    for label, env in KNOBS:
        _set_knobs(monkeypatch, env)
        hip.upload(c.sc)
        sg = hip.render(c.W, c.H, 1, 1 + spp, depth, seed, rowset=c.rs)
        hg, _ = hip.download(ldr=False)
        total, masked, direct = _scans(hip, c.W, c.H, c.rs)
        print("%s, %s: %d scans of fresh paths, %d with a tile's tables, %d direct" % (c.label, label, total, masked, direct))
        assert_same(hg, ho, "%s, %s: HDR" % (c.label, label))
        assert (sg.traversals, sg.segments) == (so.traversals, so.segments), (c.label, label)
        if label == "mask off":
            assert masked == 0 and direct == 0, (c.label, label)
            continue
        mask_limit, sphere_limit = _knob_limits(env)
        words, _ = _host_masks(c.sc, c.W, c.H, c.rs, mask_limit)
        lists, _ = _host_lists(c.sc, c.W, c.H, c.rs, mask_limit, sphere_limit)
        any_mask, any_list = bool(((words[:, 4] & 1) == 1).any()), bool((lists[:, 0] != NONE).any())
        if label == "forced":
            assert any_mask and any_list, "%s: the case has no tables, it does not belong in GPU_CASES" % c.label
        assert (masked > 0) == any_mask and (direct > 0) == any_list and direct <= masked, (c.label, label, total, masked, direct)


# ------------------------------------------------------------------------------------------------ negative radii, every scan variant
def _soup(oracle, n, seed):
    """Random sphere soup over a floor, every third radius negative (the floor's is positive)."""
    rng = np.random.default_rng(seed)
    extent = 5.0 if n < 600 else 24.0
    centers = rng.uniform(-extent, extent, size=(n, 3))
    centers[:, 1] = np.abs(centers[:, 1]) * 0.25
    radii = np.exp(rng.uniform(np.log(0.05), np.log(1.2), n))
    radii[::3] = -radii[::3]
    centers = np.concatenate([centers, [[0.0, -401.5, 0.0]]])
    radii = np.concatenate([radii, [400.0]])
    types = rng.choice([0, 0, 0, 1, 2, 3], n + 1)
    types[-1] = 0
    cam_o, cam_l = np.array([1.1, 0.45, -0.9]) * extent, np.array([0.0, 0.05, 0.0]) * extent
    return _scene(oracle, centers.astype(np.float32), radii.astype(np.float32), types, cam_o, cam_l, 45.0, 1.5, float(np.linalg.norm(cam_o - cam_l)),
                  0.02 * extent, rng)


def _layer(oracle, n, side, seed, cam_o=(9.0, 1.2, -6.0), cam_l=(0.0, 0.2, 0.0)):
    """n small spheres in a thin layer over a floor (the scene class of the cell-grid scan), every third radius negative."""
    rng = np.random.default_rng(seed)
    a, b = rng.uniform(-side, side, n), rng.uniform(-side, side, n)
    centers = np.stack([a, 0.2 + rng.uniform(0, 0.05, n), b], 1)
    radii = 0.2 * rng.uniform(0.5, 1.0, n)
    radii[::3] = -radii[::3]
    centers = np.concatenate([centers, [[0.0, -1000.0, 0.0]]])
    radii = np.concatenate([radii, [1000.0]])
    types = rng.choice([0, 0, 0, 1, 2, 3], n + 1)
    types[-1] = 0
    o, la = np.asarray(cam_o, dtype=np.float64), np.asarray(cam_l, dtype=np.float64)
    return _scene(oracle, centers.astype(np.float32), radii.astype(np.float32), types, o, la, 40.0, 1.5, float(np.linalg.norm(o - la)), 0.0, rng)


def _layout_kind(sc):
    """0: flat, 1: cell grid, 2: bounds hierarchy (rt_unit_layout_info, under the environment of the moment)."""
    from cpuraytracer_amd import _capi
    out = (C.c_uint32 * 5)()
    sph = np.ascontiguousarray(sc.spheres)
    _capi.check(_capi.load().rt_unit_layout_info(sph.ctypes.data, sph.shape[0], out))
    return int(out[0])


VARIANTS = {  # name: (scene, environment, layout kind the scene must select)
    "flat": (lambda o: _soup(o, 150, 61), {}, 0),
    "hierarchy": (lambda o: _soup(o, 1500, 62), {}, 2),
    "tree_top_16": (lambda o: _soup(o, 90, 63), {"RT_TREE_TOP": "16"}, 2),
    "grid": (lambda o: _layer(o, 3000, 30.0, 64), {}, 1),
    "valu": (lambda o: _soup(o, 150, 65), {"RT_SCAN": "valu"}, 0),
}


@pytest.mark.gpu
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_negative_radii_render_like_the_oracles_through_every_scan(oracle, monkeypatch, variant):
    """Every third radius negative, through the flat matrix-core scan, the bounds hierarchy (by size and under RT_TREE_TOP=16), the cell
    grid and RT_SCAN=valu: closest hits of the oracle's primary rays of 3,000 random (i, j, s), the traced samples of the same (so that
    scatter rays and shadow rays meet the negative spheres too) and one whole image equal the oracle's, bit for bit."""
    from cpuraytracer_amd import HipRenderer
    make, env, kind = VARIANTS[variant]
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    sc = make(oracle)
    assert (sc.spheres["r"] < 0).sum() >= sc.n // 4 and _layout_kind(sc) == kind, variant
    r = HipRenderer(0)  # the knobs are read when a context is created
    orc = oracle.Oracle()
    try:
        r.upload(sc)
        orc.upload(sc)
        W, H, m = 300, 200, 3000
        rng = np.random.default_rng(5)
        ijs = np.stack([rng.integers(0, W, m), rng.integers(0, H, m), rng.integers(1, 600, m)], 1).astype(np.uint32)
        rays = orc.primary_rays(W, H, ijs)
        want = orc.closest_hit(rays, oracle.ACCEL_PADDED_LIST)
        neg_hits = int((sc.spheres["r"][np.maximum(want[:, 1].view(np.int32), 0)] < 0)[want[:, 1].view(np.int32) >= 0].sum())
        assert neg_hits >= 40, "the sample does not meet the negative spheres"
        assert_same(r.unit_closest_hit(rays), want, "closest hits")
        rg, tg = r.unit_trace(W, H, ijs, 12, 77)
        ro, to = orc.trace(W, H, ijs, 12, 77, accel=oracle.ACCEL_PADDED_LIST)
        assert_same(rg, ro, "per-sample radiance")
        assert np.array_equal(tg, to)
        W, H, spp = 192, 50, 2
        sg = r.render(W, H, 1, 1 + spp, 12, 9)
        hg, _ = r.download(ldr=False)
        so = orc.render(W, H, 1, 1 + spp, 12, 9, accel=oracle.ACCEL_PADDED_LIST, threads=8)
        ho, _ = orc.download()
        assert_same(hg, ho, "whole image HDR")
        assert (sg.traversals, sg.segments) == (so.traversals, so.segments)
    finally:
        r.close()
        orc.close()


@pytest.mark.gpu
def test_hollow_glass_sphere(hip, oracle):
    """The usual idiom: a glass sphere of radius 0.5 holding a sphere of radius -0.45 at the same centre, on a floor under the sun, a
    diffuse sphere in its shadow.  Every refracted path crosses the negative sphere, and it occludes the shadow rays."""
    sun = np.array(oracle.build_scene("three", 1, 1.5).sun.direction[:], dtype=np.float64)  # points from the scene to the sun
    centre = np.array([0.0, 0.5, 0.0])
    behind = centre - sun / np.linalg.norm(sun) * 1.4
    behind[1] = 0.2
    centers = np.array([centre, centre, behind, [0.0, -1000.0, 0.0]])
    radii = np.array([0.5, -0.45, 0.2, 1000.0])
    sc = _scene(oracle, centers.astype(np.float32), radii.astype(np.float32), [2, 2, 0, 0], (1.2, 1.1, -2.6), (0.0, 0.35, 0.0), 35.0, 1.5, 3.0, 0.0)
    W, H, spp, depth = 192, 128, 3, 12
    hip.upload(sc)
    orc = oracle.Oracle()
    orc.upload(sc)
    sg = hip.render(W, H, 1, 1 + spp, depth, 3)
    hg, _ = hip.download(ldr=False)
    so = orc.render(W, H, 1, 1 + spp, depth, 3, accel=oracle.ACCEL_PADDED_LIST, threads=8)
    ho, _ = orc.download()
    rng = np.random.default_rng(8)
    ijs = np.stack([rng.integers(0, W, 2000), rng.integers(0, H, 2000), rng.integers(1, 200, 2000)], 1).astype(np.uint32)
    hits = orc.closest_hit(orc.primary_rays(W, H, ijs), oracle.ACCEL_PADDED_LIST)[:, 1].view(np.int32)
    orc.close()
    assert (hits == 0).sum() > 50, "the camera does not see the glass sphere"
    assert_same(hg, ho, "hollow glass sphere HDR")
    assert (sg.traversals, sg.segments) == (so.traversals, so.segments)
    assert np.isfinite(hg).all()
