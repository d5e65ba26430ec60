"""Cases and the reference model of the tiles' work order (include/rt_api.h, rt_unit_tile_order: "the contract of the order").

The model is a numpy restatement of that contract from independent sources only: the pilots' (i, j, s) from the row set through the
exported rt_rowset_global_row, their rays and first hits from the oracle (primary_rays, closest_hit over its plain list), material
types from the scene, the flags from the list headers of rt_unit_tile_spheres_host (which tests/test_primary_tables_fuzz.py holds
against the oracle), the order from numpy's stable argsort.  It includes no header of csrc and calls no device.

tests/test_work_order_cpu.py asserts, on the model alone, that the cases exercise what the device tests of tests/test_work_order.py
are there to see; this module only builds them."""
import ctypes as C
import functools

import numpy as np

PILOTS = (0, 32, 63)  # local pixels of a tile whose sample-1 rays are the pilots: first, middle, last
GLASS, METAL = 2, 1   # rt_material.type: RT_MAT_DIELECTRIC_TRANSPARENT, RT_MAT_METAL
MASK_LIMIT, SPHERE_LIMIT = 16, 24  # the library's default RT_PRIMARY_MASK_LIMIT / RT_PRIMARY_SPHERES (csrc/rt_tile_mask.h)
SQRT_DISK = 2  # RT_SAMPLER_SQRT_DISK


# ------------------------------------------------------------------------------------------------------------------ the sort's cases
SORT_NS = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 3071, 3072, 3073, 5000, 65537, 100003, 1 << 20)


def per_thread(n):
    """Tiles per thread of the one workgroup of 1024 threads: ceil(n / 1024)."""
    return (n + 1023) // 1024


def _runs(n, rng):
    """Runs of one class whose lengths cycle through per - 1, per, per + 1 (zero lengths left out): their ends drift across the
    threads' boundaries in both directions.  Neighbouring runs differ in class."""
    per = per_thread(n)
    lengths = [v for v in (per - 1, per, per + 1) if v > 0]
    out = np.zeros(n, dtype=np.uint8)
    at, k, c = 0, 0, int(rng.integers(0, 5))
    while at < n:
        ln = lengths[k % len(lengths)]
        out[at:at + ln] = c
        at += ln
        k += 1
        c = (c + 1 + int(rng.integers(0, 4))) % 5
    return out


def sort_cases():
    """(label, classes) for every n of SORT_NS crossed with the patterns of the issue; generated one at a time (the largest are 1 MiB)."""
    for n in SORT_NS:
        rng = np.random.default_rng(4200 + n)
        per = per_thread(n)
        t = np.arange(n)
        for c in range(5):
            yield "n %d, all %d" % (n, c), np.full(n, c, dtype=np.uint8)
        yield "n %d, uniform" % n, rng.integers(0, 5, n).astype(np.uint8)
        mostly = np.full(n, 2, dtype=np.uint8)
        odd = rng.random(n) < 0.01
        mostly[odd] = rng.integers(0, 5, int(odd.sum()))
        yield "n %d, 99 %% class 2" % n, mostly
        u = rng.integers(0, 5, n).astype(np.uint8)
        yield "n %d, descending" % n, np.sort(u)[::-1].copy()
        yield "n %d, ascending" % n, np.sort(u)
        yield "n %d, alternating 1 3" % n, np.where(t % 2 == 0, 1, 3).astype(np.uint8)
        yield "n %d, cycling 0..4" % n, (t % 5).astype(np.uint8)
        yield "n %d, runs of per - 1, per, per + 1 (per %d)" % (n, per), _runs(n, rng)
        spots = {"index 0": 0, "index n - 1": n - 1, "last of thread 0": per - 1, "first of thread 1": per,
                 "last of wave 0": 64 * per - 1, "first of wave 1": 64 * per}
        for what, k in spots.items():
            if 0 <= k < n:
                for base, odd_class in ((2, 4), (2, 0)):
                    a = np.full(n, base, dtype=np.uint8)
                    a[k] = odd_class
                    yield "n %d, one tile of class %d at %s (%d) among class %d" % (n, odd_class, what, k, base), a


def stable_descending(classes):
    """The order's contract: the stable sort of the tile indices by descending stored class."""
    return np.argsort(-np.asarray(classes).astype(np.int16), kind="stable").astype(np.uint32)


# ------------------------------------------------------------------------------------------------------------------ scenes
class Case:
    pass


def _rowset(kind, H):
    from cpuraytracer_amd import _capi
    if kind == "whole":
        return _capi.whole_image(H)
    if kind[0] == "band":
        return _capi.RtRowset(kind[1], kind[2], kind[2], 0, 1)
    return _capi.cyclic_rows(H, kind[1], 3, block_rows=kind[2])  # ("cyclic", shard, block_rows): nshards 3


def _pixel_ray(oracle, camera, W, H, i, j):
    """Origin and unit direction of the pilot ray of pixel (i, j) -- sample 1, no lens -- and the size of a pixel at unit distance."""
    probe = oracle.build_scene("three", 1, 1.5)
    cam = oracle.RtCamera.from_buffer_copy(bytes(camera))
    cam.aperture = 0.0
    orc = oracle.Oracle()
    orc.upload(oracle.Scene(probe.spheres, probe.materials, cam, probe.sun, probe.sky, probe.exposure_scale))
    r = orc.primary_rays(W, H, np.array([[i, j, 1], [min(i + 1, W - 1), j, 1], [max(i - 1, 0), j, 1]], dtype=np.uint32)).astype(np.float64)
    orc.close()
    d = r[:, 3:] / np.linalg.norm(r[:, 3:], axis=1)[:, None]
    return r[0, :3], d[0], float(np.linalg.norm(d[1] - d[2])) / float(min(i + 1, W - 1) - max(i - 1, 0))


def _middle_pilot(W, i, j):
    """(i, j) of the middle pilot of the tile that holds pixel (i, j) of a whole image of width W."""
    p = ((j * W + i) >> 6 << 6) + PILOTS[1]
    return p % W, p // W


CAP_W, CAP_H = 150, 120


def cap_scene(oracle):
    """The scene built for the purpose, for pictures of 150 x 120 (a tile's cone is as tall as the tile is wide, so a tile with an empty
    list needs some 32 rows of sky around it): a floor under a sky that fills the upper three quarters, seen through 20 degrees, and spheres placed along the pilot
    rays of chosen pixels, each `r` pixels in radius --
      glass, 1.2 pixels, under a middle pilot of row 1: a narrow cap over the sky; the tiles above and below it list the sphere and are
        raised, one of them in the first row, the tiles beside it have empty lists and stay flagged;
      glass, 1 pixel, under a middle pilot of row 106, alone over the floor: at this width each of the six neighbour pixels lies in
        another tile, so each raises a tile through itself alone;
      glass, 1 pixel, under a middle pilot of row 113, over the floor: the band of rows 0 to 114 ends below it;
      glass, 2.5 pixels, under (142, 119): inside the partial last tile (row 119 from column 134 on) and under no pilot of a full tile;
      metal and diffuse spheres of 5 to 6 pixels around the horizon."""
    from test_primary_tables_fuzz import _scene
    W, H = CAP_W, CAP_H
    cam_o, cam_l, vfov, aspect = (0.0, 1.0, -6.0), (0.0, 0.76, 0.0), 20.0, W / float(H)
    base = _scene(oracle, np.array([[0.0, -100.0, 0.0]], dtype=np.float32), np.array([100.0], dtype=np.float32), [0], cam_o, cam_l, vfov, aspect, 6.0, 0.0)
    spots = [_middle_pilot(W, 74, 1) + (1.2, GLASS, 0.0), _middle_pilot(W, 76, 106) + (1.0, GLASS, 0.0), _middle_pilot(W, 40, 113) + (1.0, GLASS, 0.0),
             (142, 119, 2.5, GLASS, 0.3), (20, 92, 6.0, METAL, 0.0), (110, 97, 6.0, METAL, 0.0), (60, 94, 5.0, 0, 0.0), (140, 96, 5.0, 0, 0.0),
             (90, 101, 5.0, METAL, 0.0)]
    centers, radii, types = [[0.0, -100.0, 0.0]], [100.0], [0]  # (a floor of radius 1000 is in every tile's list from one unit above it)
    for i, j, r_px, ty, down in spots:
        o, d, px = _pixel_ray(oracle, base.camera, W, H, i, j)
        t_floor = -o[1] / d[1] if d[1] < -0.09 else np.inf  # (below the horizon of the floor: about 8 degrees down)
        dist = 6.0 if not np.isfinite(t_floor) else min(6.0, 0.6 * t_floor)
        c = o + d * dist
        c[1] -= down * px * dist  # (the one in the partial tile sits a third of a pixel lower: it must stay out of the row above)
        centers.append(c)
        radii.append(r_px * px * dist)
        types.append(ty)
    return _scene(oracle, np.array(centers, dtype=np.float32), np.array(radii, dtype=np.float32), types, cam_o, cam_l, vfov, aspect, 6.0, 0.0)


# (scene, W, H, row set, aperture of the cover scene or None for the scene's own, sampler flags)
CASES = (
    ("cover", 256, 160, "whole", None, 0),                 # 640 tiles, a tile is a quarter of a row
    ("cover", 256, 160, "whole", None, SQRT_DISK),         # ... the lens sample moved by the sampler flag (the cover camera has a lens)
    ("cover", 192, 96, ("cyclic", 0, 4), 0.0, 0),          # blocks of four rows, shard 0 of 3: 96 tiles, no partial one, no lens
    ("cover", 200, 100, ("cyclic", 1, 1), None, SQRT_DISK),  # single rows, shard 1 of 3: 33 rows, 103 tiles and 8 pixels
    ("cover", 150, 90, ("band", 20, 50), None, 0),         # rows 20 to 69: 117 tiles and 12 pixels, tiles straddle rows
    ("cover", 333, 50, "whole", 0.0, 0),                   # 260 tiles and 10 pixels
    ("cover", 48, 80, "whole", None, 0),                   # narrower than a tile: 60 tiles of a row and a third
    ("cover", 40, 50, ("cyclic", 2, 1), 0.25, SQRT_DISK),  # 16 rows of 40: 10 tiles, a wide lens
    ("cover", 64, 40, "whole", None, 0),                   # a tile is a row
    ("cap", CAP_W, CAP_H, "whole", None, 0),               # 281 tiles and 16 pixels: the partial tile holds glass
    ("cap", CAP_W, CAP_H, ("band", 0, 115), None, 0),      # 269 tiles and 34 pixels: the last row lies under a glass tile
    ("cap", CAP_W, CAP_H, ("cyclic", 0, 4), None, 0),      # rows 0-3, 12-15, ...: 40 rows, 93 tiles and 48 pixels
)


@functools.lru_cache(maxsize=None)
def case(oracle, k):
    from cpuraytracer_amd import scenes
    name, W, H, rows, aperture, sampler = CASES[k]
    c = Case()
    c.k, c.W, c.H, c.sampler = k, W, H, sampler
    c.rs = _rowset(rows, H)
    if name == "cover":
        c.sc = scenes.build_scene("cover", 1, W, H, aperture=-1.0 if aperture is None else aperture)
    else:
        c.sc = cap_scene(oracle)
    c.label = "case %d: %s %dx%d, rows %s, aperture %g, sampler %d" % (k, name, W, H, rows, c.sc.camera.aperture, sampler)
    return c


# ------------------------------------------------------------------------------------------------------------------ the model
def local_to_pixel(W, rs, p):
    """(i, j) of the strip's local pixels p: column p mod W of the image row that rt_rowset_global_row gives for local row p / W."""
    from cpuraytracer_amd import _capi
    L = _capi.load()
    p = np.asarray(p, dtype=np.int64)
    lr = p // W
    rows = {int(r): int(L.rt_rowset_global_row(rs, int(r))) for r in np.unique(lr)}
    return (p - lr * W), np.array([rows[int(r)] for r in lr.reshape(-1)], dtype=np.int64).reshape(lr.shape)


def host_list_headers(sc, W, H, rs):
    """Header of every full tile's sphere list under the default limits (0: empty; 0xffff: no list), or None where the scene has no lists."""
    from cpuraytracer_amd import _capi
    L = _capi.load()
    cap = max((W * L.rt_rowset_local_rows(rs)) >> 6, 1)
    lists = np.zeros((cap, 64), dtype=np.uint16)
    n = C.c_uint32(0)
    cam = _capi.RtCamera.from_buffer_copy(bytes(sc.camera))
    _capi.check(L.rt_unit_tile_spheres_host(np.ascontiguousarray(sc.spheres).ctypes.data, sc.n, C.byref(cam), W, H, rs, MASK_LIMIT, SPHERE_LIMIT, cap,
                                            C.byref(n), lists.ctypes.data, None))
    return lists[:n.value, 0].copy() if n.value else None


def _material_class(sc, hits):
    """0 nothing hit, 1 other, 2 metal, 3 glass for rt_unit_closest_hit-format records (the type of the sphere hit first)."""
    idx = np.ascontiguousarray(hits[:, 1]).view(np.int32)
    ty = np.asarray(sc.materials["type"])[np.maximum(idx, 0)]
    return np.where(idx < 0, 0, np.where(ty == GLASS, 3, np.where(ty == METAL, 2, 1))).astype(np.int64)


def model(oracle, sc, W, H, rs, sampler, with_flags=True):
    """The contract of rt_api.h restated.  Returns a dict: n (full tiles), pilot_rays (n, 3, 6), pilot_sphere (n, 3) the sphere each
    pilot hits first (< 0: none), pilot_class (n, 3), tile_class (n,)
    before the rule, fired (n, 6) bool -- neighbour pixel k lies in a full tile of glass pilot class and the tile's own is below it --,
    after (n,) the class after the rule, flags (n,) uint8, classes (n,) uint8 the stored class, order (n,) uint32, sky (3,) float32
    the constant sample or None where no tile is flagged, and for the honesty conditions partial_class (the largest sample-1 class
    over the partial last tile's pixels, -1 without one) and near_tile (n, 6), the tile of each neighbour pixel (-1: before the strip
    or beyond its last pixel)."""
    from cpuraytracer_amd import _capi
    L = _capi.load()
    npix = W * int(L.rt_rowset_local_rows(rs))
    n = npix >> 6
    assert n >= 1
    p = (np.arange(n, dtype=np.int64)[:, None] << 6) + np.array(PILOTS, dtype=np.int64)[None, :]
    part = np.arange(n << 6, npix, dtype=np.int64)  # the partial tile's pixels: no pilots, only what the honesty conditions ask of them
    i, j = local_to_pixel(W, rs, np.concatenate([p.reshape(-1), part]))
    ijs = np.stack([i, j, np.ones_like(i)], 1).astype(np.uint32)
    orc = oracle.Oracle()
    oracle.lib().orc_set_sampler(int(sampler))
    try:
        orc.upload(sc)
        rays = orc.primary_rays(W, H, ijs)
        hits = orc.closest_hit(rays, oracle.ACCEL_LIST)
        ck = _material_class(sc, hits)
        miss = np.nonzero(ck[:3 * n] == 0)[0]
        sky = orc.trace(W, H, ijs[miss[:1]], 2, 1, accel=oracle.ACCEL_LIST)[0][0] if len(miss) else None
    finally:
        oracle.lib().orc_set_sampler(0)
        orc.close()
    pilot_class = ck[:3 * n].reshape(n, 3)
    tile_class = pilot_class.max(axis=1)
    f = np.arange(n, dtype=np.int64) << 6
    near = np.stack([f - 64, f + 64, f - W, f - W + 63, f + W, f + W + 63], 1)
    near_tile = np.where((near >= 0) & (near < npix), near >> 6, -1)
    full = (near_tile >= 0) & (near_tile < n)
    fired = full & (tile_class[np.where(full, near_tile, 0)] == 3) & (tile_class[:, None] != 3)
    after = np.where(fired.any(axis=1), 3, tile_class)
    flags = np.zeros(n, dtype=np.uint8)
    if with_flags:
        headers = host_list_headers(sc, W, H, rs)
        if headers is not None:
            assert len(headers) == n
            flags = (headers == 0).astype(np.uint8)
    classes = np.where(flags != 0, 0, after + 1).astype(np.uint8)
    out = {"n": n, "pilot_rays": rays[:3 * n].reshape(n, 3, 6), "pilot_sphere": np.ascontiguousarray(hits[:3 * n, 1]).view(np.int32).reshape(n, 3),
           "pilot_class": pilot_class, "tile_class": tile_class, "fired": fired, "after": after,
           "flags": flags, "classes": classes, "order": stable_descending(classes), "sky": sky if flags.any() else None,
           "partial_class": int(ck[3 * n:].max()) if len(part) else -1, "near_tile": near_tile}
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def case_model(oracle, k, with_flags=True):
    c = case(oracle, k)
    return model(oracle, c.sc, c.W, c.H, c.rs, c.sampler, with_flags)


def honesty(c, m):
    """What one case contributes to the honesty conditions of tests/test_work_order_cpu.py, counted on the model alone."""
    from cpuraytracer_amd import _capi
    n, W = m["n"], c.W
    rows = int(_capi.load().rt_rowset_local_rows(c.rs))
    shown = m["fired"].any(axis=1) & (m["flags"] == 0)  # raised, and the stored class shows it
    first_row = (np.arange(n) << 6) // W == 0
    last_row = ((np.arange(n) << 6) + 63) // W == rows - 1
    sole = m["fired"] & (m["fired"].sum(axis=1) == 1)[:, None]
    pc, tc = m["pilot_class"], m["tile_class"]
    alone = [(pc[:, k] == tc) & (np.delete(pc, k, axis=1).max(axis=1) < tc) for k in range(3)]
    glass_near = (m["near_tile"] >= 0) & (m["near_tile"] < n) & (tc[np.clip(m["near_tile"], 0, n - 1)] == 3)
    only_partial = (m["near_tile"] == n).any(axis=1) & (m["partial_class"] == 3) & ~glass_near.any(axis=1) & (tc != 3)
    return {"tiles per stored class": np.bincount(m["classes"], minlength=5)[:5],
            "raised through pixel k": (m["fired"] & shown[:, None]).sum(axis=0),
            "raised through pixel k alone": (sole & shown[:, None]).sum(axis=0),
            "raised in the first tile row": int((shown & first_row).sum()), "raised in the last tile row": int((shown & last_row).sum()),
            "not raised, the only glass neighbour is the partial tile": int(only_partial.sum()),
            "flagged beside a glass tile": int(((m["flags"] != 0) & glass_near.any(axis=1)).sum()),
            "decided by the first, middle, last pilot alone": [int(a.sum()) for a in alone],
            "distinct stored classes": int(len(np.unique(m["classes"])))}
