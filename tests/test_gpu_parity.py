"""GPU parity tests (-m gpu): every check goes through the C ABI of librt_hip.so and compares with
the oracle on the same seeded inputs or with the committed golden fixtures.  Bar: bit-exact —
the arithmetic contract makes GPU == oracle by construction, so the north star's 1e-4 RGB tolerance
is asserted as a consequence (max |diff| == 0 <= 1e-4), never used as slack."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

TOL_RGB = 1e-4  # BASELINE.json north_star tolerance; the tests demand 0


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_same(a, b, what):
    assert a.shape == b.shape, what
    if not np.array_equal(bits(a), bits(b)):
        d = np.nanmax(np.abs(a.astype(np.float64) - b.astype(np.float64)))
        raise AssertionError("%s: %d of %d values differ, max abs diff %g (tolerance %g)" % (
            what, int(np.count_nonzero(bits(a) != bits(b))), a.size, d, TOL_RGB))


@pytest.fixture(scope="module")
def scenes_mod(built):
    from cpuraytracer_amd import scenes
    return scenes


# ------------------------------------------------------------------------- unit level
def test_native_library_is_the_one_loaded(hip):
    from cpuraytracer_amd import LIB_PATH
    maps = open("/proc/self/maps").read()
    assert LIB_PATH in maps, "librt_hip.so is not mapped into the test process"


def test_halton_device_vs_oracle_and_known_answers(hip, oracle):
    import json
    rng = np.random.default_rng(0)
    idx = np.concatenate([np.arange(0, 6000), rng.integers(0, 2 ** 32, 6000, dtype=np.uint64)]).astype(np.uint32)
    for base in (2, 3, 4, 5, 7):
        assert_same(hip.unit_halton(idx, base), oracle.halton_array(idx, base), "halton base %d" % base)
    ka = json.load(open(os.path.join(GOLDEN, "halton_known_answers.json")))
    keys = sorted(int(k) for k in ka["halton"])
    for bi, base in enumerate(ka["bases"]):
        got = hip.unit_halton(np.array(keys, dtype=np.uint32), base)
        want = np.array([float.fromhex(ka["halton"][str(k)][bi]) for k in keys], dtype=np.float32)
        assert_same(got, want, "halton known answers base %d" % base)


def test_elementary_functions_device_vs_oracle(hip, oracle):
    rng = np.random.default_rng(1)
    x = np.concatenate([rng.uniform(0, 2 * np.pi, 300000), [0, np.pi / 2, np.pi, 1.5 * np.pi, 2 * np.pi]]).astype(np.float32)
    assert_same(hip.unit_math(0, x), oracle.math_array(0, x), "sin")
    assert_same(hip.unit_math(1, x), oracle.math_array(1, x), "cos")
    t = rng.uniform(0.0, 1.55, 50000).astype(np.float32)
    assert_same(hip.unit_math(3, t), oracle.math_array(3, t), "tan")
    xb = np.concatenate([rng.uniform(0, 1, 300000), [0, 1, 1e-30, 1e-45, 0.5, 2.0, 10.0]]).astype(np.float32)
    yb = np.concatenate([rng.uniform(0, 40, 300000), [0, 5, 40, 40, 0.4545, 3, 2]]).astype(np.float32)
    assert_same(hip.unit_math(2, xb, yb), oracle.math_array(2, xb, yb), "pow")
    for y in (0.0, 5.0, 16.0, 1 / 2.2):
        yy = np.full_like(xb, np.float32(y))
        assert_same(hip.unit_math(2, xb, yy), oracle.math_array(2, xb, yy), "pow y=%g" % y)


def test_markstein_division_is_ieee_division(hip):
    """The hit processing divides with Markstein's correction on a refined hardware reciprocal instead of the compiler's
    11-operation IEEE sequence (rt_device_math.h).  (a) the refined reciprocal equals 1/b for ALL 2^23 significands, at three
    exponents; (b) the guarded quotient equals the device's plain division and numpy's on millions of operand pairs over the
    whole exponent range (the guard's fallback included), signed zeros and the worst-case significands."""
    sig = np.arange(1 << 23, dtype=np.uint32)
    for e in (27, 127, 227):
        x = (sig | np.uint32(e << 23)).view(np.float32)
        assert_same(hip.unit_math(4, x), (np.float32(1.0) / x).astype(np.float32), "refined reciprocal, exponent %d" % (e - 127))
    rng = np.random.default_rng(3)
    n = 4_000_000
    eb = rng.integers(-30, 110, n)
    ex = eb + rng.integers(-100, 30, n)
    b = (rng.uniform(1, 2, n) * np.exp2(eb.astype(np.float64))).astype(np.float32)
    x = (rng.uniform(1, 2, n) * np.exp2(np.clip(ex, -148, 126).astype(np.float64)) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    x[:1000] = 0.0
    x[1000:2000] = -0.0
    got = hip.unit_math(5, x, b)
    assert_same(got, hip.unit_math(6, x, b), "Markstein quotient vs the device's IEEE division")
    with np.errstate(over="ignore", under="ignore"):
        assert_same(got, (x / b).astype(np.float32), "Markstein quotient vs numpy")
    xs = rng.uniform(-4, 4, 500_000).astype(np.float32)
    for bits_ in (0x3fffffff, 0x3f800000, 0x3f800001, 0x3ffffffe, 0x3fc00000):
        bb = np.full_like(xs, np.array([bits_], dtype=np.uint32).view(np.float32)[0])
        assert_same(hip.unit_math(5, xs, bb), (xs / bb).astype(np.float32), "quotients by significand %#x" % bits_)


def test_fast_square_root_is_ieee_square_root(hip):
    """The path's square root (rt_device_math.h sqrt_rn: v_sqrt_f32, v_rsq_f32 and Markstein's correction, four operations
    instead of the compiler's sixteen) must be the IEEE root.  (a) the fast form alone on EVERY float of its range [2^-80, inf):
    1.74e9 patterns against numpy's correctly rounded root; (b) the guarded form as the path calls it, and the compiler's own
    sqrtf on the device, on every kind of input -- zeros, denormals, the range's edges, negatives, inf, NaN, mixed into waves
    of ordinary values (one lane outside the fast range sends its whole wave through the compiler's sequence)."""
    lo, hi, step = 0x17800000, 0x7f800000, 1 << 26
    for base in range(lo, hi, step):
        bits_ = np.arange(base, min(base + step, hi), dtype=np.uint32)
        x = bits_.view(np.float32)
        assert_same(hip.unit_math(8, x), np.sqrt(x), "fast square root, patterns from %#x" % base)
    rng = np.random.default_rng(11)
    x = rng.integers(0, 1 << 32, 8_000_000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    specials = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, 1.1754942e-38, 1.17549435e-38, 8.27e-25, 8.2718061e-25, 3.4028235e38, -1.0],
                        dtype=np.float32)
    x[rng.integers(0, x.size, 200_000)] = specials[rng.integers(0, specials.size, 200_000)]
    pos = np.abs(rng.normal(0, 4, 4_000_000)).astype(np.float32)  # whole waves inside the fast range
    for arr in (x, pos):
        with np.errstate(invalid="ignore"):
            want = np.sqrt(arr)
        for op in (7, 9):
            got = hip.unit_math(op, arr)
            nan = np.isnan(want)
            assert np.array_equal(np.isnan(got), nan)
            assert_same(got[~nan], want[~nan], "square root, op %d" % op)


def test_camera_rays_device_vs_oracle(hip, oracle, scenes_mod):
    rng = np.random.default_rng(2)
    for name, W, H, ap in (("cover", 1200, 800, -1.0), ("cover", 1920, 1080, 2.0), ("three", 200, 100, -1.0)):
        sc = scenes_mod.build_scene(name, 1, W, H, aperture=ap)
        hip.upload(sc)
        orc = oracle.Oracle()
        orc.upload(sc)
        n = 20000
        ijs = np.stack([rng.integers(0, W, n), rng.integers(0, H, n), rng.integers(1, 1025, n)], 1).astype(np.uint32)
        ijs[:4] = [[0, 0, 1], [W - 1, H - 1, 1024], [0, H - 1, 1], [W - 1, 0, 512]]
        assert_same(hip.unit_primary_rays(W, H, ijs), orc.primary_rays(W, H, ijs), "%s primary rays" % name)


def test_closest_hit_device_vs_oracle_list_and_bvh(hip, oracle, scenes_mod):
    rng = np.random.default_rng(3)
    sc = scenes_mod.build_scene("cover", 1, 1200, 800)
    hip.upload(sc)
    orc = oracle.Oracle()
    orc.upload(sc)
    n = 20000
    o = np.stack([rng.uniform(-12, 12, n), rng.uniform(0.05, 4, n), rng.uniform(-12, 12, n)], 1)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.concatenate([o, d], 1).astype(np.float32)
    got = hip.unit_closest_hit(rays)
    assert_same(got, orc.closest_hit(rays, oracle.ACCEL_LIST), "closest hit vs list scan")
    assert_same(got, orc.closest_hit(rays, oracle.ACCEL_BVH), "closest hit vs BvhNode")
    idx = got[:, 1].copy().view(np.int32)
    assert (idx >= -1).all() and (idx < sc.n).all() and (idx >= 0).mean() > 0.3


def test_scatter_and_shade_device_vs_oracle(hip, oracle):
    from cpuraytracer_amd import _capi
    rng = np.random.default_rng(4)
    L = hip._L
    k255 = np.float32(1.0) / np.float32(255.0)
    sun = oracle.RtLight()
    sdir = np.float32(1.0) / np.sqrt(np.float32(3.0))
    for k in range(3):
        sun.direction[k] = float(sdir)
        sun.color[k] = float(np.float32((255, 247, 224)[k]) * k255)
    sun.luminance = 40000.0
    view = (C.c_float * 3)(12.0, 2.0, -2.5)
    n = 3000
    for mtype, tex in ((0, 0), (0, 1), (1, 0), (2, 0), (3, 0)):
        m = oracle.RtMaterial()
        m.type, m.tex_type, m.smoothness, m.ior, m.tiling, m.luminance = mtype, tex, 35.5 if mtype != 1 else 0.0, 1.5, 2500.0, 8000.0
        for k in range(3):
            m.rgb0[k] = float(np.float32((230, 128, 26)[k]) * k255)
            m.rgb1[k] = float(np.float32((51, 77, 26)[k]) * k255)
        nrm = rng.normal(size=(n, 3))
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        rd = rng.normal(size=(n, 3))
        rd /= np.linalg.norm(rd, axis=1, keepdims=True)
        pos = rng.uniform(-5, 5, size=(n, 3))
        draws = rng.uniform(0, 1, size=(n, 3))
        draws[: n // 3, 0] *= 0.05  # force the Fresnel-mirror branch often
        inp = np.concatenate([rd, pos, nrm, draws], 1).astype(np.float32)
        out = np.zeros((n, 11), dtype=np.float32)
        mm = _capi.RtMaterial.from_buffer_copy(bytes(m))
        ss = _capi.RtLight.from_buffer_copy(bytes(sun))
        _capi.check(L.rt_unit_scatter(hip._h, C.byref(mm), C.byref(ss), view, inp.ctypes.data, n, out.ctypes.data))
        want = np.zeros_like(out)
        O = oracle.lib()
        for i in range(n):
            f = lambda a: (C.c_float * len(a))(*[float(v) for v in a])
            nx, nz = inp[i, 6], inp[i, 8]
            uv = (C.c_float * 2)(float(np.float32(0.5) * nx + np.float32(0.5)), float(np.float32(0.5) * nz + np.float32(0.5)))
            att, dr, nd, loc = (C.c_float * 3)(), (C.c_float * 3)(), C.c_uint32(), (C.c_float * 3)()
            sc = O.orc_unit_scatter(C.byref(m), f(inp[i, 0:3]), f(inp[i, 3:6]), f(inp[i, 6:9]), uv, f(inp[i, 9:12]), att, dr, C.byref(nd))
            O.orc_unit_emit_shade(C.byref(m), C.byref(sun), view, f(inp[i, 3:6]), f(inp[i, 6:9]), uv, loc)
            if mtype == 3:
                att = (C.c_float * 3)(1.0, 1.0, 1.0)  # Emissive::Scatter leaves outAttenuation untouched; device reports 1
            want[i] = [float(sc), att[0], att[1], att[2], dr[0], dr[1], dr[2], float(nd.value), loc[0], loc[1], loc[2]]
        if mtype in (0, 1):
            # non-scattering (back-facing) hits: attenuation/direction are unspecified in the reference; compare the rest
            ns = want[:, 0] == 0
            out[ns, 1:7] = 0
            want[ns, 1:7] = 0
        assert_same(out, want, "scatter+shade material type %d tex %d" % (mtype, tex))


def test_tonemap_device_vs_oracle(hip, oracle):
    from cpuraytracer_amd import _capi
    rng = np.random.default_rng(5)
    hdr = np.concatenate([rng.uniform(0, 3, (20000, 3)), rng.uniform(0, 0.01, (5000, 3)), [[0, 0, 0], [1e6, 1e6, 1e6]]]).astype(np.float32)
    for ns in (1, 3, 128):
        out = np.zeros((hdr.shape[0], 3), dtype=np.uint8)
        _capi.check(hip._L.rt_unit_tonemap(hip._h, hdr.ctypes.data, hdr.shape[0], ns, out.ctypes.data))
        want = np.zeros_like(out)
        o = (C.c_uint8 * 3)()
        for i in range(hdr.shape[0]):
            oracle.lib().orc_tonemap((C.c_float * 3)(*[float(v) for v in hdr[i]]), ns, o)
            want[i] = list(o)
        assert_same(out, want, "tonemap n=%d" % ns)


# ----------------------------------------------------------------- golden fixtures
def test_c1_against_committed_golden(hip, scenes_mod):
    g = np.load(os.path.join(GOLDEN, "c1_three_200x100_spp1_d8.npz"))
    hip.upload(scenes_mod.build_scene("three", 1, 200, 100))
    st = hip.render(200, 100, 1, 2, 8, 1)
    hip.resolve()
    hdr, ldr = hip.download()
    assert_same(hdr, g["hdr"], "C1 HDR vs golden")
    assert_same(ldr, g["ldr"], "C1 LDR vs golden")
    assert np.max(np.abs(hdr - g["hdr"])) <= TOL_RGB
    assert st.traversals == int(g["traversals"]) and st.segments == int(g["segments"]) and st.samples == 20000


def test_cover_small_against_committed_golden(hip, scenes_mod):
    g = np.load(os.path.join(GOLDEN, "cover_96x64_spp4_d50.npz"))
    hip.upload(scenes_mod.build_scene("cover", 1, 96, 64))
    st = hip.render(96, 64, 1, 5, 50, 1)
    hip.resolve()
    hdr, ldr = hip.download()
    assert_same(hdr, g["hdr"], "cover 96x64 HDR vs golden")
    assert_same(ldr, g["ldr"], "cover 96x64 LDR vs golden")
    assert st.traversals == int(g["traversals"]) and st.segments == int(g["segments"])


def test_headline_config_per_sample_golden(hip, scenes_mod):
    g = np.load(os.path.join(GOLDEN, "c2_cover_1200x800_samples.npz"))
    hip.upload(scenes_mod.build_scene("cover", 1, 1200, 800))
    rgb, trav = hip.unit_trace(1200, 800, g["ijs"], 50, 1)
    assert_same(rgb, g["rgb"], "C2 per-sample radiance vs golden")
    assert np.array_equal(trav, g["traversals"])
    assert_same(hip.unit_primary_rays(1200, 800, g["ijs"]), g["rays"], "C2 primary rays vs golden")
    assert_same(hip.unit_closest_hit(g["rays"]), g["hits"], "C2 closest hits vs golden")


# ---------------------------------------------------------- images vs the live oracle
@pytest.mark.parametrize("name,W,H,s1,depth,ap", [
    ("three", 200, 100, 2, 8, -1.0),     # C1
    ("cover", 160, 104, 4, 50, -1.0),    # C2 geometry, small
    ("cover", 160, 90, 3, 50, 2.0),      # C4: depth-of-field camera, aperture 2.0
    ("three", 37, 23, 6, 3, 0.5),        # ragged sizes, shallow depth
    ("three", 1, 1, 3, 8, -1.0),         # one pixel: a single partial tile of the sample buffer
    ("three", 65, 1, 2, 8, -1.0),        # one full 64-pixel tile + a one-pixel tile
    ("cover", 129, 3, 130, 50, -1.0),    # more samples than a queue block per pixel row, ragged tiles
])
def test_image_parity_with_oracle(hip, oracle, scenes_mod, name, W, H, s1, depth, ap):
    sc = scenes_mod.build_scene(name, 1, W, H, aperture=ap)
    hip.upload(sc)
    orc = oracle.Oracle()
    orc.upload(sc)
    sg = hip.render(W, H, 1, s1 + 1, depth, 11)
    hip.resolve()
    hg, lg = hip.download()
    so = orc.render(W, H, 1, s1 + 1, depth, 11, threads=8)
    orc.resolve()
    ho, lo = orc.download()
    assert_same(hg, ho, "HDR")
    assert_same(lg, lo, "LDR")
    assert sg.traversals == so.traversals and sg.segments == so.segments and sg.samples == so.samples


def test_grid10k_scene_descends_the_bounds_hierarchy(hip, oracle, scenes_mod):
    # C5 geometry: 10,004 spheres -> 2,504 groups -> 4 levels of bounds; tables stay in global memory (L2)
    sc = scenes_mod.build_scene("grid10k", 1, 64, 64)
    assert sc.n == 10004
    hip.upload(sc)
    orc = oracle.Oracle()
    orc.upload(sc)
    sg = hip.render(64, 64, 1, 2, 50, 1)
    hg, _ = hip.download(ldr=False)
    so = orc.render(64, 64, 1, 2, 50, 1, accel=oracle.ACCEL_PADDED_LIST, threads=8)
    ho, _ = orc.download()
    assert_same(hg, ho, "grid10k HDR")
    assert sg.traversals == so.traversals
    # C5's own aspect and a grazing view over the whole field (many candidate nodes per ray)
    n = 1500
    rng = np.random.default_rng(8)
    ijs = np.stack([rng.integers(0, 4096, n), rng.integers(0, 4096, n), rng.integers(1, 65, n)], 1).astype(np.uint32)
    sc2 = scenes_mod.build_scene("grid10k", 1, 4096, 4096)
    hip.upload(sc2)
    orc.upload(sc2)
    rg, tg = hip.unit_trace(4096, 4096, ijs, 50, 1)
    ro, to = orc.trace(4096, 4096, ijs, 50, 1, accel=oracle.ACCEL_PADDED_LIST)
    assert_same(rg, ro, "C5 per-sample radiance")
    assert np.array_equal(tg, to)


def test_forced_global_tables_equal_lds_tables(hip, scenes_mod, monkeypatch):
    from cpuraytracer_amd import HipRenderer
    sc = scenes_mod.build_scene("cover", 1, 96, 64)
    hip.upload(sc)
    hip.render(96, 64, 1, 3, 50, 1)
    a, _ = hip.download(ldr=False)
    monkeypatch.setenv("RT_FORCE_GLOBAL_TABLES", "1")
    r2 = HipRenderer(0)
    r2.upload(sc)
    r2.render(96, 64, 1, 3, 50, 1)
    b, _ = r2.download(ldr=False)
    r2.close()
    assert_same(a, b, "LDS-staged vs global-memory tables")


def test_prepared_path_cache_equals_per_lane_generation(hip, scenes_mod, monkeypatch):
    """RT_RAY_CACHE=0 makes idle lanes generate their own path instead of popping the wave's LDS cache of 64
    prepared paths: same image, same traversal counters (tail blocks shorter than 64 paths included: 97x61 pixels)."""
    from cpuraytracer_amd import HipRenderer
    sc = scenes_mod.build_scene("cover", 1, 97, 61)
    hip.upload(sc)
    sa = hip.render(97, 61, 1, 4, 50, 1)
    a, _ = hip.download(ldr=False)
    monkeypatch.setenv("RT_RAY_CACHE", "0")
    r2 = HipRenderer(0)
    r2.upload(sc)
    sb = r2.render(97, 61, 1, 4, 50, 1)
    b, _ = r2.download(ldr=False)
    r2.close()
    assert_same(a, b, "cached vs per-lane path generation")
    assert (sa.traversals, sa.segments) == (sb.traversals, sb.segments)


# ----------------------------------------------- the scan's filter machinery
def _custom_scene(oracle, centers, radii, types, cam_origin, cam_look, vfov, aspect, aperture=0.0):
    """Flat scene from arrays (tests only): colours/smoothness fixed, camera via the oracle's Camera."""
    n = len(radii)
    sph = np.zeros(n, dtype=oracle.SPHERE_DTYPE)
    sph["cx"], sph["cy"], sph["cz"], sph["r"] = centers[:, 0], centers[:, 1], centers[:, 2], radii
    mat = np.zeros(n, dtype=oracle.MATERIAL_DTYPE)
    k255 = np.float32(1) / np.float32(255)
    mat["type"] = types
    mat["smoothness"] = np.where(np.asarray(types) == 1, 0.0, 16.0)
    mat["ior"] = 1.5
    mat["rgb0"] = (np.array([200, 120, 60], dtype=np.float32) * k255)[None, :]
    ref = oracle.build_scene("three", 1, aspect)
    cam = oracle.RtCamera()
    o = np.asarray(cam_origin, dtype=np.float64)
    la = np.asarray(cam_look, dtype=np.float64)
    oracle.lib().orc_camera_make((C.c_float * 3)(*o), (C.c_float * 3)(*la), vfov, aspect, float(np.linalg.norm(o - la)), aperture,
                                 C.byref(cam))
    return oracle.Scene(sph, mat, cam, ref.sun, ref.sky, ref.exposure_scale, "custom", 0)


def _assert_image_equals_oracle(hip, oracle, sc, W, H, spp, depth, seed=3):
    hip.upload(sc)
    orc = oracle.Oracle()
    orc.upload(sc)
    sg = hip.render(W, H, 1, 1 + spp, depth, seed)
    hg, _ = hip.download(ldr=False)
    so = orc.render(W, H, 1, 1 + spp, depth, seed, accel=oracle.ACCEL_PADDED_LIST, threads=8)
    ho, _ = orc.download()
    assert_same(hg, ho, "custom scene HDR")
    assert sg.traversals == so.traversals and sg.segments == so.segments


def test_matrix_core_scan_equals_valu_scan(hip, scenes_mod, monkeypatch):
    """RT_SCAN=valu (no MFMA filter) and the default matrix-core scan give the same bits."""
    from cpuraytracer_amd import HipRenderer
    sc = scenes_mod.build_scene("cover", 1, 160, 104)
    hip.upload(sc)
    sa = hip.render(160, 104, 1, 5, 50, 1)
    a, _ = hip.download(ldr=False)
    monkeypatch.setenv("RT_SCAN", "valu")
    r2 = HipRenderer(0)
    r2.upload(sc)
    sb = r2.render(160, 104, 1, 5, 50, 1)
    b, _ = r2.download(ldr=False)
    r2.close()
    assert_same(a, b, "matrix-core scan vs VALU scan")
    assert sa.traversals == sb.traversals


def test_bounds_hierarchy_descent_equals_flat_filter(hip, scenes_mod, monkeypatch):
    """RT_TREE_TOP=16 forces a three-level bounds hierarchy (matrix-core filter on 8 top nodes, per-lane descent
    below, tables through L2) on the cover scene; the default is the flat filter over all 126 groups."""
    from cpuraytracer_amd import HipRenderer
    sc = scenes_mod.build_scene("cover", 1, 160, 104)
    hip.upload(sc)
    sa = hip.render(160, 104, 1, 5, 50, 1)
    a, _ = hip.download(ldr=False)
    for top in ("16", "32"):
        monkeypatch.setenv("RT_TREE_TOP", top)
        r2 = HipRenderer(0)
        r2.upload(sc)
        sb = r2.render(160, 104, 1, 5, 50, 1)
        b, _ = r2.download(ldr=False)
        r2.close()
        assert_same(a, b, "hierarchy descent (top <= %s) vs flat filter" % top)
        assert sa.traversals == sb.traversals


def test_candidate_list_overflow_falls_back_exactly(hip, oracle):
    """A ray skimming a long row of 240 spheres has possible roots in up to 60 groups, more than the 20 entries the
    lane's phase-A list holds: the surplus groups are resolved on the spot, and the image must still equal the oracle's."""
    n = 240
    centers = np.stack([np.arange(n) * 0.5 - 30.0, np.zeros(n), np.full(n, 5.0)], 1).astype(np.float32)
    centers = np.concatenate([centers, [[0.0, -1000.2, 5.0]]]).astype(np.float32)
    radii = np.concatenate([np.full(n, 0.2), [1000.0]]).astype(np.float32)
    types = np.concatenate([np.tile([0, 1, 2], n // 3), [0]]).astype(np.uint32)
    # camera far to the side looking ALONG the row: primary rays cross dozens of group bounds
    sc = _custom_scene(oracle, centers, radii, types, (-45.0, 0.05, 5.0), (30.0, 0.0, 5.0), 8.0, 2.0)
    _assert_image_equals_oracle(hip, oracle, sc, 96, 48, 2, 12)


@pytest.mark.parametrize("offset,scale", [((5000.0, -3000.0, 7000.0), 1.0), ((0.0, 0.0, 0.0), 0.01), ((300.0, 50.0, -200.0), 40.0)])
def test_filter_margins_hold_far_from_the_origin_and_at_odd_scales(hip, oracle, offset, scale):
    """The filter's rounding margin scales with |o|^2 and |C|^2: translate/scale a random cluster so that those
    terms dominate the sphere sizes and check that no hit is lost (image == oracle, bit for bit)."""
    rng = np.random.default_rng(9)
    n = 150
    base = rng.uniform(-6, 6, size=(n, 3))
    base[:, 1] = np.abs(base[:, 1]) * 0.3
    radii = rng.uniform(0.05, 0.6, n)
    centers = (base * scale + np.asarray(offset)).astype(np.float32)
    radii = (radii * scale).astype(np.float32)
    floor_c = (np.array([0.0, -500.0, 0.0]) * scale + np.asarray(offset)).astype(np.float32)
    centers = np.concatenate([centers, floor_c[None, :]]).astype(np.float32)
    radii = np.concatenate([radii, [np.float32(499.7 * scale)]]).astype(np.float32)
    types = np.concatenate([rng.integers(0, 3, n), [0]]).astype(np.uint32)
    cam_o = np.array([9.0, 2.0, -7.0]) * scale + np.asarray(offset)
    cam_l = np.array([0.0, 0.5, 0.0]) * scale + np.asarray(offset)
    sc = _custom_scene(oracle, centers, radii, types, cam_o, cam_l, 40.0, 1.5, aperture=0.05 * scale)
    _assert_image_equals_oracle(hip, oracle, sc, 120, 80, 2, 20)


@pytest.mark.parametrize("seed,n", [(1, 5), (2, 37), (3, 130), (4, 511), (5, 513), (6, 700), (7, 2300), (8, 64), (9, 300), (10, 1200)])
def test_random_scenes_differential(hip, oracle, seed, n):
    """Differential fuzzing: random sphere soups (sizes over three decades, overlapping spheres, every material and
    texture kind, emissive spheres, random cameras with and without depth of field) — per-sample radiance, traversal
    counts and closest hits must equal the oracle's bit for bit.  n <= 512 runs the flat matrix-core filter, larger
    scenes the bounds hierarchy."""
    _fuzz_case(hip, oracle, seed, n, 1.0, (0.0, 0.0, 0.0))


@pytest.mark.parametrize("seed,n,scale,offset", [
    (21, 400, 1e-3, (0.0, 0.0, 0.0)), (22, 480, 1e3, (0.0, 0.0, 0.0)), (23, 350, 1.0, (2.0e4, -1.0e4, 1.5e4)),
    (24, 500, 1e2, (3.0e5, 1.0e5, -2.0e5)), (25, 120, 1e-2, (7.0, -3.0, 11.0)), (26, 1500, 10.0, (-4.0e3, 2.0e3, 9.0e3)),
    (27, 509, 1.0, (0.0, 0.0, 0.0)), (28, 33, 1e3, (1.0e6, 0.0, -1.0e6))])
def test_random_scenes_scaled_and_translated_differential(hip, oracle, seed, n, scale, offset):
    """The same differential test with the whole scene (spheres and camera) scaled over six decades and moved far from
    the origin: the split-bf16 filter's margins are relative to |o|^2 and |C|^2, the shadow index's to P0 and |c|, so
    this is where a too-small margin would lose a hit."""
    _fuzz_case(hip, oracle, seed, n, scale, offset)


def _fuzz_scene(oracle, seed, n, scale, offset):
    rng = np.random.default_rng(1000 + seed)
    offset = np.asarray(offset, dtype=np.float64)
    extent = rng.choice([3.0, 12.0, 60.0])
    centers = rng.uniform(-extent, extent, size=(n, 3))
    centers[:, 1] = np.abs(centers[:, 1]) * 0.25
    radii = np.exp(rng.uniform(np.log(0.02), np.log(1.5), n)) * extent / 12.0
    if seed % 2 == 0:  # a huge floor like the cover scene's
        centers = np.concatenate([centers, [[0.0, -400.0 - radii.max(), 0.0]]])
        radii = np.concatenate([radii, [400.0]])
    n = len(radii)
    types = rng.choice([0, 0, 0, 1, 2, 3], n).astype(np.uint32)
    cam_o = (rng.uniform(-1, 1, 3) * extent * 1.2 + [0, extent * 0.4, 0]) * scale + offset
    cam_l = rng.uniform(-0.3, 0.3, 3) * extent * scale + offset
    sc = _custom_scene(oracle, (centers * scale + offset).astype(np.float32), (radii * scale).astype(np.float32), types, cam_o, cam_l,
                       float(rng.uniform(20, 70)), 1.5, aperture=float(rng.choice([0.0, 0.3, 2.0])) * scale)
    k255 = np.float32(1) / np.float32(255)
    sc.materials["tex_type"] = rng.integers(0, 2, n)
    sc.materials["tiling"] = rng.choice([4.0, 50.0, 2500.0], n)
    sc.materials["rgb0"] = rng.integers(0, 256, (n, 3)).astype(np.float32) * k255
    sc.materials["rgb1"] = rng.integers(0, 256, (n, 3)).astype(np.float32) * k255
    sc.materials["smoothness"] = np.where(types == 1, 0.0, rng.uniform(1.0, 64.0, n)).astype(np.float32)
    sc.materials["ior"] = rng.uniform(1.1, 2.4, n).astype(np.float32)
    sc.materials["luminance"] = np.where(types == 3, rng.uniform(100.0, 20000.0, n), 0.0).astype(np.float32)
    return sc, rng


def _fuzz_case(hip, oracle, seed, n, scale, offset):
    sc, rng = _fuzz_scene(oracle, seed, n, scale, offset)
    hip.upload(sc)
    orc = oracle.Oracle()
    orc.upload(sc)
    W, H, m = 300, 200, 3000
    ijs = np.stack([rng.integers(0, W, m), rng.integers(0, H, m), rng.integers(1, 600, m)], 1).astype(np.uint32)
    rays = orc.primary_rays(W, H, ijs)
    assert_same(hip.unit_primary_rays(W, H, ijs), rays, "primary rays")
    assert_same(hip.unit_closest_hit(rays), orc.closest_hit(rays, oracle.ACCEL_PADDED_LIST), "closest hits")
    rg, tg = hip.unit_trace(W, H, ijs, 30, 77 + seed)
    ro, to = orc.trace(W, H, ijs, 30, 77 + seed, accel=oracle.ACCEL_PADDED_LIST)
    assert_same(rg, ro, "per-sample radiance")
    assert np.array_equal(tg, to)
    assert np.isfinite(rg).all()


@pytest.mark.parametrize("seed,n,W,H,spp", [(31, 60, 403, 203, 3), (32, 400, 320, 203, 2), (33, 1500, 403, 160, 2)])
def test_random_scene_images_equal_the_oracle_render(hip, oracle, seed, n, W, H, spp):
    """The same random scenes as WHOLE IMAGES (1,000+ tiles, so the work order from pilot rays is built; the queue, the ordered
    accumulation and the counters are on the path): HDR strip, traversal and segment counts equal the oracle's render."""
    sc, _ = _fuzz_scene(oracle, seed, n, 1.0, (0.0, 0.0, 0.0))
    _assert_image_equals_oracle(hip, oracle, sc, W, H, spp, 20, seed=9 + seed)


@pytest.mark.parametrize("W,H,spp,cx", [(256, 64, 2, 0.0), (256, 64, 2, 1.1), (403, 37, 3, -0.9), (64, 8, 5, 0.6)])
def test_hits_left_in_the_stash_when_every_lane_finishes_are_not_lost(hip, oracle, W, H, spp, cx):
    """Regression (round 3, hit stash): a wave whose 64 processed hits ALL end their paths (a tile looking at an Emissive
    sphere: no scatter) falls idle while earlier hits still wait in its stash; with no fresh paths left it used to leave the
    loop and lose them (missing samples, missing shadow traversals).  An emissive sphere that covers most, all, or part of
    every 64-pixel tile, few enough paths that every wave only has its static block."""
    centers = np.array([[cx, 0.0, 0.0], [0.0, -101.0, 0.0], [2.5, 0.0, 0.5]], dtype=np.float32)
    radii = np.array([1.0, 100.0, 0.5], dtype=np.float32)
    sc = _custom_scene(oracle, centers, radii, np.array([3, 0, 1], dtype=np.uint32), (0.0, 0.3, -4.0), (0.0, 0.0, 0.0), 35.0, W / float(H))
    sc.materials["luminance"] = np.array([5000.0, 0.0, 0.0], dtype=np.float32)
    _assert_image_equals_oracle(hip, oracle, sc, W, H, spp, 12, seed=5)


def _layer_scene(oracle, rng, n, side, cam_o, cam_l, vfov=40.0, plane="xz", clump=0, n_big=0, r_small=0.2):
    """n small spheres in a layer (plus a floor): the scene class of the cell-grid scan, with the knobs that stress it."""
    a, b = rng.uniform(-side, side, n), rng.uniform(-side, side, n)
    if clump:
        a[:clump], b[:clump] = rng.uniform(-1.5, 1.5, clump), rng.uniform(-1.5, 1.5, clump)
    h = np.full(n, r_small) + rng.uniform(0, 0.05, n)
    c = np.stack([a, h, b], 1) if plane == "xz" else np.stack([a, b + side + 1.0, h], 1)
    r_ = np.full(n, r_small) * rng.uniform(0.5, 1.0, n)
    t = rng.choice([0, 0, 0, 1, 2, 3], n)
    c = np.concatenate([c, [[0.0, -1000.0, 0.0]]])
    r_ = np.concatenate([r_, [1000.0]])
    t = np.concatenate([t, [0]])
    for k in range(n_big):
        c = np.concatenate([c, [[rng.uniform(-side, side), 3.0, rng.uniform(-side, side)]]])
        r_ = np.concatenate([r_, [3.0]])
        t = np.concatenate([t, [rng.choice([0, 1, 2])]])
    sc = _custom_scene(oracle, c.astype(np.float32), r_.astype(np.float32), t.astype(np.uint32), cam_o, cam_l, vfov, 1.5)
    sc.materials["luminance"] = np.where(sc.materials["type"] == 3, 3000.0, 0.0).astype(np.float32)
    return sc


@pytest.mark.parametrize("case", ["grazing", "far_camera", "wall", "clumped", "nine_big", "inside_layer", "tiny_spheres"])
def test_cell_grid_scan_stress_scenes_equal_the_oracle(hip, oracle, case):
    """Scenes built against the cell-grid scan's weak spots, as whole images vs the oracle's list semantics: rays that skim the
    whole layer (hundreds of slabs per ray), a camera thousands of units away (the per-ray reach, hence the walk's dilation, grows
    with |o|), a layer in a vertical plane (another thin axis), 1,500 spheres clumped into a few cells (runs of hundreds of entries
    per item), nine big spheres (the grid builder refuses: bounds hierarchy), a camera inside the layer, spheres of 2 cm."""
    rng = np.random.default_rng({"grazing": 1, "far_camera": 2, "wall": 3, "clumped": 4, "nine_big": 5, "inside_layer": 6, "tiny_spheres": 7}[case])
    if case == "grazing":
        sc = _layer_scene(oracle, rng, 4000, 60.0, (70.0, 0.25, 0.3), (-60.0, 0.2, 0.0), vfov=20.0)
    elif case == "far_camera":
        sc = _layer_scene(oracle, rng, 3000, 40.0, (2500.0, 900.0, -1800.0), (0.0, 0.0, 0.0), vfov=2.5)
    elif case == "wall":
        sc = _layer_scene(oracle, rng, 2500, 30.0, (5.0, 35.0, -60.0), (0.0, 31.0, 0.0), plane="xy")
    elif case == "clumped":
        sc = _layer_scene(oracle, rng, 2000, 100.0, (6.0, 3.0, -6.0), (0.0, 0.2, 0.0), clump=1500)
    elif case == "nine_big":
        sc = _layer_scene(oracle, rng, 2000, 30.0, (35.0, 8.0, -20.0), (0.0, 1.0, 0.0), n_big=9)
    elif case == "inside_layer":
        sc = _layer_scene(oracle, rng, 5000, 50.0, (0.37, 0.21, 0.41), (20.0, 0.2, 3.0), vfov=80.0)
    else:
        sc = _layer_scene(oracle, rng, 6000, 3.0, (4.0, 0.6, -3.0), (0.0, 0.02, 0.0), r_small=0.02)
    _assert_image_equals_oracle(hip, oracle, sc, 192, 128, 2, 20, seed=11)


# ------------------------------------------- properties at BASELINE.json's full size (C2)
@pytest.fixture(scope="module")
def c2_full(hip, scenes_mod):
    sc = scenes_mod.build_scene("cover", 1, 1200, 800)
    hip.upload(sc)
    st = hip.render(1200, 800, 1, 129, 50, 1)
    hip.resolve()
    hdr, ldr = hip.download()
    return sc, st, hdr, ldr


def test_c2_full_size_counts_and_idempotence(hip, c2_full):
    sc, st, hdr, ldr = c2_full
    assert st.samples == 1200 * 800 * 128 and st.passes == 1
    assert st.segments <= st.traversals <= 2 * st.segments and st.traversals >= st.samples
    assert np.isfinite(hdr).all() and (hdr >= 0).all()
    st2 = hip.render(1200, 800, 1, 129, 50, 1)
    hip.resolve()
    hdr2, ldr2 = hip.download()
    assert_same(hdr2, hdr, "second launch of the same render")
    assert_same(ldr2, ldr, "second launch LDR")
    assert st2.traversals == st.traversals and st2.segments == st.segments


def test_c2_full_size_pixels_equal_oracle_sum_of_samples(hip, oracle, c2_full):
    sc, st, hdr, ldr = c2_full
    orc = oracle.Oracle()
    orc.upload(sc)
    rng = np.random.default_rng(6)
    pix = np.stack([rng.integers(0, 1200, 48), rng.integers(0, 800, 48)], 1)
    pix[:3] = [[0, 0], [1199, 799], [600, 430]]
    out = (C.c_uint8 * 3)()
    for i, j in pix:
        ijs = np.array([[i, j, s] for s in range(1, 129)], dtype=np.uint32)
        rgb, _ = orc.trace(1200, 800, ijs, 50, 1)
        acc = np.zeros(3, dtype=np.float32)
        for s in range(128):
            acc = acc + rgb[s]  # sequential in s: the reference's summation order
        assert np.array_equal(acc.view(np.uint32), hdr[j, i].view(np.uint32)), (i, j)
        oracle.lib().orc_tonemap((C.c_float * 3)(*[float(v) for v in acc]), 128, out)
        assert list(out) == list(ldr[j, i])


def test_c2_full_size_sharded_and_progressive_and_multipass_identity(hip, c2_full):
    from cpuraytracer_amd import cyclic_rows, distributed as D
    sc, st, hdr, ldr = c2_full
    # (a) 8-way cyclic row shards reassemble to the one-shot image (C3's partition, 1 device)
    parts, trav = [], 0
    for rank in range(8):
        s = hip.render(1200, 800, 1, 129, 50, 1, rowset=cyclic_rows(800, rank, 8))
        assert s.local_rows == 100
        trav += s.traversals
        parts.append(hip.download(ldr=False)[0])
    assert trav == st.traversals
    assert_same(D.assemble(parts, 800, 8), hdr, "8 shards reassembled")
    # (b) progressive: 1..64 then 65..128 continues the accumulation
    hip.render(1200, 800, 1, 65, 50, 1)
    hip.render(1200, 800, 65, 129, 50, 1)
    assert_same(hip.download(ldr=False)[0], hdr, "progressive 64+64")
    # (c) workspace-limited multi-pass split (sample buffer smaller than the job)
    hip.set_workspace_limit(200 << 20)
    s = hip.render(1200, 800, 1, 129, 50, 1)
    hip.set_workspace_limit(64 << 30)
    assert s.passes > 1 and s.traversals == st.traversals
    assert_same(hip.download(ldr=False)[0], hdr, "multi-pass render")


def test_c3_full_size_eight_shards_equal_one_shot(hip, scenes_mod):
    """BASELINE config 3 on one device: 1200x800, spp 1024, rows in 8 cyclic shards (what each of 8 GPUs renders)
    versus the one-shot render (11.8 GB of samples: one pass in the default workspace, which is sized for 288 GB of HBM)."""
    from cpuraytracer_amd import cyclic_rows, distributed as D
    hip.upload(scenes_mod.build_scene("cover", 1, 1200, 800))
    st = hip.render(1200, 800, 1, 1025, 50, 1)
    assert st.samples == 1200 * 800 * 1024 and st.passes == 1
    hip.resolve()
    hdr, ldr = hip.download()
    parts_h, parts_l, trav = [], [], 0
    for rank in range(8):
        s = hip.render(1200, 800, 1, 1025, 50, 1, rowset=cyclic_rows(800, rank, 8))
        assert s.passes == 1 and s.local_rows == 100
        hip.resolve()
        h, l = hip.download()
        parts_h.append(h)
        parts_l.append(l)
        trav += s.traversals
    assert trav == st.traversals
    assert_same(D.assemble(parts_h, 800, 8), hdr, "C3 HDR: 8 shards vs one shot")
    assert_same(D.assemble(parts_l, 800, 8), ldr, "C3 LDR: 8 shards vs one shot")


def test_c4_full_size_depth_of_field(hip, oracle, scenes_mod):
    """BASELINE config 4: 1920x1080, spp 512, aperture 2.0 (divergent lens sampling).  Full-size properties +
    spot checks against the oracle (per-sample vectors, whole-pixel sums in the reference's order)."""
    sc = scenes_mod.build_scene("cover", 1, 1920, 1080, aperture=2.0)
    hip.upload(sc)
    st = hip.render(1920, 1080, 1, 513, 50, 1)
    assert st.samples == 1920 * 1080 * 512
    hip.resolve()
    hdr, ldr = hip.download()
    assert np.isfinite(hdr).all() and (hdr >= 0).all()
    st2 = hip.render(1920, 1080, 1, 513, 50, 1)
    assert st2.traversals == st.traversals
    assert_same(hip.download(ldr=False)[0], hdr, "C4 second launch")
    orc = oracle.Oracle()
    orc.upload(sc)
    rng = np.random.default_rng(44)
    n = 1200
    ijs = np.stack([rng.integers(0, 1920, n), rng.integers(0, 1080, n), rng.integers(1, 513, n)], 1).astype(np.uint32)
    rg, tg = hip.unit_trace(1920, 1080, ijs, 50, 1)
    ro, to = orc.trace(1920, 1080, ijs, 50, 1, accel=oracle.ACCEL_PADDED_LIST)
    assert_same(rg, ro, "C4 per-sample radiance")
    assert np.array_equal(tg, to)
    out = (C.c_uint8 * 3)()
    for i, j in ((0, 0), (1919, 1079), (960, 700), (400, 900), (1500, 650), (777, 555)):
        pij = np.array([[i, j, s] for s in range(1, 513)], dtype=np.uint32)
        rgb, _ = orc.trace(1920, 1080, pij, 50, 1, accel=oracle.ACCEL_PADDED_LIST)
        acc = np.zeros(3, dtype=np.float32)
        for s in range(512):
            acc = acc + rgb[s]
        assert np.array_equal(acc.view(np.uint32), hdr[j, i].view(np.uint32)), (i, j)
        oracle.lib().orc_tonemap((C.c_float * 3)(*[float(v) for v in acc]), 512, out)
        assert list(out) == list(ldr[j, i])


# ------------------------------------------------------------------- frame pipelining (progressive use)
@pytest.mark.parametrize("W,H,frames,spf,depth", [(1200, 800, 48, 1, 4), (161, 103, 40, 1, 2), (320, 200, 12, 3, 6), (96, 64, 30, 1, 1)])
def test_pipelined_progressive_frames_equal_the_one_shot_render(hip, scenes_mod, W, H, frames, spf, depth):
    """rt_set_frame_pipelining: stats-less 1-spp (or 3-spp) frames whose kernels carry their unfinished paths into the next
    frame's kernel.  (a) a download in mid-stream returns exactly the one-shot image of the samples committed so far (planes
    are added strictly in order); (b) after rt_synchronize the strip equals the one-shot render of all samples bit for bit."""
    from cpuraytracer_amd import HipRenderer
    sc = scenes_mod.build_scene("cover", 1, W, H)
    one = HipRenderer(0)
    one.upload(sc)
    hip.upload(sc)
    try:
        hip.set_frame_pipelining(depth)
        for f in range(frames):
            hip.render(W, H, 1 + f * spf, 1 + (f + 1) * spf, 50, 1, stats=False)
            if f == frames // 2:
                c = hip.committed_samples()
                assert 0 <= c <= (f + 1) * spf and c % spf == 0 and c >= (f + 1 - depth) * spf - spf
                if c > 0:
                    hip.resolve()
                    h_mid, l_mid = hip.download()
                    one.render(W, H, 1, 1 + c, 50, 1)
                    one.resolve()
                    h_ref, l_ref = one.download()
                    assert_same(h_mid, h_ref, "strip in mid-stream (%d of %d samples committed)" % (c, (f + 1) * spf))
                    assert_same(l_mid, l_ref, "LDR in mid-stream")
        hip.synchronize()
        assert hip.committed_samples() == frames * spf
        hip.resolve()
        hdr, ldr = hip.download()
        one.render(W, H, 1, 1 + frames * spf, 50, 1)
        one.resolve()
        h1, l1 = one.download()
        assert_same(hdr, h1, "pipelined frames vs one shot")
        assert_same(ldr, l1, "pipelined frames vs one shot, LDR")
        # a call with statistics settles the pipeline and continues the same accumulation
        st = hip.render(W, H, 1 + frames * spf, 2 + frames * spf, 50, 1)
        assert st.samples == W * H
        one.render(W, H, 1 + frames * spf, 2 + frames * spf, 50, 1)
        assert_same(hip.download(ldr=False)[0], one.download(ldr=False)[0], "continuation after the pipeline")
    finally:
        hip.set_frame_pipelining(0)
        one.close()


@pytest.mark.parametrize("scene,W,H,frames,spf,batch", [("cover", 161, 103, 41, 1, 8), ("cover", 320, 200, 13, 3, 4), ("grid10k", 96, 64, 30, 1, 16),
                                                    ("three", 65, 1, 9, 1, 2)])
def test_batched_progressive_frames_equal_the_one_shot_render(hip, scenes_mod, scene, W, H, frames, spf, batch):
    """rt_set_frame_batch: stats-less frames that continue each other are rendered `batch` sample planes per launch (any scene
    class).  (a) mid-stream the strip holds a whole number of batches and equals the one-shot render of exactly those samples;
    (b) rt_synchronize renders the rest: the strip equals the one-shot render of all samples; (c) a call with statistics, and a
    call that starts a new accumulation, settle what is pending first."""
    from cpuraytracer_amd import HipRenderer
    sc = scenes_mod.build_scene(scene, 1, W, H)
    one = HipRenderer(0)
    one.upload(sc)
    hip.upload(sc)
    try:
        hip.set_frame_batch(batch)
        for f in range(frames):
            hip.render(W, H, 1 + f * spf, 1 + (f + 1) * spf, 50, 1, stats=False)
            if f == frames // 2:
                c = hip.committed_samples()
                done = (f + 1) * spf
                assert c <= done and done - c < batch + spf and c % spf == 0
                if c > 0:
                    hip.resolve()
                    h_mid, l_mid = hip.download()
                    one.render(W, H, 1, 1 + c, 50, 1)
                    one.resolve()
                    h_ref, l_ref = one.download()
                    assert_same(h_mid, h_ref, "strip in mid-stream (%d of %d samples committed)" % (c, done))
                    assert_same(l_mid, l_ref, "LDR in mid-stream")
        hip.synchronize()
        assert hip.committed_samples() == frames * spf
        hip.resolve()
        hdr, ldr = hip.download()
        one.render(W, H, 1, 1 + frames * spf, 50, 1)
        one.resolve()
        h1, l1 = one.download()
        assert_same(hdr, h1, "batched frames vs one shot")
        assert_same(ldr, l1, "batched frames vs one shot, LDR")
        # two more frames stay pending; a call with statistics renders them first and reports only its own samples
        n0 = frames * spf
        hip.render(W, H, 1 + n0, 1 + n0 + spf, 50, 1, stats=False)
        assert hip.committed_samples() in (n0, n0 + spf)
        st = hip.render(W, H, 1 + n0 + spf, 2 + n0 + spf, 50, 1)
        assert st.samples == W * H and hip.committed_samples() == n0 + spf + 1
        one.render(W, H, 1 + n0, 2 + n0 + spf, 50, 1)
        assert_same(hip.download(ldr=False)[0], one.download(ldr=False)[0], "continuation after the batch")
        # a pending frame followed by the start of a new accumulation: the old one is settled, the new one starts clean
        hip.render(W, H, 2 + n0 + spf, 3 + n0 + spf, 50, 1, stats=False)
        hip.render(W, H, 1, 2, 50, 7, stats=False)
        hip.synchronize()
        assert hip.committed_samples() == 1
        one.render(W, H, 1, 2, 50, 7)
        assert_same(hip.download(ldr=False)[0], one.download(ldr=False)[0], "new accumulation after a pending frame")
    finally:
        hip.set_frame_batch(1)
        one.close()


@pytest.mark.parametrize("scene,W,H,frames,spf,ahead", [("cover", 161, 103, 37, 1, 8), ("cover", 320, 200, 11, 3, 4), ("grid10k", 96, 64, 21, 1, 16),
                                                    ("three", 65, 1, 9, 1, 2)])
def test_render_ahead_frames_equal_the_one_shot_render_at_every_frame(hip, scenes_mod, scene, W, H, frames, spf, ahead):
    """rt_set_frame_lookahead: a stats-less frame traces the next `ahead` sample planes with its one launch and adds only its own;
    the frames that continue it only add theirs.  After EVERY frame the strip holds exactly the samples of the calls made (display
    lag 0) and equals the one-shot render of those samples bit for bit; a frame that does not continue (another seed), a call with
    statistics and a new accumulation drop what was traced ahead without a trace of it in the strip."""
    from cpuraytracer_amd import HipRenderer
    sc = scenes_mod.build_scene(scene, 1, W, H)
    one = HipRenderer(0)
    one.upload(sc)
    hip.upload(sc)
    try:
        hip.set_frame_lookahead(ahead)
        for f in range(frames):
            hip.render(W, H, 1 + f * spf, 1 + (f + 1) * spf, 50, 1, stats=False)
            assert hip.committed_samples() == (f + 1) * spf
            if f in (0, 1, ahead - 1, ahead, frames // 2, frames - 1):
                hip.resolve()
                h_f, l_f = hip.download()
                one.render(W, H, 1, 1 + (f + 1) * spf, 50, 1)
                one.resolve()
                h_ref, l_ref = one.download()
                assert_same(h_f, h_ref, "strip after frame %d of %d" % (f + 1, frames))
                assert_same(l_f, l_ref, "LDR after frame %d" % (f + 1))
        n0 = frames * spf
        # a call with statistics continues the accumulation with a launch of its own
        st = hip.render(W, H, 1 + n0, 2 + n0, 50, 1)
        assert st.samples == W * H and hip.committed_samples() == n0 + 1
        one.render(W, H, 1 + n0, 2 + n0, 50, 1)
        assert_same(hip.download(ldr=False)[0], one.download(ldr=False)[0], "continuation with statistics")
        # a frame under ANOTHER seed does not continue what was traced ahead: sequence error as without look-ahead? no -- the
        # sample range continues, so it is rendered, by a launch of its own, with its own seed
        hip.render(W, H, 2 + n0, 3 + n0, 50, 1, stats=False)   # traces ahead under seed 1
        hip.render(W, H, 3 + n0, 4 + n0, 50, 9, stats=False)   # seed 9: own launch
        one.render(W, H, 2 + n0, 3 + n0, 50, 1)
        one.render(W, H, 3 + n0, 4 + n0, 50, 9)
        assert_same(hip.download(ldr=False)[0], one.download(ldr=False)[0], "a frame that does not continue the look-ahead")
        # new accumulation of another size while planes wait in the buffer
        hip.render(W, H, 4 + n0, 5 + n0, 50, 9, stats=False)
        W2, H2 = max(8, W // 2), max(1, H // 2)
        hip.render(W2, H2, 1, 2, 50, 4, stats=False)
        hip.render(W2, H2, 2, 3, 50, 4, stats=False)
        assert hip.committed_samples() == 2
        one.render(W2, H2, 1, 3, 50, 4)
        assert_same(hip.download(ldr=False)[0], one.download(ldr=False)[0], "new accumulation after a look-ahead")
    finally:
        hip.set_frame_lookahead(1)
        one.close()


def test_readers_render_a_pending_batch_that_starts_a_new_picture(hip, scenes_mod):
    """with an accumulation committed, a deferred call with s0 == 1 starts a NEW one -- here of a smaller image.
    rt_resolve / rt_download / rt_copy_to_device must render it first: they used to hand out the OLD strip with the old size into a
    buffer the caller sized for the new picture (heap overflow when the new strip is smaller, a stale frame otherwise)."""
    from cpuraytracer_amd import HipRenderer
    # the HIP runtime librt_hip.so itself is linked against (it is loaded already): the caller-owned device memory of this test
    maps = open("/proc/self/maps").read()
    hiprt = C.CDLL(next(l.split()[-1] for l in maps.splitlines() if "libamdhip64.so" in l))
    sc = scenes_mod.build_scene("cover", 1, 160, 100)
    one = HipRenderer(0)
    one.upload(sc)
    hip.upload(sc)
    try:
        hip.render(160, 100, 1, 5, 50, 1)  # committed: 160x100, four samples
        hip.set_frame_batch(8)
        for (W, H, seed) in ((96, 40, 3), (200, 120, 4)):  # smaller, then larger than the committed strip
            hip.render(W, H, 1, 2, 50, seed, stats=False)  # deferred; starts a new accumulation
            hip.render(W, H, 2, 4, 50, seed, stats=False)  # continues the pending batch
            hip.resolve()
            h_new, l_new = hip.download()
            assert h_new.shape == (H, W, 3) and hip.committed_samples() == 3
            one.render(W, H, 1, 4, 50, seed)
            one.resolve()
            h_ref, l_ref = one.download()
            assert_same(h_new, h_ref, "download of a pending batch that starts a new %dx%d picture" % (W, H))
            assert_same(l_new, l_ref, "LDR of that picture")
            # device-to-device reader: the same strip, and not a byte beyond it
            n = H * W * 3 + 1024
            fill = np.full(n, np.float32(-7.0), dtype=np.float32)
            dev = C.c_void_p()
            assert hiprt.hipMalloc(C.byref(dev), C.c_size_t(4 * n)) == 0
            try:
                assert hiprt.hipMemcpy(dev, C.c_void_p(fill.ctypes.data), C.c_size_t(4 * n), 1) == 0  # host to device
                hip.render(W, H, 1, 2, 50, seed + 10, stats=False)  # again a pending start on top of a committed accumulation
                hip.copy_to_device(dev.value, None)
                hip.synchronize()
                got = np.zeros(n, dtype=np.float32)
                assert hiprt.hipMemcpy(C.c_void_p(got.ctypes.data), dev, C.c_size_t(4 * n), 2) == 0  # device to host
            finally:
                hiprt.hipFree(dev)
            one.render(W, H, 1, 2, 50, seed + 10)
            assert_same(got[:H * W * 3].reshape(H, W, 3), one.download(ldr=False)[0], "copy_to_device of a pending new picture")
            assert (got[H * W * 3:] == -7.0).all()
    finally:
        hip.set_frame_batch(1)
        one.close()


@pytest.mark.parametrize("W,H", [(64, 32), (72, 30)])  # whole 64-pixel tiles; a partial last tile
def test_switching_progressive_modes_mid_accumulation_keeps_the_one_shot_strip(scenes_mod, W, H):
    """One accumulation through every way rt_render sequences its calls, switched while it runs: a batch of 3, a lookahead of 4, a call
    with statistics, pipelining at depth 2, then the workspace limit at its 1 MiB minimum and calls of 100 samples that need several
    passes.  After every reader the HDR strip equals, bit for bit, the one-shot render of the same sample count on a second context,
    and rt_committed_samples is the count the contract of rt_api.h gives.  Public entries only."""
    from cpuraytracer_amd import HipRenderer
    sc = scenes_mod.build_scene("three", 1, W, H)
    ctx, one = HipRenderer(0), HipRenderer(0)
    depth, seed = 8, 1

    def frame(s, stats=False):
        return ctx.render(W, H, s, s + 1, depth, seed, stats=stats)

    def read(n, what):
        assert ctx.committed_samples() == n, what
        ctx.resolve()
        hdr = ctx.download(ldr=False)[0]
        one.render(W, H, 1, 1 + n, depth, seed)
        assert_same(hdr, one.download(ldr=False)[0], "%s: the strip after %d samples" % (what, n))

    try:
        ctx.upload(sc)
        one.upload(sc)
        ctx.set_frame_batch(3)
        for s in (1, 2, 3, 4):
            frame(s)
        read(3, "batch of 3, one call pending")       # the reader hands out the committed strip and leaves the call pending
        ctx.set_frame_batch(1)                         # ... which the setter renders
        ctx.set_frame_lookahead(4)
        frame(5)                                       # traces planes 5..8, adds plane 5
        read(5, "lookahead of 4, first call")
        frame(6)                                       # only adds
        read(6, "lookahead of 4, second call")
        st = frame(7, stats=True)                      # a launch of its own; what was traced ahead is dropped
        assert st.samples == W * H and st.passes == 1
        read(7, "call with statistics")
        ctx.set_frame_lookahead(1)
        ctx.set_frame_pipelining(2)
        for s in (8, 9, 10):
            frame(s)
        c = ctx.committed_samples()
        assert 7 <= c <= 10                            # up to 2 of the newest calls' planes are in flight (and the last commit with them)
        read(c, "pipelining at depth 2, mid-stream")
        ctx.set_frame_pipelining(0)                    # settles what is in flight
        read(10, "pipelining switched off")
        ctx.set_workspace_limit(1 << 20)               # 40 (72x30) or 42 (64x32) sample planes
        ctx.render(W, H, 11, 111, depth, seed, stats=False)
        read(110, "100 samples under a 1 MiB workspace")
        st = ctx.render(W, H, 111, 211, depth, seed)
        assert st.passes > 1 and st.samples == 100 * W * H
        read(210, "the same again, with statistics")
    finally:
        ctx.close()
        one.close()


# ------------------------------------------------------------------ the scene's LIST of lights (material.cpp:4-13)
def _far_camera(oracle, aspect):
    """A camera high above the scene looking at the horizon: most floor hits lie hundreds of units out, beyond every footprint
    index's radius P0, so the shadow rays of those hits take the any-hit over every entry (any_hit_all)."""
    cam = oracle.RtCamera()
    o = (C.c_float * 3)(0.0, 40.0, -60.0)
    l = (C.c_float * 3)(0.0, 0.0, 400.0)
    oracle.lib().orc_camera_make(o, l, 35.0, aspect, 10.0, 0.0, C.byref(cam))
    return cam


@pytest.mark.parametrize("name,W,H,spp,n_lights,far", [("cover", 160, 100, 4, 2, False), ("cover", 144, 96, 3, 3, False), ("cover", 96, 64, 3, 0, False),
                                                       ("cover", 128, 80, 2, 3, True), ("grid10k", 112, 112, 2, 2, False), ("three", 100, 50, 4, 8, False)])
def test_light_list_images_equal_the_oracle(hip, oracle, scenes_mod, name, W, H, spp, n_lights, far):
    """rt_scene_upload with the reference's m_lights as a LIST (spheres-app.h:38; Material::Shade adds the lights in list order,
    material.cpp:4-13): two, three and eight directional lights -- one of them below the horizon (nDotL = 0, and its shadow rays
    run into the floor), one nearly parallel to the first -- and the empty list.  HDR, LDR and the traversal counters (one shadow
    ray per light and hit) equal the oracle's, for the flat, the cell-grid and the tiny-scene kernels, and for hit points far
    outside the footprint indices."""
    sc = scenes_mod.build_scene(name, 1, W, H)
    pool = [sc.sun,
            oracle.make_light((-0.6, 0.7, 0.35), (0.35, 0.55, 1.0), 25000.0),
            oracle.make_light((0.3, -1.0, 0.2), (1.0, 0.2, 0.2), 30000.0),     # below the horizon of the floor
            oracle.make_light((1.0, 1.02, 0.99), (0.2, 1.0, 0.3), 9000.0),     # nearly the first light's direction
            oracle.make_light((0.0, 1.0, 0.0), (1.0, 1.0, 1.0), 5000.0),
            oracle.make_light((-1.0, 0.25, -1.0), (0.9, 0.8, 0.1), 12000.0),
            oracle.make_light((0.2, 0.4, -1.0), (0.5, 0.5, 0.9), 7000.0),
            oracle.make_light((-0.1, 0.9, 0.6), (0.3, 0.3, 0.3), 20000.0)]
    sc.lights = pool[:n_lights]
    if far:
        sc.camera = _far_camera(oracle, W / float(H))
    hip.upload(sc)
    orc = oracle.Oracle()
    orc.upload(sc)
    sg = hip.render(W, H, 1, 1 + spp, 50, 3)
    hip.resolve()
    hg, lg = hip.download()
    so = orc.render(W, H, 1, 1 + spp, 50, 3, threads=8)
    orc.resolve()
    ho, lo = orc.download()
    assert_same(hg, ho, "%s with %d lights: HDR" % (name, n_lights))
    assert_same(lg, lo, "%s with %d lights: LDR" % (name, n_lights))
    assert (sg.traversals, sg.segments) == (so.traversals, so.segments)
    if n_lights >= 2 and not far:
        # the list matters: the same scene under the first light alone is another picture
        sc.lights = pool[:1]
        hip.upload(sc)
        hip.render(W, H, 1, 1 + spp, 50, 3)
        assert not np.array_equal(hip.download(ldr=False)[0], hg)
    del sc.lights


def test_one_light_as_a_list_is_the_single_light_scene(hip, scenes_mod):
    """n_lights == 1 runs the single-light kernels: a scene with lights = [sun] and the scene without the attribute give the same
    bits (and the committed full-size digests keep pinning that path)."""
    sc = scenes_mod.build_scene("cover", 1, 192, 128)
    hip.upload(sc)
    s0 = hip.render(192, 128, 1, 5, 50, 1)
    h0 = hip.download(ldr=False)[0]
    sc.lights = [sc.sun]
    hip.upload(sc)
    s1 = hip.render(192, 128, 1, 5, 50, 1)
    assert_same(hip.download(ldr=False)[0], h0, "lights = [sun]")
    assert s0.traversals == s1.traversals and s0.segments == s1.segments
    del sc.lights


@pytest.mark.parametrize("name,W,H", [("cover", 160, 100), ("grid10k", 112, 80)])
def test_colours_that_are_not_bytes_take_the_unpacked_material_records(hip, oracle, scenes_mod, monkeypatch, name, W, H):
    """The packed 16-byte material record (rt_shade.h load_material16) holds colours as bytes -- every colour the reference can hold
    (XMLoadColor of an XMCOLOR; the oracle, like the reference, stores its textures as XMCOLOR, so colours off that grid are outside
    the parity contract).  The ABI takes floats all the same: a scene with colours that are NOT byte * (1 / 255) must not be packed
    (packing would snap them) -- under RT_MATS16=1 it renders the same bits as with the 48-byte records (the default), and other bits
    than its snapped twin; the snapped scene, packed, equals the oracle."""
    sc = scenes_mod.build_scene(name, 1, W, H)
    imgs = []
    for delta in (np.float32(3.1e-4), np.float32(0.0)):
        m = sc.materials.copy()
        m["rgb0"][::3] = np.clip(m["rgb0"][::3] + delta, 0, 1)
        m["rgb1"][::5] = np.clip(m["rgb1"][::5] + delta, 0, 1)
        sc2 = type(sc)(sc.spheres, m, sc.camera, sc.sun, sc.sky, sc.exposure_scale, sc.name, sc.seed)
        sg, hg, _ = _render_with_env(monkeypatch, {"RT_MATS16": "1"}, sc2, W, H, 4, seed=2)
        s48, h48, _ = _render_with_env(monkeypatch, {"RT_MATS16": "0"}, sc2, W, H, 4, seed=2)
        assert_same(hg, h48, "%s, colour offset %g: RT_MATS16=1 vs the 48-byte records" % (name, delta))
        assert (sg.traversals, sg.segments) == (s48.traversals, s48.segments)
        imgs.append(hg)
        if delta == 0.0:
            orc = oracle.Oracle()
            orc.upload(sc2)
            so = orc.render(W, H, 1, 4, 50, 2, threads=8)
            assert_same(hg, orc.download()[0], "%s, byte colours vs the oracle" % name)
            assert (sg.traversals, sg.segments) == (so.traversals, so.segments)
    assert not np.array_equal(imgs[0], imgs[1])


def test_pipelining_falls_back_where_the_variant_does_not_apply(hip, scenes_mod):
    """grid10k runs the hierarchy scan, which has no carrying variant: the same calls run unpipelined and stay exact."""
    sc = scenes_mod.build_scene("grid10k", 1, 96, 96)
    hip.upload(sc)
    hip.render(96, 96, 1, 5, 50, 1)
    want = hip.download(ldr=False)[0]
    try:
        hip.set_frame_pipelining(3)
        for s in range(1, 5):
            hip.render(96, 96, s, s + 1, 50, 1, stats=False)
        hip.synchronize()
        assert hip.committed_samples() == 4
        assert_same(hip.download(ldr=False)[0], want, "grid10k progressive with pipelining requested")
    finally:
        hip.set_frame_pipelining(0)


# ------------------------------------------------------------------- sampler variants
@pytest.mark.parametrize("flags", [1, 2, 3], ids=["cosine-hemisphere", "sqrt-disk", "cosine+sqrt-disk"])
def test_sampler_variants_device_vs_oracle(hip, oracle, scenes_mod, flags):
    """rt_set_sampler: cosine-weighted hemisphere and area-uniform lens disk behind flags, bit-exact against the oracle's
    same flags at three levels: lens offsets / primary rays (aperture 2.0), DielectricOpaque::Scatter on scripted draws,
    and a cover-scene image with its traversal counters.  The image must differ from the reference-mapping image."""
    from cpuraytracer_amd import _capi
    W, H = 96, 64
    sc = scenes_mod.build_scene("cover", 1, W, H, aperture=2.0)
    hip.upload(sc)
    hip.set_sampler(0)
    hip.render(W, H, 1, 4, 50, 1)
    base = hip.download(ldr=False)[0]
    orc = oracle.Oracle()
    orc.upload(sc)
    try:
        hip.set_sampler(flags)
        oracle.lib().orc_set_sampler(flags)
        # (a) primary rays
        rng = np.random.default_rng(21)
        ijs = np.stack([rng.integers(0, W, 4000), rng.integers(0, H, 4000), rng.integers(1, 600, 4000)], 1).astype(np.uint32)
        assert_same(hip.unit_primary_rays(W, H, ijs), orc.primary_rays(W, H, ijs), "primary rays, sampler %d" % flags)
        # (b) opaque scatter on scripted draws (the diffuse branch consumes u1, u2)
        k255 = np.float32(1.0) / np.float32(255.0)
        sun = oracle.RtLight()
        for k in range(3):
            sun.direction[k] = float(np.float32(1.0) / np.sqrt(np.float32(3.0)))
            sun.color[k] = 1.0
        sun.luminance = 40000.0
        view = (C.c_float * 3)(12.0, 2.0, -2.5)
        m = oracle.RtMaterial()
        m.type, m.tex_type, m.smoothness, m.ior, m.tiling, m.luminance = 0, 0, 35.5, 1.5, 1.0, 0.0
        for k in range(3):
            m.rgb0[k] = float(np.float32((230, 128, 26)[k]) * k255)
        n = 2000
        nrm = rng.normal(size=(n, 3))
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        rd = -nrm + 0.3 * rng.normal(size=(n, 3))  # front facing
        rd /= np.linalg.norm(rd, axis=1, keepdims=True)
        draws = rng.uniform(0, 1, size=(n, 3))
        draws[:, 0] = 0.9 + 0.1 * draws[:, 0]  # the coin falls on the diffuse side
        inp = np.concatenate([rd, rng.uniform(-5, 5, size=(n, 3)), nrm, draws], 1).astype(np.float32)
        out = np.zeros((n, 11), dtype=np.float32)
        mm = _capi.RtMaterial.from_buffer_copy(bytes(m))
        ss = _capi.RtLight.from_buffer_copy(bytes(sun))
        _capi.check(hip._L.rt_unit_scatter(hip._h, C.byref(mm), C.byref(ss), view, inp.ctypes.data, n, out.ctypes.data))
        f = lambda a: (C.c_float * len(a))(*[float(v) for v in a])
        want_dir = np.zeros((n, 3), dtype=np.float32)
        front = np.einsum("ij,ij->i", inp[:, 0:3].astype(np.float64), inp[:, 6:9].astype(np.float64)) < -0.05
        assert front.mean() > 0.95
        for i in np.flatnonzero(front):
            uv = (C.c_float * 2)(float(np.float32(0.5) * inp[i, 6] + np.float32(0.5)), float(np.float32(0.5) * inp[i, 8] + np.float32(0.5)))
            att, dr, nd = (C.c_float * 3)(), (C.c_float * 3)(), C.c_uint32()
            scd = oracle.lib().orc_unit_scatter(C.byref(m), f(inp[i, 0:3]), f(inp[i, 3:6]), f(inp[i, 6:9]), uv, f(inp[i, 9:12]), att, dr,
                                                C.byref(nd))
            assert scd == 1 and nd.value == 3 and out[i, 0] == 1.0 and out[i, 7] == 3.0
            want_dir[i] = list(dr)
        assert_same(out[front, 4:7], want_dir[front], "diffuse directions, sampler %d" % flags)
        # (c) image
        sg = hip.render(W, H, 1, 4, 50, 1)
        hip.resolve()
        hg, lg = hip.download()
        so = orc.render(W, H, 1, 4, 50, 1, accel=oracle.ACCEL_PADDED_LIST, threads=8)
        orc.resolve()
        ho, lo = orc.download()
        assert_same(hg, ho, "HDR, sampler %d" % flags)
        assert_same(lg, lo, "LDR, sampler %d" % flags)
        assert (sg.traversals, sg.segments) == (so.traversals, so.segments)
        assert not np.array_equal(hg, base)
        # a running accumulation cannot switch mappings
        from cpuraytracer_amd import RtError
        hip.set_sampler(0)
        with pytest.raises(RtError) as e:
            hip.render(W, H, 4, 5, 50, 1)
        assert e.value.code == 6  # RT_ERR_SEQUENCE
    finally:
        hip.set_sampler(0)
        oracle.lib().orc_set_sampler(0)
    with pytest.raises(Exception):
        hip.set_sampler(8)


def test_gpu_image_agrees_with_the_reference_halton_counter_estimator(hip, oracle, scenes_mod):
    """SURVEY.md §8f N3 on the GPU side: the HIP render (per-path xoshiro streams) against the oracle driven by the
    reference's own per-material global Halton counters (material.h:34,50-51,67; serial, so reproducible).  Per-pixel
    parity with the original binary is impossible; the two are the same estimator, so the converged
    images agree within Monte-Carlo error, measured by two HIP renders with different seeds."""
    W, H, spp = 96, 64, 256
    sc = scenes_mod.build_scene("cover", 1, W, H)
    try:
        oracle.lib().orc_use_reference_halton_counters(1)
        orc = oracle.Oracle()
        orc.upload(sc)  # fresh materials: counters start at 0 like a fresh process
        orc.render(W, H, 1, 1 + spp, 50, 1, accel=oracle.ACCEL_PADDED_LIST, threads=1)
        ref, _ = orc.download()
    finally:
        oracle.lib().orc_use_reference_halton_counters(0)
    hip.upload(sc)
    imgs = []
    for seed in (1, 2):
        hip.render(W, H, 1, 1 + spp, 50, seed)
        imgs.append(hip.download(ldr=False)[0])
    a, b = imgs[0] / spp, imgs[1] / spp
    ref = ref / spp
    assert np.allclose(ref.mean(axis=(0, 1)), a.mean(axis=(0, 1)), rtol=0.02)
    noise = np.sqrt(np.mean((a - b) ** 2)) / np.sqrt(2)  # per-pixel std of one estimate
    rms = np.sqrt(np.mean((ref - a) ** 2))
    assert rms < 2.0 * noise, (rms, noise)
    blk = lambda x: x.reshape(8, 8, 12, 8, 3).mean(axis=(1, 3))  # 8x8-block averages: noise / 8
    assert np.max(np.abs(blk(ref) - blk(a))) < 8.0 * noise / 8.0 + 0.01 * blk(a).max()


# ------------------------------------------------ launch/layout knobs: every combination gives the same bits
def _render_with_env(monkeypatch, env, sc, W, H, s1, depth=50, seed=1, launch=False):
    """Render on a fresh context created under `env` (the knobs are read at rt_create).  launch=True: also what the launcher reports
    of that render's trace launch (HipRenderer.last_trace_launch)."""
    from cpuraytracer_amd import HipRenderer
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    r2 = HipRenderer(0)
    try:
        r2.upload(sc)
        st = r2.render(W, H, 1, s1, depth, seed)
        tl = r2.last_trace_launch()
        r2.resolve()
        hdr, ldr = r2.download()
    finally:
        r2.close()
        for k in env:
            monkeypatch.delenv(k, raising=False)
    return (st, hdr, ldr, tl) if launch else (st, hdr, ldr)


def _row(n):
    """Kernel word (rt_unit_launch_plan word [25], single light) of row n of csrc/rt_trace_variants.h, from the census' table."""
    import trace_variant_cases
    row, _, _, args = trace_variant_cases._ROWS[n]
    assert row == n
    return trace_variant_cases.kernel_word(*args)


def _env_id(env):
    return ",".join("%s=%s" % kv for kv in sorted(env.items()))


def _assert_kernel(tl, want, env):
    from cpuraytracer_amd import renderer
    assert tl.kernel_word == want, "under %s the launch took %s (row %d), not %s" % (
        env, renderer.decode_kernel_word(tl.kernel_word), tl.row, renderer.decode_kernel_word(want))


# The cover scene's default kernel: the flat scan with the hit stash and the materials through L2 (row 16).  Each knob set names the
# row it is meant to reach: another one where it trades a variant "instead of" the default's, row 16 itself for the knobs of the
# queue, the shadow rays, the tile order and the packed materials, which change what the same kernel is given.
_COVER_KNOBS = [
    ({"RT_SHADOW_GRID": "0"}, 16),                                  # every shadow ray on the two-state scan fallback
    ({"RT_MATS_LDS": "0"}, 18),                                     # material table through L2: the stash kernel without all its tables in LDS
    ({"RT_BLOCK_THREADS": "256"}, 39),                              # the path-cache kernels of the smaller workgroups
    ({"RT_BLOCK_THREADS": "512"}, 35),
    ({"RT_BLOCK_THREADS": "512", "RT_BLOCKS_PER_CU": "2"}, 36),     # ... half the LDS each: no room for the caches
    ({"RT_BLOCK_THREADS": "256", "RT_BLOCKS_PER_CU": "4"}, 40),
    ({"RT_BLOCKS_PER_CU": "2"}, 32),                                # more workgroups than fit: the surplus starts as others end; neither stash nor cache fits
    ({"RT_SCAN": "valu", "RT_BLOCKS_PER_CU": "2", "RT_SHADOW_GRID": "0"}, 47),
    ({"RT_SHADOW_GRID": "0", "RT_MATS_LDS": "0", "RT_RAY_CACHE": "0", "RT_BLOCK_THREADS": "512"}, 38),
    ({"RT_TILE_ORDER": "0"}, 16),                                   # tiles in image order instead of expensive-first
    ({"RT_SINGLE_DIRECT": "0"}, 16),                                # one-sphere groups through the sphere-level filter like the rest
    ({"RT_QUEUE_BLOCK": "256", "RT_QUEUE_STATIC": "0"}, 16),        # queue geometry: bigger blocks, nothing static
    ({"RT_STASH": "0"}, 31),                                        # the prepared-path cache variants instead of the hit stash
    ({"RT_STASH": "0", "RT_RAY_CACHE": "0"}, 32),                   # neither: idle lanes generate their own paths
    ({"RT_STASH_CAP": "16"}, 17),                                   # smallest stash: dropping the material table no longer buys eight records, so it stays in LDS
    ({"RT_STASH_CAP": "63"}, 16),                                   # largest stash (the default)
    ({"RT_MATS_L2": "0"}, 17),                                      # the material table in LDS and a smaller stash (default: through L2)
    ({"RT_GRID": "2"}, 1),                                          # the cell-grid scan (tables in LDS) instead of the matrix-core filter
    ({"RT_GRID": "2", "RT_MATS_LDS": "0"}, 6),                      # ... with its tables through L2
    ({"RT_GRID": "2", "RT_STASH": "0", "RT_SHADOW_GRID": "0"}, 3),  # ... its path caches do not fit beside cover's tables: neither
    ({"RT_MATS16": "1"}, 16),                                       # the packed 16-byte material records instead of the 48-byte ones through L2
    ({"RT_MATS16": "2"}, 16),                                       # the packed records staged into LDS (56-record stash)
    ({"RT_MATS16": "1", "RT_MATS_LDS": "0", "RT_STASH": "0"}, 33),
]


@pytest.mark.parametrize("env,row", _COVER_KNOBS, ids=[_env_id(e) for e, _ in _COVER_KNOBS])
def test_launch_and_layout_knobs_give_the_same_bits(hip, scenes_mod, monkeypatch, env, row):
    W, H, s1 = 161, 103, 5  # ragged: the last tile of the sample buffer is 9 pixels wide
    if "RT_TILE_ORDER" in env:
        W, H = 483, 309       # enough tiles (2,331) for the expensive-first work order to be built at all; still ragged
    sc = scenes_mod.build_scene("cover", 1, W, H)
    hip.upload(sc)
    sa = hip.render(W, H, 1, s1, 50, 1)
    _assert_kernel(hip.last_trace_launch(), _row(16), {})
    hip.resolve()
    a, la = hip.download()
    sb, b, lb, tl = _render_with_env(monkeypatch, env, sc, W, H, s1, launch=True)
    _assert_kernel(tl, _row(row), env)
    assert_same(a, b, "HDR under %s" % env)
    assert_same(la, lb, "LDR under %s" % env)
    assert (sa.traversals, sa.segments, sa.samples) == (sb.traversals, sb.segments, sb.samples)


# grid10k's default kernel: the cell grid with its tables in global memory, the cells in LDS and the hit stash (row 6).  RT_TREE_LDS,
# RT_TREE_TOP, RT_SHADOW_CELLS, RT_SG_SPH, RT_STASH_CAP and RT_MATS16 change tables or capacities of the kernel a scene gets anyway.
# RT_GRID_SG_LDS=1 alone is DECLINED on this scene -- its shadow index (78 x 133 cells, 40,038 entries: 98 KiB) leaves no stash of 24
# records beside the cells -- and so takes row 6 like the default; under RT_SHADOW_CELLS=32 the index fits and the knob reaches the
# kernel it exists for (row 4).
_GRID10K_KNOBS = [
    ({"RT_TREE_LDS": "0"}, 6), ({"RT_TREE_LDS": "0", "RT_SHADOW_GRID": "0"}, 6), ({"RT_BLOCK_THREADS": "512"}, 11),
    ({"RT_MATS_LDS": "0", "RT_TREE_TOP": "32"}, 6), ({"RT_ALWAYS_BIG": "1"}, 14),
    ({"RT_GRID": "0"}, 14), ({"RT_GRID": "0", "RT_TREE_LDS": "0", "RT_STASH": "0"}, 21), ({"RT_GRID": "0", "RT_BLOCK_THREADS": "512"}, 23),
    ({"RT_STASH": "0"}, 7), ({"RT_STASH": "0", "RT_RAY_CACHE": "0"}, 8), ({"RT_BLOCK_THREADS": "256", "RT_BLOCKS_PER_CU": "2"}, 13),
    ({"RT_STASH_CAP": "17"}, 6), ({"RT_GRID_SG_LDS": "1"}, 6), ({"RT_GRID_QUANT": "1"}, 5), ({"RT_GRID_QUANT": "1", "RT_STASH_CAP": "24"}, 5),
    ({"RT_SHADOW_CELLS": "64"}, 6), ({"RT_SHADOW_CELLS": "128", "RT_GRID": "0"}, 14), ({"RT_SG_SPH": "1"}, 6), ({"RT_SG_SPH": "1", "RT_GRID": "0"}, 14),
    ({"RT_MATS16": "1"}, 6), ({"RT_MATS16": "1", "RT_GRID": "0"}, 14),
    ({"RT_GRID_SG_LDS": "1", "RT_SHADOW_CELLS": "32"}, 4),
]


@pytest.mark.parametrize("env,row", _GRID10K_KNOBS, ids=[_env_id(e) for e, _ in _GRID10K_KNOBS])
def test_hierarchy_scan_knobs_give_the_same_bits(hip, scenes_mod, monkeypatch, env, row):
    """grid10k (10,004 spheres: the cell-grid scan by default): the bounds hierarchy instead (RT_GRID=0: 2,504 groups, four levels of
    bounds, through LDS or L2, a narrower top level, the big spheres inside it with RT_ALWAYS_BIG=1), smaller workgroups, the path
    cache instead of the hit stash, neither, a small stash; the quantised one-sphere bounds in LDS (RT_GRID_QUANT=1, rt_scan.h
    GridQuant); the shadow index in LDS (RT_GRID_SG_LDS=1 with an index small enough); coarser shadow indices than the 256 x 256
    cells large scenes get.  Every set names the kernel it reaches."""
    sc = scenes_mod.build_scene("grid10k", 1, 96, 96)
    hip.upload(sc)
    sa = hip.render(96, 96, 1, 3, 50, 1)
    _assert_kernel(hip.last_trace_launch(), _row(6), {})
    hip.resolve()
    a, la = hip.download()
    sb, b, lb, tl = _render_with_env(monkeypatch, env, sc, 96, 96, 3, launch=True)
    _assert_kernel(tl, _row(row), env)
    assert_same(a, b, "grid10k HDR under %s" % env)
    assert_same(la, lb, "grid10k LDR under %s" % env)
    assert (sa.traversals, sa.segments) == (sb.traversals, sb.segments)


@pytest.mark.parametrize("name,env", [("cover", {}), ("cover", {"RT_SCAN": "valu"}), ("cover", {"RT_TREE_TOP": "16"}),
                                      ("cover", {"RT_FORCE_GLOBAL_TABLES": "1"}), ("grid10k", {}), ("grid10k", {"RT_TREE_LDS": "0"}),
                                      ("three", {})],
                         ids=lambda v: v if isinstance(v, str) else ",".join("%s=%s" % kv for kv in sorted(v.items())) or "default")
def test_closest_hit_unit_runs_the_production_scan(oracle, scenes_mod, monkeypatch, name, env):
    """rt_unit_closest_hit launches the scan variant rt_render uses for the scene (matrix-core filter + pooled resolve,
    hierarchy descent, or the VALU scan) — A4/A6/A7 unit parity on shipped code: t, original index, position, normal and
    uv equal the oracle's list scan AND its BvhNode traversal for random rays from inside, outside and missing.  (None of them is
    aimed: silhouette grazers, surface starters, ties and the other directed rays are tests/test_scan_rays.py's.)"""
    from cpuraytracer_amd import HipRenderer
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    r = HipRenderer(0)
    try:
        sc = scenes_mod.build_scene(name, 1, 300, 200)
        r.upload(sc)
        orc = oracle.Oracle()
        orc.upload(sc)
        rng = np.random.default_rng(17)
        n = 3000 + 37  # not a multiple of the wave: dead lanes in the last wave
        o = rng.uniform(-14, 14, (n, 3)).astype(np.float32)
        o[:, 1] = rng.uniform(0.05, 4, n)
        d = rng.normal(size=(n, 3)).astype(np.float32)
        d[: n // 4] *= np.float32(3.7)          # un-normalised directions: a != 1
        d[n // 4: n // 2, 1] = -np.abs(d[n // 4: n // 2, 1])  # towards the floor
        o[-50:] = (0.0, 1.0, 0.0)                # from the centre of the big glass sphere (inside hits)
        rays = np.concatenate([o, d], 1)
        hg = r.unit_closest_hit(rays)
        ho_list = orc.closest_hit(rays, accel=oracle.ACCEL_LIST)
        ho_bvh = orc.closest_hit(rays, accel=oracle.ACCEL_BVH)
        assert_same(ho_list, ho_bvh, "oracle list scan vs BvhNode")
        assert_same(hg, ho_list, "%s closest hit under %s" % (name, env))
        assert (hg[:, 1].view(np.int32) >= 0).sum() > n // 4
    finally:
        r.close()


@pytest.mark.parametrize("name", ["cover", "grid10k"])
def test_closest_hit_of_rays_whose_direction_is_far_from_unit_length(hip, oracle, scenes_mod, name):
    """The exact phase divides by a = d.d through Markstein's correction when a is in [2^-19, 2^100] (rt_scan.h pooled_root) and takes
    square roots through the four-operation form when the discriminant is in [2^-80, inf) (rt_device_math.h sqrt_rn); ONE lane outside
    sends its whole wave through the compiler's sequences.  Directions scaled by 2^-12 (a = 2^-24) and by 2^52 (a = 2^104), alone and
    mixed into waves of ordinary rays: t, index, position, normal and uv equal the oracle's list scan.  (With |d| = 2^52 every root
    is ~1e-15, below the reference's bias of 0.001: those rays exercise the guards and hit nothing, in the oracle as on the device.)"""
    sc = scenes_mod.build_scene(name, 1, 300, 200)
    hip.upload(sc)
    orc = oracle.Oracle()
    orc.upload(sc)
    rng = np.random.default_rng(23)
    n = 64 * 60
    o = rng.uniform(-10, 10, (n, 3)).astype(np.float32)
    o[:, 1] = rng.uniform(0.05, 3, n)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d[:, 1] = -np.abs(d[:, 1]) * np.float32(0.3)
    scale = np.ones(n, dtype=np.float32)
    scale[: 64 * 10] = np.float32(2.0 ** -12)          # whole waves of short directions
    scale[64 * 10: 64 * 20] = np.float32(2.0 ** 52)    # whole waves of long ones
    mixed = np.arange(64 * 20, n)
    scale[mixed[::7]] = np.float32(2.0 ** -12)         # one lane in seven: mixed waves
    scale[mixed[3::11]] = np.float32(2.0 ** 52)
    rays = np.concatenate([o, d * scale[:, None]], 1).astype(np.float32)
    hg = hip.unit_closest_hit(rays)
    ho = orc.closest_hit(rays, accel=oracle.ACCEL_LIST)
    assert_same(hg, ho, "%s: closest hit of rays with |d| = 2^-12, 1, 2^52" % name)
    hit = hg[:, 1].view(np.int32) >= 0
    assert hit[: 64 * 10].sum() > 300 and hit[64 * 10: 64 * 20].sum() == 0 and hit[64 * 20:].sum() > 1000


def test_c5_full_size_properties(hip, oracle, scenes_mod):
    """BASELINE config 5 at full size: 10,004 spheres, 4096x4096, spp 64 (1.07 G paths through the hierarchy scan, one
    pass).  Counts, idempotence of a second launch, and six whole-pixel sums + LDR bytes against the oracle."""
    W = H = 4096
    sc = scenes_mod.build_scene("grid10k", 1, W, H)
    assert sc.n == 10004
    hip.upload(sc)
    st = hip.render(W, H, 1, 65, 50, 1)
    assert st.samples == W * H * 64 and st.passes == 1
    assert st.segments <= st.traversals <= 2 * st.segments and st.traversals >= st.samples
    hip.resolve()
    hdr, ldr = hip.download()
    assert np.isfinite(hdr).all() and (hdr >= 0).all()
    st2 = hip.render(W, H, 1, 65, 50, 1)
    assert (st2.traversals, st2.segments) == (st.traversals, st.segments)
    hdr2 = hip.download(ldr=False)[0]
    assert_same(hdr2, hdr, "C5 second launch")
    del hdr2
    orc = oracle.Oracle()
    orc.upload(sc)
    out = (C.c_uint8 * 3)()
    for i, j in ((0, 0), (4095, 4095), (2048, 2600), (1000, 3000), (3100, 2200), (2047, 1900)):
        pij = np.array([[i, j, s] for s in range(1, 65)], dtype=np.uint32)
        rgb, _ = orc.trace(W, H, pij, 50, 1, accel=oracle.ACCEL_PADDED_LIST)
        acc = np.zeros(3, dtype=np.float32)
        for s in range(64):
            acc = acc + rgb[s]
        assert np.array_equal(acc.view(np.uint32), hdr[j, i].view(np.uint32)), (i, j)
        oracle.lib().orc_tonemap((C.c_float * 3)(*[float(v) for v in acc]), 64, out)
        assert list(out) == list(ldr[j, i])


def test_two_rank_bench_rehearsal_gathers_the_one_rank_image(hip, scenes_mod, tmp_path):
    """The torch.distributed leg of bench.py (row shards + gather + assemble) as two fresh rank processes sharing the one
    GPU (RT_BENCH_REHEARSAL=1: gloo, strips through host memory): the gathered LDR image must equal the 1-rank render."""
    import json
    import subprocess
    out = tmp_path / "img.npy"
    env = dict(os.environ, RT_BENCH_REHEARSAL="1", RT_BENCH_DUMP_LDR=str(out), MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    port = 29500 + (os.getpid() % 400)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0", "--no-cpu-baseline"]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
    rec = json.loads(line)
    assert rec["n_gpus"] == 2 and "REHEARSAL" in rec["data"] and rec["config"]["spp"] == 256
    got = np.load(out)
    sc = scenes_mod.build_scene("cover", 1, 1200, 800)
    hip.upload(sc)
    hip.render(1200, 800, 1, 257, 50, 1)
    hip.resolve()
    _, ldr = hip.download(hdr=False)
    assert_same(got, ldr, "2-rank gathered image vs 1-rank render")


def test_seed_changes_image_and_depth_zero_is_direct_only(hip, scenes_mod):
    sc = scenes_mod.build_scene("cover", 1, 96, 64)
    hip.upload(sc)
    hip.render(96, 64, 1, 3, 50, 1)
    a = hip.download(ldr=False)[0]
    hip.render(96, 64, 1, 3, 50, 2)
    b = hip.download(ldr=False)[0]
    assert not np.array_equal(a, b)
    st = hip.render(96, 64, 1, 2, 0, 1)
    assert st.segments == st.samples and st.traversals <= 2 * st.samples


# ------------------------------------------------------------------- error behaviour
def test_error_codes(hip, scenes_mod):
    from cpuraytracer_amd import HipRenderer, RtError, _capi
    r = HipRenderer(0)
    with pytest.raises(RtError) as e:
        r.render(8, 8, 1, 2, 8, 1)
    assert e.value.code == 3  # RT_ERR_NO_SCENE
    r.upload(scenes_mod.build_scene("three", 1, 8, 8))
    for args in ((0, 8, 1, 2), (8, 8, 0, 2), (8, 8, 2, 2)):
        with pytest.raises(RtError) as e:
            r.render(args[0], args[1], args[2], args[3], 8, 1)
        assert e.value.code == 2
    with pytest.raises(RtError) as e:
        r.render(8, 8, 3, 4, 8, 1)  # accumulation must start at s0 == 1
    assert e.value.code == 6
    r.render(8, 8, 1, 3, 8, 1)
    with pytest.raises(RtError) as e:
        r.render(8, 8, 5, 6, 8, 1)  # gap
    assert e.value.code == 6
    with pytest.raises(RtError) as e:
        r.render(8, 8, 1, 2, 8, 1, rowset=_capi.RtRowset(4, 8, 4, 0, 1))  # rows beyond H
    assert e.value.code == 2
    with pytest.raises(RtError):
        HipRenderer(4096)
    # a centre or a radius that is not finite: no bound can be built from it -- refused with a message, the scene in place stays
    r.render(8, 8, 1, 2, 8, 1)
    want, _ = r.download(ldr=False)
    for field, value in (("r", np.nan), ("r", np.inf), ("cx", -np.inf), ("cy", np.nan)):
        sc = scenes_mod.build_scene("three", 1, 8, 8)
        sc.spheres[field][1] = value
        with pytest.raises(RtError) as e:
            r.upload(sc)
        assert e.value.code == 2 and "sphere 1" in str(e.value) and "not finite" in str(e.value)
    r.render(8, 8, 1, 2, 8, 1)
    got, _ = r.download(ldr=False)
    assert_same(got, want, "the scene uploaded before the refused ones")
    r.close()


def test_depth_limits_beyond_the_stash_records_range_take_the_cache_variant(hip, oracle, scenes_mod):
    """The hit stash keeps the depth beside the scan entry in one 32-bit field; a depth limit of 65,536 or more (the reference
    uses 50) selects the prepared-path-cache variant instead, with the same results."""
    sc = scenes_mod.build_scene("cover", 1, 96, 64)
    hip.upload(sc)
    orc = oracle.Oracle()
    orc.upload(sc)
    for depth in (65535, 70000):
        sg = hip.render(96, 64, 1, 3, depth, 5)
        hg, _ = hip.download(ldr=False)
        so = orc.render(96, 64, 1, 3, depth, 5, accel=oracle.ACCEL_PADDED_LIST, threads=8)
        ho, _ = orc.download()
        assert_same(hg, ho, "HDR at depth limit %d" % depth)
        assert (sg.traversals, sg.segments) == (so.traversals, so.segments)


def test_scene_size_limit_is_an_error_not_a_truncation(hip, oracle):
    """Work lists, the shadow index and the closest-hit keys carry scan-entry ids in 16 bits: a scene beyond 65,535 scan entries
    (about 65,000 spheres) is refused by rt_scene_upload with RT_ERR_INVALID_ARG; 60,000 spheres are accepted and render through
    the cell-grid scan exactly like the oracle."""
    from cpuraytracer_amd import HipRenderer, RtError
    rng = np.random.default_rng(70)

    def scene(n, side):
        c = np.stack([rng.uniform(-side, side, n), np.full(n, 0.2), rng.uniform(-side, side, n)], 1).astype(np.float32)
        c = np.concatenate([c, [[0.0, -1000.0, 0.0]]]).astype(np.float32)
        r_ = np.concatenate([np.full(n, 0.2), [1000.0]]).astype(np.float32)
        t = np.concatenate([rng.choice([0, 0, 0, 1, 2], n), [0]]).astype(np.uint32)
        return _custom_scene(oracle, c, r_, t, (12.0, 2.0, -2.5), (0.0, 1.0, 0.0), 25.0, 1.5)
    r = HipRenderer(0)
    try:
        with pytest.raises(RtError) as e:
            r.upload(scene(70_000, 130.0))
        assert e.value.code == 2 and "65,535" in str(e.value)
        with pytest.raises(RtError):
            r.render(8, 8, 1, 2, 8, 1)  # the refused upload left no scene behind
    finally:
        r.close()
    _assert_image_equals_oracle(hip, oracle, scene(60_000, 120.0), 96, 64, 2, 20, seed=4)


def test_cli_writes_the_same_ppm(hip, oracle, scenes_mod, tmp_path):
    import subprocess
    from conftest import ROOT
    out = str(tmp_path / "c1.ppm")
    cli = os.path.join(ROOT, "cpuraytracer_amd", "lib", "spheres")
    p = subprocess.run([cli, "--scene", "three", "--width", "200", "--height", "100", "--spp", "1", "--depth", "8", "--out", out, "--quiet"],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    data = open(out, "rb").read()
    assert data.startswith(b"P6\n200 100\n255\n")
    g = np.load(os.path.join(GOLDEN, "c1_three_200x100_spp1_d8.npz"))
    assert data[len(b"P6\n200 100\n255\n"):] == g["ldr"].tobytes()


def test_cli_progressive_frames_with_pipelining_write_the_one_shot_ppm(hip, tmp_path):
    """The headless app in the reference's mode (one sample per frame, app.cpp:56-76) with frames in flight: same PPM as
    the one-shot run."""
    import subprocess
    from conftest import ROOT
    cli = os.path.join(ROOT, "cpuraytracer_amd", "lib", "spheres")
    outs = []
    for extra in (["--frame-spp", "24"], ["--frame-spp", "1", "--pipeline", "6"], ["--frame-spp", "1", "--batch", "5"]):
        out = str(tmp_path / ("p%d.ppm" % len(outs)))
        p = subprocess.run([cli, "--scene", "cover", "--width", "240", "--height", "160", "--spp", "24", "--out", out, "--quiet"] + extra,
                           capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr
        outs.append(open(out, "rb").read())
    assert outs[0] == outs[1] == outs[2] and len(outs[0]) == len(b"P6\n240 160\n255\n") + 240 * 160 * 3


def test_cli_multi_gpu_driver_with_rccl_gather(hip, tmp_path):
    """`spheres --gpus 1`: the single-process multi-device driver (thread per GPU, ncclGather of the padded strips to
    device 0, host de-interleave).  One device is all this box has; the partition/gather arithmetic for G > 1 is
    covered by the 8-shard test above and the gloo tests."""
    import subprocess
    from conftest import ROOT
    out = str(tmp_path / "c1_mgpu.ppm")
    cli = os.path.join(ROOT, "cpuraytracer_amd", "lib", "spheres")
    p = subprocess.run([cli, "--scene", "three", "--width", "200", "--height", "100", "--spp", "1", "--depth", "8", "--gpus", "1", "--out", out],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    g = np.load(os.path.join(GOLDEN, "c1_three_200x100_spp1_d8.npz"))
    data = open(out, "rb").read()
    assert data[len(b"P6\n200 100\n255\n"):] == g["ldr"].tobytes()
    p = subprocess.run([cli, "--gpus", "64", "--width", "8", "--height", "8", "--spp", "1"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 1 and "exceeds" in p.stderr


def test_host_mirror_api(hip, oracle):
    """Code written against the reference's class API (Camera, Sphere, BvhNode, DielectricOpaque, DirectionalLight,
    Random::Halton*) runs against the host mirror, whose per-ray methods evaluate on the device; values == oracle."""
    import json
    import subprocess
    from conftest import ROOT
    exe = os.path.join(ROOT, "cpuraytracer_amd", "lib", "api_selftest")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    j = json.loads(p.stdout)
    O = oracle.lib()
    f32 = lambda v: np.asarray(v, dtype=np.float32)
    assert np.float32(j["halton_100_3"]) == np.float32(O.orc_halton(100, 3))
    o2, o3 = (C.c_float * 2)(), (C.c_float * 3)()
    O.orc_halton_disk(7, 4, 5, o2)
    O.orc_halton_hemisphere(3, 5, 7, o3)
    assert np.array_equal(f32(j["disk_7"]), f32(list(o2))) and np.array_equal(f32(j["hemi_3"]), f32(list(o3)))
    # camera ray: oracle's Camera with the same constructor arguments
    cam = oracle.RtCamera()
    o = np.array([12, 2, -2.5]); la = np.array([0, 1, 0])
    focal = float(np.sqrt(np.float32(np.float32(np.float32(144) + np.float32(1)) + np.float32(6.25))))
    O.orc_camera_make((C.c_float * 3)(*o), (C.c_float * 3)(*la), 25.0, 1.5, focal, 0.4, C.byref(cam))
    sc = oracle.build_scene("three", 1, 1.5)
    sc.camera = cam
    orc = oracle.Oracle()
    orc.upload(sc)
    # Camera::GetRay(uv, offset) through the hit of the C1 spheres
    ray = np.array([[0.1, 0.05, 0.0, 0, 0, 0]], dtype=np.float32)
    d = np.array([0.05, -0.02, 1.0], dtype=np.float32)
    n2 = np.float32(np.float32(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    ray[0, 3:] = d / np.sqrt(n2)
    h = orc.closest_hit(ray)[0]
    assert j["sphere_hit"] == 1 and np.float32(j["sphere_t"]) == h[0]
    assert np.array_equal(f32(j["sphere_pos"]), h[2:5]) and np.array_equal(f32(j["sphere_normal"]), h[5:8]) and np.array_equal(f32(j["sphere_uv"]), h[8:10])
    m = oracle.RtMaterial.from_buffer_copy(sc.materials[0].tobytes())
    att, dr, nd, loc = (C.c_float * 3)(), (C.c_float * 3)(), C.c_uint32(), (C.c_float * 3)()
    f = lambda a: (C.c_float * len(a))(*[float(v) for v in a])
    scat = O.orc_unit_scatter(C.byref(m), f(ray[0, 3:]), f(h[2:5]), f(h[5:8]), f(h[8:10]), f([0.5, 0.3, 0.7]), att, dr, C.byref(nd))
    assert j["scattered"] == scat == 1 and np.array_equal(f32(j["attenuation"]), f32(list(att))) and np.array_equal(f32(j["scatter_dir"]), f32(list(dr)))
    O.orc_unit_emit_shade(C.byref(m), C.byref(sc.sun), (C.c_float * 3)(12.0, 2.0, -2.5), f(h[2:5]), f(h[5:8]), f(h[8:10]), loc)
    shadow = orc.closest_hit(np.concatenate([h[2:5], f32(list(sc.sun.direction))])[None, :])[0]
    occluded = shadow[1:2].view(np.int32)[0] >= 0  # light.cpp:13-18: an occluded sun contributes nothing
    assert np.array_equal(f32(j["shade"]), np.zeros(3, dtype=np.float32) if occluded else f32(list(loc)))
    assert j["scene_moved_out"] == 1 and j["bvh_hit"] == 1
    hb = orc.closest_hit(np.array([[0.45, 1.0, 0.55, 0, -1, 0]], dtype=np.float32))[0]
    assert np.float32(j["bvh_t"]) == hb[0] and np.array_equal(f32(j["bvh_normal"]), hb[5:8])
    assert j["shade_in_shadow"] == [0.0, 0.0, 0.0]
