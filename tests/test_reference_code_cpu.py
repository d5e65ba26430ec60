"""The oracle (oracle/rt_oracle.cpp) against the reference's OWN code: quasi-random.cpp, texture.cpp, light.cpp, camera.cpp,
material.cpp and ray-tracing.cpp, compiled unmodified over the stand-in headers of oracle/ref_shim/ into oracle/_ref/libref.so
(oracle/Makefile, oracle/ref_api.h).  CPU only.  Every comparison is bitwise (uint32 views; NaNs compare by bits).  The only
differences allowed:

* libm.  The reference's objects call this C library's sinf/cosf/tanf; the oracle its own correctly rounded kernels, by design
  (dxmath_restate.h, "elementary-function contract").  Wherever the two differ in a function that calls one of these, the test
  recomputes the ORACLE's formula in binary32 numpy with ref_libm's value in place of the oracle's and must get the
  reference's bits exactly.  (The numpy formulas are themselves checked: with the oracle's sin/cos they must give the oracle's
  bits at every index.)  The share excused this way is capped: 3 % of the indices below 300,000 for HaltonSampleDisk(i, 4, 5)
  and HaltonSampleHemisphere(i, 5, 7).
* BvhNode against the list scan: exact ties and the grazing hits its binary32 slab test loses, both detected from the list's
  result and capped at 1 in 10^4 rays per scene (scenes built to contain ties are exempt from the cap and must give the
  reference's tie winner).

Every sequence of ref_* calls is serial (the reference's counters are not thread safe); the oracle's list scans of the scene
tests run on a second thread meanwhile.  The second half of the file replays tests/golden/reference_code_answers.npz -- inputs
and the outputs recorded from libref.so by tests/golden/make_reference_code_answers.py -- so the pin also holds where the
reference does not exist."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

F = np.float32
TWO_PI = F(2.0) * F(3.141592654)  # 2.f * XM_PI, folded in binary32 (doubling is exact)
BIAS = F(0.001)                   # ray-tracing.cpp:52
OPAQUE, METAL, GLASS, EMISSIVE = 0, 1, 2, 3


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def rows_differ(a, b):
    return (bits(a) != bits(b)).reshape(a.shape[0], -1).any(axis=1)


def assert_same(a, b, what):
    d = rows_differ(np.asarray(a).reshape(len(a), -1), np.asarray(b).reshape(len(b), -1))
    assert not d.any(), "%s: %d of %d rows differ, first at %d: %r vs %r" % (what, d.sum(), d.size, np.argmax(d), np.asarray(a)[np.argmax(d)], np.asarray(b)[np.argmax(d)])


# ------------------------------------------------------------------ the oracle's formulas in binary32 numpy (libm rule)
def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross3(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def normalize3(v):
    with np.errstate(all="ignore"):
        ln = np.sqrt(dot3(v, v))
        return np.where((ln == 0)[..., None], F(0), v / ln[..., None])


def disk_formula(u_theta, u_r, cosf, sinf):
    """HaltonSampleDisk on its two uniforms with the given cos/sin: theta = 2 pi u, (r cos theta, r sin theta)"""
    theta = TWO_PI * u_theta
    return np.stack([u_r * cosf(theta), u_r * sinf(theta)], -1)


def hemisphere_formula(u1, u2, cosf, sinf):
    """HaltonSampleHemisphere on its two uniforms: r = sqrt(1 - u1^2), phi = 2 pi u2, (r cos phi, r sin phi, u1)"""
    r = np.sqrt(F(1) - u1 * u1)
    phi = TWO_PI * u2
    return np.stack([r * cosf(phi), r * sinf(phi), u1], -1)


def diffuse_direction(normal, hemi):
    """DielectricOpaque's diffuse bounce: basis about the normal, the hemisphere sample projected into it, normalised"""
    up = np.where((np.abs(normal[..., 0]) < F(0.5))[..., None], np.array([1, 0, 0], F), np.array([0, 1, 0], F))
    b1 = cross3(up, normal)
    b2 = cross3(normal, b1)
    sd = (hemi[..., 0:1] * b1 + hemi[..., 1:2] * b2) + hemi[..., 2:3] * normal
    return normalize3(sd)


def camera_formula(origin, look_at, vfov, aspect, tanf):
    """Camera::Camera's members m_x, m_y, m_originImagePlane (xyz) with the given tan"""
    theta = F(vfov) * F(3.141592654) / F(180.0)
    hh = tanf(np.array([theta / F(2.0)], F))[0]
    hw = F(aspect) * hh
    w = normalize3(look_at - origin)
    u = normalize3(cross3(np.array([0, 1, 0], F), w))
    v = cross3(w, u)
    return hw * u, hh * v, origin + F(1) * w


# ------------------------------------------------------------------ fixtures
@pytest.fixture(scope="module")
def ref(built):
    """oracle/_ref/libref.so.  Skips only where neither the library nor the reference exists (a machine the library did not
    travel to); with the reference present, a missing or unloadable library is a failure."""
    from oracle import ref_py
    if not os.path.exists(ref_py.LIB_PATH) and not ref_py.reference_present():
        pytest.skip("neither oracle/_ref/libref.so nor the reference's sources exist on this machine")
    ref_py.lib()  # raises (= the tests fail) where the library is missing or does not load
    return ref_py


@pytest.fixture()
def counter_mode(oracle):
    L = oracle.lib()
    L.orc_use_reference_halton_counters(1)
    yield
    L.orc_use_reference_halton_counters(0)
    L.orc_use_nested_radiance(0)
    L.orc_use_reference_bvh_tie_rule(1)


def orc_math(oracle):
    return (lambda x: oracle.math_array(1, x)), (lambda x: oracle.math_array(0, x)), (lambda x: oracle.math_array(3, x))


def ref_math(ref):
    return (lambda x: ref.libm(ref.COS, x)), (lambda x: ref.libm(ref.SIN, x)), (lambda x: ref.libm(ref.TAN, x))


def orc_disk(oracle, idx, b1, b2):
    out = np.zeros((len(idx), 2), F)
    buf = (C.c_float * 2)()
    fn = oracle.lib().orc_halton_disk
    for k, i in enumerate(idx):
        fn(int(i), b1, b2, buf)
        out[k] = buf[0], buf[1]
    return out


def orc_hemisphere(oracle, idx, b1, b2):
    out = np.zeros((len(idx), 3), F)
    buf = (C.c_float * 3)()
    fn = oracle.lib().orc_halton_hemisphere
    for k, i in enumerate(idx):
        fn(int(i), b1, b2, buf)
        out[k] = buf[0], buf[1], buf[2]
    return out


def material_record(oracle, kind, tex=0, smoothness=16.0, ior=1.5, tiling=4.0, rgb0=(0.5, 0.5, 0.5), rgb1=(0.1, 0.2, 0.3), luminance=0.0):
    m = np.zeros(1, dtype=oracle.MATERIAL_DTYPE)
    m["type"], m["tex_type"], m["smoothness"], m["ior"], m["tiling"], m["luminance"] = kind, tex, smoothness, ior, tiling, luminance
    m["rgb0"], m["rgb1"] = rgb0, rgb1
    return m


def flat_scene(oracle, spheres, materials=None, lights=None, camera=None):
    base = oracle.build_scene("three", 1, 2.0)
    sph = np.zeros(len(spheres), dtype=oracle.SPHERE_DTYPE)
    a = np.asarray(spheres, dtype=np.float32).reshape(-1, 4)
    sph["cx"], sph["cy"], sph["cz"], sph["r"] = a[:, 0], a[:, 1], a[:, 2], a[:, 3]
    if materials is None:
        materials = np.repeat(material_record(oracle, OPAQUE), len(sph))
    sc = oracle.Scene(sph, materials, camera if camera is not None else base.camera, base.sun, base.sky, base.exposure_scale)
    if lights is not None:
        sc.lights = list(lights)
    return sc


# ================================================================== (a) Halton and its mappings
def test_halton_sample_every_index_to_a_million_and_beyond_32_bits(ref, oracle):
    """HaltonSample, bases 2, 3, 4, 5, 7, indices 0 .. 10^6, bit for bit; then 2^32 +- k and 2^40 through the 64-bit entry point.
    The reference takes uint64_t and so does the oracle's Random::HaltonSample (orc_halton).  The PRODUCT never forms an index
    above 2^32 - 1: rt_unit_halton takes uint32_t, the sample index s of rt_render is a uint32_t, and the lens index s + i + j
    is far below 2^32 for any image the API accepts; the counters of the reference's materials, which could pass 2^32, are
    replaced by the per-path stream.  So above 2^32 only the oracle is pinned here, not a kernel."""
    idx = np.arange(0, 10**6 + 1, dtype=np.uint64)
    for base in (2, 3, 4, 5, 7):
        assert_same(ref.halton(idx, base), oracle.halton_array(idx.astype(np.uint32), base), "HaltonSample base %d" % base)
    big = np.array([2**32 + k for k in range(-17, 18)] + [2**40, 2**40 - 1, 2**40 + 1, 2**63, 2**64 - 1], dtype=np.uint64)
    fn = oracle.lib().orc_halton
    for base in (2, 3, 4, 5, 7):
        got = np.array([fn(int(i), base) for i in big], F)
        assert_same(ref.halton(big, base), got, "HaltonSample base %d above 2^32" % base)
    # what a 32-bit index does with these: it wraps, and is then a different sample (documented above, not a defect)
    assert not same(ref.halton(big[:35], 3), oracle.halton_array((big[:35] & np.uint64(0xffffffff)).astype(np.uint32), 3))


def test_halton_2d_and_ring(ref, oracle):
    idx = np.arange(0, 300000, dtype=np.uint64)
    i32 = idx.astype(np.uint32)
    for b1, b2 in ((2, 3), (5, 7), (4, 5)):
        assert_same(ref.halton_2d(idx, b1, b2), np.stack([oracle.halton_array(i32, b1), oracle.halton_array(i32, b2)], 1), "HaltonSample2D")
    # HaltonSampleRing (dead code in the reference; the oracle keeps it without a C entry point): the libm rule on its formula
    rcos, rsin, _ = ref_math(ref)
    theta = TWO_PI * oracle.halton_array(i32, 2)
    got = ref.halton_ring(idx, 2)
    assert_same(got, np.stack([rcos(theta), rsin(theta)], 1), "HaltonSampleRing = (cos, sin)(2 pi u) with the reference's libm")
    ocos, osin, _ = orc_math(oracle)
    share = rows_differ(got, np.stack([ocos(theta), osin(theta)], 1)).mean()
    print("ring: %.3f %% of indices differ through libm" % (100 * share))
    assert share <= 0.03


def test_halton_disk_and_hemisphere_under_the_libm_rule(ref, oracle):
    n = 300000
    idx = np.arange(n, dtype=np.uint64)
    i32 = idx.astype(np.uint32)
    rcos, rsin, _ = ref_math(ref)
    ocos, osin, _ = orc_math(oracle)
    # disk (4, 5)
    r_disk, o_disk = ref.halton_disk(idx, 4, 5), orc_disk(oracle, idx, 4, 5)
    u4, u5 = oracle.halton_array(i32, 4), oracle.halton_array(i32, 5)
    assert_same(o_disk, disk_formula(u4, u5, ocos, osin), "numpy disk formula == the oracle's")
    assert_same(r_disk, disk_formula(u4, u5, rcos, rsin), "HaltonSampleDisk explained by libm alone")
    share_d = rows_differ(r_disk, o_disk).mean()
    # hemisphere (5, 7)
    r_hem, o_hem = ref.halton_hemisphere(idx, 5, 7), orc_hemisphere(oracle, idx, 5, 7)
    u7 = oracle.halton_array(i32, 7)
    assert_same(o_hem, hemisphere_formula(u5, u7, ocos, osin), "numpy hemisphere formula == the oracle's")
    assert_same(r_hem, hemisphere_formula(u5, u7, rcos, rsin), "HaltonSampleHemisphere explained by libm alone")
    share_h = rows_differ(r_hem, o_hem).mean()
    print("libm share: disk(4,5) %.3f %%, hemisphere(5,7) %.3f %% of %d indices" % (100 * share_d, 100 * share_h, n))
    assert share_d <= 0.03 and share_h <= 0.03
    # the square root is NOT under the rule: IEEE on both sides
    x = np.abs(np.random.default_rng(5).normal(size=100000)).astype(F)
    assert_same(ref.libm(ref.SQRT, x), np.sqrt(x), "sqrtf")


# ================================================================== (b) Sphere::Intersect
def emulate_first_root(o, d, c, r):
    """binary32 emulation of the sphere test's first root (used only to PICK inputs at the near bound and at the tangent)"""
    oc = o - c
    a, b = dot3(d, d), dot3(oc, d)
    cc = dot3(oc, oc) - F(r) * F(r)
    disc = b * b - a * cc
    with np.errstate(all="ignore"):
        return disc, (-b - np.sqrt(disc)) / a


def rays_for_sphere(rng, c, r, n):
    """n rays around sphere (c, r): origin outside / inside / on the surface, tangent rays, directions of length 1e-3..1e3"""
    c64, ra = np.asarray(c, np.float64), abs(float(r)) if r != 0 else 1.0
    k = n // 5
    unit = lambda m: (lambda v: v / np.linalg.norm(v, axis=1, keepdims=True))(rng.normal(size=(m, 3)))
    parts = []
    # outside, aimed at a point within 1.5 r of the centre (hits and misses)
    o = c64 + unit(k) * ra * rng.uniform(1.01, 30, (k, 1))
    t = c64 + unit(k) * ra * rng.uniform(0, 1.5, (k, 1))
    parts.append((o, t - o))
    # inside
    o = c64 + unit(k) * ra * rng.uniform(0, 0.999, (k, 1))
    parts.append((o, unit(k)))
    # exactly on the surface as binary32 gives it: c + r n, then any direction (outward, inward, tangent)
    nrm = unit(k)
    o = (np.asarray(c, F) + F(ra) * nrm.astype(F)).astype(np.float64)
    dd = unit(k)
    dd[: k // 3] = np.cross(nrm[: k // 3], dd[: k // 3])  # tangent to the surface
    parts.append((o, dd))
    # tangent rays: from outside towards a silhouette point, then the origin nudged by -2..2 ulp
    o = c64 + unit(k) * ra * rng.uniform(1.5, 20, (k, 1))
    oc = c64 - o
    L = np.linalg.norm(oc, axis=1, keepdims=True)
    perp = np.cross(oc, unit(k))
    perp /= np.linalg.norm(perp, axis=1, keepdims=True)
    sil = c64 + perp * ra * np.sqrt(np.maximum(0, 1 - (ra / L) ** 2)) - oc / L * (ra * ra / L)
    parts.append((o, sil - o))
    # the rest: random rays through the neighbourhood
    m = n - 4 * k
    o = c64 + rng.normal(size=(m, 3)) * ra * 3
    parts.append((o, unit(m)))
    o = np.concatenate([p[0] for p in parts])
    d = np.concatenate([p[1] for p in parts])
    d = d / np.linalg.norm(d, axis=1, keepdims=True) * 10 ** rng.uniform(-3, 3, (n, 1)) ** (rng.random((n, 1)) < 0.5)
    rays = np.concatenate([o, d], 1).astype(F)
    steps = rng.integers(-2, 3, k)
    col = rays[3 * k:4 * k, 1].copy()
    for s in (-2, -1, 1, 2):
        sel = steps == s
        for _ in range(abs(s)):
            col[sel] = np.nextafter(col[sel], F(np.inf if s > 0 else -np.inf))
    rays[3 * k:4 * k, 1] = col
    return rays


def near_bound_rays(c, r):
    """Rays along +z from the origin at sphere (0, 0, cz), r: directions (0, 0, s) picked, by emulation, so that the first root
    lands exactly on the bias 0.001f and within 2 ulp either side of it."""
    cz = np.nextafter(F(c[2]), F(np.inf)) if False else F(c[2])
    s = F(1) + np.arange(-60000, 60000, dtype=np.float64).astype(F) * F(2.0 ** -23)
    d = np.stack([np.zeros_like(s), np.zeros_like(s), s], 1)
    o = np.zeros_like(d)
    _, t = emulate_first_root(o, d, np.array([c[0], c[1], cz], F), r)
    lo, hi = np.nextafter(np.nextafter(BIAS, F(0)), F(0)), np.nextafter(np.nextafter(BIAS, F(1)), F(1))
    sel = (t >= lo) & (t <= hi)
    return np.concatenate([o[sel], d[sel]], 1), t[sel]


def test_sphere_intersect_is_the_reference_code(ref, oracle):
    """>= 10^6 rays: origin outside / inside / exactly on the surface, tangent rays with discriminant 0 and a few ulp either side,
    hits exactly at the near bound (the bias of ray-tracing.cpp:52) and just either side, direction lengths 1e-3..1e3, centres
    out to 1e6, radii 1e-3..1e3, radius 0 and a negative radius.  Compared: hit flag, t, position, normal, uv.
    The reference passes no tmin/tmax; its only bound is the bias.
    Radius 0 and a negative radius are well defined in the reference (r enters as r*r in the test and as a divisor of the
    normal: r = 0 can only hit through rounding and then divides by zero, r < 0 gives the inward normal), so the oracle must
    equal it there too -- recorded below by the same bitwise comparison."""
    rng = np.random.default_rng(20240521)
    spheres = [(0, 0, 0, 1), (0, 0, 1, 0.5), (0, -1000, 0, 1000), (0, -100.5, 1, 100), (4, 1, 0, 1), (0.3, 0.2, -7.1, 0.2)]
    for _ in range(36):
        r = 10 ** rng.uniform(-3, 3)
        c = rng.normal(size=3) * 10 ** rng.uniform(-1, 6) / np.sqrt(3)
        spheres.append((c[0], c[1], c[2], r))
    spheres += [(0.5, 0.25, 2, 0.0), (0.5, 0.25, 2, -0.75), (1e6, -1e6, 1e6, 1e-3), (1e6, 1e6, -1e6, 1e3)]
    total = tangent_zero = tangent_pos = tangent_neg = 0
    orc = oracle.Oracle()
    for (cx, cy, cz, r) in spheres:
        rays = rays_for_sphere(rng, (cx, cy, cz), r, 22000)
        sph = np.array([cx, cy, cz, r], F)
        disc, _ = emulate_first_root(rays[:, :3], rays[:, 3:], sph[:3], sph[3])
        tiny = np.abs(disc) <= F(8) * np.spacing(np.maximum(dot3(rays[:, 3:], rays[:, 3:]), F(1e-30)) * np.abs(dot3(rays[:, :3] - sph[:3], rays[:, :3] - sph[:3])))
        tangent_zero += int((disc == 0).sum())
        tangent_pos += int((tiny & (disc > 0)).sum())
        tangent_neg += int((tiny & (disc < 0)).sum())
        orc.upload(flat_scene(oracle, [sph]))
        want = ref.sphere_intersect(sph, rays)
        got = orc.closest_hit(rays, oracle.ACCEL_LIST)
        assert_same(want, got, "Sphere::Intersect, sphere %r" % (sph,))
        hit = want[:, 1].view(np.int32) >= 0
        if r > 0:
            assert 0.02 < hit.mean() < 0.98
        total += len(rays)
    # the near bound: small spheres just in front of the origin
    eq = below = above = 0
    for cz, r in ((0.001 + 2.0 ** -10, 2.0 ** -10), (0.0135, 0.0125), (1.001, 1.0), (0.2510, 0.25)):
        sph = np.array([0, 0, cz, r], F)
        rays, t = near_bound_rays(sph[:3], sph[3])
        eq, below, above = eq + int((t == BIAS).sum()), below + int((t < BIAS).sum()), above + int((t > BIAS).sum())
        orc.upload(flat_scene(oracle, [sph]))
        want, got = ref.sphere_intersect(sph, rays), orc.closest_hit(rays, oracle.ACCEL_LIST)
        assert_same(want, got, "near bound, sphere %r" % (sph,))
        # the guard itself: a first root at or below the bias is not returned
        first = want[:, 0] == t
        assert not first[t <= BIAS].any() and first[t > BIAS].all()
        total += len(rays)
    # exact tangents: |c| = 0, r = 2^k, origin (-2r, r (1 + j eps), 0), direction along x: the discriminant is 0 at j = 0
    for kexp in (-3, 0, 5):
        r = F(2.0 ** kexp)
        j = np.arange(-4, 5)
        o = np.stack([np.full(9, -2 * r, F), r * (F(1) + j.astype(F) * F(2.0 ** -23)), np.zeros(9, F)], 1)
        for s in (0.25, 1.0, 8.0):
            rays = np.concatenate([o, np.tile(np.array([s, 0, 0], F), (9, 1))], 1)
            sph = np.array([0, 0, 0, r], F)
            disc, _ = emulate_first_root(rays[:, :3], rays[:, 3:], sph[:3], sph[3])
            assert (disc[j == 0] == 0).all() and (disc[j < 0] >= 0).all() and (disc[j > 0] <= 0).all() and (disc > 0).any() and (disc < 0).any()
            tangent_zero += int((disc == 0).sum())
            orc.upload(flat_scene(oracle, [sph]))
            want = ref.sphere_intersect(sph, rays)
            assert_same(want, orc.closest_hit(rays, oracle.ACCEL_LIST), "exact tangent")
            assert (want[:, 1].view(np.int32)[disc <= 0] == -1).all() and (want[:, 1].view(np.int32)[disc > 0] == 0).all()
            total += 9
    print("sphere test: %d rays; discriminant == 0: %d, within 8 ulp above / below 0: %d / %d; first root == bias: %d, below: %d, above: %d"
          % (total, tangent_zero, tangent_pos, tangent_neg, eq, below, above))
    assert total >= 10**6 and tangent_zero > 0 and tangent_pos > 0 and tangent_neg > 0 and eq > 0 and below > 0 and above > 0


# ================================================================== (c) scene scans
def scene_rays(rng, sph, n):
    """Rays at a sphere list: origins around it, aimed at sphere centres, at silhouettes (grazing), and at random"""
    c = np.stack([sph["cx"], sph["cy"], sph["cz"]], 1).astype(np.float64)
    r = np.abs(sph["r"].astype(np.float64))
    small = r < 50
    pick = np.flatnonzero(small) if small.any() else np.arange(len(r))
    centre = np.median(c[pick], axis=0)
    extent = max(1.0, float(np.percentile(np.linalg.norm(c[pick] - centre, axis=1) + r[pick], 90)))
    o = centre + rng.normal(size=(n, 3)) * extent * np.array([1.2, 0.3, 1.2])
    o[:, 1] = np.abs(o[:, 1] - centre[1]) + centre[1] + 0.01
    k = rng.choice(pick, n)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    mode = rng.random(n)
    target = c[k] + u * (r[k] * np.where(mode < 0.45, rng.uniform(0, 1, n), np.where(mode < 0.6, 1 + rng.normal(size=n) * 1e-5, 3.0)))[:, None]
    d = target - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([o, d], 1).astype(F)


# Which hits may BvhNode lose?  Its slab test (BoundingBox::Intersects) and the sphere test are both binary32 and disagree near a
# box's boundary -- and, for origins far from a small sphere, well outside it: the discriminant's error (<= 16 eps a G,
# G ~ 2 |o|^2 + 2 (|c| + r)^2, rt_oracle.h) then exceeds r^2, the list "hits" a sphere the exact ray misses, and the tree rightly
# never visits it.  Detected from the list's result: the EXACT ray (binary64) does not pass through the winning sphere's box
# shrunk by delta on every side, delta = 1e-6 (|o| + |c| + r): about 17 eps of the largest coordinate difference the slab test
# forms, against the ~8 eps its subtractions, reciprocal, products and the merged boxes' centre/extent rounding can add up to.
# A ray through the shrunk leaf box is at least delta inside every enclosing box too, so no level of the tree may reject it.
SLAB_DELTA = 1e-6


def passes_shrunk_box(rays, c, r):
    o, d = rays[:, :3].astype(np.float64), rays[:, 3:].astype(np.float64)
    c, r = c.astype(np.float64), np.abs(r.astype(np.float64))
    delta = SLAB_DELTA * (np.linalg.norm(o, axis=1) + np.linalg.norm(c, axis=1) + r)
    half = (r - delta)[:, None]
    with np.errstate(all="ignore"):
        t1, t2 = (c - half - o) / d, (c + half - o) / d
    par = d == 0
    inside = np.abs(c - o) <= half
    tmin = np.where(par, -np.inf, np.minimum(t1, t2)).max(axis=1)
    tmax = np.where(par, np.inf, np.maximum(t1, t2)).min(axis=1)
    return (half[:, 0] > 0) & (tmin <= tmax) & (tmax >= 0) & (inside | ~par).all(axis=1)


def classify_bvh(list_hits, bvh_hits, rays, sph):
    """-> (equal, tie, lost, unexplained) masks of BvhNode's result against the list scan's"""
    diff = rows_differ(list_hits, bvh_hits)
    li, bi = list_hits[:, 1].view(np.int32), bvh_hits[:, 1].view(np.int32)
    tie = diff & (li >= 0) & (bi >= 0) & (li != bi) & (bits(list_hits[:, 0]) == bits(bvh_hits[:, 0]))
    # the list has a hit the tree lost: the tree then reports a miss or a strictly farther sphere
    cand = diff & ~tie & (li >= 0) & ((bi < 0) | (bvh_hits[:, 0] > list_hits[:, 0]))
    lost = np.zeros_like(cand)
    q = np.flatnonzero(cand)
    if len(q):
        w = sph[li[q]]
        lost[q] = ~passes_shrunk_box(rays[q], np.stack([w["cx"], w["cy"], w["cz"]], 1), w["r"])
    return ~diff, tie, lost, diff & ~tie & ~lost


def random_scene(rng, oracle, n):
    sph = np.zeros(n, dtype=oracle.SPHERE_DTYPE)
    sph["cx"], sph["cz"] = rng.uniform(-15, 15, n), rng.uniform(-15, 15, n)
    sph["r"] = 10 ** rng.uniform(-1.3, 0.2, n)
    sph["cy"] = np.where(rng.random(n) < 0.7, sph["r"], rng.uniform(0, 4, n))
    return sph


def run_scan_scene(ref, oracle, label, sph, rays, tie_scene=False, same_tree=False):
    sc = flat_scene(oracle, np.stack([sph["cx"], sph["cy"], sph["cz"], sph["r"]], 1))
    out = {}

    def oracle_side():  # the oracle's scans on a second thread (its own context; ctypes releases the GIL)
        orc = oracle.Oracle()
        orc.upload(sc)
        out["list"] = orc.closest_hit(rays, oracle.ACCEL_LIST)
        out["bvh"] = orc.closest_hit(rays, oracle.ACCEL_BVH)
        orc.close()

    th = threading.Thread(target=oracle_side)
    th.start()
    rs = ref.Scene(sc.spheres, bvh_srand=1)
    r_list, r_bvh = rs.list_closest(rays), rs.bvh_closest(rays)
    rs.close()
    th.join()
    assert_same(r_list, out["list"], "%s: list scan (hit index included)" % label)
    n = len(rays)
    eq_r, tie_r, lost_r, bad_r = classify_bvh(r_list, r_bvh, rays, sc.spheres)
    eq_o, tie_o, lost_o, bad_o = classify_bvh(out["list"], out["bvh"], rays, sc.spheres)
    assert not bad_r.any(), "%s: reference BvhNode differs from the list on %d rays that are neither ties nor grazing losses" % (label, bad_r.sum())
    assert not bad_o.any(), "%s: oracle BvhNode differs from the list on %d rays that are neither ties nor grazing losses" % (label, bad_o.sum())
    special = tie_r | lost_r | tie_o | lost_o
    assert_same(r_bvh[~special], out["bvh"][~special], "%s: BvhNode" % label)
    share = special.mean()
    print("%-22s n=%5d rays=%d hits=%.2f  ties ref/orc %d/%d  slab-test losses ref/orc %d/%d  share %.2e"
          % (label, len(sph), n, (r_list[:, 1].view(np.int32) >= 0).mean(), tie_r.sum(), tie_o.sum(), lost_r.sum(), lost_o.sum(), share))
    if not tie_scene:
        assert share <= 1e-4, "%s: ties + grazing losses are %.2e of the rays" % (label, share)
    if same_tree:
        # every split axis sorts these spheres alike, so both trees are the same tree whatever std::rand() returns: the
        # oracle must hand every exact tie to the sphere the REFERENCE hands it to
        assert tie_r.sum() > 0.05 * n
        assert_same(r_bvh, out["bvh"], "%s: the reference's tie winner" % label)
    return share


def test_list_and_bvh_scans_are_the_reference_code(ref, oracle, counter_mode):
    """cover, three, grid10k and 20 random scenes (n = 1 .. 2,300): the driver's loop of Sphere::Intersect == ORC_ACCEL_LIST on
    2 * 10^5 rays each, hit index included; the reference's BvhNode == ORC_ACCEL_BVH except on exact ties and on the hits its slab
    test loses, both detected from the list's result (classify_bvh) and capped at 1e-4 of the rays.  The two trees are not the same tree
    (split axes: this C library's std::rand() % 3 there, a private generator in the oracle), which is why results are compared.
    Tie scenes: duplicated spheres.  In the 'diagonal' ones every sphere has cx == cy == cz, so all three axes sort alike and
    the trees coincide: there the oracle must give the reference's tie winner (orc_use_reference_bvh_tie_rule(1), the default)."""
    rng = np.random.default_rng(77)
    n_rays = 200000
    oracle.lib().orc_use_reference_bvh_tie_rule(1)
    for name, aspect in (("three", 2.0), ("cover", 1.5), ("grid10k", 1.0)):
        sc = oracle.build_scene(name, 1, aspect)
        run_scan_scene(ref, oracle, name, sc.spheres, scene_rays(rng, sc.spheres, n_rays))
    sizes = [1, 2300] + [int(round(np.exp(v))) for v in rng.uniform(np.log(2), np.log(2300), 18)]
    for k, n in enumerate(sizes):
        sph = random_scene(rng, oracle, n)
        run_scan_scene(ref, oracle, "random %d" % k, sph, scene_rays(rng, sph, n_rays))
    # ties, general position: the list's lower-index rule on both sides; the trees' winners may differ (different trees)
    sph = random_scene(rng, oracle, 150)
    sph = np.concatenate([sph, sph[:60]])
    run_scan_scene(ref, oracle, "duplicates", sph, scene_rays(rng, sph, n_rays), tie_scene=True)
    # ties, same tree
    for n in (1, 3, 32, 150):
        v = np.sort(rng.uniform(-8, 8, n)).astype(F)
        sph = np.zeros(2 * n, dtype=oracle.SPHERE_DTYPE)
        sph["cx"] = sph["cy"] = sph["cz"] = np.repeat(v, 2)
        sph["r"] = np.repeat(10 ** rng.uniform(-1, 0.3, n), 2).astype(F)
        run_scan_scene(ref, oracle, "diagonal duplicates", sph, scene_rays(rng, sph, n_rays), tie_scene=True, same_tree=True)


# ================================================================== (d) Camera
def camera_members(cam):
    return np.frombuffer(bytes(cam), dtype=np.float32).copy()


def test_camera_constructor_and_get_ray(ref, oracle):
    """Camera::Camera for 200 random parameter sets and the five BASELINE cameras: every member of rt_camera; where tan differs
    (libm rule) the oracle's formula with the reference's tanf must give the reference's members.  Then GetRay for 10^5
    (uv, lens offset) quadruples on each camera, both sides holding the same members."""
    rng = np.random.default_rng(11)
    _, _, rtan = ref_math(ref)
    _, _, otan = orc_math(oracle)
    cover_focal = float(np.sqrt(dot3(np.array([12, 1, -2.5], F), np.array([12, 1, -2.5], F))))
    sets = [((0, 0, 0), (0, 0, 1), 90.0, 2.0, 1.0, 0.0), ((12, 2, -2.5), (0, 1, 0), 25.0, 1.5, cover_focal, 0.4),
            ((12, 2, -2.5), (0, 1, 0), 25.0, 1.5, cover_focal, 0.4), ((12, 2, -2.5), (0, 1, 0), 25.0, 1920 / 1080.0, cover_focal, 2.0),
            ((12, 2, -2.5), (0, 1, 0), 25.0, 1.0, cover_focal, 0.4)]
    for name, aspect, ap, k in (("three", 2.0, -1.0, 0), ("cover", 1.5, -1.0, 1), ("cover", 1920 / 1080.0, 2.0, 3), ("grid10k", 1.0, -1.0, 4)):
        o, l, fov, asp, foc, aper = sets[k]
        got = ref.camera_make(np.array(o, F), np.array(l, F), fov, asp, foc, aper)
        want = camera_members(oracle.build_scene(name, 1, aspect, ap).camera)
        if not same(camera_members(got), want):  # only through tan
            mx, my, oip = camera_formula(np.array(o, F), np.array(l, F), fov, asp, rtan)
            assert same(camera_members(got)[[4, 5, 6, 8, 9, 10, 12, 13, 14]], np.concatenate([mx, my, oip]))
            assert same(camera_members(got)[[0, 1, 2, 3, 7, 11, 15, 16, 17]], want[[0, 1, 2, 3, 7, 11, 15, 16, 17]])
    for _ in range(200):
        o = (rng.normal(size=3) * 10 ** rng.uniform(-1, 2)).astype(F)
        l = (o + rng.normal(size=3) * 10 ** rng.uniform(-1, 2)).astype(F)
        sets.append((tuple(o), tuple(l), float(rng.uniform(1, 170)), float(rng.uniform(0.3, 3)), float(10 ** rng.uniform(-1, 2)), float(rng.choice([0.0, rng.uniform(0, 3)]))))
    excused = 0
    for (o, l, fov, asp, foc, aper) in sets:
        o, l = np.array(o, F), np.array(l, F)
        fov, asp, foc, aper = (float(F(v)) for v in (fov, asp, foc, aper))
        got = camera_members(ref.camera_make(o, l, fov, asp, foc, aper))
        cam = oracle.RtCamera()
        oracle.lib().orc_camera_make(o.ctypes.data_as(C.POINTER(C.c_float)), l.ctypes.data_as(C.POINTER(C.c_float)), fov, asp, foc, aper, C.byref(cam))
        want = camera_members(cam)
        mx, my, oip = camera_formula(o, l, fov, asp, otan)
        assert same(want[[4, 5, 6, 8, 9, 10, 12, 13, 14]], np.concatenate([mx, my, oip])), "numpy camera formula == the oracle's"
        if not same(got, want):
            excused += 1
            mx, my, oip = camera_formula(o, l, fov, asp, rtan)
            patched = want.copy()
            patched[[4, 5, 6, 8, 9, 10, 12, 13, 14]] = np.concatenate([mx, my, oip])
            assert same(got, patched), "Camera::Camera differs beyond tanf: %r vs %r" % (got, want)
        q = np.concatenate([rng.uniform(-0.2, 1.2, (100000, 2)), rng.uniform(-1, 1, (100000, 2))], 1).astype(F)
        q[:8] = [[0, 0, 0, 0], [1, 1, 0, 0], [0.5, 0.5, 0, 0], [0.5, 0.5, 1, 0], [0.5, 0.5, 0, -1], [0, 1, -1, 1], [1, 0, 1, 1], [0.5, 0.5, -0.0, 0.0]]
        assert_same(ref.camera_ray(cam, q), oracle.camera_rays(cam, q), "Camera::GetRay")
    print("camera: %d of %d constructors differ through tanf (explained)" % (excused, len(sets)))
    assert excused <= 0.1 * len(sets)


# ================================================================== (e) textures and materials
def colours(rng, byte):
    c = rng.uniform(0, 1, 3)
    return tuple(np.rint(c * 255) / 255.0) if byte else tuple(c)


def test_textures_on_a_grid_with_the_cell_boundaries(ref, oracle):
    rng = np.random.default_rng(3)
    for tiling in (1.0, 2.0, 4.0, 7.0, 10.0, 2500.0, 0.5, 3.3):
        g = np.arange(0, 2 * int(max(tiling, 1)) + 1 if tiling < 100 else 41) / (tiling if tiling < 100 else 10.0)
        g = np.concatenate([g, np.nextafter(g.astype(F), F(-1)), np.nextafter(g.astype(F), F(9)), rng.uniform(-1, 2, 50), [-0.0, 1.0, -1.0 / 3]]).astype(F)
        uv = np.stack(np.meshgrid(g, g), -1).reshape(-1, 2)
        for byte in (True, False):
            m = material_record(oracle, OPAQUE, tex=1, tiling=tiling, rgb0=colours(rng, byte), rgb1=colours(rng, byte))
            assert_same(ref.texture_eval(m, uv), oracle.texture_eval(m, uv), "CheckerTexture tiling %g" % tiling)
            m["tex_type"] = 0
            assert_same(ref.texture_eval(m, uv[:500]), oracle.texture_eval(m, uv[:500]), "ConstTexture")


def material_sets(rng, oracle, kind, n_sets):
    out = []
    for k in range(n_sets):
        smooth = (0.0, 1.0, 16.0)[k] if k < 3 else float(rng.choice([rng.uniform(0, 1), rng.uniform(1, 64)]))
        ior = (1.0, 1.5, 2.4, 0.7, 0.95)[k % 5] if k < 10 else float(rng.uniform(0.5, 3))
        out.append(material_record(oracle, kind, tex=int(kind != GLASS and k % 3 == 1), smoothness=smooth, ior=ior, tiling=float(rng.choice([2.0, 10.0, 2500.0])),
                                   rgb0=colours(rng, k % 2 == 0), rgb1=colours(rng, k % 4 < 2), luminance=float(rng.choice([1.0, 8000.0, rng.uniform(0, 100)]))))
    return out


def hits_for(rng, n, ior):
    """n (ray origin, direction, pos, normal, uv): random incidence, grazing, from inside (n.d > 0), the TIR boundary"""
    nrm = rng.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    tan = np.cross(nrm, rng.normal(size=(n, 3)))
    tan /= np.linalg.norm(tan, axis=1, keepdims=True)
    cosv = rng.uniform(-1, 1, n)
    k = n // 8
    cosv[:k] = rng.normal(size=k) * 1e-6                       # grazing, either side
    cosv[k:k + 8] = [0, 1, -1, 1e-8, -1e-8, 1e-4, -1e-4, 0.5]
    crit = np.sqrt(max(0.0, 1 - min(1.0, 1 / ior ** 2))) if ior > 1 else np.sqrt(max(0.0, 1 - min(1.0, ior ** 2)))
    cosv[2 * k:3 * k] = crit * (1 + rng.normal(size=k) * 1e-6)   # total internal reflection boundary, from inside
    cosv[3 * k:4 * k] = -crit * (1 + rng.normal(size=k) * 1e-6)  # and the same angle from outside
    d = -cosv[:, None] * nrm + np.sqrt(np.maximum(0, 1 - cosv ** 2))[:, None] * tan
    d *= np.where(rng.random(n) < 0.5, 1.0, 10 ** rng.uniform(-1, 1, n))[:, None]
    pos = rng.normal(size=(n, 3)) * 5
    nrm32 = nrm.astype(F)
    nrm32[4 * k:5 * k, 0] = rng.choice([0.5, -0.5, np.nextafter(F(0.5), F(0)), 0.0], k)  # the basis switch |n.x| < 0.5
    uv = rng.uniform(0, 1, (n, 2))
    return np.concatenate([pos - d, d, pos, nrm32, uv], 1).astype(F)


def explain_diffuse(ref, oracle, cnt, normal, r_dir, o_dir, label):
    """libm rule for the diffuse bounce: rows whose scattered direction differs must be diffuse bounces (m_sampleIndex advanced)
    whose HaltonSampleHemisphere differs through cos/sin, and the oracle's formula on the reference's sample must give the
    reference's direction.  Returns the number of rows excused."""
    d = rows_differ(r_dir, o_dir)
    if not d.any():
        return 0
    assert (cnt[d, 2] == cnt[d, 0] + 1).all(), "%s: a direction differs where no hemisphere sample was drawn" % label
    idx = cnt[d, 0]
    r_hem, o_hem = ref.halton_hemisphere(idx, 5, 7), orc_hemisphere(oracle, idx, 5, 7)
    rcos, rsin, _ = ref_math(ref)
    i32 = idx.astype(np.uint32)
    assert (idx < 2**32).all()
    assert_same(r_hem, hemisphere_formula(oracle.halton_array(i32, 5), oracle.halton_array(i32, 7), rcos, rsin), label + ": hemisphere sample explained by libm")
    assert rows_differ(r_hem, o_hem).all(), "%s: a direction differs although the hemisphere samples agree" % label
    assert_same(r_dir[d], diffuse_direction(normal[d], r_hem), label + ": diffuse direction = the oracle's formula on the reference's sample")
    assert_same(o_dir[d], diffuse_direction(normal[d], o_hem), label + ": numpy diffuse formula == the oracle's")
    return int(d.sum())


def test_scatter_is_the_reference_code(ref, oracle, counter_mode):
    """Per material kind 50 parameter sets x 10^4 hits, fed in the same order to the reference's material object and to ONE oracle
    material object in reference-counter mode (orc_unit_scatter_n, use_counters): scattered flag, attenuation, scattered origin and
    direction.  Then the same hits with the uniforms the reference's counters produced (ref_halton at the recorded counter values)
    scripted into the oracle: same outputs, and the draws the oracle consumed == the reference's counter deltas -- one per
    m_reflectionProbabilitySampleIndex step (Metal's dead coin included), two (bases 5 and 7) per m_sampleIndex step of
    DielectricOpaque, one (base 7) per m_sampleIndex step of DielectricTransparent."""
    rng = np.random.default_rng(5150)
    n_hits, excused, rows = 10000, 0, 0
    for kind in (OPAQUE, METAL, GLASS, EMISSIVE):
        for m in material_sets(rng, oracle, kind, 50):
            label = "kind %d smoothness %g ior %g" % (kind, m["smoothness"][0], m["ior"][0])
            h = hits_for(rng, n_hits, float(m["ior"][0]))
            mat = ref.Material(m)
            r_out, cnt = mat.scatter(h)
            mat.close()
            zeros = np.zeros((n_hits, 3), F)
            o_out = oracle.scatter_n(m, np.concatenate([h, zeros], 1), use_counters=True)
            assert_same(r_out[:, :7], o_out[:, :7], label + ": flag, attenuation, origin (counter mode)")
            excused += explain_diffuse(ref, oracle, cnt, h[:, 9:12], r_out[:, 7:10], o_out[:, 7:10], label)
            # scripted: the uniforms the reference's counters stand for
            d_s, d_r = (cnt[:, 2] - cnt[:, 0]).astype(np.int64), (cnt[:, 3] - cnt[:, 1]).astype(np.int64)
            draws = np.zeros((n_hits, 3), F)
            if kind == OPAQUE:
                draws[:, 0], draws[:, 1], draws[:, 2] = ref.halton(cnt[:, 1], 3), ref.halton(cnt[:, 0], 5), ref.halton(cnt[:, 0], 7)
                want_draws = d_r + 2 * d_s
                assert set(np.unique(d_r)) <= {0, 1} and (d_s <= d_r).all()
            elif kind == METAL:
                draws[:, 0] = ref.halton(cnt[:, 1], 3)
                want_draws = d_r
                front = dot3(-h[:, 3:6], h[:, 9:12]) > 0
                assert (d_r == front).all() and (d_s == 0).all()  # the coin is drawn for every front-side hit
            elif kind == GLASS:
                draws[:, 0] = ref.halton(cnt[:, 0], 7)
                want_draws = d_s
                assert (d_s == 1).all() and (d_r == 0).all()
            else:
                want_draws = np.zeros(n_hits, np.int64)
                assert (d_s == 0).all() and (d_r == 0).all() and (r_out == 0).all()
            s_out = oracle.scatter_n(m, np.concatenate([h, draws], 1), use_counters=False)
            assert_same(r_out[:, :7], s_out[:, :7], label + ": flag, attenuation, origin (scripted uniforms)")
            assert np.array_equal(s_out[:, 10].astype(np.int64), want_draws), label + ": draws consumed"
            explain_diffuse(ref, oracle, cnt, h[:, 9:12], r_out[:, 7:10], s_out[:, 7:10], label + " (scripted)")
            assert_same(o_out[:, :10], s_out[:, :10], label + ": counter mode == scripted uniforms inside the oracle")
            rows += n_hits
            if kind != EMISSIVE:
                assert 0.02 < r_out[:, 0].mean() <= 1.0
    print("scatter: %d hits, %d (%.3f %%) diffuse directions differ through libm, all explained" % (rows, excused, 100.0 * excused / rows))
    assert excused <= 0.05 * rows


def shade_lights(oracle, rng, n):
    fixed = [oracle.make_light((0, 1, 0), (1.0, 0.97, 0.88), 40000.0), oracle.make_light((1, 1, 1), (1.0, 0.97, 0.88), 40000.0)]
    out = []
    for k in range(n):
        out.append(fixed[k] if k < 2 else oracle.make_light(rng.normal(size=3), rng.uniform(0, 1, 3), float(10 ** rng.uniform(0, 5))))
    return out


def surface_hits(rng, n):
    """hits ON the unit sphere at the origin: pos = normal (so occlusion queries start on the subject's own surface); a block
    with normal.y == 0 exactly (light (0,1,0) exactly on the horizon: nDotL == 0) and one with normal.y < 0 (below it)"""
    nrm = rng.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm = nrm.astype(F)
    k = n // 6
    nrm[:k, 1] = 0.0
    nrm[k:2 * k, 1] = -np.abs(nrm[k:2 * k, 1])
    nrm[2 * k, :] = [1, 0, 0]
    uv = np.stack([F(0.5) * nrm[:, 0] + F(0.5), F(0.5) * nrm[:, 2] + F(0.5)], 1)
    return np.concatenate([nrm, nrm, uv], 1).astype(F)


def test_emit_and_shade_are_the_reference_code(ref, oracle):
    """Emit + Shade for every material kind: 50 parameter sets x 10^4 hits with one light (against orc_unit_emit_shade's scene form,
    orc_unit_emit_shade_scene); then 0, 2, 3 and 8 lights in list order, with and without occluders, including a light exactly on
    and below the surface's horizon.  Both sides shade sphere 0 of the SAME sphere list and test occlusion against that list."""
    rng = np.random.default_rng(99)
    occluders = [(0, 3, 0, 1), (2.5, 2.5, 2.5, 0.8), (-3, 0.5, 1, 1.5), (0, 1.5, 0, 0.25)]
    orc = oracle.Oracle()
    horizon = below = occluded_any = 0
    for kind in (OPAQUE, METAL, GLASS, EMISSIVE):
        for k, m in enumerate(material_sets(rng, oracle, kind, 50)):
            label = "kind %d set %d" % (kind, k)
            mat = ref.Material(m)
            configs = [(1, False, 10000)]
            if k < 12:
                configs += [(nl, occ, 2000) for nl in (0, 2, 3, 8, 1) for occ in (False, True)]
            for n_lights, with_occ, n in configs:
                lights = shade_lights(oracle, rng, n_lights)
                spheres = [(0, 0, 0, 1)] + (occluders if with_occ else [])
                mats = np.concatenate([m] + [material_record(oracle, OPAQUE)] * (len(spheres) - 1))
                sc = flat_scene(oracle, spheres, mats, lights)
                orc.upload(sc)
                rs = ref.Scene(sc.spheres)
                hits = surface_hits(rng, n)
                vo = (rng.normal(size=3) * 10).astype(F)
                shade, occ = mat.shade(hits, lights, vo, rs)
                want = mat.emit(hits) + shade
                got = orc.emit_shade_scene(0, vo, hits)
                assert_same(want, got, "%s, %d lights, occluders %s" % (label, n_lights, with_occ))
                if n_lights == 1:
                    assert_same(mat.light_shade(hits, lights[0], vo, rs), shade, label + ": DirectionalLight::Shade alone")
                    if not with_occ and k < 3:  # the existing single-light entry point (unoccluded by construction)
                        vis = occ[:, 0] == 0
                        for q in np.flatnonzero(vis)[:200]:
                            out = (C.c_float * 3)()
                            P = lambda a: np.ascontiguousarray(a, F).ctypes.data_as(C.POINTER(C.c_float))
                            oracle.lib().orc_unit_emit_shade(C.byref(oracle.RtMaterial.from_buffer_copy(m.tobytes())), C.byref(lights[0]), P(vo), P(hits[q, 0:3]), P(hits[q, 3:6]), P(hits[q, 6:8]), out)
                            assert same(np.array(list(out), F), want[q])
                if n_lights:
                    nl0 = dot3(hits[:, 3:6], np.array(list(lights[0].direction), F))
                    horizon += int((nl0 == 0).sum())
                    below += int((nl0 < 0).sum())
                    occluded_any += int((occ == 1).sum())
                    assert (occ <= 1).all()  # every light casts its shadow ray, in list order
                    if kind != EMISSIVE:
                        dark = (occ == 1).all(axis=1)
                        assert (shade[dark] == 0).all()
                rs.close()
            mat.close()
    print("shade: hits with nDotL == 0: %d, below the horizon: %d, occluded light queries: %d" % (horizon, below, occluded_any))
    assert horizon > 1000 and below > 1000 and occluded_any > 1000
    # DirectionalLight's constructor (normalise, XMLoadColor of the XMCOLOR) against the oracle's records
    for _ in range(200):
        d, c, lum = rng.normal(size=3) * 10 ** rng.uniform(-2, 2), rng.uniform(-0.1, 1.1, 3), float(rng.uniform(0, 1e5))
        got, want = ref.light_make(d.astype(F), *[float(F(v)) for v in c], lum), oracle.make_light(d, c, lum)
        assert bytes(got) == bytes(want)
    assert bytes(ref.light_make(np.array([1, 1, 1], F), 1.0, 0.97, 0.88, 40000.0)) == bytes(oracle.build_scene("cover", 1, 1.5).sun)


# ================================================================== (f) one whole path
def drive_paths(ref, oracle, name, aspect, W, H, pixels, max_depth):
    """GetHitColor driven from Python through the ref_* calls, written from the oracle's documented contract (oracle_api.h,
    rt_oracle.h): primary ray = Camera::GetRay(uv = (i + h2(s), j + h3(s)) / (W, H), offset = HaltonSampleDisk(s + i + j, 4, 5));
    per bounce: closest hit over the list -> Scatter (always called on a hit; draws even at the depth limit) -> Emit + Shade with
    the camera origin (every light queries occlusion over the list) -> recurse while depth < max_depth and scattered; a miss
    returns the sky's Emit.  Radiance in the reference's nesting L = (E + S) + a * L_next, innermost hit (E + S) + 0; times the
    exposure.  Serial, with reference-counter sampling on both sides.
    libm: where the lens sample or a hemisphere sample differs through cos/sin, the reference's value is first checked against
    the oracle's formula (explanation rule) and the path then CONTINUES with the oracle's value, so that every later query of
    every later path can still be compared (the counters are shared by all paths)."""
    sc = oracle.build_scene(name, 1, aspect)
    orc = oracle.Oracle()
    orc.upload(sc)
    rs = ref.Scene(sc.spheres)
    mats = [ref.Material(sc.materials[k:k + 1]) for k in range(sc.n)]
    sky = ref.Material(np.frombuffer(bytes(sc.sky), dtype=oracle.MATERIAL_DTYPE))
    sky_emit = sky.emit(np.zeros((1, 8), F))[0]
    cam_origin = np.array(list(sc.camera.origin)[:3], F)
    lights = [sc.sun]
    sun_dir = np.array(list(sc.sun.direction), F)
    rcos, rsin, _ = ref_math(ref)
    exposure = F(sc.exposure_scale)
    excused_paths = n_queries = 0
    for (i, j, s) in pixels:
        excused = False
        h2, h3 = ref.halton(np.array([s], np.uint64), 2)[0], ref.halton(np.array([s], np.uint64), 3)[0]
        uv = (F(F(i) + h2) / F(W), F(F(j) + h3) / F(H))
        lens_idx = np.array([s + i + j], np.uint64)
        off = ref.halton_disk(lens_idx, 4, 5)[0]
        o_off = orc_disk(oracle, lens_idx, 4, 5)[0]
        if not same(off, o_off):
            u4, u5 = ref.halton(lens_idx, 4), ref.halton(lens_idx, 5)
            assert same(off, disk_formula(u4, u5, rcos, rsin)[0])
            excused, off = True, o_off
        ray = ref.camera_ray(sc.camera, np.array([[uv[0], uv[1], off[0], off[1]]], F))[0]
        queries, local, atten = [], [], []
        tail = None
        depth = 0
        while True:
            hit = rs.list_closest(ray[None, :])[0]
            idx = int(hit[1:2].view(np.int32)[0])
            if idx < 0:
                queries.append(list(ray) + [0.0, -1.0])
                tail = sky_emit
                break
            queries.append(list(ray) + [0.0, hit[0]])
            h8 = hit[2:10][None, :]
            out, cnt = mats[idx].scatter(np.concatenate([ray, hit[2:10]])[None, :])
            out, cnt = out[0], cnt[0]
            new_dir = out[7:10]
            if sc.materials["type"][idx] == OPAQUE and cnt[2] == cnt[0] + 1:  # a diffuse bounce drew hemisphere sample cnt[0]
                r_hem, o_hem = ref.halton_hemisphere(cnt[0:1], 5, 7), orc_hemisphere(oracle, cnt[0:1], 5, 7)
                if not same(r_hem, o_hem):
                    assert same(new_dir, diffuse_direction(hit[5:8][None, :], r_hem)[0]), "diffuse bounce not explained by libm"
                    excused, new_dir = True, diffuse_direction(hit[5:8][None, :], o_hem)[0]
            shade, occ = mats[idx].shade(h8, lights, cam_origin, rs)
            local.append(mats[idx].emit(h8)[0] + shade[0])
            atten.append(out[1:4])
            queries.append(list(hit[2:5]) + list(sun_dir) + [1.0, float(occ[0, 0])])
            if not (depth < max_depth and out[0] != 0):
                break
            ray = np.concatenate([out[4:7], new_dir]).astype(F)
            depth += 1
        L = tail if tail is not None else np.zeros(3, F)
        for k in range(len(local) - 1, -1, -1):
            innermost = (k == len(local) - 1) and tail is None
            L = local[k] + np.zeros(3, F) if innermost else local[k] + atten[k] * L
        want_rgb = (L * exposure).astype(F)
        got_q, got_rgb = orc.trace_path(W, H, i, j, s, max_depth, 1, accel=oracle.ACCEL_LIST, cap=256)
        want_q = np.array(queries, F)
        assert want_q.shape == got_q.shape, "pixel (%d, %d, %d): %d queries, the oracle made %d" % (i, j, s, len(want_q), len(got_q))
        assert_same(want_q, got_q, "pixel (%d, %d, %d): queries" % (i, j, s))
        assert same(want_rgb, got_rgb), "pixel (%d, %d, %d): colour %r vs %r" % (i, j, s, want_rgb, got_rgb)
        excused_paths += excused
        n_queries += len(queries)
    for m in mats:
        m.close()
    rs.close()
    return excused_paths, n_queries


def test_whole_paths_compose_the_reference_pieces(ref, oracle, counter_mode):
    """2,000 primary rays of `three` and 2,000 of `cover`, depth 50: every recorded query (origin, direction, kind, result) and
    the final colour of orc_unit_trace_path in counter mode with the nested radiance, against the reference's pieces composed
    in Python (drive_paths).  Paths touched by the libm rule are compared in full as well (drive_paths explains how); their
    share is printed and capped at 5 % of the paths of a scene."""
    oracle.lib().orc_use_nested_radiance(1)
    rng = np.random.default_rng(4242)
    for name, aspect, W, H in (("three", 2.0, 200, 100), ("cover", 1.5, 1200, 800)):
        pixels = [(int(rng.integers(0, W)), int(rng.integers(0, H)), int(rng.integers(1, 129))) for _ in range(2000)]
        excused, nq = drive_paths(ref, oracle, name, aspect, W, H, pixels, 50)
        print("%s: 2000 paths, %d queries, %d paths (%.2f %%) touched by the libm rule -- compared in full all the same" % (name, nq, excused, excused / 20.0))
        assert excused <= 0.05 * 2000


# ================================================================== the recorded answers (no reference needed)
def test_oracle_equals_the_answers_recorded_from_the_reference_code(oracle, counter_mode):
    """tests/golden/reference_code_answers.npz holds inputs and the outputs libref.so gave for them (written by
    tests/golden/make_reference_code_answers.py; recorded data, no program text), plus the values ITS libm returned where the
    libm rule applies.  The oracle must reproduce every recorded output; disk / hemisphere / diffuse directions / tan-dependent
    camera members through the oracle's formula on the recorded libm values."""
    g = np.load(os.path.join(GOLDEN, "reference_code_answers.npz"))
    # (a)
    for base in (2, 3, 4, 5, 7):
        assert_same(g["halton_%d" % base], oracle.halton_array(g["halton_index"].astype(np.uint32), base), "HaltonSample base %d" % base)
    fn = oracle.lib().orc_halton
    assert_same(g["halton_big_3"], np.array([fn(int(i), 3) for i in g["halton_big_index"]], F), "HaltonSample above 2^32")
    lut = lambda key: (lambda x, k=key: (assert_same(x, g[k + "_arg"], k + " argument"), g[k])[1])
    idx = g["map_index"].astype(np.uint32)
    u4, u5, u7 = (oracle.halton_array(idx, b) for b in (4, 5, 7))
    assert_same(g["disk"], disk_formula(u4, u5, lut("disk_cos"), lut("disk_sin")), "HaltonSampleDisk")
    assert_same(g["hemisphere"], hemisphere_formula(u5, u7, lut("hem_cos"), lut("hem_sin")), "HaltonSampleHemisphere")
    share = rows_differ(g["disk"], orc_disk(oracle, idx, 4, 5)).mean(), rows_differ(g["hemisphere"], orc_hemisphere(oracle, idx, 5, 7)).mean()
    print("recorded answers: disk %.2f %%, hemisphere %.2f %% differ from the oracle through libm" % (100 * share[0], 100 * share[1]))
    assert max(share) <= 0.03
    # (b)
    orc = oracle.Oracle()
    for k in range(len(g["sphere"])):
        orc.upload(flat_scene(oracle, [g["sphere"][k]]))
        assert_same(g["sphere_hits"][k], orc.closest_hit(g["sphere_rays"][k], oracle.ACCEL_LIST), "Sphere::Intersect %r" % (g["sphere"][k],))
    # (d)
    for k in range(len(g["camera_params"])):
        p = g["camera_params"][k]
        o, l = p[0:3].copy(), p[3:6].copy()
        cam = oracle.RtCamera()
        oracle.lib().orc_camera_make(o.ctypes.data_as(C.POINTER(C.c_float)), l.ctypes.data_as(C.POINTER(C.c_float)), float(p[6]), float(p[7]), float(p[8]), float(p[9]), C.byref(cam))
        want = camera_members(cam)
        tanf = lambda x, k=k: (assert_same(x, g["camera_tan_arg"][k:k + 1], "tan argument"), g["camera_tan"][k:k + 1])[1]
        mx, my, oip = camera_formula(o, l, float(p[6]), float(p[7]), tanf)
        want[[4, 5, 6, 8, 9, 10, 12, 13, 14]] = np.concatenate([mx, my, oip])
        assert same(g["camera_members"][k], want), "Camera::Camera %r" % (p,)
        rec = oracle.RtCamera.from_buffer_copy(g["camera_members"][k].tobytes())
        assert_same(g["camera_rays"][k], oracle.camera_rays(rec, g["camera_uv_offset"][k]), "Camera::GetRay")
    # (e)
    for k in range(len(g["material"])):
        m = g["material"][k:k + 1].view(oracle.MATERIAL_DTYPE).reshape(1)
        h, r_out, cnt = g["scatter_in"][k], g["scatter_out"][k], g["scatter_counters"][k]
        o_out = oracle.scatter_n(m, np.concatenate([h, np.zeros((len(h), 3), F)], 1), use_counters=True)
        assert_same(r_out[:, :7], o_out[:, :7], "scatter %d: flag, attenuation, origin" % k)
        d = rows_differ(r_out[:, 7:10], o_out[:, 7:10])
        if d.any():
            assert (cnt[d, 2] == cnt[d, 0] + 1).all()
            assert_same(r_out[d, 7:10], diffuse_direction(h[d, 9:12], g["scatter_hemisphere"][k][d]), "scatter %d: diffuse direction on the recorded sample" % k)
            assert rows_differ(g["scatter_hemisphere"][k][d], orc_hemisphere(oracle, cnt[d, 0], 5, 7)).all()
        assert d.mean() <= 0.05
        rows = cnt[:, 2] == cnt[:, 0] + 1
        if m["type"][0] == OPAQUE and rows.any():  # the recorded samples themselves, through the recorded cos / sin
            i32 = cnt[rows, 0].astype(np.uint32)
            pick = lambda key: (lambda x, kk=key: g[kk][k][rows])
            assert_same(g["scatter_hemisphere"][k][rows], hemisphere_formula(oracle.halton_array(i32, 5), oracle.halton_array(i32, 7), pick("scatter_cos"), pick("scatter_sin")), "recorded hemisphere samples")
        lights = [oracle.RtLight.from_buffer_copy(g["shade_lights"][k][q].tobytes()) for q in range(int(g["shade_n_lights"][k]))]
        sc = flat_scene(oracle, g["shade_spheres"], np.concatenate([m] + [material_record(oracle, OPAQUE)] * (len(g["shade_spheres"]) - 1)), lights)
        orc.upload(sc)
        assert_same(g["shade_out"][k], orc.emit_shade_scene(0, g["shade_view_origin"][k], g["shade_hits"][k]), "Emit + Shade %d" % k)
        assert_same(g["texture_out"][k], oracle.texture_eval(m, g["texture_uv"]), "texture %d" % k)
