"""The spatial variance source, the part that needs no GPU (include/rt_api.h "spatial variance estimate"; csrc/rt_denoise.h, DESIGN.md
5.9): the host twins (rt_unit_denoise_variance_host, rt_unit_temporal_variance_host -- the source the kernels compile) against a numpy
binary32 restatement of the contract (tests/denoise_spatial_common.py), bit for bit, on synthetic strips and on the CPU oracle's orbit;
what the estimate does to a constant picture and at an edge of the guides; the moments source; the refusals; the selftest."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from denoise_spatial_common import (BILINEAR, MOMENTS, NEAREST, SPATIAL, host_denoise_spatial, host_temporal_spatial, np_denoise_spatial, np_spatial_prepare,
                                    np_temporal_spatial, variance_struct)
from temporal_common import F, NO_TARGET, assert_same_step, history_of, oracle_frame, orbit_scene
from test_denoise_cpu import DEFAULTS, ZERO_K, host_denoise, random_strips
from test_noise_estimate_cpu import assert_same_bits

RT_ERR_INVALID_ARG, RT_ERR_SEQUENCE = 2, 6
# neither dimension a multiple of the 32 x 8 tile; strips smaller than the window (at 5 x 3 and 1 x 1 most taps lie outside)
SHAPES = [(96, 64), (70, 41), (5, 3), (1, 1)]


@pytest.fixture(scope="module")
def scenes(built):
    from cpuraytracer_amd import scenes
    return scenes


@pytest.mark.parametrize("R", [1, 2, 3])
@pytest.mark.parametrize("W,rows", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_twin_equals_numpy(built, W, rows, R):
    rng = np.random.default_rng(100 * W + rows)
    count = {}
    for n, m in ((1, 1), (4, 3), (1, 5)):  # one sample; m != n
        S, _, feat, _, sky = random_strips(rng, W, rows, n, m)
        for what, over in (("defaults", {}), ("all k = 0", ZERO_K), ("one level", dict(levels=1, k_depth=50.0, k_colour=4.0))):
            P = dict(DEFAULTS, **over)
            c, v, g = np_spatial_prepare(S, n, feat, m, P, R, count if what == "defaults" else None)
            want = np_denoise_spatial(S, n, feat, m, P, R)
            got = host_denoise_spatial(S, n, feat, m, P, R)  # sq is a null pointer
            tag = "%d x %d, R %d, n %d m %d, %s" % (W, rows, R, n, m, what)
            assert_same_bits(got["state"], want["state"], tag + ": prepared state")
            assert_same_bits(got["rgb"], want["rgb"], tag + ": den")
            assert_same_bits(got["var"], want["var"], tag + ": den_var")
            assert_same_bits(got["state"][..., :3], S / F(n), tag + ": c0")
            assert np.isfinite(got["state"]).all() and (got["state"][..., 3] >= 0).all() and np.isfinite(got["rgb"]).all() and (got["var"] >= 0).all()
    # not vacuous: taps fell outside the strip; beyond a handful of pixels the guides stopped some taps and the picture has spread
    assert count["skipped"] > 0
    if W * rows > 100:
        assert count["stopped"] > 0 and (v > 0).any()
    if W * rows == 1:
        assert (got["state"][..., 3] == 0).all()  # a lone pixel has no spread


@pytest.mark.parametrize("R", [1, 2, 3])
def test_band_of_rows(built, scenes, R):
    """Rows [8, 32) of a 96 x 64 image through the temporal twin (the entry that knows first_row): on an empty history the prepared state
    is the strip's own -- the band's first and last rows are edges of the picture, taps beyond them are skipped -- and a second frame
    over that history equals numpy for both fetches."""
    W, H, first, rows = 96, 64, 8, 24
    rng = np.random.default_rng(7 + R)
    S, _, feat, _, sky = random_strips(rng, W, rows, 1, 2)
    ids = np.where(sky, 0xFFFFFFFF, rng.integers(0, 4, (rows, W))).astype(np.uint32)
    cam0, cam1 = (orbit_scene(scenes, "cover", W, H, d).camera for d in (0.0, 0.5))
    for fetch in (NEAREST, BILINEAR):
        got = host_temporal_spatial(S, 1, feat, 2, ids, W, H, cam0, R, first_row=first, fetch=fetch)
        want = np_temporal_spatial(S, 1, feat, 2, ids, W, H, cam0, R, first_row=first, fetch=fetch)
        assert_same_step(got, want, "band, R %d, fetch %d, empty history" % (R, fetch))
        alone = host_denoise_spatial(S, 1, feat, 2, DEFAULTS, R)
        assert_same_bits(got["state"], alone["state"], "the band's prepared state is the strip's own")
        assert_same_bits(got["rgb"], alone["rgb"], "... and so is its den")
        assert (got["len"] == 1).all() and (got["target"] == NO_TARGET).all()
        got2 = host_temporal_spatial(S[::-1], 1, feat, 2, ids, W, H, cam1, R, hist=history_of(got), first_row=first, fetch=fetch, T=dict(use_id=0))
        want2 = np_temporal_spatial(S[::-1], 1, feat, 2, ids, W, H, cam1, R, hist=history_of(want), first_row=first, fetch=fetch, T=dict(use_id=0))
        assert_same_step(got2, want2, "band, R %d, fetch %d, second frame" % (R, fetch))
        assert_same_bits(got2["guides"], want2["guides"], "guides")


def flat(W, rows, colour, n=1):
    return np.broadcast_to(np.asarray(colour, F) * F(n), (rows, W, 3)).astype(F)


@pytest.mark.parametrize("R", [1, 2, 3])
def test_constant_picture_has_no_variance(built, R):
    """Every pixel the same colour, random guides: s1 = c sw and s2 = c^2 sw up to rounding, so v0 is rounding noise at most -- and
    EXACTLY 0 where the colour's channels are powers of two, since then w c and w c^2 only move w's exponent and every sum is sw's."""
    rng = np.random.default_rng(3)
    W, rows = 37, 19
    _, _, feat, _, _ = random_strips(rng, W, rows, 1, 2)
    for n in (1, 4):
        got = host_denoise_spatial(flat(W, rows, (0.5, 2.0, 0.125), n), n, feat, 2, DEFAULTS, R)
        assert (got["state"][..., 3] == 0).all() and (got["var"] == 0).all()
        assert_same_bits(got["rgb"], flat(W, rows, (0.5, 2.0, 0.125)), "a constant picture comes back")
    # any colour: |d| <= a few roundings of c^2 per channel (49 taps of two roundings each, two divisions, one product)
    col = (0.3, 0.7, 1.9)
    got = host_denoise_spatial(flat(W, rows, col), 1, feat, 2, DEFAULTS, R)
    assert (got["state"][..., 3] <= 128 * 2.0 ** -24 * sum(c * c for c in col)).all()


@pytest.mark.parametrize("R", [1, 2, 3])
def test_guides_keep_two_flat_regions_apart(built, R):
    """Two half-planes of constant colours 0.5 and 0.25 (exact arithmetic: see above) whose guides differ by far more than the stops allow
    in every one of the four terms.  Each region's own spread is 0, so v0 is whatever leaks across the edge: a tap across weighs
    w = 1 / (1 + x), at most R of a window's 2R + 1 columns lie across, so the far side's share of the weight is p <= R w / (R w + R + 1),
    and a two-valued picture's weighted variance is p (1 - p) dc^2 <= p dc^2.  With all four k at their defaults that is under 1 % of
    the step; switching each k off IN TURN leaves three terms that still hold it under 2 %; switching all four off gives the plain
    variance of the window, R / (2R + 1) of it across."""
    W, rows = 24, 11
    left = np.arange(W)[None, :] < W // 2
    S = np.where(left[..., None], F(0.5), F(0.25)) * np.ones((rows, W, 3), F)
    feat = np.zeros((rows, W, 8), F)
    feat[..., 0:3] = np.where(left[..., None], F(0.1), F(0.9))                                   # albedo: |da|^2 = 1.92
    feat[..., 3:6] = np.where(left[..., None], np.array([1, 0, 0], F), np.array([0, 1, 0], F))   # normal: |dn|^2 = 2
    feat[..., 6] = np.where(left, F(4.0), F(8.0))                                                 # depth: (dz / zm)^2 = 1/4
    feat[..., 7] = np.where(left, F(1.0), F(0.25))                                                # coverage: dc^2 = 0.5625
    dc2 = 3 * 0.25 ** 2  # the squared colour step, channels summed
    near = np.abs(np.arange(W) - (W // 2 - 0.5)) < R  # columns whose window crosses the edge
    terms = dict(k_normal=2.0, k_albedo=1.92, k_depth=0.25, k_coverage=0.5625)

    def v0(P):
        return host_denoise_spatial(S, 1, feat, 1, dict(DEFAULTS, **P), R)["state"][..., 3]

    def bound(P):
        # a tap across weighs w = 1 / (1 + x); of a window at most R of 2R+1 columns lie across, so their share p of the weight is at
        # most R w / (R w + (R + 1)), and a two-point distribution's variance is p (1 - p) dc^2 <= p dc^2 per channel
        x = sum(dict(DEFAULTS, **P)[k] * t for k, t in terms.items())
        w = 1.0 / (1.0 + x)
        return dc2 * (R * w) / (R * w + R + 1) * (1 + 1e-5) + 1e-7

    full = v0({})
    assert (full[:, ~near] == 0).all(), "pixels whose window stays on their side have no spread at all"
    assert (full <= bound({})).all() and bound({}) < 0.01 * dc2
    for off in terms:
        v = v0({off: 0.0})
        assert (v <= bound({off: 0.0})).all(), (off, float(v.max()), bound({off: 0.0}))
        assert (v[:, ~near] == 0).all() and bound({off: 0.0}) < 0.02 * dc2, off
    open_ = v0(ZERO_K)
    # no stop at all: the pixel beside the edge sees R of 2R+1 columns across: p (1 - p) dc^2 with p = R / (2R + 1)
    p = R / (2.0 * R + 1.0)
    want = p * (1 - p) * dc2
    assert abs(open_[5, W // 2] - want) <= 1e-5 * want and open_[5, W // 2] > 10 * bound({"k_normal": 0.0})
    assert (open_[:, ~near] == 0).all()


def test_moments_source_is_the_existing_twins(built, scenes):
    from cpuraytracer_amd import _capi
    rng = np.random.default_rng(11)
    W, rows, n, m = 37, 19, 4, 3
    S, Q, feat, _, sky = random_strips(rng, W, rows, n, m)
    P = dict(DEFAULTS, levels=2)
    want = host_denoise(S, Q, n, feat, m, P)
    for R in (3, 77):  # (the radius is not read under the moments source)
        got = host_denoise_spatial(S, n, feat, m, P, R, sq=Q, source=MOMENTS)
        assert_same_bits(got["rgb"], want[0], "moments: den")
        assert_same_bits(got["var"], want[1], "moments: den_var")
    got = _capi.unit_denoise_variance_host(S, Q, n, feat, m, params=_capi.denoise_params(**P), variance=None)
    assert_same_bits(got["rgb"], want[0], "NULL vparams: den")
    ids = rng.integers(0, 4, (rows, W)).astype(np.uint32)
    cam0, cam1 = (orbit_scene(scenes, "cover", W, rows, d).camera for d in (0.0, 0.5))
    for fetch in (NEAREST, BILINEAR):
        hist_a = hist_b = None
        for cam in (cam0, cam1):
            a = _capi.unit_temporal_host(S, Q, n, feat, m, ids, W, rows, cam, history=hist_a, fetch=fetch)
            b = host_temporal_spatial(S, n, feat, m, ids, W, rows, cam, 3, hist=hist_b, fetch=fetch, sq=Q, source=MOMENTS)
            assert_same_step(b, a, "moments source, fetch %d" % fetch)
            hist_a, hist_b = history_of(a), history_of(b)


@pytest.fixture(scope="module")
def orbit(oracle, scenes):
    """The CPU oracle's strips along the orbit (computed once, never changed): cover scene, 70 x 41, ONE sample per frame, 0.5 degrees
    per frame, seed 1 + f, three frames."""
    W, H = 70, 41
    out = []
    for f in range(3):
        sc = orbit_scene(scenes, "cover", W, H, 0.5 * f)
        out.append((sc.camera,) + oracle_frame(oracle, sc, W, H, range(H), 1, 50, 1 + f))
    for fr in out:
        for a in fr[1:]:
            a.setflags(write=False)
    return W, H, out


@pytest.mark.parametrize("fetch", [NEAREST, BILINEAR], ids=["nearest", "bilinear"])
def test_twin_equals_numpy_on_the_oracles_orbit(built, orbit, fetch):
    W, H, frames = orbit
    for R in (1, 3):
        hh = hn = None
        for f, (cam, S, _, feat, ids) in enumerate(frames):
            got = host_temporal_spatial(S, 1, feat, 1, ids, W, H, cam, R, hist=hh, fetch=fetch, T=dict(max_history=8))
            want = np_temporal_spatial(S, 1, feat, 1, ids, W, H, cam, R, hist=hn, fetch=fetch, T=dict(max_history=8))
            assert_same_step(got, want, "frame %d, R %d, fetch %d" % (f, R, fetch))
            hh, hn = history_of(got), history_of(want)
        acc = got["target"] != NO_TARGET
        assert acc.mean() > 0.5 and (~acc).any() and got["len"].max() == 3  # the history was used, and the move rejected some pixels
        assert (got["state"][..., 3] > 0).any()


def test_refusals_and_defaults(built):
    from cpuraytracer_amd import _capi
    L = _capi.load()
    d = _capi.RtVarianceParams(9, 9)
    assert L.rt_variance_default_params(C.byref(d)) == 0 and (d.source, d.radius) == (MOMENTS, 1)  # (docs/EXPERIMENTS.md: the grid chose the radius)
    assert L.rt_variance_default_params(None) == RT_ERR_INVALID_ARG
    assert C.sizeof(_capi.RtVarianceParams) == 8
    z = np.zeros(8, F)
    o3, o1, o4 = np.zeros(3, F), np.zeros(1, F), np.zeros(4, F)
    ptr = lambda a: a.ctypes.data if a is not None else None

    def call(V, hdr=z, sq=z, n=2):
        return L.rt_unit_denoise_variance_host(ptr(hdr), ptr(sq), n, ptr(z), 1, 1, 1, None, C.byref(V) if V is not None else None, ptr(o3), ptr(o1), ptr(o4))

    def tcall(V, sq=z, n=2, fetch=NEAREST):
        cam = _capi.RtCamera()
        ids = np.zeros(1, np.uint32)
        return L.rt_unit_temporal_variance_host(ptr(z), ptr(sq), n, ptr(z), 1, ptr(ids), 1, 1, 0, 1, C.byref(cam), None, None, None, None, None, None, None, fetch,
                                                C.byref(V) if V is not None else None, ptr(o3), ptr(o1), ptr(o4), None, None, None)

    for f in (call, tcall):
        assert f(variance_struct(SPATIAL, 3)) == 0 and f(variance_struct(SPATIAL, 1), n=1) == 0
        for radius in (0, 4):
            assert f(variance_struct(SPATIAL, radius)) == RT_ERR_INVALID_ARG, radius
        assert f(variance_struct(2, 3)) == RT_ERR_INVALID_ARG  # an unknown source
        assert L.rt_last_error()
        assert f(variance_struct(MOMENTS, 0)) == 0  # the radius is read only under SPATIAL
        # a null sq is accepted only under SPATIAL
        assert f(variance_struct(SPATIAL, 2), sq=None) == 0
        assert f(variance_struct(MOMENTS, 3), sq=None) == RT_ERR_INVALID_ARG and f(None, sq=None) == RT_ERR_INVALID_ARG
        # n = 0 holds no picture; n = 1 is enough for the spatial source only
        assert f(variance_struct(SPATIAL, 3), n=0) == RT_ERR_SEQUENCE
        assert f(variance_struct(MOMENTS, 3), n=1) == RT_ERR_SEQUENCE and f(None, n=1) == RT_ERR_SEQUENCE
    assert tcall(variance_struct(SPATIAL, 3), fetch=2) == RT_ERR_INVALID_ARG
    # the device entries fail cleanly without a context (no GPU is touched)
    assert L.rt_denoise_variance(None, None, None, None) == RT_ERR_INVALID_ARG
    assert L.rt_denoise_temporal_variance(None, None, None, NEAREST, None, None) == RT_ERR_INVALID_ARG
    with pytest.raises(TypeError):
        _capi.variance_params(window=3)


def test_api_surface(built):
    from cpuraytracer_amd import HipRenderer, _capi
    import inspect
    L = _capi.load()
    assert L.rt_api_version() == 2  # additions only
    for name in ("rt_variance_default_params", "rt_denoise_variance", "rt_denoise_temporal_variance", "rt_unit_denoise_variance_host",
                 "rt_unit_temporal_variance_host"):
        assert hasattr(L, name) and name in _capi.EXPORTS, name
    assert (_capi.RT_VARIANCE_MOMENTS, _capi.RT_VARIANCE_SPATIAL) == (0, 1)
    for name in ("denoise", "denoise_temporal"):
        assert inspect.signature(getattr(HipRenderer, name)).parameters["variance"].default is None


def test_selftest_plain_and_sanitized(built, tmp_path):
    """host/denoise_spatial_selftest.cpp: random strips, radii, ragged shapes and row bands through the twins -- as built with the
    library, and compiled here under ASan + UBSan (a stand-alone program: the buffers end with the strip, sq is a null pointer)."""
    exe = os.path.join(ROOT, "cpuraytracer_amd", "lib", "denoise_spatial_selftest")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "denoise_spatial_selftest ok" in p.stdout, p.stdout + p.stderr
    host = os.path.join(ROOT, "cpuraytracer_amd", "csrc", "host")
    san = str(tmp_path / "denoise_spatial_selftest_san")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fno-fast-math", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                         "-o", san] + [os.path.join(host, f) for f in ("denoise_spatial_selftest.cpp", "rt_temporal_host.cpp", "rt_denoise_host.cpp")],
                        capture_output=True, text=True, timeout=600)
    assert cc.returncode == 0, cc.stderr[-3000:]
    p = subprocess.run([san, "60"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "denoise_spatial_selftest ok" in p.stdout, p.stdout + p.stderr[-3000:]
