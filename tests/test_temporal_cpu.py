"""Temporal accumulation, the part that needs no GPU (csrc/rt_temporal.h, DESIGN.md "Temporal accumulation"): the frame step compiled
for the host (rt_unit_temporal_host, the same source the kernel compiles) against a numpy binary32 restatement of its contract
(tests/temporal_common.py), bit for bit, on synthetic strips and on strips of the CPU oracle along an orbit; the identity, the
validation rules one at a time and at their bounds, the rejections, and the API surface."""
import ctypes as C

import numpy as np
import pytest

from temporal_common import (COVER_PIVOT, F, NO_TARGET, TDEFAULTS, THREE_PIVOT, assert_same_step, history_of, host_temporal, np_reproject, np_temporal,
                             oracle_frame, orbit_scene)
from test_denoise_cpu import DEFAULTS, host_denoise, np_denoise, random_strips
from test_noise_estimate_cpu import assert_same_bits

RT_ERR_INVALID_ARG, RT_ERR_SEQUENCE = 2, 6
BAND = (8, 24)  # first_row, num_rows of the 96 x 64 picture


@pytest.fixture(scope="module")
def scenes(built):
    from cpuraytracer_amd import scenes
    return scenes


@pytest.fixture(scope="module")
def orbit(oracle, scenes):
    """The CPU oracle's strips along the orbit (computed once, never changed): the cover scene, 2 spp per frame, 0.5 degrees per frame,
    seed 1 + f -- four frames at 96 x 64, two at 70 x 41 and over the band of rows; one frame of `three`."""
    out = {}
    for key, W, H, rows, frames in (("96x64", 96, 64, range(64), 4), ("70x41", 70, 41, range(41), 2), ("band", 96, 64, range(BAND[0], BAND[0] + BAND[1]), 2)):
        out[key] = []
        for f in range(frames):
            sc = orbit_scene(scenes, "cover", W, H, 0.5 * f)
            out[key].append((sc.camera,) + oracle_frame(oracle, sc, W, H, rows, 2, 50, 1 + f))
    sc = orbit_scene(scenes, "three", 96, 64, 0.0, THREE_PIVOT)
    out["three"] = [(sc.camera,) + oracle_frame(oracle, sc, 96, 64, range(64), 2, 8, 1)]
    for frames in out.values():
        for fr in frames:
            for a in fr[1:]:
                a.setflags(write=False)
    return out


def run_both(frames, W, H, P=None, T=None, first_row=0):
    """The frames through the twin and through numpy, each on its own history; every step compared."""
    hh = hn = None
    steps = []
    for f, (cam, S, Q, feat, ids) in enumerate(frames):
        got = host_temporal(S, Q, 2, feat, 2, ids, W, H, cam, hh, P, T, first_row)
        want = np_temporal(S, Q, 2, feat, 2, ids, W, H, cam, hn, P, T, first_row)
        assert_same_step(got, want, "frame %d" % f)
        assert_same_bits(got["guides"], want["guides"], "frame %d: guides" % f)
        hh, hn = history_of(got), history_of(want)
        steps.append(got)
    return steps


@pytest.mark.parametrize("levels", [1, 3])
def test_twin_equals_numpy_on_the_oracles_orbit(built, orbit, levels):
    steps = run_both(orbit["96x64"], 96, 64, P=dict(levels=levels), T=dict(max_history=8))
    # not vacuous: the history was used, and the camera move rejected some pixels and shifted others
    last = steps[-1]
    acc = last["target"] != NO_TARGET
    own = np.arange(96 * 64, dtype=np.uint32).reshape(64, 96)
    assert acc.mean() > 0.5 and (~acc).any() and (last["target"][acc] != own[acc]).any()
    assert last["len"].max() == 4 and (last["len"][~acc] == 1).all()


def test_twin_equals_numpy_ragged_and_band(built, orbit):
    run_both(orbit["70x41"], 70, 41)
    steps = run_both(orbit["band"], 96, 64, first_row=BAND[0])
    assert (steps[-1]["target"] != NO_TARGET).mean() > 0.5  # (test_rejections_by_geometry: what the band's first row decides)


@pytest.mark.parametrize("W,rows,first,H", [(37, 19, 0, 19), (70, 41, 0, 41), (96, 24, 8, 64)], ids=["37x19", "70x41", "band"])
def test_twin_equals_numpy_on_synthetic_strips(built, scenes, W, rows, first, H):
    """Seeded, finite strips: histories whose guides are the frame's own, perturbed, with random ids, lengths (0 = holds nothing) and
    states, under the defaults, loose and tight tolerances, with and without ids."""
    rng = np.random.default_rng(1000 * W + rows)
    n, m = 4, 3
    cams = [orbit_scene(scenes, "cover", W, H, d).camera for d in (0.0, 0.5, -2.0)]
    for case, (T, P) in enumerate([({}, {}), (dict(use_id=0, depth_tol=0.5, normal_tol=2.0, coverage_tol=1.0, max_history=3), dict(levels=1)),
                                   (dict(depth_tol=0.0, normal_tol=0.0, coverage_tol=0.0, max_history=64), dict(levels=2)),
                                   (dict(max_history=1), dict(levels=1))]):
        S, Q, feat, kind, sky = random_strips(rng, W, rows, n, m)
        ids = np.where(sky, NO_TARGET, rng.integers(0, 3, (rows, W))).astype(np.uint32)
        g = feat / F(m)
        hg = g.copy()
        some = rng.random((rows, W)) < 0.3
        hg[some, 3:7] = (hg[some, 3:7] * (1.0 + 0.05 * rng.standard_normal((int(some.sum()), 4)))).astype(F)
        hist = dict(camera=cams[0], state=(2.0 * rng.random((rows, W, 4))).astype(F), guides=hg,
                    ids=np.where(rng.random((rows, W)) < 0.8, ids, 7).astype(np.uint32), len=rng.integers(0, 12, (rows, W)).astype(np.uint32))
        accepted = 0
        for cam in cams:
            got = host_temporal(S, Q, n, feat, m, ids, W, H, cam, hist, P, T, first)
            want = np_temporal(S, Q, n, feat, m, ids, W, H, cam, hist, P, T, first)
            assert_same_step(got, want, "%d x %d, case %d" % (W, rows, case))
            assert np.isfinite(got["state"]).all() and (got["len"] >= 1).all() and (got["len"] <= dict(TDEFAULTS, **T)["max_history"]).all()
            accepted += int((got["target"] != NO_TARGET).sum())
        assert accepted > 0 or case == 2, case


@pytest.mark.parametrize("name", ["96x64", "three"])
def test_identity(built, orbit, name):
    """The same camera and the frame's own guides as history: every pixel finds itself, and frame f ends with len == min(f, max_history)."""
    cam, S, Q, feat, ids = orbit[name][0]
    W, H = 96, 64
    own = np.arange(W * H, dtype=np.uint32).reshape(H, W)
    hist = None
    for f in range(1, 11):
        got = host_temporal(S, Q, 2, feat, 2, ids, W, H, cam, hist, dict(levels=1), dict(max_history=8))
        if f == 1:
            assert (got["target"] == NO_TARGET).all()
        else:
            assert np.array_equal(got["target"], own), "frame %d: %d pixels did not find themselves" % (f, int((got["target"] != own).sum()))
        assert (got["len"] == min(f, 8)).all(), f
        hist = history_of(got)
    sky = feat[..., 7] == 0
    assert sky.any() and (~sky).any()


def test_max_history_1_and_empty_history(built, orbit):
    cam0, S0, Q0, feat0, ids0 = orbit["96x64"][0]
    cam1, S1, Q1, feat1, ids1 = orbit["96x64"][1]
    W, H = 96, 64
    first = host_temporal(S0, Q0, 2, feat0, 2, ids0, W, H, cam0)
    # an empty history: the filter alone, in the twin and in numpy
    want = host_denoise(S0, Q0, 2, feat0, 2, DEFAULTS)
    assert_same_bits(first["rgb"], want[0], "empty history: den")
    assert_same_bits(first["var"], want[1], "empty history: den_var")
    ref = np_denoise(S0, Q0, 2, feat0, 2, DEFAULTS)
    mine = np_temporal(S0, Q0, 2, feat0, 2, ids0, W, H, cam0)
    assert_same_bits(mine["rgb"], ref[0], "numpy, empty history: den")
    assert_same_bits(mine["var"], ref[1], "numpy, empty history: den_var")
    assert (first["len"] == 1).all() and (first["target"] == NO_TARGET).all()
    # max_history = 1 never blends: the state is the prepare pass's, whatever is accepted
    plain = host_temporal(S1, Q1, 2, feat1, 2, ids1, W, H, cam1)
    one = host_temporal(S1, Q1, 2, feat1, 2, ids1, W, H, cam1, history_of(first), T=dict(max_history=1))
    assert (one["target"] != NO_TARGET).any() and (one["len"] == 1).all()
    assert_same_bits(one["state"], plain["state"], "max_history = 1: state")
    blended = host_temporal(S1, Q1, 2, feat1, 2, ids1, W, H, cam1, history_of(first))
    assert (blended["state"] != plain["state"]).any() and np.array_equal(blended["target"], one["target"])


def plain_frame(scenes, W=5, rows=3, z=8.0):
    """A strip of hit pixels that all accept their own history: coverage 1, normal (1, 0, 0), depth z, id 4, one feature sample."""
    cam = orbit_scene(scenes, "cover", W, rows, 0.0).camera
    S = np.full((rows, W, 3), 1.0, F)
    Q = np.full((rows, W, 3), 0.75, F)
    feat = np.zeros((rows, W, 8), F)
    feat[..., 0:3] = 0.5
    feat[..., 3] = 1.0
    feat[..., 6] = z
    feat[..., 7] = 1.0
    ids = np.full((rows, W), 4, np.uint32)
    hist = dict(camera=cam, state=np.full((rows, W, 4), 0.25, F), guides=feat.copy(), ids=ids.copy(), len=np.full((rows, W), 3, np.uint32))
    return cam, S, Q, feat, ids, hist


def accepted(cam, S, Q, feat, ids, hist, T=None):
    rows, W = ids.shape
    got = host_temporal(S, Q, 2, feat, 1, ids, W, rows, cam, hist, dict(levels=1), T)
    want = np_temporal(S, Q, 2, feat, 1, ids, W, rows, cam, hist, dict(levels=1), T)
    assert_same_step(got, want, "validation")
    return got["target"] != NO_TARGET, got


def below(x):
    return float(np.nextafter(F(x), F(-1)))


def test_each_validation_rule_alone(built, scenes):
    cam, S, Q, feat, ids, hist = plain_frame(scenes)
    ok, got = accepted(cam, S, Q, feat, ids, hist)
    assert ok.all() and (got["len"] == 2).all()  # (the history's 3, capped by the default max_history = 2)
    assert np.array_equal(got["target"], np.arange(15, dtype=np.uint32).reshape(3, 5))
    p = (1, 2)

    def only(change, T=None):
        h = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in hist.items()}
        change(h)
        ok, got = accepted(cam, S, Q, feat, ids, h, T)
        others = np.ones_like(ok)
        others[p] = False
        assert ok[others].all(), "the other pixels are still accepted"
        assert (got["len"][p] == 2) == bool(ok[p])
        return bool(ok[p])

    def set_at(key, idx, val):
        def change(h):
            h[key][p + idx if idx else p] = val
        return change

    # the history holds nothing there
    assert not only(set_at("len", (), 0))
    # id
    assert not only(set_at("ids", (), 5)) and only(set_at("ids", (), 5), dict(use_id=0))
    # normal: |dn|^2 = 1/16 exactly -- accepted at the bound, rejected one ulp below it
    assert only(set_at("guides", (3,), 0.75), dict(normal_tol=0.0625)) and not only(set_at("guides", (3,), 0.75), dict(normal_tol=below(0.0625)))
    assert not only(set_at("guides", (3,), 0.5))  # (1/4 > the default 0.1)
    # coverage: |dc| = 1/4 exactly (depth sum 6 keeps the history's depth at 8)
    def cover_34(h):
        h["guides"][p + (7,)] = 0.75
        h["guides"][p + (6,)] = 6.0
    assert only(cover_34, dict(coverage_tol=0.25)) and not only(cover_34, dict(coverage_tol=below(0.25)))
    # sky against hit, both ways: a hit pixel on a sky history fails gh[7] > 0 even with every tolerance open
    wide = dict(coverage_tol=2.0, normal_tol=10.0, depth_tol=1e30, use_id=0)
    def sky_hist(h):
        h["guides"][p + (slice(3, 8),)] = 0.0
    assert not only(sky_hist, wide)
    feat_sky = feat.copy()
    feat_sky[p + (slice(3, 8),)] = 0.0
    ok, _ = accepted(cam, S, Q, feat_sky, ids, hist, wide)
    assert not ok[p] and ok.sum() == 14          # a sky pixel on a hit history fails gh[7] == 0
    h2 = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in hist.items()}
    sky_hist(h2)
    ok, _ = accepted(cam, S, Q, feat_sky, ids, h2)
    assert ok.all()                              # sky on sky is accepted under the defaults
    # depth: the smallest depth_tol that accepts, from the restatement's own numbers -- accepted there, rejected one ulp below
    g = feat
    _, _, _, dist, _ = np_reproject(g, 5, 3, 0, 3, cam, cam)
    zh = F(8.5)
    dz = dist[p] - zh
    zm = max(dist[p], zh)
    lhs, zm2 = dz * dz, zm * zm
    lo, hi = 0, int(np.array(1.0, F).view(np.uint32))  # bit patterns of non-negative floats order like the floats
    while lo < hi:
        mid = (lo + hi) // 2
        t = np.array(mid, np.uint32).view(F)
        if lhs <= (t * t) * zm2:
            hi = mid
        else:
            lo = mid + 1
    tol = float(np.array(lo, np.uint32).view(F))
    assert 0.05 < tol < 0.07  # (|8 - 8.5| / 8.5)
    assert only(set_at("guides", (6,), 8.5), dict(depth_tol=tol)) and not only(set_at("guides", (6,), 8.5), dict(depth_tol=below(tol)))
    assert not only(set_at("guides", (6,), 8.5), dict(depth_tol=0.02))


def test_rejections_by_geometry(built, scenes, orbit):
    from cpuraytracer_amd import _capi
    W, H = 96, 64
    cam, S, Q, feat, ids = orbit["96x64"][0]
    first = host_temporal(S, Q, 2, feat, 2, ids, W, H, cam)
    g = first["guides"]
    # the history's camera turned 180 degrees where it stands: everything lies behind it
    back = dict(history_of(first), camera=scenes.orbit_camera(cam, 180.0, tuple(cam.origin[k] for k in range(3))))
    _, _, _, _, why = np_reproject(g, W, H, 0, H, cam, back["camera"])
    assert (why["zw"] <= 0).all()
    got = host_temporal(S, Q, 2, feat, 2, ids, W, H, cam, back)
    assert (got["target"] == NO_TARGET).all() and (got["len"] == 1).all()
    assert_same_bits(got["state"], first["state"], "all rejected: the state is the prepare pass's")
    # a wide turn about the look-at point: targets fall outside the columns on one side
    side = dict(history_of(first), camera=scenes.orbit_camera(cam, 12.0, COVER_PIVOT))
    ok, _, _, _, why = np_reproject(g, W, H, 0, H, cam, side["camera"])
    out_cols = (why["zw"] > 0) & ~((why["fx"] >= 0) & (why["fx"] < W))
    assert out_cols.any() and ok.any()
    got = host_temporal(S, Q, 2, feat, 2, ids, W, H, cam, side, T=dict(use_id=0, depth_tol=1e30, normal_tol=1e30, coverage_tol=2.0))
    want = np_temporal(S, Q, 2, feat, 2, ids, W, H, cam, side, T=dict(use_id=0, depth_tol=1e30, normal_tol=1e30, coverage_tol=2.0))
    assert_same_step(got, want, "wide turn")
    assert (got["target"][out_cols] == NO_TARGET).all() and (got["target"] != NO_TARGET).any()
    # the band: a history camera that stands higher sends targets below the band's last row, inside the picture
    camb, Sb, Qb, featb, idsb = orbit["band"][0]
    firstb = host_temporal(Sb, Qb, 2, featb, 2, idsb, W, H, camb, first_row=BAND[0])
    up = _capi.RtCamera.from_buffer_copy(bytes(camb))
    up.origin[1] += 0.5
    up.origin_image_plane[1] += 0.5
    ok, _, _, _, why = np_reproject(firstb["guides"], W, H, BAND[0], BAND[1], camb, up)
    in_picture = (why["zw"] > 0) & (why["fx"] >= 0) & (why["fx"] < W) & (why["fy"] >= 0) & (why["fy"] < H)
    out_band = in_picture & ~((why["fy"] >= BAND[0]) & (why["fy"] < BAND[0] + BAND[1]))
    assert out_band.any() and ok.any()
    open_T = dict(use_id=0, depth_tol=1e30, normal_tol=1e30, coverage_tol=2.0)
    got = host_temporal(Sb, Qb, 2, featb, 2, idsb, W, H, camb, dict(history_of(firstb), camera=up), T=open_T, first_row=BAND[0])
    want = np_temporal(Sb, Qb, 2, featb, 2, idsb, W, H, camb, dict(history_of(firstb), camera=up), T=open_T, first_row=BAND[0])
    assert_same_step(got, want, "band, camera raised")
    assert (got["target"][out_band] == NO_TARGET).all()
    acc = got["target"] != NO_TARGET
    assert acc.any() and (got["target"][acc] < W * BAND[1]).all()


def test_defaults_and_refusals(built, scenes):
    from cpuraytracer_amd import _capi
    L = _capi.load()
    d = _capi.RtTemporalParams()
    assert L.rt_temporal_default_params(C.byref(d)) == 0
    assert (d.max_history, d.use_id) == (2, 1) and (F(d.depth_tol), F(d.normal_tol), F(d.coverage_tol)) == (F(0.1), F(0.1), F(0.25))
    assert L.rt_temporal_default_params(None) == RT_ERR_INVALID_ARG
    assert C.sizeof(_capi.RtTemporalParams) == 20
    cam, S, Q, feat, ids, hist = plain_frame(scenes)

    def call(T=None, n=2, m=1, W=5, H=3, first=0, rows=3, hist_cam=hist["camera"], hdr=S):
        out = np.zeros((3, 5, 3), F)
        return L.rt_unit_temporal_host(hdr.ctypes.data if hdr is not None else None, Q.ctypes.data, n, feat.ctypes.data, m, ids.ctypes.data, W, H, first,
                                       rows, C.byref(cam), C.byref(hist_cam) if hist_cam is not None else None, hist["state"].ctypes.data,
                                       hist["guides"].ctypes.data, hist["ids"].ctypes.data, hist["len"].ctypes.data, None,
                                       C.byref(T) if T is not None else None, out.ctypes.data, None, None, None, None, None)

    assert call() == 0 and call(d) == 0  # NULL parameters are the defaults; any output may be absent
    for bad in (dict(max_history=0), dict(max_history=65)):
        assert call(_capi.temporal_params(**bad)) == RT_ERR_INVALID_ARG, bad
    assert call(_capi.temporal_params(max_history=1)) == 0 and call(_capi.temporal_params(max_history=64)) == 0
    for name in ("depth_tol", "normal_tol", "coverage_tol"):
        for bad in (-1.0, float("nan"), float("inf"), -float("inf")):
            assert call(_capi.temporal_params(**{name: bad})) == RT_ERR_INVALID_ARG, (name, bad)
        assert call(_capi.temporal_params(**{name: 0.0})) == 0, name
    assert L.rt_last_error()
    assert call(n=1) == RT_ERR_SEQUENCE and call(m=0) == RT_ERR_SEQUENCE
    assert call(W=0) == RT_ERR_INVALID_ARG and call(rows=0) == RT_ERR_INVALID_ARG and call(first=1) == RT_ERR_INVALID_ARG
    assert call(hist_cam=None) == RT_ERR_INVALID_ARG and call(hdr=None) == RT_ERR_INVALID_ARG
    with pytest.raises(TypeError):
        _capi.temporal_params(levels=3)


def test_api_surface(built):
    from cpuraytracer_amd import HipRenderer, _capi
    L = _capi.load()
    assert L.rt_api_version() == 2  # additions only
    for name in ("rt_temporal_default_params", "rt_denoise_temporal", "rt_temporal_reset", "rt_download_temporal", "rt_unit_temporal_host"):
        assert hasattr(L, name) and name in _capi.EXPORTS and getattr(L, name).argtypes is not None, name
    # the device entries fail cleanly on a null context (no GPU is touched)
    assert L.rt_denoise_temporal(None, None, None, None) == RT_ERR_INVALID_ARG
    assert L.rt_temporal_reset(None) == RT_ERR_INVALID_ARG
    assert L.rt_download_temporal(None, None, None, None) == RT_ERR_INVALID_ARG
    for name in ("denoise_temporal", "temporal_reset", "download_temporal"):
        assert callable(getattr(HipRenderer, name))


def test_orbit_camera(built, scenes):
    from cpuraytracer_amd import _capi
    cam = scenes.build_scene("cover", 1, 96, 64).camera
    vec = lambda c, name: np.array([getattr(c, name)[k] for k in range(3)], dtype=np.float64)
    before = bytes(cam)
    full = scenes.orbit_camera(cam, 360.0, COVER_PIVOT)
    assert bytes(cam) == before and isinstance(full, _capi.RtCamera) and full is not cam  # a pure function of the record
    for name in ("origin", "x", "y", "origin_image_plane"):
        # sin(2 pi) in binary64 is 2.4e-16: the turn moves a coordinate by that much of the other, far below half an ulp of binary32
        assert np.abs(vec(full, name) - vec(cam, name)).max() <= 2.0 ** -23 * np.abs(vec(cam, name)).max(), name
    assert (full.aperture, full.focal_length) == (cam.aperture, cam.focal_length)
    assert bytes(scenes.orbit_camera(cam, 0.0, COVER_PIVOT)) == before
    q = scenes.orbit_camera(cam, 90.0, COVER_PIVOT)
    piv = np.array(COVER_PIVOT)
    for name in ("x", "y"):  # vectors keep their lengths: three roundings of 2^-24 relative each
        assert abs(np.linalg.norm(vec(q, name)) - np.linalg.norm(vec(cam, name))) <= 4 * 2.0 ** -24 * np.linalg.norm(vec(cam, name)), name
    for name in ("origin", "origin_image_plane"):  # points keep their distance from the pivot's axis and their height
        a, b = vec(cam, name) - piv, vec(q, name) - piv
        assert abs(np.hypot(a[0], a[2]) - np.hypot(b[0], b[2])) <= 8 * 2.0 ** -24 * np.abs(vec(cam, name)).max() and a[1] == b[1], name
    # a quarter turn: (x, z) -> (z, -x) about the pivot
    a, b = vec(cam, "origin") - piv, vec(q, "origin") - piv
    assert abs(b[0] - a[2]) < 1e-5 and abs(b[2] + a[0]) < 1e-5
    assert q.x[1] == cam.x[1] and q.y[1] == cam.y[1]
