"""The bilinear history fetch of the temporal step, the part that needs no GPU (csrc/rt_temporal.h, DESIGN.md "Temporal accumulation"):
rt_unit_temporal_host_fetch, compiled from the source the kernel compiles, against a numpy binary32 restatement of its contract
(tests/temporal_bilinear_common.py), bit for bit, on the CPU oracle's orbit and on synthetic strips whose histories hold NaN and Inf
wherever a tap must not take part; properties that do not come from the restatement (a constant, a ramp, taps invalidated one at a
time, the strip's borders, a static camera); the refusals, the defaults, the API surface and the stand-alone self-test."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from temporal_bilinear_common import BILINEAR, NEAREST, TDEFAULTS4, host_temporal_fetch, np_taps, np_temporal_bilinear
from temporal_common import F, NO_TARGET, TDEFAULTS, assert_same_step, history_of, np_prepare, np_reproject, oracle_frame, orbit_scene
from test_denoise_cpu import random_strips
from test_noise_estimate_cpu import assert_same_bits
from test_temporal_cpu import BAND, orbit, plain_frame, scenes  # noqa: F401  (orbit, scenes: that file's fixtures, its orbit protocol)

RT_ERR_INVALID_ARG, RT_ERR_SEQUENCE = 2, 6
OPEN = dict(use_id=1, depth_tol=1e30, normal_tol=1e30, coverage_tol=2.0)  # only the id and the length can invalidate a tap


def run_both(frames, W, H, P=None, T=None, first_row=0):
    """The frames through the twin and through numpy with the bilinear fetch, each on its own history; every step compared."""
    hh = hn = None
    steps = []
    for f, (cam, S, Q, feat, ids) in enumerate(frames):
        got = host_temporal_fetch(S, Q, 2, feat, 2, ids, W, H, cam, hh, P, T, first_row)
        want = np_temporal_bilinear(S, Q, 2, feat, 2, ids, W, H, cam, hn, P, T, first_row)
        assert_same_step(got, want, "frame %d" % f)
        assert_same_bits(got["guides"], want["guides"], "frame %d: guides" % f)
        hh, hn = history_of(got), history_of(want)
        steps.append(want)
    return steps


@pytest.mark.parametrize("levels", [1, 3])
def test_twin_equals_numpy_on_the_oracles_orbit(built, orbit, levels):
    steps = run_both(orbit["96x64"], 96, 64, P=dict(levels=levels), T=dict(max_history=8))
    # not vacuous: most pixels are accepted, some are rejected, some are accepted on fewer than four taps, targets moved
    last = steps[-1]
    acc = last["target"] != NO_TARGET
    own = np.arange(96 * 64, dtype=np.uint32).reshape(64, 96)
    assert acc.mean() > 0.5 and (~acc).any() and (last["target"][acc] != own[acc]).any()
    assert np.array_equal(acc, last["taps"] > 0) and (last["taps"][acc] < 4).any() and (last["taps"] == 4).any()
    assert last["len"].max() == 4 and (last["len"][~acc] == 1).all()


def test_twin_equals_numpy_ragged_and_band(built, orbit):
    run_both(orbit["70x41"], 70, 41, T=dict(max_history=8))
    steps = run_both(orbit["band"], 96, 64, T=dict(max_history=8), first_row=BAND[0])
    assert (steps[-1]["target"] != NO_TARGET).mean() > 0.5


def poisoned(hist, used, rng):
    """The history with NaN, +Inf and -Inf in the state of every pixel that no tap that takes part reads."""
    h = dict(hist, state=hist["state"].copy())
    bad = np.array([np.nan, np.inf, -np.inf], F)
    fill = bad[rng.integers(0, 3, h["state"].shape)]
    h["state"][~used] = fill[~used]
    return h


@pytest.mark.parametrize("W,rows,first,H", [(37, 19, 0, 19), (70, 41, 0, 41), (96, 24, 8, 64)], ids=["37x19", "70x41", "band"])
def test_twin_equals_numpy_on_synthetic_strips_with_poisoned_taps(built, scenes, W, rows, first, H):
    """Seeded strips as in tests/test_temporal_cpu.py.  For every camera the restatement says which history pixels some tap that takes
    part reads; every other pixel's state becomes NaN or Inf -- pixels that are tapped but invalid (by id, by length, by a guide) among
    them -- and the twin must give the restatement's bits, all finite: a tap that does not take part is never added."""
    rng = np.random.default_rng(2000 * W + rows)
    n, m = 4, 3
    cams = [orbit_scene(scenes, "cover", W, H, d).camera for d in (0.0, 0.5, -2.0)]
    for case, (T, P) in enumerate([({}, {}), (dict(use_id=0, depth_tol=0.5, normal_tol=2.0, coverage_tol=1.0, max_history=5), dict(levels=1)),
                                   (dict(depth_tol=0.0, normal_tol=0.0, coverage_tol=0.0, max_history=64), dict(levels=2)),
                                   (dict(max_history=1), dict(levels=1))]):
        S, Q, feat, kind, sky = random_strips(rng, W, rows, n, m)
        ids = np.where(sky, NO_TARGET, rng.integers(0, 3, (rows, W))).astype(np.uint32)
        hg = (feat / F(m)).copy()
        some = rng.random((rows, W)) < 0.3
        hg[some, 3:7] = (hg[some, 3:7] * (1.0 + 0.05 * rng.standard_normal((int(some.sum()), 4)))).astype(F)
        hist = dict(camera=cams[0], state=(2.0 * rng.random((rows, W, 4))).astype(F), guides=hg,
                    ids=np.where(rng.random((rows, W)) < 0.8, ids, 7).astype(np.uint32), len=rng.integers(0, 12, (rows, W)).astype(np.uint32))
        accepted = tapped_invalid_by_id = tapped_outside = 0
        for cam in cams:
            clean = np_temporal_bilinear(S, Q, n, feat, m, ids, W, H, cam, hist, P, T, first, levels=False)
            used = np.zeros(rows * W, bool)
            used[clean["q"][clean["take"]]] = True
            h = poisoned(hist, used.reshape(rows, W), rng)
            ok, dist, inside, ql, qx, w = np_taps(clean["guides"], W, H, first, rows, cam, hist["camera"])
            tapped = np.zeros(rows * W, bool)
            tapped[(ql * W + qx)[inside & (w > 0)]] = True
            wrong_id = (hist["ids"][ql, qx] != ids[None]) & inside & (w > 0)
            tapped_invalid_by_id += int((wrong_id & ~used[ql * W + qx]).sum()) if dict(TDEFAULTS4, **T)["use_id"] else 0
            tapped_outside += int((ok[None] & ~inside).sum())
            assert (tapped & ~used).any(), "no pixel is tapped without taking part: nothing is poisoned where it matters"
            got = host_temporal_fetch(S, Q, n, feat, m, ids, W, H, cam, h, P, T, first)
            want = np_temporal_bilinear(S, Q, n, feat, m, ids, W, H, cam, h, P, T, first)
            assert_same_step(got, want, "%d x %d, case %d" % (W, rows, case))
            assert_same_bits(want["state"], clean["state"], "the poison reaches the restatement")
            assert np.isfinite(got["state"]).all() and np.isfinite(got["rgb"]).all() and np.isfinite(got["var"]).all()
            assert (got["len"] >= 1).all() and (got["len"] <= dict(TDEFAULTS4, **T)["max_history"]).all()
            accepted += int((got["target"] != NO_TARGET).sum())
        assert accepted > 0 or case == 2, case
        assert tapped_outside > 0 and (tapped_invalid_by_id > 0 or not dict(TDEFAULTS4, **T)["use_id"]), case


def axis_camera():
    """Looks down -z from the origin with x = (1, 0, 0) and y = (0, 1/2, 0): every product of the reprojection of a sky pixel is exact in y."""
    from cpuraytracer_amd import _capi
    c = _capi.RtCamera()
    for k, (o, x, y, p) in enumerate(zip((0, 0, 0), (1, 0, 0), (0, 0.5, 0), (0, 0, -1))):
        c.origin[k], c.x[k], c.y[k], c.origin_image_plane[k] = o, x, y, p
    return c


def test_taps_of_weight_zero_are_never_added(built):
    """The band of a 96 x 64 picture under one axis-aligned camera: a sky pixel of row y reprojects to fy = y + 0.5 exactly, so ry = 0.5,
    ty = 0 and the two taps of row y + 1 weigh exactly 0.  The even local rows are sky, the odd ones hit pixels that no history accepts
    (the history is all sky), so the history's odd rows are read only by taps of weight 0 -- and hold NaN and Inf."""
    W, H, first, rows = 96, 64, BAND[0], BAND[1]
    cam = axis_camera()
    rng = np.random.default_rng(7)
    S = (rng.random((rows, W, 3)) * 2).astype(F)
    Q = (S * S * F(0.7)).astype(F)
    feat = np.zeros((rows, W, 8), F)
    feat[..., 0:3] = 0.5
    odd = (np.arange(rows) % 2 == 1)
    feat[odd, 3], feat[odd, 6], feat[odd, 7] = 1.0, 9.0, 1.0
    ids = np.where(odd[:, None], 3, NO_TARGET).astype(np.uint32) * np.ones((1, W), np.uint32)
    hguides = np.zeros((rows, W, 8), F)
    hguides[..., 0:3] = 0.25
    state = (rng.random((rows, W, 4)) + 0.5).astype(F)
    state[odd] = np.array([np.nan, np.inf, -np.inf, np.nan], F)
    hist = dict(camera=cam, state=state, guides=hguides, ids=np.full((rows, W), NO_TARGET, np.uint32), len=np.full((rows, W), 2, np.uint32))
    ok, dist, inside, ql, qx, w = np_taps(feat, W, H, first, rows, cam, cam)
    even = ~odd
    assert ok[even].all() and (w[2][even] == 0).all() and (w[3][even] == 0).all() and (w[0][even] + w[1][even] > 0).all()
    assert inside[2][even][:-1].all(), "the taps of weight 0 lie inside the strip: only their weight keeps them out"
    got = host_temporal_fetch(S, Q, 2, feat, 1, ids, W, H, cam, hist, dict(levels=1), dict(max_history=8))
    want = np_temporal_bilinear(S, Q, 2, feat, 1, ids, W, H, cam, hist, dict(levels=1), dict(max_history=8))
    assert_same_step(got, want, "weight 0")
    assert np.isfinite(got["state"]).all() and np.isfinite(got["rgb"]).all()
    assert (got["target"][even] != NO_TARGET).all() and (got["len"][even] == 3).all() and (got["target"][odd] == NO_TARGET).all()
    assert ((got["target"][even] // W) % 2 == 0).all(), "every target is a row of its own parity"


def old_entry(S, Q, n, feat, m, ids, W, H, cam, hist, P, T, first_row=0):
    """rt_unit_temporal_host itself (cpuraytracer_amd._capi.unit_temporal_host goes through the entry with a fetch)."""
    from cpuraytracer_amd import _capi
    L = _capi.load()
    rows = ids.shape[0]
    S, Q, feat = (np.ascontiguousarray(a, F) for a in (S, Q, feat))
    ids = np.ascontiguousarray(ids, np.uint32)
    out = {"rgb": np.zeros((rows, W, 3), F), "var": np.zeros((rows, W), F), "state": np.zeros((rows, W, 4), F), "guides": np.zeros((rows, W, 8), F),
           "len": np.zeros((rows, W), np.uint32), "target": np.zeros((rows, W), np.uint32)}
    keep = [np.ascontiguousarray(hist["state"], F), np.ascontiguousarray(hist["guides"], F), np.ascontiguousarray(hist["ids"], np.uint32),
            np.ascontiguousarray(hist["len"], np.uint32)]
    c, hc = _capi.RtCamera.from_buffer_copy(bytes(cam)), _capi.RtCamera.from_buffer_copy(bytes(hist["camera"]))
    ps, ts = _capi.denoise_params(**P), _capi.temporal_params(**T)
    _capi.check(L.rt_unit_temporal_host(S.ctypes.data, Q.ctypes.data, n, feat.ctypes.data, m, ids.ctypes.data, W, H, first_row, rows, C.byref(c), C.byref(hc),
                                        keep[0].ctypes.data, keep[1].ctypes.data, keep[2].ctypes.data, keep[3].ctypes.data, C.byref(ps), C.byref(ts),
                                        out["rgb"].ctypes.data, out["var"].ctypes.data, out["state"].ctypes.data, out["guides"].ctypes.data,
                                        out["len"].ctypes.data, out["target"].ctypes.data))
    return out


def test_fetch_nearest_is_the_old_entry(built, orbit):
    for key, W, H, first in (("96x64", 96, 64, 0), ("band", 96, 64, BAND[0])):
        cam0, S0, Q0, feat0, ids0 = orbit[key][0]
        cam1, S1, Q1, feat1, ids1 = orbit[key][1]
        hist = history_of(host_temporal_fetch(S0, Q0, 2, feat0, 2, ids0, W, H, cam0, None, first_row=first))
        P, T = dict(levels=2), dict(max_history=8)
        got = host_temporal_fetch(S1, Q1, 2, feat1, 2, ids1, W, H, cam1, hist, P, T, first, fetch=NEAREST)
        want = old_entry(S1, Q1, 2, feat1, 2, ids1, W, H, cam1, hist, P, T, first)
        assert_same_step(got, want, key)
        assert_same_bits(got["guides"], want["guides"], key + ": guides")
        other = host_temporal_fetch(S1, Q1, 2, feat1, 2, ids1, W, H, cam1, hist, P, T, first, fetch=BILINEAR)
        assert (other["state"] != got["state"]).any()


def black_frame(scenes, W, rows, deg, z=8.0):
    """plain_frame's guides under a turned camera, with hdr = sq = 0: c = 0 and v = 0, so with a history of len 1 the blended state is
    exactly half the fetched colour and a quarter of the fetched variance (a = b = 1/2)."""
    cam0, S, Q, feat, ids, hist = plain_frame(scenes, W, rows, z)
    cam = orbit_scene(scenes, "cover", W, rows, deg).camera
    hist = dict(hist, len=np.ones((rows, W), np.uint32))
    return cam, np.zeros_like(S), np.zeros_like(Q), feat, ids, hist


def fetched(got):
    """(ch, vh) of the accepted pixels of a black_frame step."""
    return got["state"][..., 0:3].astype(np.float64) * 2.0, got["state"][..., 3].astype(np.float64) * 4.0


def taps64(feat, W, H, first, rows, cam, hist, T):
    """Every tap's take, index and weight from the restatement's geometry, for reference values computed in binary64."""
    out = np_temporal_bilinear(np.zeros((rows, W, 3), F), np.zeros((rows, W, 3), F), 2, feat, 1, hist["ids"], W, H, cam, hist, None, T, first, levels=False)
    _, _, _, _, _, w = np_taps(out["guides"], W, H, first, rows, cam, hist["camera"])
    return out, w.astype(np.float64)


def test_constant_history(built, scenes):
    W, rows = 37, 19
    cam, S, Q, feat, ids, hist = black_frame(scenes, W, rows, 0.5)
    const = np.array([0.3, 1.7, 2.5, 0.9], F)
    hist = dict(hist, state=np.broadcast_to(const, (rows, W, 4)).copy())
    got = host_temporal_fetch(S, Q, 2, feat, 1, ids, W, rows, cam, hist, dict(levels=1), OPEN)
    acc = got["target"] != NO_TARGET
    assert acc.mean() > 0.8 and (got["len"][acc] == 2).all()
    ch, vh = fetched(got)
    ulp = np.spacing(const[0:3]).astype(np.float64)
    assert (np.abs(ch[acc] - const[0:3].astype(np.float64)) <= 2 * ulp).all()
    ref, w = taps64(feat, W, rows, 0, rows, cam, hist, OPEN)
    sw, sww = (w * ref["take"]).sum(0), (w * w * ref["take"]).sum(0)
    want = float(const[3]) * sww[acc] / sw[acc] ** 2
    assert np.allclose(vh[acc], want, rtol=1e-5, atol=0) and (vh[acc] <= float(const[3]) * (1 + 1e-6)).all()
    assert (vh[acc] < 0.9 * float(const[3])).any(), "interpolating between pixels lowers the variance somewhere"


def ramp_history(hist, W, rows, first=0):
    y, x = np.mgrid[0:rows, 0:W]
    y = y + first
    state = np.stack([0.5 + 0.25 * x + 0.125 * y, 3.0 - 0.0625 * x + 0.5 * y, 1.0 + 0.03125 * x, np.full(x.shape, 0.5)], axis=-1).astype(F)
    return dict(hist, state=state), lambda fx, fy: np.stack([0.5 + 0.25 * fx + 0.125 * fy, 3.0 - 0.0625 * fx + 0.5 * fy, 1.0 + 0.03125 * fx], axis=-1)


@pytest.mark.parametrize("W,rows,first,H", [(37, 19, 0, 19), (96, 24, 8, 64)], ids=["37x19", "band"])
def test_ramp_history(built, scenes, W, rows, first, H):
    """A colour that is linear in x and y comes back as its value at the reprojected point, (fx - 0.5, fy - 0.5) in pixel-centre
    coordinates, wherever all four taps take part; with fewer (the strip's borders) as the mean of those that do, renormalised."""
    cam0, S, Q, feat, ids, hist = plain_frame(scenes, W, rows)
    cam0 = orbit_scene(scenes, "cover", W, H, 0.0).camera
    cam = orbit_scene(scenes, "cover", W, H, 0.7).camera
    hist = dict(hist, camera=cam0, len=np.ones((rows, W), np.uint32))
    S, Q = np.zeros_like(S), np.zeros_like(Q)
    hist, ramp = ramp_history(hist, W, rows, first)
    got = host_temporal_fetch(S, Q, 2, feat, 1, ids, W, H, cam, hist, dict(levels=1), OPEN, first)
    ref, w = taps64(feat, W, H, first, rows, cam, hist, OPEN)
    assert np.array_equal(got["target"], ref["target"])
    ch, _ = fetched(got)
    _, _, _, _, why = np_reproject(ref["guides"], W, H, first, rows, cam, cam0)
    four = ref["taps"] == 4
    assert four.mean() > 0.5
    want = ramp(why["fx"].astype(np.float64) - 0.5, why["fy"].astype(np.float64) - 0.5)
    assert np.allclose(ch[four], want[four], rtol=1e-5, atol=0)
    # fewer than four: the strip's borders.  A clamped tap would pull the colour towards the border pixel; a skipped one renormalises.
    part = (ref["taps"] > 0) & (ref["taps"] < 4)
    assert part.any()
    flat = hist["state"].reshape(-1, 4)[..., 0:3].astype(np.float64)
    with np.errstate(invalid="ignore"):  # (0 / 0 where no tap takes part)
        mean = (w[..., None] * ref["take"][..., None] * flat[ref["q"]]).sum(0) / (w * ref["take"]).sum(0)[..., None]
    assert np.allclose(ch[part], mean[part], rtol=1e-5, atol=0)
    ys, xs = np.nonzero(part)
    assert ((xs == 0) | (xs == W - 1) | (ys == 0) | (ys == rows - 1)).any(), "border pixels lose taps here"  # (others: a weight of exactly 0)
    assert (got["target"][part] < W * rows).all()


def test_each_tap_invalidated_alone_and_all_four(built, scenes):
    W, rows = 9, 7
    cam, S, Q, feat, ids, hist = black_frame(scenes, W, rows, 0.7)
    hist, _ = ramp_history(hist, W, rows)
    ref, w = taps64(feat, W, rows, 0, rows, cam, hist, OPEN)
    p = (3, 4)
    assert ref["taps"][p] == 4 and (w[:, p[0], p[1]] > 0).all()
    q = ref["q"][:, p[0], p[1]]
    wp = w[:, p[0], p[1]]
    flat = hist["state"].reshape(-1, 4)[..., 0:3].astype(np.float64)
    order = [int(q[k]) for k in sorted(range(4), key=lambda k: (-wp[k], k))]

    def step(bad):
        h = dict(hist, ids=hist["ids"].copy())
        h["ids"].reshape(-1)[q[list(bad)]] = 5
        got = host_temporal_fetch(S, Q, 2, feat, 1, ids, W, rows, cam, h, dict(levels=1), OPEN)
        want = np_temporal_bilinear(S, Q, 2, feat, 1, ids, W, rows, cam, h, dict(levels=1), OPEN)
        assert_same_step(got, want, "taps %s invalid" % (bad,))
        return got, want

    for k in range(4):
        got, want = step((k,))
        assert want["taps"][p] == 3 and got["len"][p] == 2
        rest = [j for j in range(4) if j != k]
        mean = (wp[rest, None] * flat[q[rest]]).sum(0) / wp[rest].sum()
        assert np.allclose(fetched(got)[0][p], mean, rtol=1e-5, atol=0), k
        assert got["target"][p] == [t for t in order if t != q[k]][0], "the greatest of the taps that are left"
        # with the id not looked at the tap is back
        T0 = dict(OPEN, use_id=0)
        h = dict(hist, ids=hist["ids"].copy())
        h["ids"].reshape(-1)[q[k]] = 5
        assert np_temporal_bilinear(S, Q, 2, feat, 1, ids, W, rows, cam, h, dict(levels=1), T0)["taps"][p] == 4
        assert host_temporal_fetch(S, Q, 2, feat, 1, ids, W, rows, cam, h, dict(levels=1), T0)["target"][p] == order[0]
    got, want = step((0, 1, 2, 3))
    assert want["taps"][p] == 0 and got["len"][p] == 1 and got["target"][p] == NO_TARGET
    assert (got["state"][p] == 0).all(), "rejected: the prepare pass's state"
    others = np.ones((rows, W), bool)
    others[p] = False
    for yy, xx in zip(*np.nonzero(others)):
        if not np.isin(ref["q"][:, yy, xx][ref["take"][:, yy, xx]], q).any():
            assert got["target"][yy, xx] == ref["target"][yy, xx]


def test_strip_borders(built, scenes, orbit):
    """First and last column and row, and the band's first row: a tap at x0 = -1, at column W or in a row outside the strip is skipped."""
    for key, W, H, first in (("96x64", 96, 64, 0), ("band", 96, 64, BAND[0])):
        cam0, S0, Q0, feat0, ids0 = orbit[key][0]
        rows = ids0.shape[0]
        _, _, g = np_prepare(S0, Q0, 2, feat0, 2)
        from cpuraytracer_amd import _capi
        seen = set()
        for dx, dy in ((0.02, 0.01), (-0.02, -0.01)):
            moved = _capi.RtCamera.from_buffer_copy(bytes(cam0))
            for k, d in ((0, dx), (1, dy)):
                moved.origin[k] += d
                moved.origin_image_plane[k] += d
            ok, dist, inside, ql, qx, w = np_taps(g, W, H, first, rows, cam0, moved)
            lost = ok[None] & ~inside
            if lost[:, :, 0].any():
                seen.add("first column")
            if lost[:, :, W - 1].any():
                seen.add("last column")
            if lost[:, 0, :].any():
                seen.add("first row")
            if lost[:, rows - 1, :].any():
                seen.add("last row")
            hist = dict(history_of(host_temporal_fetch(S0, Q0, 2, feat0, 2, ids0, W, H, cam0, None, first_row=first)), camera=moved)
            T = dict(OPEN, use_id=0, max_history=8)
            got = host_temporal_fetch(S0, Q0, 2, feat0, 2, ids0, W, H, cam0, hist, dict(levels=1), T, first)
            want = np_temporal_bilinear(S0, Q0, 2, feat0, 2, ids0, W, H, cam0, hist, dict(levels=1), T, first)
            assert_same_step(got, want, key)
            acc = got["target"] != NO_TARGET
            assert (got["target"][acc] < W * rows).all()
            edge = lost.any(0) & acc
            assert edge.any() and (want["taps"][edge] < 4).all()
        assert seen == {"first column", "last column", "first row", "last row"}, (key, seen)


def test_static_camera_ten_seeds(built, oracle, scenes):
    """One camera, seeds 1..10 from the CPU oracle: the guides do not depend on the seed, so every pixel's greatest tap is itself and
    the history fills up to max_history."""
    W, H = 48, 32
    sc = orbit_scene(scenes, "cover", W, H, 0.0)
    own = np.arange(W * H, dtype=np.uint32).reshape(H, W)
    hist = None
    for f in range(1, 11):
        S, Q, feat, ids = oracle_frame(oracle, sc, W, H, range(H), 2, 50, f)
        got = host_temporal_fetch(S, Q, 2, feat, 2, ids, W, H, sc.camera, hist, dict(levels=1), dict(max_history=8))
        if f == 1:
            assert (got["target"] == NO_TARGET).all()
        else:
            assert np.array_equal(got["target"], own), "frame %d: %d pixels did not find themselves" % (f, int((got["target"] != own).sum()))
        assert (got["len"] == min(f, 8)).all(), f
        hist = history_of(got)


def test_defaults_and_refusals(built, scenes):
    from cpuraytracer_amd import _capi
    L = _capi.load()
    d1, d4, d = _capi.RtTemporalParams(), _capi.RtTemporalParams(), _capi.RtTemporalParams()
    assert L.rt_temporal_default_params(C.byref(d)) == 0
    assert L.rt_temporal_default_params_fetch(NEAREST, C.byref(d1)) == 0 and bytes(d1) == bytes(d)
    assert L.rt_temporal_default_params_fetch(BILINEAR, C.byref(d4)) == 0
    assert (d4.max_history, d4.use_id) == (3, 1) and (F(d4.depth_tol), F(d4.normal_tol), F(d4.coverage_tol)) == (F(0.1), F(0.1), F(0.25))
    assert {k: getattr(d4, k) for k in ("max_history", "use_id")} == {k: TDEFAULTS4[k] for k in ("max_history", "use_id")} and TDEFAULTS["max_history"] == 2
    for bad in (0, 2, 3, 5, 0xFFFFFFFF):
        assert L.rt_temporal_default_params_fetch(bad, C.byref(d)) == RT_ERR_INVALID_ARG, bad
    assert L.rt_temporal_default_params_fetch(BILINEAR, None) == RT_ERR_INVALID_ARG
    cam, S, Q, feat, ids, hist = plain_frame(scenes)

    def call(T=None, fetch=BILINEAR, n=2, m=1, W=5, H=3, first=0, rows=3, hist_cam=hist["camera"], hdr=S):
        out = np.zeros((3, 5, 3), F)
        return L.rt_unit_temporal_host_fetch(hdr.ctypes.data if hdr is not None else None, Q.ctypes.data, n, feat.ctypes.data, m, ids.ctypes.data, W, H,
                                             first, rows, C.byref(cam), C.byref(hist_cam) if hist_cam is not None else None, hist["state"].ctypes.data,
                                             hist["guides"].ctypes.data, hist["ids"].ctypes.data, hist["len"].ctypes.data, None,
                                             C.byref(T) if T is not None else None, fetch, out.ctypes.data, None, None, None, None, None)

    assert call() == 0 and call(d4) == 0 and call(fetch=NEAREST) == 0  # NULL parameters are that fetch's defaults; any output may be absent
    for bad in (0, 2, 5):
        assert call(fetch=bad) == RT_ERR_INVALID_ARG, bad
        assert b"fetch" in L.rt_last_error()
    for bad in (dict(max_history=0), dict(max_history=65)):
        assert call(_capi.temporal_params_fetch(BILINEAR, **bad)) == RT_ERR_INVALID_ARG, bad
    assert call(_capi.temporal_params_fetch(BILINEAR, max_history=1)) == 0 and call(_capi.temporal_params_fetch(BILINEAR, max_history=64)) == 0
    for name in ("depth_tol", "normal_tol", "coverage_tol"):
        for bad in (-1.0, float("nan"), float("inf"), -float("inf")):
            assert call(_capi.temporal_params_fetch(BILINEAR, **{name: bad})) == RT_ERR_INVALID_ARG, (name, bad)
        assert call(_capi.temporal_params_fetch(BILINEAR, **{name: 0.0})) == 0, name
    assert call(n=1) == RT_ERR_SEQUENCE and call(m=0) == RT_ERR_SEQUENCE
    assert call(W=0) == RT_ERR_INVALID_ARG and call(rows=0) == RT_ERR_INVALID_ARG and call(first=1) == RT_ERR_INVALID_ARG
    assert call(hist_cam=None) == RT_ERR_INVALID_ARG and call(hdr=None) == RT_ERR_INVALID_ARG
    # the 2^24 limit on a side, refused before anything is read
    big = (1 << 24) + 1
    assert call(W=big, H=1, rows=1) == RT_ERR_INVALID_ARG and call(W=1, H=big, first=0, rows=1) == RT_ERR_INVALID_ARG
    with pytest.raises(TypeError):
        _capi.temporal_params_fetch(BILINEAR, levels=3)
    with pytest.raises(_capi.RtError):
        _capi.temporal_params_fetch(2)
    # the default of fetch 4 is what the twin uses when tparams is NULL
    cam, S, Q, feat, ids, hist = plain_frame(scenes)
    got = _capi.unit_temporal_host(S, Q, 2, feat, 1, ids, 5, 3, cam, history=hist, fetch=BILINEAR)
    assert (got["len"] == 3).all()  # (the history's 3, capped by max_history = 3 to 2, plus one)
    assert (_capi.unit_temporal_host(S, Q, 2, feat, 1, ids, 5, 3, cam, history=hist)["len"] == 2).all()  # fetch 1: max_history = 2


def test_api_surface(built):
    from cpuraytracer_amd import HipRenderer, _capi
    L = _capi.load()
    assert L.rt_api_version() == 2  # additions only
    header = open(os.path.join(ROOT, "include", "rt_api.h")).read()
    for name in ("rt_temporal_default_params_fetch", "rt_denoise_temporal_fetch", "rt_unit_temporal_host_fetch"):
        assert hasattr(L, name) and name in _capi.EXPORTS and getattr(L, name).argtypes is not None and (" " + name + "(") in header, name
    assert "RT_TEMPORAL_FETCH_NEAREST = 1" in header and "RT_TEMPORAL_FETCH_BILINEAR = 4" in header
    assert (_capi.RT_TEMPORAL_FETCH_NEAREST, _capi.RT_TEMPORAL_FETCH_BILINEAR) == (1, 4)
    # the device entry fails cleanly on a null context, whatever the fetch (no GPU is touched)
    for fetch in (1, 4, 2):
        assert L.rt_denoise_temporal_fetch(None, None, None, fetch, None) == RT_ERR_INVALID_ARG
    assert inspect.signature(HipRenderer.denoise_temporal).parameters["fetch"].default == 1
    assert inspect.signature(_capi.unit_temporal_host).parameters["fetch"].default == 1
    assert callable(_capi.temporal_params_fetch)


def test_standalone_selftest(built):
    """host/temporal_bilinear_selftest.cpp: random strips, histories and cameras; the taps formed a second time."""
    exe = os.path.join(ROOT, "cpuraytracer_amd", "lib", "temporal_bilinear_selftest")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "temporal_bilinear_selftest ok: 400 cases" in p.stdout
