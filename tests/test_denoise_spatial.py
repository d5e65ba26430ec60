"""The spatial variance source on the device (rt_denoise_variance, rt_denoise_temporal_variance; csrc/rt_denoise.hip
rt_denoise_prepare_spatial_kernel): the kernels against the host twins compiled from the same source (which
tests/test_denoise_spatial_cpu.py pins to a numpy restatement), bit for bit, on strips the device itself rendered at ONE sample per pixel
with the noise estimate off; that the moments source is the existing entries; that pipelined frames stay in flight; that nothing else
in the context changes; alternation over one history; the refusals; what the chain buys against a 1024-spp picture; the Python views,
the device copy and the CLI."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from denoise_spatial_common import (BILINEAR, MOMENTS, NEAREST, QUALITY, SPATIAL, host_denoise_spatial, host_temporal_spatial, mse, rel_mse,
                                    variance_struct)
from temporal_common import NO_TARGET, history_of, orbit_scene
from test_denoise_cpu import DEFAULTS, params_struct
from test_noise_estimate_cpu import assert_same_bits

pytestmark = pytest.mark.gpu

RT_ERR_INVALID_ARG, RT_ERR_SEQUENCE = 2, 6
CLI = os.path.join(ROOT, "cpuraytracer_amd", "lib", "spheres")
DIRECT, STAGED = 1, 2
BAND = (8, 24, 24, 0, 1)  # rows 8..31 of the 96 x 64 picture as one contiguous row set


@pytest.fixture(scope="module")
def scenes(built):
    from cpuraytracer_amd import scenes
    return scenes


@pytest.fixture()
def dr(built):
    """A context of its own: the history and the switches these tests flip never reach the session's renderer."""
    from cpuraytracer_amd import HipRenderer
    r = HipRenderer(0)
    yield r
    r.close()


def rowset_of(rs):
    from cpuraytracer_amd import _capi
    return _capi.RtRowset(*rs) if rs else None


def render_frame(r, scenes, W, H, f, rs=None, deg=0.5, n=1, m=1, seed=None, noise=False):
    """Frame f of the orbit: the camera turned deg * f degrees, an upload, samples 1..n with seed 1 + f, features after m samples."""
    sc = orbit_scene(scenes, "cover", W, H, deg * f)
    r.upload(sc)
    r.set_noise_estimate(noise)
    r.render(W, H, 1, 1 + n, 50, (1 + f) if seed is None else seed, rowset=rowset_of(rs))
    r.render_features(W, H, 1, 1 + m, rowset=rowset_of(rs))
    return sc.camera


def strips(r, moments=False):
    """What the spatial source reads, as the device holds it: hdr [rows, W, 3], feat [rows, W, 8], ids [rows, W] (and sq on request)."""
    hdr, _ = r.download(ldr=False)
    d = r.download_features()
    feat = np.ascontiguousarray(np.concatenate([d["albedo"], d["normal"], d["depth"][..., None], d["coverage"][..., None]], axis=-1))
    return (hdr, feat, d["id"]) + ((r.download_moments(),) if moments else ())


def device_step(r, V, P=None, fetch=NEAREST, T=None):
    from cpuraytracer_amd import _capi
    r.denoise_temporal(params_struct(dict(DEFAULTS, **P)) if P else None, _capi.temporal_params_fetch(fetch, **T) if T else None, fetch=fetch, variance=V)
    d, t = r.download_denoised(), r.download_temporal()
    return dict(rgb=d["rgb"], var=d["var"], ldr=d["ldr"], **t)


def same_step(got, want, what):
    assert_same_bits(got["rgb"], want["rgb"], what + ": den")
    assert_same_bits(got["var"], want["var"], what + ": den_var")
    assert_same_bits(got["state"], want["state"], what + ": state")
    assert np.array_equal(got["len"], want["len"]), what + ": len"
    assert np.array_equal(got["target"], want["target"]), what + ": target"


def forms_for(levels, knob):
    return [STAGED if (knob == "1" and (1 << l) <= 4) else DIRECT for l in range(levels)] + [0] * (5 - levels)


@pytest.mark.parametrize("R", [1, 2, 3])
def test_device_equals_host_twin(dr, scenes, monkeypatch, R):
    """Cover scene, 96 x 64, ONE sample, the noise estimate off, features after 2 samples (m != n): rt_denoise_variance for 1, 3 and 5
    levels under both RT_DENOISE_STAGE values, and the prepared (c0, v0) itself -- read back as the history that
    rt_denoise_temporal_variance leaves on an empty one, for both fetches."""
    W, H = 96, 64
    render_frame(dr, scenes, W, H, 0, n=1, m=2)
    S, feat, ids = strips(dr)
    V = variance_struct(SPATIAL, R)
    cam = orbit_scene(scenes, "cover", W, H, 0.0).camera
    for levels in (1, 3, 5):
        P = dict(DEFAULTS, levels=levels)
        want = host_denoise_spatial(S, 1, feat, 2, P, R)
        for knob in ("0", "1"):
            monkeypatch.setenv("RT_DENOISE_STAGE", knob)
            ms = dr.denoise(params_struct(P), timed=(levels == 3), variance=V)
            assert (ms is not None and ms > 0.0) if levels == 3 else ms is None
            assert dr.denoise_forms() == forms_for(levels, knob)
            d = dr.download_denoised()
            what = "R %d, %d levels, stage %s" % (R, levels, knob)
            assert_same_bits(d["rgb"], want["rgb"], what + ": den")
            assert_same_bits(d["var"], want["var"], what + ": den_var")
            for fetch in (NEAREST, BILINEAR):
                dr.temporal_reset()
                got = device_step(dr, V, P, fetch)
                assert_same_bits(got["state"], want["state"], what + ", fetch %d: prepared state" % fetch)
                assert_same_bits(got["rgb"], want["rgb"], what + ", fetch %d: den on an empty history" % fetch)
                assert (got["len"] == 1).all() and (got["target"] == NO_TARGET).all()
    # not vacuous: the picture has spread, the filter moved it, and the radius matters
    assert (want["state"][..., 3] > 0).any() and (want["rgb"] != S).any()
    other = host_denoise_spatial(S, 1, feat, 2, P, R % 3 + 1)
    assert (other["state"][..., 3] != want["state"][..., 3]).any()


SHAPES = {"70x41": (70, 41, None), "5x3": (5, 3, None), "band": (96, 64, BAND)}


@pytest.mark.parametrize("fetch", [NEAREST, BILINEAR], ids=["nearest", "bilinear"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_ragged_shapes_and_band_along_the_orbit(dr, scenes, monkeypatch, shape, fetch):
    """Partial tiles in both directions around whole ones; less than one tile and less than one window; a band of rows of a taller image.
    Two frames of the orbit at one sample each, every radius, the second frame on the history the first left."""
    W, H, rs = SHAPES[shape]
    first_row = rs[0] if rs else 0
    T = dict(max_history=8)
    for R in (1, 2, 3):
        monkeypatch.setenv("RT_DENOISE_STAGE", str(R % 2))
        V = variance_struct(SPATIAL, R)
        P = dict(levels=2 + R)
        dr.temporal_reset()
        hist = None
        for f in range(2):
            cam = render_frame(dr, scenes, W, H, f, rs, n=1, m=1)
            S, feat, ids = strips(dr)
            got = device_step(dr, V, P, fetch, T)
            want = host_temporal_spatial(S, 1, feat, 1, ids, W, H, cam, R, hist=hist, P=P, T=T, first_row=first_row, fetch=fetch)
            same_step(got, want, "%s, R %d, fetch %d, frame %d" % (shape, R, fetch, f))
            hist = history_of(want)
        if W * H > 100:
            assert (got["target"] != NO_TARGET).mean() > 0.5 and got["len"].max() == 2  # the history was used


def test_moments_source_is_the_existing_entries(dr, scenes):
    """source = RT_VARIANCE_MOMENTS: rt_denoise's and rt_denoise_temporal_fetch's bits, refusals and history."""
    from cpuraytracer_amd import _capi
    W, H = 70, 41
    M = variance_struct(MOMENTS, 3)
    render_frame(dr, scenes, W, H, 0, n=4, m=4, noise=True)
    dr.denoise()
    a = dr.download_denoised()
    dr.denoise(variance=M)
    b = dr.download_denoised()
    assert_same_bits(b["rgb"], a["rgb"], "moments: den")
    assert_same_bits(b["var"], a["var"], "moments: den_var")
    for fetch in (NEAREST, BILINEAR):
        steps = []
        for V in (None, M):
            dr.temporal_reset()
            for f in range(2):
                render_frame(dr, scenes, W, H, f, n=2, m=2, noise=True)
                out = device_step(dr, V, fetch=fetch)
            steps.append(out)
        same_step(steps[1], steps[0], "moments source, fetch %d" % fetch)
    # its preconditions too: one sample, or the switch off, is refused as rt_denoise refuses it
    render_frame(dr, scenes, W, H, 0, n=1, m=1, noise=True)
    for call in (lambda: dr.denoise(variance=M), lambda: dr.denoise_temporal(variance=M)):
        with pytest.raises(_capi.RtError) as e:
            call()
        assert e.value.code == RT_ERR_SEQUENCE


def test_one_sample_with_the_noise_switch_off(dr, scenes):
    from cpuraytracer_amd import _capi
    W, H = 37, 19
    cam = render_frame(dr, scenes, W, H, 0, n=1, m=1, noise=False)
    for call in (lambda: dr.denoise(), lambda: dr.denoise_temporal(), lambda: dr.denoise_temporal(fetch=BILINEAR)):
        with pytest.raises(_capi.RtError) as e:
            call()
        assert e.value.code == RT_ERR_SEQUENCE, e.value
    with pytest.raises(_capi.RtError):
        dr.download_moments()  # there is no strip of second moments at all
    S, feat, ids = strips(dr)
    V = variance_struct(SPATIAL)
    assert V.radius == 1
    dr.denoise(variance=V)
    want = host_denoise_spatial(S, 1, feat, 1, DEFAULTS, V.radius)
    assert_same_bits(dr.download_denoised()["rgb"], want["rgb"], "rt_denoise_variance at n = 1, switch off")
    got = device_step(dr, V, fetch=BILINEAR)
    same_step(got, host_temporal_spatial(S, 1, feat, 1, ids, W, H, cam, V.radius, fetch=BILINEAR), "rt_denoise_temporal_variance at n = 1, switch off")


def test_pipelined_frames_stay_in_flight(dr, scenes):
    """rt_set_frame_pipelining(4), the noise estimate off, stats-less 1-spp frames: the spatial entries read the strip as rt_resolve does --
    the committed samples, a count the device holds -- and settle nothing: no trace launch is added by the calls, the next frame is
    still the carrying kernel, and the render ends on the one-shot bits."""
    from cpuraytracer_amd import HipRenderer
    W, H, frames, depth = 161, 103, 24, 4
    sc = scenes.build_scene("cover", 1, W, H)
    V = variance_struct(SPATIAL, 2)
    dr.upload(sc)
    dr.render_features(W, H, 1, 3)
    dr.set_frame_pipelining(depth)
    try:
        for f in range(frames):
            dr.render(W, H, 1 + f, 2 + f, 50, 1, stats=False)
            if f == frames // 2:
                before = dr.trace_launches()
                assert dr.last_trace_launch().kCarry
                dr.denoise(variance=V)
                dr.denoise_temporal(fetch=BILINEAR, variance=V)
                assert dr.trace_launches() == before, "the calls flushed the pipeline"
                c = dr.committed_samples()
                assert 0 < c <= f + 1
                hdr = dr.download(ldr=False)[0]
                d, t = dr.download_denoised(), dr.download_temporal()
        assert dr.last_trace_launch().kCarry and dr.trace_launches() >= before + frames - 1 - frames // 2
        dr.synchronize()
        assert dr.committed_samples() == frames
        got_end = dr.download(ldr=False)[0]
    finally:
        dr.set_frame_pipelining(0)
    feat, ids = strips(dr)[1:]
    want = host_temporal_spatial(hdr, c, feat, 2, ids, W, H, sc.camera, 2, fetch=BILINEAR)
    assert_same_bits(d["rgb"], want["rgb"], "mid-stream, %d of %d samples committed: den" % (c, frames // 2 + 1))
    assert_same_bits(t["state"], want["state"], "mid-stream: state")
    one = HipRenderer(0)
    try:
        one.upload(sc)
        one.render(W, H, 1, 1 + frames, 50, 1)
        assert_same_bits(got_end, one.download(ldr=False)[0], "pipelined frames with denoise calls between them vs one shot")
    finally:
        one.close()


def test_independence(dr, scenes):
    """The spatial entries between the frames of a progressive render: hdr, ldr, feat and the ids keep their bits, and the render ends
    on the one-shot picture."""
    from cpuraytracer_amd import HipRenderer
    W, H = 96, 64
    sc = scenes.build_scene("cover", 1, W, H)
    V = variance_struct(SPATIAL, 3)
    dr.upload(sc)
    for s in range(1, 5):
        dr.render(W, H, s, s + 1, 50, 1, stats=False)
    dr.render_features(W, H, 1, 9)
    dr.resolve()
    before = (dr.download(), dr.download_features())
    dr.denoise(variance=V)
    dr.denoise_temporal(params_struct(dict(levels=5)), fetch=BILINEAR, variance=V, timed=True)
    after = (dr.download(), dr.download_features())
    assert_same_bits(after[0][0], before[0][0], "hdr")
    assert np.array_equal(after[0][1], before[0][1]), "ldr"
    for key in ("albedo", "normal", "depth", "coverage"):
        assert_same_bits(after[1][key], before[1][key], key)
    assert np.array_equal(after[1]["id"], before[1]["id"])
    assert dr.committed_samples() == 4 and dr.feature_samples() == 8
    for s in range(5, 9):
        dr.render(W, H, s, s + 1, 50, 1, stats=False)
        if s == 6:
            dr.denoise(variance=V)
    dr.synchronize()
    one = HipRenderer(0)
    try:
        one.upload(sc)
        one.render(W, H, 1, 9, 50, 1)
        assert_same_bits(dr.download(ldr=False)[0], one.download(ldr=False)[0], "the continued render vs the one-shot render")
    finally:
        one.close()


def test_alternating_sources_and_fetches_over_one_history(dr, scenes):
    W, H = 70, 41
    plan = [(SPATIAL, 3, BILINEAR), (MOMENTS, 1, NEAREST), (SPATIAL, 1, NEAREST), (MOMENTS, 2, BILINEAR), (SPATIAL, 2, BILINEAR)]
    hist = None
    T = dict(max_history=8)
    for f, (source, R, fetch) in enumerate(plan):
        cam = render_frame(dr, scenes, W, H, f, n=2, m=2, noise=True)
        S, feat, ids, Q = strips(dr, moments=True)
        got = device_step(dr, variance_struct(source, R), None, fetch, T)
        want = host_temporal_spatial(S, 2, feat, 2, ids, W, H, cam, R, hist=hist, T=T, fetch=fetch, sq=Q, source=source)
        same_step(got, want, "frame %d: source %d, R %d, fetch %d" % (f, source, R, fetch))
        hist = history_of(want)
    assert got["len"].max() == len(plan)


def test_refusals_keep_history_and_snapshot(dr, scenes):
    from cpuraytracer_amd import _capi
    W, H = 37, 19
    V = variance_struct(SPATIAL, 2)
    render_frame(dr, scenes, W, H, 0)
    device_step(dr, V)
    render_frame(dr, scenes, W, H, 1)
    kept = device_step(dr, V)

    def refused(fn, code):
        with pytest.raises(_capi.RtError) as e:
            fn()
        assert e.value.code == code, e.value

    for bad in (variance_struct(SPATIAL, 0), variance_struct(SPATIAL, 4), variance_struct(2, 3)):
        refused(lambda: dr.denoise(variance=bad), RT_ERR_INVALID_ARG)
        refused(lambda: dr.denoise_temporal(variance=bad), RT_ERR_INVALID_ARG)
    refused(lambda: dr.denoise(params_struct(dict(levels=6)), variance=V), RT_ERR_INVALID_ARG)
    refused(lambda: dr.denoise_temporal(fetch=2, variance=V), RT_ERR_INVALID_ARG)
    refused(lambda: dr.denoise_temporal(tparams=_capi.temporal_params(max_history=0), variance=V), RT_ERR_INVALID_ARG)
    dr.clear_features()
    refused(lambda: dr.denoise(variance=V), RT_ERR_SEQUENCE)           # no feature strips
    refused(lambda: dr.denoise_temporal(variance=V), RT_ERR_SEQUENCE)
    dr.render_features(W + 1, H, 1, 2)
    refused(lambda: dr.denoise(variance=V), RT_ERR_SEQUENCE)           # ... of another size
    dr.clear()
    refused(lambda: dr.denoise(variance=V), RT_ERR_SEQUENCE)           # n == 0
    refused(lambda: dr.denoise_temporal(variance=V), RT_ERR_SEQUENCE)
    d, t = dr.download_denoised(), dr.download_temporal()
    same_step(dict(rgb=d["rgb"], var=d["var"], **t), kept, "after the refusals")
    assert np.array_equal(d["ldr"], kept["ldr"])
    # a cyclic row set: its local rows are not neighbours
    two = _capi.RtRowset(0, H, 1, 0, 2)
    dr.render(W, H, 1, 2, 50, 1, rowset=two)
    dr.render_features(W, H, 1, 2, rowset=two)
    refused(lambda: dr.denoise(variance=V), RT_ERR_INVALID_ARG)
    assert_same_bits(dr.download_temporal()["state"], kept["state"], "a refused call keeps the history")


# The numpy restatement over the CPU oracle's strips (tools/denoise_spatial_grid.py; docs/EXPERIMENTS.md "Spatial variance estimate")
# measured MSE x 0.2402 and relative MSE x 0.1851 for this protocol -- the device has those strips' bits, so the figure is the same
# number -- and the bounds are those ratios rounded up to the next 0.05.
QUALITY_BOUND_MSE, QUALITY_BOUND_REL = 0.25, 0.20


def test_quality_against_1024_spp(dr, scenes):
    """Cover scene, 240 x 160, depth 50: eight frames of ONE sample (seed 1 + f) from a camera that turns 0.5 degrees per frame, the
    noise estimate off, the spatial source with its default radius, the bilinear fetch with its defaults; the last frame's result
    against samples 1..1024 of the last camera (never the filter's own output).  MSE and relative MSE must be below the unfiltered
    1-spp last frame's -- a filter that does not beat its input is not shipped -- and within the measured ratios' bounds."""
    W, H, frames = QUALITY["W"], QUALITY["H"], QUALITY["frames"]
    V = variance_struct(SPATIAL)
    for f in range(frames):
        render_frame(dr, scenes, W, H, f, deg=QUALITY["deg"])
        dr.denoise_temporal(fetch=BILINEAR, variance=V)
    raw = dr.download(ldr=False)[0]
    den = dr.download_denoised()["rgb"]
    dr.render(W, H, 2, 1 + QUALITY["ref_spp"], QUALITY["depth"], frames)
    ref = dr.download(ldr=False)[0] / np.float32(QUALITY["ref_spp"])
    r_mse, r_rel = mse(den, ref) / mse(raw, ref), rel_mse(den, ref) / rel_mse(raw, ref)
    print("spatial variance quality 240x160, 8 x 1 spp: MSE %.5f -> %.5f (x %.4f), relMSE %.5f -> %.5f (x %.4f)"
          % (mse(raw, ref), mse(den, ref), r_mse, rel_mse(raw, ref), rel_mse(den, ref), r_rel))
    assert r_mse < 1.0 and r_rel < 1.0, (r_mse, r_rel)
    assert r_mse <= QUALITY_BOUND_MSE and r_rel <= QUALITY_BOUND_REL, (r_mse, r_rel)


DEVICE_COPY_CHILD = """
import sys
import numpy as np
import torch
torch.cuda.init()  # torch's HIP runtime first, as in bench.py: the library then shares it
sys.path.insert(0, sys.argv[1])
from cpuraytracer_amd import HipRenderer, _capi, scenes
W, H = 96, 64
r = HipRenderer(0)
V = _capi.variance_params(source=_capi.RT_VARIANCE_SPATIAL, radius=2)
out = {}
for f in range(2):
    sc = scenes.build_scene("cover", 1, W, H)
    sc.camera = scenes.orbit_camera(sc.camera, 0.5 * f, (0.0, 1.0, 0.0))
    r.upload(sc)
    r.render(W, H, 1, 2, 50, 1 + f)
    r.render_features(W, H, 1, 2)
    if f == 0:
        r.denoise(variance=V)
        out["first"] = r.download_denoised()["rgb"]
    ms = r.denoise_temporal(timed=(f == 1), fetch=4, variance=V)
rgb_t = torch.full((H, W, 3), -1.0, dtype=torch.float32, device="cuda:0")
var_t = torch.full((H, W), -1.0, dtype=torch.float32, device="cuda:0")
ldr_t = torch.full((H, W, 3), 7, dtype=torch.uint8, device="cuda:0")
torch.cuda.synchronize()
r.copy_denoised_to_device(rgb_t.data_ptr(), var_t.data_ptr(), ldr_t.data_ptr())
r.synchronize()
d = r.download_denoised()
t = r.download_temporal()
np.savez(sys.argv[2], rgb_t=rgb_t.cpu().numpy(), var_t=var_t.cpu().numpy(), ldr_t=ldr_t.cpu().numpy(), ms=np.float64(ms), **out, **d, **t)
r.close()
"""


def test_python_views_and_device_copy(dr, scenes, tmp_path):
    """In a process of its own: torch has to bring up its HIP runtime before the library opens the device (bench.py's order)."""
    W, H = 96, 64
    out = str(tmp_path / "copy.npz")
    p = subprocess.run([sys.executable, "-c", DEVICE_COPY_CHILD, ROOT, out], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    z = np.load(out)
    V = variance_struct(SPATIAL, 2)
    for f in range(2):
        render_frame(dr, scenes, W, H, f)
        if f == 0:
            dr.denoise(variance=V)
            assert_same_bits(z["first"], dr.download_denoised()["rgb"], "child process: denoise(variance=)")
        want = device_step(dr, V, fetch=BILINEAR)
    assert z["rgb"].shape == (H, W, 3) and z["rgb"].dtype == np.float32 and z["var"].shape == (H, W) and z["state"].shape == (H, W, 4)
    assert float(z["ms"]) > 0.0
    for k in ("rgb", "var", "state"):
        assert_same_bits(z[k], want[k], "child process: " + k)
    assert np.array_equal(z["len"], want["len"]) and np.array_equal(z["target"], want["target"]) and np.array_equal(z["ldr"], want["ldr"])
    assert_same_bits(z["rgb_t"], z["rgb"], "device copy: rgb")
    assert_same_bits(z["var_t"], z["var"], "device copy: var")
    assert np.array_equal(z["ldr_t"], z["ldr"])


def test_cli_one_sample_orbit(dr, scenes, tmp_path):
    W, H, frames = 96, 64, 3
    ppm, den = str(tmp_path / "a.ppm"), str(tmp_path / "x.ppm")
    base = [CLI, "--width", str(W), "--height", str(H), "--seed", "5", "--quiet", "--out", ppm, "--denoise-out", den]
    p = subprocess.run(base + ["--spp", "1", "--orbit-frames", str(frames), "--denoise-variance", "spatial"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    V = variance_struct(SPATIAL)
    for f in range(frames):
        render_frame(dr, scenes, W, H, f, seed=5 + f)
        dr.resolve()
        want = device_step(dr, V)
    head = b"P6\n%d %d\n255\n" % (W, H)
    data = open(den, "rb").read()
    assert data.startswith(head) and data[len(head):] == want["ldr"].tobytes()
    assert open(ppm, "rb").read()[len(head):] == dr.download()[1].tobytes()  # --out is the last frame as rendered
    assert (want["len"] == 2).any()
    # the radius and the fetch reach the call; a single picture at one sample works too
    p = subprocess.run(base + ["--spp", "1", "--orbit-frames", "2", "--orbit-fetch", "bilinear", "--denoise-variance", "spatial", "--denoise-radius", "3"],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    dr.temporal_reset()
    for f in range(2):
        render_frame(dr, scenes, W, H, f, seed=5 + f)
        want = device_step(dr, variance_struct(SPATIAL, 3), fetch=BILINEAR)
    assert open(den, "rb").read()[len(head):] == want["ldr"].tobytes()
    p = subprocess.run(base + ["--spp", "1", "--denoise-variance", "spatial", "--denoise-radius", "2"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    render_frame(dr, scenes, W, H, 0, seed=5)
    dr.denoise(variance=variance_struct(SPATIAL, 2))
    assert open(den, "rb").read()[len(head):] == dr.download_denoised()["ldr"].tobytes()
    # refused with a message or the usage, nothing rendered: one sample under the moments source; a radius outside 1..3; no --denoise-out
    for extra in (["--spp", "1", "--orbit-frames", "2", "--denoise-out", den], ["--spp", "1", "--orbit-frames", "2", "--denoise-out", den, "--denoise-variance", "moments"],
                  ["--spp", "1", "--denoise-out", den, "--denoise-variance", "spatial", "--denoise-radius", "4"], ["--spp", "2", "--denoise-variance", "spatial"]):
        p = subprocess.run([CLI, "--width", "8", "--height", "8"] + extra, capture_output=True, text=True, timeout=120)
        assert p.returncode == 2, extra
