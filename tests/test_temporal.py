"""Temporal accumulation on the device (rt_denoise_temporal; csrc/rt_temporal.h, rt_denoise.hip): the kernel against the host twin
compiled from the same source (which tests/test_temporal_cpu.py pins to a numpy restatement of the contract), bit for bit and frame by
frame along an orbit the device itself rendered; the history's lifetime; that nothing else in the context changes; what the history
buys against a 1024-spp picture; the Python views, the device copy and the CLI."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from temporal_common import COVER_PIVOT, NO_TARGET, history_of, host_temporal, orbit_scene
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


def render_frame(r, scenes, W, H, f, rs=None, deg=0.5, spp=2, depth=50, name="cover", seed=None):
    """Frame f of the orbit: the camera turned deg * f degrees, an upload, samples 1..spp with seed 1 + f, the feature pass."""
    sc = orbit_scene(scenes, name, W, H, deg * f)
    r.upload(sc)
    r.set_noise_estimate(True)
    r.render(W, H, 1, 1 + spp, depth, (1 + f) if seed is None else seed, rowset=rowset_of(rs))
    r.render_features(W, H, 1, 1 + spp, rowset=rowset_of(rs))
    return sc.camera


def strips(r):
    """What rt_denoise_temporal reads, as the device holds it: hdr, sq [rows, W, 3], feat [rows, W, 8], ids [rows, W]."""
    hdr, _ = r.download(ldr=False)
    d = r.download_features()
    feat = np.concatenate([d["albedo"], d["normal"], d["depth"][..., None], d["coverage"][..., None]], axis=-1)
    return hdr, r.download_moments(), np.ascontiguousarray(feat), d["id"]


def tonemap(r, rgb):
    from cpuraytracer_amd import _capi
    flat = np.ascontiguousarray(rgb, dtype=np.float32).reshape(-1, 3)
    out = np.zeros((flat.shape[0], 3), np.uint8)
    _capi.check(r._L.rt_unit_tonemap(r._h, flat.ctypes.data, flat.shape[0], 1, out.ctypes.data))
    return out.reshape(rgb.shape)


def device_step(r, P=None, T=None):
    from cpuraytracer_amd import _capi
    r.denoise_temporal(params_struct(dict(DEFAULTS, **P)) if P else None, _capi.temporal_params(**T) if T else None)
    d, t = r.download_denoised(), r.download_temporal()
    return dict(rgb=d["rgb"], var=d["var"], ldr=d["ldr"], **t)


def same_step(got, want, what):
    assert_same_bits(got["rgb"], want["rgb"], what + ": den")
    assert_same_bits(got["var"], want["var"], what + ": den_var")
    assert_same_bits(got["state"], want["state"], what + ": state")
    assert np.array_equal(got["len"], want["len"]), what + ": len"
    assert np.array_equal(got["target"], want["target"]), what + ": target"


SHAPES = {"96x64": (96, 64, None, 4), "70x41": (70, 41, None, 2), "band": (96, 64, BAND, 2)}


@pytest.mark.parametrize("levels", [1, 3, 5])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_device_equals_host_twin(dr, scenes, monkeypatch, shape, levels):
    """Frame by frame along the orbit (2 spp, 0.5 degrees per frame, seed 1 + f), each on the history the frame before left, with no
    level staged in LDS and with every level that fits: den, den_var, ldr, state, len and target."""
    W, H, rs, frames = SHAPES[shape]
    P, T = dict(levels=levels), dict(max_history=8)  # (beyond the default 2, so that the lengths along the orbit differ)
    first_row = rs[0] if rs else 0
    for knob in ("0", "1"):
        monkeypatch.setenv("RT_DENOISE_STAGE", knob)
        dr.temporal_reset()
        hist = None
        for f in range(frames):
            cam = render_frame(dr, scenes, W, H, f, rs)
            S, Q, feat, ids = strips(dr)
            got = device_step(dr, P, T)
            want = host_temporal(S, Q, 2, feat, 2, ids, W, H, cam, hist, P, T, first_row)
            what = "%s, %d levels, stage %s, frame %d" % (shape, levels, knob, f)
            same_step(got, want, what)
            assert np.array_equal(got["ldr"], tonemap(dr, got["rgb"])), what + ": ldr"
            steps = [1 << l for l in range(levels)]
            assert dr.denoise_forms() == [STAGED if knob == "1" and s <= 4 else DIRECT for s in steps] + [0] * (5 - levels)
            hist = history_of(want)
        # not vacuous: the history was used, the move shifted targets and rejected some pixels
        acc = got["target"] != NO_TARGET
        own = np.arange(acc.size, dtype=np.uint32).reshape(acc.shape)
        assert acc.mean() > 0.5 and (~acc).any() and (got["target"][acc] != own[acc]).any() and got["len"].max() == frames


def test_empty_history_is_rt_denoise(dr, scenes):
    W, H = 96, 64
    render_frame(dr, scenes, W, H, 0)
    dr.denoise()
    want = dr.download_denoised()
    got = device_step(dr)
    for k in ("rgb", "var"):
        assert_same_bits(got[k], want[k], k)
    assert np.array_equal(got["ldr"], want["ldr"])
    assert (got["len"] == 1).all() and (got["target"] == NO_TARGET).all()


def test_static_camera_fills_the_history(dr, scenes):
    """Ten frames from one camera, seeds 1..10: the feature pass does not depend on the seed, so every pixel finds itself."""
    W, H = 96, 64
    from cpuraytracer_amd import _capi
    own = np.arange(W * H, dtype=np.uint32).reshape(H, W)
    for f in range(1, 11):
        render_frame(dr, scenes, W, H, 0, seed=f)
        dr.denoise_temporal(None, _capi.temporal_params(max_history=8))
        t = dr.download_temporal()
        assert (t["len"] == min(f, 8)).all(), f
        assert np.array_equal(t["target"], own) if f > 1 else (t["target"] == NO_TARGET).all()


def test_quarter_turn(dr, scenes):
    W, H = 96, 64
    render_frame(dr, scenes, W, H, 0, deg=90.0)
    ids0 = dr.download_features()["id"]
    dr.denoise_temporal()
    render_frame(dr, scenes, W, H, 1, deg=90.0)
    ids1 = dr.download_features()["id"]
    dr.denoise_temporal()
    t = dr.download_temporal()
    acc = t["target"] != NO_TARGET
    assert (t["target"][acc] < W * H).all()
    assert np.array_equal(ids1[acc], ids0.reshape(-1)[t["target"][acc]])
    assert (t["len"][~acc] == 1).all() and (t["len"][acc] == 2).all() and (~acc).any()


def test_independence_and_history_lifetime(dr, scenes):
    from cpuraytracer_amd import _capi
    W, H = 96, 64
    # the one-shot picture the continued render must end on
    sc1 = orbit_scene(scenes, "cover", W, H, 0.5)
    dr.upload(sc1)
    dr.set_noise_estimate(True)
    dr.render(W, H, 1, 9, 50, 2)
    one_shot = (dr.download(ldr=False)[0], dr.download_moments())
    # frame 0, then frame 1 after an upload: the history survives rt_scene_upload
    render_frame(dr, scenes, W, H, 0)
    first = device_step(dr)
    render_frame(dr, scenes, W, H, 1)
    dr.resolve()
    dr.denoise()
    plain = dr.download_denoised()
    before = (dr.download(), dr.download_moments(), dr.download_features())
    got = device_step(dr)
    assert (got["target"] != NO_TARGET).mean() > 0.5 and (got["rgb"] != plain["rgb"]).any()
    after = (dr.download(), dr.download_moments(), dr.download_features())
    assert_same_bits(after[0][0], before[0][0], "hdr")
    assert np.array_equal(after[0][1], before[0][1]), "ldr"
    assert_same_bits(after[1], before[1], "sq")
    for key in ("albedo", "normal", "depth", "coverage"):
        assert_same_bits(after[2][key], before[2][key], key)
    assert np.array_equal(after[2]["id"], before[2]["id"])
    assert dr.committed_samples() == 2 and dr.feature_samples() == 2
    # rt_denoise after it gives the bits it gave before, and leaves the history alone
    dr.denoise()
    again = dr.download_denoised()
    assert_same_bits(again["rgb"], plain["rgb"], "rt_denoise after the temporal call")
    assert np.array_equal(again["ldr"], plain["ldr"])
    t = dr.download_temporal()
    assert_same_bits(t["state"], got["state"], "the history after rt_denoise")
    # a render that continues ends on the one-shot bits
    dr.render(W, H, 3, 9, 50, 2)
    assert_same_bits(dr.download(ldr=False)[0], one_shot[0], "the continued render vs the one-shot render")
    assert_same_bits(dr.download_moments(), one_shot[1], "its second moments")
    # after rt_temporal_reset the next call equals rt_denoise, and the history is empty until then
    dr.temporal_reset()
    with pytest.raises(_capi.RtError) as e:
        dr.download_temporal()
    assert e.value.code == RT_ERR_SEQUENCE
    render_frame(dr, scenes, W, H, 1)
    fresh = device_step(dr)
    assert_same_bits(fresh["rgb"], plain["rgb"], "after the reset")
    assert (fresh["len"] == 1).all()
    # a changed size starts an empty history; back at the first size the history of the other size is no history either
    render_frame(dr, scenes, 70, 41, 1)
    dr.denoise()
    small = dr.download_denoised()
    got = device_step(dr)
    assert_same_bits(got["rgb"], small["rgb"], "another size")
    assert got["len"].shape == (41, 70) and (got["len"] == 1).all()
    render_frame(dr, scenes, W, H, 1)
    assert (device_step(dr)["len"] == 1).all()
    assert first["len"].shape == (H, W)


def test_refusals_keep_history_and_snapshot(dr, scenes):
    from cpuraytracer_amd import _capi
    W, H = 96, 64

    def refused(fn, code=RT_ERR_SEQUENCE):
        with pytest.raises(_capi.RtError) as e:
            fn()
        assert e.value.code == code, e.value

    sc = orbit_scene(scenes, "cover", W, H, 0.0)
    dr.upload(sc)
    refused(lambda: dr.download_temporal())
    dr.render(W, H, 1, 3, 50, 1)
    dr.render_features(W, H, 1, 3)
    refused(lambda: dr.denoise_temporal())                 # the noise switch is off
    dr.set_noise_estimate(True)
    dr.render(W, H, 1, 2, 50, 1)
    refused(lambda: dr.denoise_temporal())                 # n == 1
    dr.render(W, H, 2, 3, 50, 1)
    dr.clear_features()
    refused(lambda: dr.denoise_temporal())                 # no feature strips
    dr.render_features(W + 1, H, 1, 2)
    refused(lambda: dr.denoise_temporal())                 # feature strips of another size
    dr.render_features(W, H, 1, 2, rowset=_capi.RtRowset(0, H - 1, H - 1, 0, 1))
    refused(lambda: dr.denoise_temporal())                 # ... of another row set
    dr.render_features(W, H, 1, 3)
    refused(lambda: dr.download_temporal())                # refused calls left no history
    refused(lambda: dr.download_denoised())                # ... and no result
    good = device_step(dr)
    for bad in (dict(levels=0), dict(levels=6), dict(k_depth=-1.0), dict(k_colour=float("nan")), dict(var_floor=0.0)):
        refused(lambda: dr.denoise_temporal(params_struct(bad)), RT_ERR_INVALID_ARG)
    for bad in (dict(max_history=0), dict(max_history=65), dict(depth_tol=-1.0), dict(normal_tol=float("nan")), dict(coverage_tol=float("inf"))):
        refused(lambda: dr.denoise_temporal(None, _capi.temporal_params(**bad)), RT_ERR_INVALID_ARG)
    two = _capi.RtRowset(0, H, 1, 0, 2)                    # a cyclic row set: its local rows are not neighbours
    dr.render(W, H, 1, 3, 50, 1, rowset=two)
    dr.render_features(W, H, 1, 3, rowset=two)
    refused(lambda: dr.denoise_temporal(), RT_ERR_INVALID_ARG)
    d, t = dr.download_denoised(), dr.download_temporal()
    assert_same_bits(d["rgb"], good["rgb"], "a refused call keeps the snapshot")
    assert_same_bits(t["state"], good["state"], "a refused call keeps the history")
    assert np.array_equal(t["len"], good["len"]) and np.array_equal(t["target"], good["target"])
    # ... and the kept history is used by the next good call
    dr.render(W, H, 1, 3, 50, 1)
    dr.render_features(W, H, 1, 3)
    assert (device_step(dr)["len"] == 2).all()


def rel_mse(x, ref):
    x, ref = x.astype(np.float64), ref.astype(np.float64)
    return float(np.mean((x - ref) ** 2 / (ref ** 2 + 0.01)))


# Measured 0.696 and 0.724, by the host twin over the CPU oracle's strips and on the device alike (the path is deterministic); asserted
# at the measured value plus a fifth, the margin tests/test_denoise.py took: other seeds and tie-breaks move the ratios by about that.
QUALITY_BOUND_MSE, QUALITY_BOUND_REL = 0.835, 0.869


def test_quality_against_1024_spp(dr, scenes):
    """Cover scene, 240 x 160, depth 50, eight frames of 2 spp along the orbit (0.5 degrees per frame, seeds 1..8), the defaults.  The
    last frame's temporal result against rt_denoise on that frame alone, both measured against samples 1..1024 at the last camera
    (never a filter's output): MSE and relative MSE mean((x - ref)^2 / (ref^2 + 0.01))."""
    W, H, frames = 240, 160, 8
    for f in range(frames):
        render_frame(dr, scenes, W, H, f)
        dr.denoise_temporal()
    temporal = dr.download_denoised()["rgb"]
    dr.denoise()
    single = dr.download_denoised()["rgb"]
    dr.render(W, H, 3, 1025, 50, frames)
    ref = dr.download(ldr=False)[0] / np.float32(1024)
    mse = lambda x: float(np.mean((x.astype(np.float64) - ref.astype(np.float64)) ** 2))
    r_mse, r_rel = mse(temporal) / mse(single), rel_mse(temporal, ref) / rel_mse(single, ref)
    print("temporal quality 240x160, 8 frames of 2 spp: MSE %.5f -> %.5f (x %.3f), relMSE %.5f -> %.5f (x %.3f)"
          % (mse(single), mse(temporal), r_mse, rel_mse(single, ref), rel_mse(temporal, ref), r_rel))
    assert r_mse < 1.0 and r_rel < 1.0, (r_mse, r_rel)
    assert r_mse <= QUALITY_BOUND_MSE and r_rel <= QUALITY_BOUND_REL, (r_mse, r_rel)


DEVICE_COPY_CHILD = """
import sys
import numpy as np
import torch
torch.cuda.init()  # torch's HIP runtime first, as in bench.py: the library then shares it
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
from cpuraytracer_amd import HipRenderer, scenes
from temporal_common import orbit_scene
W, H = 96, 64
r = HipRenderer(0)
for f in range(2):
    r.upload(orbit_scene(scenes, "cover", W, H, 0.5 * f))
    r.set_noise_estimate(True)
    r.render(W, H, 1, 3, 50, 1 + f)
    r.render_features(W, H, 1, 3)
    ms = r.denoise_temporal(timed=(f == 1))
rgb_t = torch.full((H, W, 3), -1.0, dtype=torch.float32, device="cuda:0")
var_t = torch.full((H, W), -1.0, dtype=torch.float32, device="cuda:0")
ldr_t = torch.full((H, W, 3), 7, dtype=torch.uint8, device="cuda:0")
torch.cuda.synchronize()
r.copy_denoised_to_device(rgb_t.data_ptr(), var_t.data_ptr(), ldr_t.data_ptr())
r.synchronize()
d = r.download_denoised()
t = r.download_temporal()
np.savez(sys.argv[2], rgb_t=rgb_t.cpu().numpy(), var_t=var_t.cpu().numpy(), ldr_t=ldr_t.cpu().numpy(), ms=np.float64(ms), **d, **t)
r.close()
"""


def test_python_views_and_device_copy(dr, scenes, tmp_path):
    """In a process of its own: torch has to bring up its HIP runtime before the library opens the device (bench.py's order)."""
    W, H = 96, 64
    out = str(tmp_path / "copy.npz")
    p = subprocess.run([sys.executable, "-c", DEVICE_COPY_CHILD, ROOT, out], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    z = np.load(out)
    for f in range(2):
        render_frame(dr, scenes, W, H, f)
        want = device_step(dr)
    assert z["state"].shape == (H, W, 4) and z["state"].dtype == np.float32
    assert z["len"].shape == (H, W) and z["len"].dtype == np.uint32 and z["target"].shape == (H, W) and z["target"].dtype == np.uint32
    assert float(z["ms"]) > 0.0
    for k in ("rgb", "var", "state"):
        assert_same_bits(z[k], want[k], "child process: " + k)
    assert np.array_equal(z["len"], want["len"]) and np.array_equal(z["target"], want["target"]) and np.array_equal(z["ldr"], want["ldr"])
    assert_same_bits(z["rgb_t"], z["rgb"], "device copy: rgb")
    assert_same_bits(z["var_t"], z["var"], "device copy: var")
    assert np.array_equal(z["ldr_t"], z["ldr"])


def test_cli_orbit(dr, scenes, tmp_path):
    W, H, frames, deg = 96, 64, 3, 0.75
    ppm, den = str(tmp_path / "a.ppm"), str(tmp_path / "x.ppm")
    base = [CLI, "--width", str(W), "--height", str(H), "--spp", "2", "--seed", "5", "--quiet", "--out", ppm]
    p = subprocess.run(base + ["--denoise-out", den, "--orbit-frames", str(frames), "--orbit-deg", str(deg)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    for f in range(frames):
        render_frame(dr, scenes, W, H, f, deg=deg, seed=5 + f)
        dr.resolve()
        want = device_step(dr)
    head = b"P6\n%d %d\n255\n" % (W, H)
    data = open(den, "rb").read()
    assert data.startswith(head) and data[len(head):] == want["ldr"].tobytes()
    assert open(ppm, "rb").read()[len(head):] == dr.download()[1].tobytes()  # --out is the last frame as rendered
    assert (want["len"] == 2).any() and (want["target"] != NO_TARGET).any()
    # the flags need --denoise-out and refuse --gpus and --target-error: a message, nothing rendered
    for extra in (["--orbit-frames", "2"], ["--orbit-deg", "1", "--denoise-out", den, "--gpus", "1"],
                  ["--orbit-frames", "2", "--denoise-out", den, "--target-error", "0.1"]):
        p = subprocess.run([CLI, "--width", "8", "--height", "8", "--spp", "2"] + extra, capture_output=True, text=True, timeout=120)
        assert p.returncode == 2 and "--orbit-frames" in p.stderr, extra
