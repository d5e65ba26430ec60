"""Denoise on the device (rt_denoise; csrc/rt_denoise.h, rt_denoise.hip): the kernels against the host twin compiled from the same
source (which tests/test_denoise_cpu.py pins to a numpy restatement of the contract), bit for bit, on strips the device itself
rendered: every number of levels, both kernel forms, ragged shapes and a band of rows; the sequencing rules; that nothing else in the
context changes; the tonemap; what the filter buys against a 1024-spp picture; the Python views, the device copy and the CLI."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_denoise_cpu import DEFAULTS, host_denoise, params_struct
from test_noise_estimate_cpu import assert_same_bits

pytestmark = pytest.mark.gpu

RT_ERR_INVALID_ARG, RT_ERR_SEQUENCE = 2, 6
CLI = os.path.join(ROOT, "cpuraytracer_amd", "lib", "spheres")
OTHER = dict(k_normal=3.0, k_depth=50.0, k_albedo=7.5, k_coverage=0.0, k_colour=4.0, var_floor=1e-4)
DIRECT, STAGED = 1, 2
STAGED_BY_DEFAULT = (1, 2)   # the measured cut (csrc/host/rt_denoise_launch.h StageByDefault): steps whose taps are staged in LDS
FITS_LDS = (1, 2, 4)         # steps whose tile and halo fit the 64 KiB the staged form may take


def forms_for(levels, knob):
    steps = [1 << l for l in range(levels)]
    staged = {None: STAGED_BY_DEFAULT, "0": (), "1": FITS_LDS}[knob]
    return [STAGED if s in staged else DIRECT for s in steps] + [0] * (5 - levels)


@pytest.fixture(scope="module")
def scenes_mod(built):
    from cpuraytracer_amd import scenes
    return scenes


@pytest.fixture()
def dr(built):
    """A context of its own: the switches these tests flip never reach the session's renderer."""
    from cpuraytracer_amd import HipRenderer
    r = HipRenderer(0)
    yield r
    r.close()


def strips(r):
    """What rt_denoise reads, as the device holds it: hdr, sq [rows, W, 3], feat [rows, W, 8]."""
    hdr, _ = r.download(ldr=False)
    d = r.download_features()
    feat = np.concatenate([d["albedo"], d["normal"], d["depth"][..., None], d["coverage"][..., None]], axis=-1)
    return hdr, r.download_moments(), np.ascontiguousarray(feat)


def prepare(r, sc, W, H, n, m, rowset=None, depth=50, seed=1):
    r.upload(sc)
    r.set_noise_estimate(True)
    r.render(W, H, 1, 1 + n, depth, seed, rowset=rowset)
    r.render_features(W, H, 1, 1 + m, rowset=rowset)


def check(r, want, what):
    d = r.download_denoised()
    assert_same_bits(d["rgb"], want[0], what + ": rgb")
    assert_same_bits(d["var"], want[1], what + ": var")
    return d


@pytest.fixture(scope="module")
def cover(scenes_mod, built):
    """The cover scene at 96 x 64: the device's strips after samples 1..8 and the host twin's answers (computed once, never changed)."""
    from cpuraytracer_amd import HipRenderer
    W, H = 96, 64
    sc = scenes_mod.build_scene("cover", 1, W, H)
    r = HipRenderer(0)
    try:
        prepare(r, sc, W, H, 8, 8)
        S = strips(r)
    finally:
        r.close()
    wants = {}
    for name, over in (("defaults", {}), ("other", OTHER)):
        for levels in range(1, 6):
            P = dict(DEFAULTS, levels=levels, **over)
            wants[(name, levels)] = (P, host_denoise(S[0], S[1], 8, S[2], 8, P))
    for a in S + tuple(w for _, ws in wants.values() for w in ws):
        a.setflags(write=False)
    return sc, W, H, S, wants


@pytest.mark.parametrize("knob", [None, "0", "1"], ids=["cut", "stage0", "stage1"])
def test_device_equals_host_twin(dr, cover, monkeypatch, knob):
    sc, W, H, S, wants = cover
    if knob is None:
        monkeypatch.delenv("RT_DENOISE_STAGE", raising=False)
    else:
        monkeypatch.setenv("RT_DENOISE_STAGE", knob)
    prepare(dr, sc, W, H, 8, 8)
    for a, b, what in zip(strips(dr), S, ("hdr", "sq", "feat")):
        assert_same_bits(a, b, "this context's " + what)
    assert dr.denoise_forms() == [0] * 5
    for (name, levels), (P, want) in wants.items():
        ms = dr.denoise(params_struct(P) if (name, levels) != ("defaults", 3) else None, timed=(levels % 2 == 0))
        assert (ms is not None and ms > 0.0) if levels % 2 == 0 else ms is None
        assert dr.denoise_forms() == forms_for(levels, knob), (name, levels, knob)
        check(dr, want, "%s, %d levels, RT_DENOISE_STAGE=%s" % (name, levels, knob))
    # not vacuous: the picture has noise and the filter moved it; the parameter sets differ
    d3, o3 = wants[("defaults", 3)][1], wants[("other", 3)][1]
    assert (d3[1] > 0).any() and (d3[0] != S[0] / np.float32(8)).any() and (d3[0] != o3[0]).any()


RAGGED = [(5, 3, None), (37, 19, None), (70, 41, None), (200, 9, None), (70, 41, (8, 19, 19, 0, 1))]


@pytest.mark.parametrize("W,H,rs", RAGGED, ids=["5x3", "37x19", "70x41", "200x9", "band"])
def test_ragged_shapes(dr, scenes_mod, monkeypatch, W, H, rs):
    """Less than one tile; partial tiles in both directions around whole ones; one row of tiles; and a band of rows of a taller image,
    whose first and last rows are filtered as edges of the picture.  Features after 3 samples, picture after 8."""
    from cpuraytracer_amd import _capi
    sc = scenes_mod.build_scene("cover", 1, W, H)
    rowset = _capi.RtRowset(*rs) if rs else None
    prepare(dr, sc, W, H, 8, 3, rowset=rowset)
    S = strips(dr)
    rows = rs[1] if rs else H
    assert S[0].shape == (rows, W, 3) and S[2].shape == (rows, W, 8)
    for levels in (5, 2):
        P = dict(DEFAULTS, levels=levels)
        want = host_denoise(S[0], S[1], 8, S[2], 3, P)
        for knob in ("0", "1"):
            monkeypatch.setenv("RT_DENOISE_STAGE", knob)
            dr.denoise(params_struct(P))
            assert dr.denoise_forms() == forms_for(levels, knob)
            check(dr, want, "%d x %d %s, %d levels, stage %s" % (W, H, rs, levels, knob))


def test_sequencing(dr, cover, scenes_mod):
    from cpuraytracer_amd import _capi
    sc, W, H, S, wants = cover

    def refused(fn, code=RT_ERR_SEQUENCE):
        with pytest.raises(_capi.RtError) as e:
            fn()
        assert e.value.code == code, e.value

    dr.upload(sc)
    refused(lambda: dr.download_denoised())                # download before any denoise
    refused(lambda: dr.copy_denoised_to_device(None, None, None))
    dr.render(W, H, 1, 9, 50, 1)
    dr.render_features(W, H, 1, 9)
    refused(lambda: dr.denoise())                          # the noise switch is off
    dr.set_noise_estimate(True)
    dr.render(W, H, 1, 2, 50, 1)
    refused(lambda: dr.denoise())                          # n == 1
    dr.render(W, H, 2, 9, 50, 1)
    dr.clear_features()
    refused(lambda: dr.denoise())                          # no feature strips
    dr.render_features(W + 1, H, 1, 2)
    refused(lambda: dr.denoise())                          # feature strips of another size
    dr.render_features(W, H, 1, 2, rowset=_capi.RtRowset(0, H - 1, H - 1, 0, 1))
    refused(lambda: dr.denoise())                          # ... of another row set
    dr.render_features(W, H, 1, 9)
    for bad in (dict(levels=0), dict(levels=6), dict(k_depth=-1.0), dict(k_colour=float("nan")), dict(var_floor=0.0)):
        refused(lambda: dr.denoise(params_struct(bad)), RT_ERR_INVALID_ARG)
    refused(lambda: dr.download_denoised())                # a refused call leaves no result
    dr.denoise()
    check(dr, wants[("defaults", 3)][1], "after the refusals")
    # a cyclic row set: its local rows are not neighbours
    two = _capi.RtRowset(0, H, 1, 0, 2)
    dr.render(W, H, 1, 5, 50, 1, rowset=two)
    dr.render_features(W, H, 1, 5, rowset=two)
    refused(lambda: dr.denoise(), RT_ERR_INVALID_ARG)
    check(dr, wants[("defaults", 3)][1], "a refused call keeps the snapshot")
    # rt_scene_upload voids the result
    dr.upload(scenes_mod.build_scene("three", 1, W, H))
    refused(lambda: dr.download_denoised())
    assert dr.denoise_forms() == [0] * 5


@pytest.mark.parametrize("lookahead", [1, 4], ids=["plain", "lookahead4"])
def test_independence(dr, cover, lookahead):
    """rt_denoise between the frames of a progressive render: every strip it does not own keeps its bits, and the render ends on the
    one-shot picture."""
    sc, W, H, S, wants = cover
    dr.upload(sc)
    dr.set_noise_estimate(True)
    dr.set_frame_lookahead(lookahead)
    for s in range(1, 5):
        dr.render(W, H, s, s + 1, 50, 1, stats=False)
    dr.render_features(W, H, 1, 9)
    dr.resolve()
    before = (dr.download(), dr.download_moments(), dr.download_features())
    dr.denoise()
    mid = dr.download_denoised()
    dr.denoise(params_struct(dict(levels=5)), timed=True)
    after = (dr.download(), dr.download_moments(), dr.download_features())
    assert_same_bits(after[0][0], before[0][0], "hdr")
    assert np.array_equal(after[0][1], before[0][1]), "ldr"
    assert_same_bits(after[1], before[1], "sq")
    for key in ("albedo", "normal", "depth", "coverage"):
        assert_same_bits(after[2][key], before[2][key], key)
    assert np.array_equal(after[2]["id"], before[2]["id"])
    assert dr.committed_samples() == 4 and dr.feature_samples() == 8
    # the four-sample picture was what the filter saw (features after 8 samples: m != n)
    feat = S[2]
    want4 = host_denoise(before[0][0], before[1], 4, feat, 8, DEFAULTS)
    assert_same_bits(mid["rgb"], want4[0], "denoised after four frames")
    for s in range(5, 9):
        dr.render(W, H, s, s + 1, 50, 1, stats=False)
        if s == 6:
            dr.denoise()
    dr.synchronize()
    assert_same_bits(dr.download(ldr=False)[0], S[0], "the continued render vs the one-shot render")
    assert_same_bits(dr.download_moments(), S[1], "its second moments")
    dr.denoise()
    check(dr, wants[("defaults", 3)][1], "denoised at the end")
    dr.set_frame_lookahead(1)


def test_ldr_is_the_tonemap_of_the_result(dr, cover, oracle):
    sc, W, H, S, wants = cover
    prepare(dr, sc, W, H, 8, 8)
    dr.resolve()
    ldr_before = dr.download()[1]
    dr.denoise()
    d = check(dr, wants[("defaults", 3)][1], "defaults")
    rgb = d["rgb"].reshape(-1, 3)
    want = np.zeros((rgb.shape[0], 3), np.uint8)
    out = (C.c_uint8 * 3)()
    lib = oracle.lib()
    for i in range(rgb.shape[0]):
        lib.orc_tonemap((C.c_float * 3)(*[float(v) for v in rgb[i]]), 1, out)
        want[i] = list(out)
    assert np.array_equal(d["ldr"].reshape(-1, 3), want)
    assert np.array_equal(dr.download()[1], ldr_before) and (d["ldr"] != ldr_before).any()  # the picture's own LDR strip is not touched


def rel_mse(x, ref):
    x, ref = x.astype(np.float64), ref.astype(np.float64)
    return float(np.mean((x - ref) ** 2 / (ref ** 2 + 0.01)))


def test_quality_against_1024_spp(dr, scenes_mod):
    """Cover scene, 240 x 160, seed 1, depth 50, samples 1..4, the defaults, against samples 1..1024 of the same render (never the
    filter's own output).  MSE and relative MSE mean((x - ref)^2 / (ref^2 + 0.01)) must each fall to at most 0.65 of the raw 4-spp
    mean's.  A numpy prototype over the CPU oracle's strips measured 0.53 and 0.47; the path is deterministic."""
    W, H = 240, 160
    sc = scenes_mod.build_scene("cover", 1, W, H)
    prepare(dr, sc, W, H, 4, 4)
    raw = dr.download(ldr=False)[0] / np.float32(4)
    dr.denoise()
    den = dr.download_denoised()["rgb"]
    dr.render(W, H, 5, 1025, 50, 1)
    ref = dr.download(ldr=False)[0] / np.float32(1024)
    mse = lambda x: float(np.mean((x.astype(np.float64) - ref.astype(np.float64)) ** 2))
    r_mse, r_rel = mse(den) / mse(raw), rel_mse(den, ref) / rel_mse(raw, ref)
    print("denoise quality 240x160 4 spp: MSE %.5f -> %.5f (x %.3f), relMSE %.5f -> %.5f (x %.3f)"
          % (mse(raw), mse(den), r_mse, rel_mse(raw, ref), rel_mse(den, ref), r_rel))
    assert r_mse <= 0.65 and r_rel <= 0.65, (r_mse, r_rel)


DEVICE_COPY_CHILD = """
import sys
import numpy as np
import torch
torch.cuda.init()  # torch's HIP runtime first, as in bench.py: the library then shares it
sys.path.insert(0, sys.argv[1])
from cpuraytracer_amd import HipRenderer, scenes
W, H = 96, 64
r = HipRenderer(0)
r.upload(scenes.build_scene("cover", 1, W, H))
r.set_noise_estimate(True)
r.render(W, H, 1, 9, 50, 1)
r.render_features(W, H, 1, 9)
r.denoise()
rgb_t = torch.full((H, W, 3), -1.0, dtype=torch.float32, device="cuda:0")
var_t = torch.full((H, W), -1.0, dtype=torch.float32, device="cuda:0")
ldr_t = torch.full((H, W, 3), 7, dtype=torch.uint8, device="cuda:0")
only_var = torch.zeros_like(var_t)
torch.cuda.synchronize()
r.copy_denoised_to_device(rgb_t.data_ptr(), var_t.data_ptr(), ldr_t.data_ptr())
r.copy_denoised_to_device(None, only_var.data_ptr(), None)  # any pointer may be absent
r.synchronize()
d = r.download_denoised()
np.savez(sys.argv[2], rgb_t=rgb_t.cpu().numpy(), var_t=var_t.cpu().numpy(), ldr_t=ldr_t.cpu().numpy(), only_var=only_var.cpu().numpy(), **d)
r.close()
"""


def test_python_views_and_device_copy(built, cover, tmp_path):
    """In a process of its own: torch has to bring up its HIP runtime before the library opens the device (bench.py's order)."""
    sc, W, H, S, wants = cover
    out = str(tmp_path / "copy.npz")
    p = subprocess.run([sys.executable, "-c", DEVICE_COPY_CHILD, ROOT, out], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    z = np.load(out)
    want = wants[("defaults", 3)][1]
    assert z["rgb"].shape == (H, W, 3) and z["rgb"].dtype == np.float32 and z["var"].shape == (H, W) and z["var"].dtype == np.float32
    assert z["ldr"].shape == (H, W, 3) and z["ldr"].dtype == np.uint8
    assert_same_bits(z["rgb"], want[0], "download_denoised: rgb")
    assert_same_bits(z["var"], want[1], "download_denoised: var")
    assert_same_bits(z["rgb_t"], z["rgb"], "device copy: rgb")
    assert_same_bits(z["var_t"], z["var"], "device copy: var")
    assert_same_bits(z["only_var"], z["var"], "device copy, var alone")
    assert np.array_equal(z["ldr_t"], z["ldr"])


def test_cli_denoise_out(dr, cover, tmp_path):
    sc, W, H, S, wants = cover
    ppm, plain, den = str(tmp_path / "a.ppm"), str(tmp_path / "b.ppm"), str(tmp_path / "x.ppm")
    base = [CLI, "--width", str(W), "--height", str(H), "--spp", "8", "--frame-spp", "8", "--quiet"]
    p = subprocess.run(base + ["--out", ppm, "--denoise-out", den], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    p = subprocess.run(base + ["--out", plain], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    assert open(ppm, "rb").read() == open(plain, "rb").read()  # --out is the file written without the option
    prepare(dr, sc, W, H, 8, 8)
    dr.denoise()
    d = check(dr, wants[("defaults", 3)][1], "defaults")
    head = b"P6\n%d %d\n255\n" % (W, H)
    data = open(den, "rb").read()
    assert data.startswith(head) and data[len(head):] == d["ldr"].tobytes()
    assert data != open(ppm, "rb").read()
    # --denoise-levels reaches the filter
    p = subprocess.run(base + ["--out", ppm, "--denoise-out", den, "--denoise-levels", "1"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    dr.denoise(params_struct(dict(levels=1)))
    assert open(den, "rb").read()[len(head):] == dr.download_denoised()["ldr"].tobytes()
    # several GPUs: refused with a message, nothing rendered
    p = subprocess.run([CLI, "--gpus", "1", "--width", "8", "--height", "8", "--spp", "2", "--denoise-out", den], capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 2 and "--gpus" in p.stderr and "--denoise-out" in p.stderr
