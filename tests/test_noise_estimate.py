"""Noise estimate on the device (rt_set_noise_estimate; csrc/rt_noise.h, rt_kernels.h rt_accumulate_moments_kernel): the strip of
second moments against the oracle's per-sample radiances, the same bits along every route an accumulation can take, the error map
against the host twin, the order-independent summary against numpy, the sequencing rules, the stop rule and the CLI."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_noise_estimate_cpu import assert_same_bits, host_estimate, np_estimate, sequential_sums

pytestmark = pytest.mark.gpu

RT_ERR_SEQUENCE = 6
FLOOR = 0.01
CLI = os.path.join(ROOT, "cpuraytracer_amd", "lib", "spheres")


@pytest.fixture(scope="module")
def scenes_mod(built):
    from cpuraytracer_amd import scenes
    return scenes


@pytest.fixture()
def nr(built):
    """A context of its own: the switches these tests flip never reach the session's renderer."""
    from cpuraytracer_amd import HipRenderer
    r = HipRenderer(0)
    yield r
    r.close()


def same_u32(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape, what
    bad = a.view(np.uint32) != b.view(np.uint32)
    assert not bad.any(), "%s: %d of %d floats differ, first at %s" % (what, int(bad.sum()), bad.size, np.argwhere(bad)[0])


def oracle_strips(oracle, sc, W, H, rows, s0, s1, depth, seed):
    """hdr and sq of the global rows `rows`, from the oracle's per-sample radiances added sequentially in binary32."""
    orc = oracle.Oracle()
    orc.upload(sc)
    jj, ii = np.meshgrid(np.asarray(rows), np.arange(W), indexing="ij")
    planes = []
    for s in range(s0, s1):
        ijs = np.stack([ii.ravel(), jj.ravel(), np.full(ii.size, s)], axis=1).astype(np.uint32)
        planes.append(orc.trace(W, H, ijs, depth, seed)[0])
    orc.close()
    S, Q = sequential_sums(np.stack(planes))
    return S.reshape(len(rows), W, 3), Q.reshape(len(rows), W, 3)


def strips(r):
    r.synchronize()
    return r.download(ldr=False)[0], r.download_moments()


def test_moments_equal_the_oracles_samples(nr, oracle, scenes_mod):
    W, H, spp, depth, seed = 96, 64, 16, 50, 1
    sc = scenes_mod.build_scene("cover", 1, W, H)
    nr.upload(sc)
    nr.set_noise_estimate(True)
    nr.render(W, H, 1, 1 + spp, depth, seed)
    nr.resolve()
    hdr, ldr = nr.download()
    sq = nr.download_moments()
    So, Qo = oracle_strips(oracle, sc, W, H, range(H), 1, 1 + spp, depth, seed)
    same_u32(hdr, So, "hdr vs the oracle's samples")
    same_u32(sq, Qo, "sq vs the oracle's samples")
    assert (sq > 0).any()
    # the switch changes nothing that existed: hdr and the LDR bytes of a render without it
    nr.set_noise_estimate(False)
    nr.render(W, H, 1, 1 + spp, depth, seed)
    nr.resolve()
    hdr0, ldr0 = nr.download()
    same_u32(hdr, hdr0, "hdr with the switch on vs off")
    assert np.array_equal(ldr, ldr0)


def test_short_last_tile(nr, oracle, scenes_mod):
    """50 x 37 = 1850 pixels = 28 tiles of 64 and one of 58: the last tile's planes are 58 pixels apart."""
    W, H, spp, depth, seed = 50, 37, 16, 50, 1
    assert (W * H) % 64 != 0
    sc = scenes_mod.build_scene("cover", 1, W, H)
    nr.upload(sc)
    nr.set_noise_estimate(True)
    nr.render(W, H, 1, 1 + spp, depth, seed)
    hdr, sq = strips(nr)
    So, Qo = oracle_strips(oracle, sc, W, H, range(H), 1, 1 + spp, depth, seed)
    same_u32(hdr, So, "ragged image: hdr vs the oracle's samples")
    same_u32(sq, Qo, "ragged image: sq vs the oracle's samples")
    # ... and through the add-only launches of render-ahead (first / count) and a continued accumulation
    nr.set_frame_lookahead(4)
    for s in range(1, 1 + spp):
        nr.render(W, H, s, s + 1, depth, seed, stats=False)
    h2, q2 = strips(nr)
    nr.set_frame_lookahead(1)
    same_u32(h2, hdr, "ragged image, render-ahead: hdr")
    same_u32(q2, sq, "ragged image, render-ahead: sq")
    nr.render(W, H, 1, 6, depth, seed)
    nr.render(W, H, 6, 1 + spp, depth, seed)
    h3, q3 = strips(nr)
    same_u32(h3, hdr, "ragged image, two calls: hdr")
    same_u32(q3, sq, "ragged image, two calls: sq")


def test_same_bits_along_every_route(nr, scenes_mod):
    from cpuraytracer_amd import _capi
    W, H, depth, seed = 192, 128, 50, 1
    sc = scenes_mod.build_scene("cover", 1, W, H)
    nr.upload(sc)
    nr.set_noise_estimate(True)
    st = nr.render(W, H, 1, 17, depth, seed)
    assert st.passes == 1
    hdr, sq = strips(nr)
    assert (sq > 0).any()

    def check(what):
        h, q = strips(nr)
        same_u32(h, hdr, what + ": hdr")
        same_u32(q, sq, what + ": sq")

    nr.render(W, H, 1, 6, depth, seed)
    nr.render(W, H, 6, 17, depth, seed)
    check("calls 1..6 and 6..17")

    nr.set_workspace_limit(1 << 20)  # 192 * 128 * 12 bytes per sample plane: three planes per pass
    st = nr.render(W, H, 1, 17, depth, seed)
    assert st.passes >= 3
    check("%d passes" % st.passes)
    nr.set_workspace_limit(8 << 30)

    nr.set_frame_batch(4)
    for s in range(1, 17):
        nr.render(W, H, s, s + 1, depth, seed, stats=False)
        if s == 6:  # the readers hand out the committed strips while frames 5, 6 are pending: sq stays in step with hdr
            assert nr.committed_samples() == 4
            h, q = nr.download(ldr=False)[0], nr.download_moments()
    check("frame batch of 4")
    nr.set_frame_batch(1)
    nr.render(W, H, 1, 5, depth, seed)
    h4, q4 = strips(nr)
    same_u32(h, h4, "frame batch, mid-stream: hdr")
    same_u32(q, q4, "frame batch, mid-stream: sq")

    nr.set_frame_lookahead(4)
    for s in range(1, 17):
        nr.render(W, H, s, s + 1, depth, seed, stats=False)
        if s == 6:  # two of the four planes traced ahead are in the strips, two wait in the sample buffer
            h, q = nr.download(ldr=False)[0], nr.download_moments()
    check("render-ahead of 4")
    nr.set_frame_lookahead(1)
    nr.render(W, H, 1, 7, depth, seed)
    h6, q6 = strips(nr)
    same_u32(h, h6, "render-ahead, mid-stream: hdr")
    same_u32(q, q6, "render-ahead, mid-stream: sq")

    nr.set_frame_pipelining(4)  # with the switch on every call renders unpipelined, silently
    for s in range(1, 17):
        nr.render(W, H, s, s + 1, depth, seed, stats=False)
        assert nr.committed_samples() == s
    check("frame pipelining of 4 (falls back)")
    nr.set_frame_pipelining(0)

    # two shards of single rows, stitched by rt_rowset_global_row
    L = _capi.load()
    fh, fq = np.zeros_like(hdr), np.zeros_like(sq)
    for shard in (0, 1):
        rs = _capi.cyclic_rows(H, shard, 2)
        nr.render(W, H, 1, 17, depth, seed, rowset=rs)
        h, q = strips(nr)
        assert h.shape[0] == q.shape[0] == H // 2
        for lr in range(h.shape[0]):
            gr = L.rt_rowset_global_row(rs, lr)
            fh[gr], fq[gr] = h[lr], q[lr]
    same_u32(fh, hdr, "two cyclic shards: hdr")
    same_u32(fq, sq, "two cyclic shards: sq")


def test_map_and_summary(nr, scenes_mod):
    W, H, spp, depth, seed = 96, 64, 16, 50, 1
    nr.upload(scenes_mod.build_scene("cover", 1, W, H))
    nr.set_noise_estimate(True)
    nr.render(W, H, 1, 1 + spp, depth, seed)
    hdr, sq = strips(nr)
    for floor in (FLOOR, 0.0, 2.0):
        m = nr.noise_map(floor=floor)
        assert m.shape == (H, W, 2)
        assert_same_bits(m.reshape(-1, 2), host_estimate(hdr, sq, spp, floor), "rt_noise_map vs the host twin, floor %g" % floor)
        assert_same_bits(m, np_estimate(hdr, sq, spp, floor), "rt_noise_map vs numpy, floor %g" % floor)
        rel = m[..., 1].ravel()
        fin = np.isfinite(rel)
        thr = np.array([0.0, 1e-6, 0.01, 0.05, 0.1, 0.2, 0.5, 10.0], dtype=np.float32)
        want = np.array([int((~fin | (rel > t)).sum()) for t in thr], dtype=np.uint32)
        want_max = np.float32(rel[fin].max()) if fin.any() else np.float32(0)
        answers = [nr.noise_summary(thr, floor=floor) for _ in range(3)]
        for counts, mx in answers:
            assert np.array_equal(counts, want), (counts, want)
            assert np.float32(mx).view(np.uint32) == want_max.view(np.uint32)
        assert floor != FLOOR or (0 < want[5] < W * H and want[7] == 0)  # a picture at 16 spp: some pixels noisy, none absurd
    counts, mx = nr.noise_summary([], floor=FLOOR)
    assert counts.shape == (0,) and mx > 0
    with pytest.raises(Exception) as e:
        nr.noise_summary(np.zeros(9), floor=FLOOR)
    assert e.value.code == 2  # RT_ERR_INVALID_ARG: at most 8 thresholds


def test_sequencing(nr, scenes_mod):
    from cpuraytracer_amd import RtError
    W, H, depth, seed = 96, 64, 8, 1
    nr.upload(scenes_mod.build_scene("three", 1, W, H))

    def refused(fn):
        with pytest.raises(RtError) as e:
            fn()
        assert e.value.code == RT_ERR_SEQUENCE, e.value
    readers = (nr.download_moments, nr.noise_map, lambda: nr.noise_summary([0.1]))

    nr.render(W, H, 1, 4, depth, seed)  # the default is off
    for fn in readers:
        refused(fn)
    nr.set_noise_estimate(True)  # voids the accumulation: nothing to read, nothing to continue
    for fn in readers:
        refused(fn)
    refused(lambda: nr.render(W, H, 4, 5, depth, seed))
    nr.render(W, H, 1, 2, depth, seed)  # one sample: moments exist, the estimate does not
    assert nr.download_moments().shape == (H, W, 3)
    refused(nr.noise_map)
    refused(lambda: nr.noise_summary([0.1]))
    nr.render(W, H, 2, 3, depth, seed)
    assert nr.noise_map().shape == (H, W, 2)
    nr.noise_summary([0.1])
    nr.set_noise_estimate(True)  # no change: the accumulation goes on
    nr.render(W, H, 3, 4, depth, seed)
    nr.clear()
    for fn in readers:
        refused(fn)
    nr.render(W, H, 1, 3, depth, seed)
    nr.noise_map()
    nr.set_noise_estimate(False)  # toggled in the middle: the next continuing call fails, as after rt_set_sampler
    refused(lambda: nr.render(W, H, 3, 4, depth, seed))
    nr.render(W, H, 1, 3, depth, seed)
    refused(nr.download_moments)
    nr.upload(scenes_mod.build_scene("three", 1, W, H))  # rt_scene_upload voids both strips
    nr.set_noise_estimate(True)
    nr.render(W, H, 1, 3, depth, seed)
    nr.upload(scenes_mod.build_scene("three", 1, W, H))
    for fn in readers:
        refused(fn)


def test_stop_rule(nr, scenes_mod):
    """rel_error 0.2 / fraction 0.02 on the cover scene at 96 x 64: the oracle's samples put 2.7 % of the pixels above 0.2 at 16 spp and
    1.8 % at 20 spp, so the loop has to take five steps of four and stop on the criterion, well inside max_spp."""
    W, H, depth, seed = 96, 64, 50, 1
    rel_error, fraction, step, max_spp = 0.2, 0.02, 4, 64
    nr.upload(scenes_mod.build_scene("cover", 1, W, H))
    spp = nr.render_until(W, H, depth, seed, rel_error, fraction=fraction, step_spp=step, max_spp=max_spp, floor=FLOOR)
    assert spp % step == 0 and 2 * step <= spp < max_spp, spp
    counts, _ = nr.noise_summary([rel_error], floor=FLOOR)  # the strips the loop left behind are those of `spp` samples
    assert nr.committed_samples() == spp

    def fraction_above(n):
        nr.render(W, H, 1, 1 + n, depth, seed)
        hdr, sq = strips(nr)
        rel = np_estimate(hdr, sq, n, FLOOR)[..., 1]
        return int((~np.isfinite(rel) | (rel > np.float32(rel_error))).sum()) / (W * H)
    at, before = fraction_above(spp), fraction_above(spp - step)
    print("stop rule: spp %d, fraction above %.4f (%.4f one step earlier), limit %.4f" % (spp, at, before, fraction))
    assert at == int(counts[0]) / (W * H)
    assert at <= fraction < before
    # max_spp ends the loop where the criterion cannot
    assert nr.render_until(W, H, depth, seed, 1e-6, fraction=0.0, step_spp=3, max_spp=10, floor=FLOOR) == 9


def test_cli_noise_options(nr, scenes_mod, tmp_path):
    W, H, spp, depth = 200, 100, 4, 8
    pfm, ppm = str(tmp_path / "noise.pfm"), str(tmp_path / "c1.ppm")
    p = subprocess.run([CLI, "--scene", "three", "--width", str(W), "--height", str(H), "--spp", str(spp), "--frame-spp", str(spp), "--depth", str(depth),
                        "--out", ppm, "--noise-out", pfm, "--quiet"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    nr.upload(scenes_mod.build_scene("three", 1, W, H))
    nr.set_noise_estimate(True)
    nr.render(W, H, 1, 1 + spp, depth, 1)
    nr.resolve()
    m = nr.noise_map()
    head = b"Pf\n%d %d\n-1.0\n" % (W, H)
    data = open(pfm, "rb").read()
    assert data.startswith(head)
    assert data[len(head):] == np.ascontiguousarray(m[..., 0]).tobytes()
    assert (m[..., 0] > 0).any()
    assert open(ppm, "rb").read()[len(b"P6\n200 100\n255\n"):] == nr.download()[1].tobytes()

    # --target-error: the loop of render_until, stepping by --frame-spp
    W, H, depth = 96, 64, 50
    p = subprocess.run([CLI, "--scene", "cover", "--width", str(W), "--height", str(H), "--frame-spp", "4", "--depth", str(depth), "--target-error", "0.2",
                        "--target-fraction", "0.02", "--max-spp", "64", "--out", ppm, "--quiet"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    reached = [json.loads(l) for l in p.stdout.splitlines() if "spp_reached" in l]
    assert len(reached) == 1
    nr.upload(scenes_mod.build_scene("cover", 1, W, H))
    assert reached[0]["spp_reached"] == nr.render_until(W, H, depth, 1, 0.2, fraction=0.02, step_spp=4, max_spp=64, floor=FLOOR)
    nr.resolve()
    assert open(ppm, "rb").read()[len(b"P6\n96 64\n255\n"):] == nr.download()[1].tobytes()

    # several GPUs: refused with a message, nothing rendered
    for extra in (["--noise-out", pfm], ["--target-error", "0.2"]):
        p = subprocess.run([CLI, "--gpus", "2", "--width", "8", "--height", "8", "--spp", "2"] + extra, capture_output=True, text=True, timeout=120)
        assert p.returncode == 2 and "--gpus" in p.stderr and "second moments" in p.stderr
