"""Feature buffers on the device (rt_render_features; csrc/rt_features.h, rt_kernels.h rt_features_kernel): first-hit albedo, normal,
depth, coverage and object id against the oracle's own composition (its primary rays -> its list scan -> its Texture::Evaluate, summed
sequentially in binary32), bit for bit: along every route a sample range can be split, on ragged shapes and row sets, through every
scan variant, with a lens and both disk mappings, with a hollow sphere; the sequencing rules; independence from rt_render in both
directions; the device copy, the Python views and the CLI."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_feature_buffers_cpu import NO_ID, oracle_features, same_bits

pytestmark = pytest.mark.gpu

RT_ERR_INVALID_ARG, RT_ERR_SEQUENCE = 2, 6
CLI = os.path.join(ROOT, "cpuraytracer_amd", "lib", "spheres")


@pytest.fixture(scope="module")
def scenes_mod(built):
    from cpuraytracer_amd import scenes
    return scenes


@pytest.fixture()
def fr(built):
    """A context of its own: the switches these tests flip never reach the session's renderer."""
    from cpuraytracer_amd import HipRenderer
    r = HipRenderer(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def cover(scenes_mod, oracle):
    """The cover scene at 96 x 64 and the oracle's strips after samples 1..8 (computed once, never changed)."""
    W, H = 96, 64
    sc = scenes_mod.build_scene("cover", 1, W, H)
    feat, ids = oracle_features(oracle, sc, W, H, range(H), 1, 9)
    feat.setflags(write=False)
    ids.setflags(write=False)
    return sc, W, H, (feat, ids)


def raw(r):
    """The strips as the C ABI hands them out: feat [rows, W, 8], id [rows, W]."""
    d = r.download_features()
    feat = np.concatenate([d["albedo"], d["normal"], d["depth"][..., None], d["coverage"][..., None]], axis=-1)
    return np.ascontiguousarray(feat), d["id"]


def check(r, want, what):
    feat, ids = raw(r)
    same_bits(feat, want[0], what + ": feat")
    assert np.array_equal(ids, want[1]), what + ": id"


def test_equal_to_the_oracle(fr, cover):
    sc, W, H, want8 = cover
    fr.upload(sc)
    assert fr.feature_samples() == 0
    fr.render_features(W, H, 1, 9)
    assert fr.feature_samples() == 8
    check(fr, want8, "cover, samples 1..8")
    feat, ids = want8
    # not vacuous: hits and misses, partly covered pixels, every kind of albedo, an id that depends on the last sample
    cov = feat[..., 7]
    assert (cov == 0).any() and (cov == 8).any() and ((cov > 0) & (cov < 8)).any()
    kinds = {(int(m["type"]), int(m["tex_type"])) for m in sc.materials[np.unique(ids[ids != NO_ID])]}
    assert {(0, 0), (0, 1), (1, 0), (2, 0)} <= kinds, kinds
    assert (ids == NO_ID).any() and len(np.unique(ids)) > 10


def test_same_bits_along_every_route(fr, cover):
    sc, W, H, want8 = cover
    fr.upload(sc)
    for timed in (False, True):
        ms = fr.render_features(W, H, 1, 9, timed=timed)
        assert (ms is not None and ms > 0.0) if timed else ms is None
        check(fr, want8, "1..9 in one call, timed=%s" % timed)
        fr.render_features(W, H, 1, 4, timed=timed)
        fr.render_features(W, H, 4, 9, timed=timed)
        assert fr.feature_samples() == 8
        check(fr, want8, "1..4 then 4..9, timed=%s" % timed)
        for s in range(1, 9):
            fr.render_features(W, H, s, s + 1, timed=timed)
        assert fr.feature_samples() == 8
        check(fr, want8, "eight one-sample calls, timed=%s" % timed)


@pytest.mark.parametrize("W,H,rs", [(100, 37, None), (7, 3, None), (96, 64, (3, 30, 4, 1, 3))], ids=["100x37", "7x3", "rowset"])
def test_ragged_shapes(fr, oracle, scenes_mod, W, H, rs):
    """3,700 pixels: the last wave is partial; 21 pixels: less than one wave; a strip of a sharded row set: local != global rows."""
    from cpuraytracer_amd import _capi
    sc = scenes_mod.build_scene("cover", 1, W, H)
    fr.upload(sc)
    rowset = _capi.RtRowset(*rs) if rs else None
    L = _capi.load()
    rows = [L.rt_rowset_global_row(rowset, k) for k in range(L.rt_rowset_local_rows(rowset))] if rs else list(range(H))
    if rs:
        assert rows == [7, 8, 9, 10, 19, 20, 21, 22, 31, 32]  # blocks 1, 4, 7 of four rows from row 3 on (block 7 is cut at row 33)
    fr.render_features(W, H, 1, 3, rowset=rowset)
    fr.render_features(W, H, 3, 5, rowset=rowset)
    want = oracle_features(oracle, sc, W, H, rows, 1, 5)
    check(fr, want, "%d x %d" % (W, H))
    assert (want[0][..., 7] > 0).any() and (want[0][..., 7] == 0).any()


VARIANTS = [
    ("cover", 96, 64, 8, {}),                                # flat matrix-core filter, tables in LDS
    ("cover", 96, 64, 8, {"RT_SCAN": "valu"}),               # VALU scan, tables in LDS
    ("cover", 96, 64, 8, {"RT_FORCE_GLOBAL_TABLES": "1"}),   # VALU scan, tables in global memory
    ("cover", 96, 64, 8, {"RT_GRID": "2"}),                  # cell grid over a small scene
    ("grid10k", 128, 128, 2, {}),                            # cell grid
    ("grid10k", 128, 128, 2, {"RT_GRID": "0"}),              # bounds hierarchy
    ("three", 64, 32, 4, {}),
]


@pytest.fixture(scope="module")
def variant_wants(scenes_mod, oracle, cover):
    """The oracle's strips per (scene, size, spp) of VARIANTS, computed once."""
    out = {("cover", 96, 64, 8): (cover[0], cover[3])}
    for name, W, H, spp, _ in VARIANTS:
        if (name, W, H, spp) not in out:
            sc = scenes_mod.build_scene(name, 1, W, H)
            out[(name, W, H, spp)] = (sc, oracle_features(oracle, sc, W, H, range(H), 1, 1 + spp))
    return out


@pytest.mark.parametrize("name,W,H,spp,env", VARIANTS, ids=["%s-%s" % (v[0], "-".join("%s=%s" % kv for kv in v[4].items()) or "default") for v in VARIANTS])
def test_every_scan_variant(built, monkeypatch, variant_wants, name, W, H, spp, env):
    from cpuraytracer_amd import HipRenderer
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sc, want = variant_wants[(name, W, H, spp)]
    r = HipRenderer(0)  # the knobs are read at rt_create and at rt_scene_upload
    try:
        r.upload(sc)
        r.render_features(W, H, 1, 1 + spp)
        check(r, want, "%s %s" % (name, env))
    finally:
        r.close()
    assert (want[0][..., 7] > 0).any() and (want[0][..., 7] == 0).any()


@pytest.mark.parametrize("flags", [0, 2], ids=["linear-disk", "sqrt-disk"])
def test_lens_and_sampler(fr, oracle, scenes_mod, flags):
    from cpuraytracer_amd import _capi
    W, H, spp = 96, 64, 4
    sc = scenes_mod.build_scene("cover", 1, W, H, aperture=2.0)
    assert sc.camera.aperture == 2.0
    fr.upload(sc)
    fr.set_sampler(flags)
    fr.render_features(W, H, 1, 1 + spp)
    wants = {}
    try:
        for f in (0, 2):
            oracle.lib().orc_set_sampler(f)
            wants[f] = oracle_features(oracle, sc, W, H, range(H), 1, 1 + spp) if f == flags else oracle_features(oracle, sc, W, H, range(28, 36), 1, 2)
    finally:
        oracle.lib().orc_set_sampler(0)
    check(fr, wants[flags], "aperture 2.0, sampler flags %d" % flags)
    # the flag moves the lens offsets, and at this aperture that shows: one sample of the middle rows differs between the mappings
    oracle.lib().orc_set_sampler(flags)
    try:
        mine = oracle_features(oracle, sc, W, H, range(28, 36), 1, 2)
    finally:
        oracle.lib().orc_set_sampler(0)
    assert not np.array_equal(mine[0], wants[2 - flags][0])
    # unchanged flags change nothing; changed flags void the strips in the middle of an accumulation
    fr.set_sampler(flags)
    fr.render_features(W, H, 1 + spp, 2 + spp)
    assert fr.feature_samples() == spp + 1
    fr.set_sampler(2 - flags)
    assert fr.feature_samples() == 0
    with pytest.raises(_capi.RtError) as e:
        fr.render_features(W, H, 2 + spp, 3 + spp)
    assert e.value.code == RT_ERR_SEQUENCE


def test_signed_radius(fr, oracle, scenes_mod):
    """A hollow sphere (r < 0) in view: the normal plane is the oracle's, turned inward; depth and id do not depend on the sign."""
    W, H = 64, 32
    sc = scenes_mod.build_scene("three", 1, W, H)
    assert sc.n == 3
    solid = oracle_features(oracle, sc, W, H, range(H), 1, 2)
    seen = np.unique(solid[1][solid[1] != NO_ID])
    k = int(seen[np.argmax([(solid[1] == q).sum() for q in seen])])  # the sphere that covers most pixels
    sc.spheres = sc.spheres.copy()
    sc.spheres["r"][k] = -sc.spheres["r"][k]
    assert sc.spheres["r"][k] < 0
    hollow1 = oracle_features(oracle, sc, W, H, range(H), 1, 2)
    on = hollow1[1] == k
    assert on.sum() > 50
    # one sample decides these strips: the oracle's normals on the hollow sphere are the solid one's negated, everything else is equal
    assert np.array_equal(hollow1[0][on][:, 3:6], -solid[0][on][:, 3:6]) and (hollow1[0][on][:, 3:6] != 0).any()
    same_bits(hollow1[0][..., 6], solid[0][..., 6], "depth does not depend on the sign")
    assert np.array_equal(hollow1[1], solid[1])
    fr.upload(sc)
    fr.render_features(W, H, 1, 2)
    check(fr, hollow1, "hollow sphere, one sample")
    fr.render_features(W, H, 2, 4)
    check(fr, oracle_features(oracle, sc, W, H, range(H), 1, 4), "hollow sphere, three samples")


def test_sequencing(fr, cover, scenes_mod):
    from cpuraytracer_amd import _capi
    sc, W, H, want8 = cover
    L = fr._L

    def refused(fn, code=RT_ERR_SEQUENCE):
        with pytest.raises(_capi.RtError) as e:
            fn()
        assert e.value.code == code, e.value
        assert L.rt_last_error()

    fr.upload(sc)
    refused(lambda: fr.download_features())                      # download before any render
    refused(lambda: fr.copy_features_to_device(None, None))
    refused(lambda: fr.render_features(W, H, 3, 5))              # a first call must start at 1 (or follow rt_clear_features)
    # argument errors
    refused(lambda: fr.render_features(W, H, 0, 4), RT_ERR_INVALID_ARG)
    refused(lambda: fr.render_features(W, H, 4, 4), RT_ERR_INVALID_ARG)
    refused(lambda: fr.render_features(W, H, 5, 4), RT_ERR_INVALID_ARG)
    refused(lambda: fr.render_features(0, H, 1, 2), RT_ERR_INVALID_ARG)
    refused(lambda: fr.render_features(W, 0, 1, 2), RT_ERR_INVALID_ARG)
    fr.render_features(W, H, 1, 5)
    refused(lambda: fr.render_features(W, H, 6, 9))              # a gap
    refused(lambda: fr.render_features(W, H, 4, 9))              # an overlap
    refused(lambda: fr.render_features(W, H, 2, 5))              # a repeated range (not from 1)
    refused(lambda: fr.render_features(W + 1, H, 5, 9))          # another W
    refused(lambda: fr.render_features(W, H - 1, 5, 9))          # another H
    refused(lambda: fr.render_features(W, H, 5, 9, rowset=_capi.RtRowset(0, H, 1, 0, 2)))  # another row set
    assert fr.feature_samples() == 4                            # a refused call changes nothing
    fr.render_features(W, H, 5, 9)
    check(fr, want8, "continued after refused calls")
    # rt_clear (and a render) do not touch the strips
    fr.clear()
    check(fr, want8, "after rt_clear")
    assert fr.feature_samples() == 8
    # rt_clear_features restarts at any s0
    fr.clear_features()
    assert fr.feature_samples() == 0
    refused(lambda: fr.download_features())
    fr.render_features(W, H, 9, 10)
    assert fr.feature_samples() == 1
    refused(lambda: fr.render_features(W, H, 9, 10))             # the clear was used up: the same range again does not continue
    fr.render_features(W, H, 10, 11)
    assert fr.feature_samples() == 2
    # rt_scene_upload voids the strips
    fr.render_features(W, H, 1, 3)
    fr.upload(scenes_mod.build_scene("three", 1, W, H))
    assert fr.feature_samples() == 0
    refused(lambda: fr.download_features())
    refused(lambda: fr.render_features(W, H, 3, 4))
    fr.render_features(W, H, 1, 2)
    assert fr.feature_samples() == 1


@pytest.mark.parametrize("mode", ["plain", "batch", "lookahead", "pipelining"])
def test_independent_of_rt_render(fr, cover, mode):
    """Eight continuing 1-spp rt_render calls with a feature call between every two: the picture is the one without feature calls and
    the one-shot render; the feature strips are those taken with no rt_render in between."""
    sc, W, H, want8 = cover
    depth, seed = 50, 1
    fr.upload(sc)
    fr.render(W, H, 1, 9, depth, seed)
    fr.resolve()
    hdr1, ldr1 = fr.download()

    def switch(on):
        if mode == "batch":
            fr.set_frame_batch(4 if on else 1)
        elif mode == "lookahead":
            fr.set_frame_lookahead(4 if on else 1)
        elif mode == "pipelining":
            fr.set_frame_pipelining(2 if on else 0)

    def frames(with_features):
        fr.clear()
        fr.clear_features()
        switch(True)
        for s in range(1, 9):
            fr.render(W, H, s, s + 1, depth, seed, stats=False)
            if with_features:
                fr.render_features(W, H, s, s + 1, timed=(s % 2 == 0))
        fr.synchronize()  # the flush
        fr.resolve()
        out = fr.download()
        switch(False)
        return out

    hdr_a, ldr_a = frames(False)
    hdr_b, ldr_b = frames(True)
    same_bits(hdr_b, hdr_a, mode + ": hdr with and without feature calls")
    assert np.array_equal(ldr_b, ldr_a)
    same_bits(hdr_b, hdr1, mode + ": hdr vs the one-shot render")
    assert np.array_equal(ldr_b, ldr1)
    assert fr.feature_samples() == 8
    check(fr, want8, mode + ": feature strips taken between rt_render calls")


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
r.render_features(W, H, 1, 9)
feat_t = torch.full((H, W, 8), -1.0, dtype=torch.float32, device="cuda:0")
id_t = torch.full((H, W), 7, dtype=torch.int32, device="cuda:0")
only_feat, only_id = torch.zeros_like(feat_t), torch.zeros_like(id_t)
torch.cuda.synchronize()
r.copy_features_to_device(feat_t.data_ptr(), id_t.data_ptr())
r.copy_features_to_device(only_feat.data_ptr(), None)  # either pointer may be absent
r.copy_features_to_device(None, only_id.data_ptr())
r.synchronize()
d = r.download_features()
feat = np.concatenate([d["albedo"], d["normal"], d["depth"][..., None], d["coverage"][..., None]], axis=-1)
np.savez(sys.argv[2], feat_t=feat_t.cpu().numpy(), id_t=id_t.cpu().numpy(), only_feat=only_feat.cpu().numpy(), only_id=only_id.cpu().numpy(),
         feat=feat, ids=d["id"])
r.close()
"""


def test_device_copy(built, cover, tmp_path):
    """In a process of its own: torch has to bring up its HIP runtime before the library opens the device (bench.py's order), and
    this session's library is loaded already."""
    import sys
    sc, W, H, want8 = cover
    out = str(tmp_path / "copy.npz")
    p = subprocess.run([sys.executable, "-c", DEVICE_COPY_CHILD, ROOT, out], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    z = np.load(out)
    same_bits(z["feat_t"], z["feat"], "device copy: feat")
    assert np.array_equal(z["id_t"].view(np.uint32), z["ids"])
    same_bits(z["only_feat"], z["feat"], "device copy, feat alone")
    assert np.array_equal(z["only_id"].view(np.uint32), z["ids"])
    same_bits(z["feat"], want8[0], "feat vs the oracle")
    assert np.array_equal(z["ids"], want8[1])


def test_python_views(fr, cover):
    sc, W, H, want8 = cover
    fr.upload(sc)
    fr.render_features(W, H, 1, 9)
    d, n = fr.download_features(normalize=True), fr.download_features()
    assert set(d) == {"albedo", "normal", "depth", "coverage", "id"}
    assert d["albedo"].shape == (H, W, 3) and d["normal"].shape == (H, W, 3) and d["depth"].shape == (H, W) and d["coverage"].shape == (H, W)
    assert d["id"].shape == (H, W) and d["id"].dtype == np.uint32
    eight = np.float32(8)
    for key, lo in (("albedo", 0), ("normal", 3)):
        assert d[key].dtype == np.float32
        same_bits(d[key], want8[0][..., lo:lo + 3] / eight, key)
        same_bits(n[key], want8[0][..., lo:lo + 3], key + " (raw)")
    same_bits(d["depth"], want8[0][..., 6] / eight, "depth")
    same_bits(d["coverage"], want8[0][..., 7] / eight, "coverage")
    assert (d["coverage"] >= 0).all() and (d["coverage"] <= 1).all() and (d["coverage"] == 1).any() and (d["coverage"] == 0).any()
    assert np.array_equal(d["id"], want8[1]) and np.array_equal(n["id"], want8[1])


def test_cli_features_out(fr, scenes_mod, tmp_path):
    W, H, spp = 96, 64, 4
    prefix, ppm = str(tmp_path / "feat"), str(tmp_path / "cover.ppm")
    p = subprocess.run([CLI, "--width", str(W), "--height", str(H), "--spp", str(spp), "--frame-spp", str(spp), "--quiet", "--out", ppm,
                        "--features-out", prefix], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    fr.upload(scenes_mod.build_scene("cover", 1, W, H))
    fr.render_features(W, H, 1, 1 + spp)
    d = fr.download_features(normalize=True)
    for key, magic in (("albedo", b"PF"), ("normal", b"PF"), ("depth", b"Pf"), ("coverage", b"Pf")):
        head = magic + b"\n%d %d\n-1.0\n" % (W, H)
        data = open("%s.%s.pfm" % (prefix, key), "rb").read()
        assert data.startswith(head), key
        assert data[len(head):] == np.ascontiguousarray(d[key]).tobytes(), key
    assert (d["coverage"] > 0).any() and (d["depth"] > 0).any()
    # the picture is the one rendered without the option
    fr.render(W, H, 1, 1 + spp, 50, 1)
    fr.resolve()
    assert open(ppm, "rb").read()[len(b"P6\n96 64\n255\n"):] == fr.download()[1].tobytes()
    # several GPUs: refused with a message, nothing rendered
    p = subprocess.run([CLI, "--gpus", "1", "--width", "8", "--height", "8", "--spp", "2", "--features-out", prefix], capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 2 and "--gpus" in p.stderr and "feature strips" in p.stderr
