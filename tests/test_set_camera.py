"""rt_set_camera on the device: a camera move without a scene upload.  The core comparison takes two contexts: A uploads the scene
with camera C0, renders something and calls set_camera(C1); B uploads the scene with C1.  From there both run the same calls, and
everything they hand out is compared bit for bit.  C1 is C0 turned 20 degrees about the look-at point, so the origin moves."""
import ctypes as C
import time

import numpy as np
import pytest

import trace_variant_cases as tvc
from temporal_common import COVER_PIVOT, NO_TARGET, orbit_scene
from test_noise_estimate_cpu import assert_same_bits

pytestmark = pytest.mark.gpu

RT_ERR_INVALID_ARG, RT_ERR_NO_SCENE, RT_ERR_SEQUENCE = 2, 3, 6
BAND = (8, 24, 24, 0, 1)  # rows 8..31 of the 96 x 64 picture as one contiguous row set (tests/test_temporal.py)
TURN = 20.0
FIELDS = [(name, k) for name in ("origin", "x", "y", "origin_image_plane") for k in range(3)] + [("aperture", None), ("focal_length", None)]


@pytest.fixture(scope="module")
def scenes(built):
    from cpuraytracer_amd import scenes
    return scenes


@pytest.fixture()
def ctxs(built):
    """Contexts of the test's own, closed afterwards."""
    from cpuraytracer_amd import HipRenderer
    made = []

    def make():
        made.append(HipRenderer(0))
        return made[-1]
    yield make
    for r in made:
        r.close()


def rowset_of(rs):
    from cpuraytracer_amd import _capi
    return _capi.RtRowset(*rs) if rs else None


def turned(scenes, camera, degrees=TURN):
    return scenes.orbit_camera(camera, degrees, COVER_PIVOT)


def with_camera(sc, camera):
    import copy
    out = copy.copy(sc)
    out.camera = camera
    return out


def cam_bytes(cam):
    return bytes(cam)


def code_of(fn, *args, **kw):
    from cpuraytracer_amd import _capi
    try:
        fn(*args, **kw)
    except _capi.RtError as e:
        return e.code, str(e)
    return 0, ""


def tile_tables(r, W, H, rs):
    """The masks and the lists the unit entries hand out for the picture (lists: up to each tile's count)."""
    from cpuraytracer_amd import _capi
    L = _capi.load()
    rs = rowset_of(rs) or _capi.whole_image(H)
    cap = (W * L.rt_rowset_local_rows(rs)) >> 6
    words = np.zeros((max(cap, 1), 8), dtype=np.uint32)
    gos = np.zeros(20000, dtype=np.uint32)
    n = C.c_uint32(0)
    _capi.check(L.rt_unit_tile_masks(r._h, W, H, rs, cap, C.byref(n), words.ctypes.data, gos.shape[0], gos.ctypes.data, None))
    nm = n.value
    lists = np.zeros((max(cap, 1), 64), dtype=np.uint16)
    _capi.check(L.rt_unit_tile_spheres(r._h, W, H, rs, cap, C.byref(n), lists.ctypes.data, None))
    lists = lists[:n.value].copy()
    for t in range(lists.shape[0]):  # (the slots behind a count are unspecified)
        cnt = int(lists[t, 0])
        lists[t, 1 + (0 if cnt == 0xffff else cnt):] = 0
    return {"mask_tiles": np.array([nm]), "masks": words[:nm].copy(), "groups": gos, "list_tiles": np.array([lists.shape[0]]), "lists": lists}


def everything(r, W, H, rs, spp, depth, seed, tables=False, temporal=True):
    """One accumulation with statistics, its resolve, the feature pass, the denoise family and some unit entries: all that is compared."""
    out = {}
    st = r.render(W, H, 1, 1 + spp, depth, seed, rowset=rowset_of(rs))
    out["stats"] = np.array([st.samples, st.traversals, st.segments, st.local_rows, st.passes], dtype=np.uint64)
    launch = r.last_trace_launch()
    out["launch"] = launch
    out["kernel"] = tuple((f, getattr(launch, f)) for f in launch._fields if f in ("row", "lights") or f.startswith("k"))  # the kernel variant
    out["far_state"] = r.last_trace_far_state()
    r.resolve()
    out["hdr"], out["ldr"] = r.download()
    out["sq"] = r.download_moments()
    r.render_features(W, H, 1, 1 + spp, rowset=rowset_of(rs))
    for k, a in r.download_features().items():
        out["feat_" + k] = a
    r.denoise()
    for k, a in r.download_denoised().items():
        out["den_" + k] = a
    if temporal:
        r.denoise_temporal(fetch=4)
        for k, a in dict(r.download_denoised(), **r.download_temporal()).items():
            out["tmp_" + k] = a
    rows = out["hdr"].shape[0]
    first = rs[0] if rs else 0
    ijs = np.array([[i, first + j, s] for s in (1, 2) for j in (0, rows // 2, rows - 1) for i in (0, W // 3, W - 1)], dtype=np.uint32)
    out["unit_rays"] = r.unit_primary_rays(W, H, ijs)
    out["unit_rgb"], out["unit_trav"] = r.unit_trace(W, H, ijs, depth, seed)
    if tables:
        out.update(tile_tables(r, W, H, rs))
    return out


def assert_same_everything(got, want, what):
    assert set(got) == set(want)
    for k in want:
        label = "%s: %s" % (what, k)
        if isinstance(want[k], np.ndarray) and want[k].dtype.kind == "f":
            assert_same_bits(got[k], want[k], label)
        elif isinstance(want[k], np.ndarray):
            assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), label
        elif k != "launch":  # (its grid and queue cut follow the flagged tiles' count, which arrives when it arrives: "kernel" is compared)
            assert got[k] == want[k], label


def move_against_upload(ctxs, scenes, sc0, W, H, rs, spp, depth=50, seed=1, tables=False, before=None):
    """Context A: upload with C0, render something, set_camera(C1).  Context B: upload with C1.  Then the same calls on both."""
    c1 = turned(scenes, sc0.camera)
    assert cam_bytes(c1)[:12] != cam_bytes(sc0.camera)[:12]  # the origin moves
    a, b = ctxs(), ctxs()
    a.upload(sc0)
    a.set_noise_estimate(True)
    if before:
        before(a)
    else:
        a.render(W, H, 1, 3, depth, seed, rowset=rowset_of(rs))
    a.set_camera(c1)
    b.upload(with_camera(sc0, c1))
    b.set_noise_estimate(True)
    got = everything(a, W, H, rs, spp, depth, seed, tables)
    want = everything(b, W, H, rs, spp, depth, seed, tables)
    assert_same_everything(got, want, "set_camera against upload")
    assert cam_bytes(a.get_camera()) == cam_bytes(c1) == cam_bytes(b.get_camera())
    return a, b, got


@pytest.mark.parametrize("shape", ["96x64", "70x41", "band"])
def test_cover_scene_flat_scan_with_masks_lists_and_sky_flags(ctxs, scenes, shape):
    W, H, rs = {"96x64": (96, 64, None), "70x41": (70, 41, None), "band": (96, 64, BAND)}[shape]
    sc0 = scenes.build_scene("cover", 1, W, H)
    full = shape == "96x64"

    def before(a):  # the old camera's tables, features and snapshot are all there to be voided
        everything(a, W, H, rs, 2, 50, 1, tables=full, temporal=False)  # (no history: B has none either)
    a, b, got = move_against_upload(ctxs, scenes, sc0, W, H, rs, 4, tables=full, before=before)
    assert got["launch"].kScan == 1
    if full:
        assert got["mask_tiles"][0] == (W * H) >> 6 and got["list_tiles"][0] == (W * H) >> 6
        assert (got["lists"][:, 0] == 0).any() and (got["lists"][:, 0] != 0).any()  # sky tiles and others
        # the old camera's tables were other tables
        old = ctxs()
        old.upload(sc0)
        old.render(W, H, 1, 2, 50, 1)
        assert not np.array_equal(tile_tables(old, W, H, rs)["masks"], got["masks"])


@pytest.mark.parametrize("grid", ["cells", "hierarchy"])
def test_grid10k_cell_grid_and_hierarchy_scans(ctxs, scenes, monkeypatch, grid):
    """Recipe rows 6 and 14 of trace_variant_cases: grid10k as it is, and under RT_GRID=0."""
    if grid == "hierarchy":
        monkeypatch.setenv("RT_GRID", "0")
    else:
        monkeypatch.delenv("RT_GRID", raising=False)
    W, H = 64, 48
    sc0 = tvc.build_scene("grid10k", W, H)
    a, b, got = move_against_upload(ctxs, scenes, sc0, W, H, None, 2)
    assert got["launch"].kScan == (3 if grid == "cells" else 2)


def three_lights_glossy(scenes, oracle, W, H):
    sc = scenes.build_scene("cover", 1, W, H)
    small = (sc.materials["type"] == 0) & (sc.spheres["r"] < 100.0)
    sc.materials["smoothness"][small] = 48.0
    sc.lights = [sc.sun, oracle.make_light((-0.6, 0.7, 0.35), (0.35, 0.55, 1.0), 25000.0), oracle.make_light((-0.1, 0.9, 0.6), (0.3, 0.3, 0.3), 20000.0)]
    return sc


def test_three_lights_and_glossy_materials(ctxs, scenes, oracle):
    """Lights 1 and 2 read the camera origin from their records in device memory (Shade's view direction): the move patches them on
    the stream.  Also against the oracle's render under C1."""
    W, H, spp = 96, 64, 4
    sc0 = three_lights_glossy(scenes, oracle, W, H)
    a, b, got = move_against_upload(ctxs, scenes, sc0, W, H, None, spp)
    assert got["launch"].lights
    sc1 = with_camera(sc0, turned(scenes, sc0.camera))
    orc = oracle.Oracle()
    orc.upload(sc1)
    so = orc.render(W, H, 1, 1 + spp, 50, 1, threads=8)
    orc.resolve()
    ho, lo = orc.download()
    orc.close()
    assert_same_bits(got["hdr"], ho, "three lights after set_camera: HDR against the oracle")
    assert np.array_equal(got["ldr"], lo)
    assert (int(got["stats"][1]), int(got["stats"][2])) == (so.traversals, so.segments)


@pytest.mark.parametrize("mode", ["batch", "lookahead", "pipelining"])
def test_progressive_modes(ctxs, scenes, mode):
    W, H, depth, seed = 96, 64, 50, 1
    sc0 = scenes.build_scene("cover", 1, W, H)
    c1 = turned(scenes, sc0.camera)
    a, b = ctxs(), ctxs()

    def setting(r):
        if mode == "batch":
            r.set_frame_batch(8)
        elif mode == "lookahead":
            r.set_frame_lookahead(16)
        else:
            r.set_frame_pipelining(4)
    a.upload(sc0)
    setting(a)
    frames = 2 if mode == "lookahead" else 3
    for f in range(1, 1 + frames):
        a.render(W, H, f, f + 1, depth, seed, stats=False)
    a.set_camera(c1)
    code, msg = code_of(a.render, W, H, frames + 1, frames + 2, depth, seed, stats=False)
    assert code == RT_ERR_SEQUENCE, msg
    b.upload(with_camera(sc0, c1))
    setting(b)
    pics = []
    for r in (a, b):
        for f in range(1, 9):
            r.render(W, H, f, f + 1, depth, seed, stats=False)
        r.synchronize()
        assert r.committed_samples() == 8
        r.resolve()
        pics.append(r.download())
    assert_same_bits(pics[0][0], pics[1][0], "%s: eight frames after set_camera: HDR" % mode)
    assert np.array_equal(pics[0][1], pics[1][1])
    # ... and equal the one-shot render (no plane of the old camera was picked up)
    one = ctxs()
    one.upload(with_camera(sc0, c1))
    one.render(W, H, 1, 9, depth, seed)
    assert_same_bits(pics[0][0], one.download(ldr=False)[0], "%s: eight frames after set_camera against one call" % mode)


def test_a_move_voids_features_and_snapshot_and_get_camera_returns_the_record(ctxs, scenes):
    W, H = 96, 64
    sc0 = scenes.build_scene("cover", 1, W, H)
    c1 = turned(scenes, sc0.camera)
    r = ctxs()
    assert code_of(r.get_camera)[0] == RT_ERR_NO_SCENE
    r.upload(sc0)
    assert cam_bytes(r.get_camera()) == cam_bytes(sc0.camera)
    r.set_noise_estimate(True)
    everything(r, W, H, None, 2, 50, 1)
    r.download_features(), r.download_denoised()
    r.set_camera(c1)
    assert code_of(r.download_features)[0] == RT_ERR_SEQUENCE
    assert code_of(r.download_denoised)[0] == RT_ERR_SEQUENCE
    assert code_of(r.download)[0] == RT_ERR_SEQUENCE
    assert code_of(r.render, W, H, 3, 4, 50, 1)[0] == RT_ERR_SEQUENCE
    assert cam_bytes(r.get_camera()) == cam_bytes(c1)


def one_shot(ctxs, sc, W, H, spp, depth=50, seed=1):
    r = ctxs()
    r.upload(sc)
    r.set_noise_estimate(True)
    r.render(W, H, 1, 1 + spp, depth, seed)
    r.resolve()
    return r.download() + (r.download_moments(),)


def test_the_same_record_changes_nothing(ctxs, scenes):
    from cpuraytracer_amd import _capi
    W, H = 96, 64
    sc0 = scenes.build_scene("cover", 1, W, H)
    r = ctxs()
    r.upload(sc0)
    r.set_noise_estimate(True)
    r.render(W, H, 1, 3, 50, 1)
    r.render_features(W, H, 1, 3)
    r.denoise()
    feat, den = r.download_features(), r.download_denoised()
    same = _capi.RtCamera.from_buffer_copy(bytes(sc0.camera))
    for name in ("origin", "x", "y", "origin_image_plane"):  # the fourth components are neither read nor compared
        getattr(same, name)[3] = float("nan")
    r.set_camera(same)
    assert cam_bytes(r.get_camera()) == cam_bytes(sc0.camera)
    for k, a in r.download_features().items():  # still served
        assert np.array_equal(a.view(np.uint32), feat[k].view(np.uint32)), k
    for k, a in r.download_denoised().items():
        assert np.array_equal(a.view(np.uint8), den[k].view(np.uint8)), k
    r.render(W, H, 3, 5, 50, 1)  # continues
    r.resolve()
    want = one_shot(ctxs, sc0, W, H, 4)
    assert_same_bits(r.download()[0], want[0], "continued across set_camera(C0): HDR")
    assert np.array_equal(r.download()[1], want[1])
    assert_same_bits(r.download_moments(), want[2], "continued across set_camera(C0): moments")
    # a pending batch stays pending
    r.set_frame_batch(8)
    r.render(W, H, 5, 6, 50, 1, stats=False)
    r.set_camera(sc0.camera)
    assert r.committed_samples() == 4
    r.synchronize()
    assert r.committed_samples() == 5


def test_refusals_come_before_any_side_effect(ctxs, scenes):
    from cpuraytracer_amd import _capi
    L = _capi.load()
    W, H = 96, 64
    sc0 = scenes.build_scene("cover", 1, W, H)
    c1 = turned(scenes, sc0.camera)
    r = ctxs()
    assert code_of(r.set_camera, c1)[0] == RT_ERR_NO_SCENE
    r.upload(sc0)
    r.set_noise_estimate(True)
    r.render(W, H, 1, 2, 50, 1)
    s = 2
    assert L.rt_set_camera(r._h, None) == RT_ERR_INVALID_ARG and L.rt_set_camera(None, C.byref(c1)) == RT_ERR_INVALID_ARG
    assert L.rt_get_camera(r._h, None) == RT_ERR_INVALID_ARG
    for name, k in FIELDS:
        for bad in (float("nan"), float("inf"), -float("inf")):
            cam = _capi.RtCamera.from_buffer_copy(bytes(c1))
            if k is None:
                setattr(cam, name, bad)
            else:
                getattr(cam, name)[k] = bad
            code, msg = code_of(r.set_camera, cam)
            assert code == RT_ERR_INVALID_ARG and ("rt_set_camera: %s is not finite" % name) in msg, (name, k, bad, msg)
        assert cam_bytes(r.get_camera()) == cam_bytes(sc0.camera)
        r.render(W, H, s, s + 1, 50, 1, stats=False)  # the running accumulation continues
        s += 1
    r.resolve()
    want = one_shot(ctxs, sc0, W, H, s - 1)
    assert_same_bits(r.download()[0], want[0], "continued across the refusals: HDR")
    assert np.array_equal(r.download()[1], want[1])
    assert_same_bits(r.download_moments(), want[2], "continued across the refusals: moments")
    # a NaN in a fourth component is accepted: the record is C1
    cam = _capi.RtCamera.from_buffer_copy(bytes(c1))
    cam.x[3] = float("nan")
    r.set_camera(cam)
    assert cam_bytes(r.get_camera()) == cam_bytes(cam)
    assert code_of(r.render, W, H, s, s + 1, 50, 1)[0] == RT_ERR_SEQUENCE


def orbit_steps(r, scenes, W, H, frames, spp, spatial, fetch, move):
    """The orbit's frames on r, frame by frame: den, den_var, LDR, state, len, target.  move: "upload" or "set_camera"."""
    from cpuraytracer_amd import _capi
    V = _capi.variance_params(source=1) if spatial else None
    out = []
    for f in range(frames):
        sc = orbit_scene(scenes, "cover", W, H, 0.5 * f)
        if f == 0 or move == "upload":
            r.upload(sc)
            r.set_noise_estimate(not spatial)
        else:
            r.set_camera(sc.camera)
        r.render(W, H, 1, 1 + spp, 50, 1 + f)
        r.render_features(W, H, 1, 1 + spp)
        r.denoise_temporal(fetch=fetch, variance=V)
        out.append(dict(r.download_denoised(), **r.download_temporal()))
    return out


@pytest.mark.parametrize("fetch", [1, 4])
@pytest.mark.parametrize("source", ["moments", "spatial"])
def test_the_history_survives_the_move(ctxs, scenes, source, fetch):
    """A four-frame orbit through set_camera against the same orbit through upload, frame by frame."""
    W, H, frames = 96, 64, 4
    spatial = source == "spatial"
    got = orbit_steps(ctxs(), scenes, W, H, frames, 1 if spatial else 2, spatial, fetch, "set_camera")
    want = orbit_steps(ctxs(), scenes, W, H, frames, 1 if spatial else 2, spatial, fetch, "upload")
    for f in range(frames):
        for k in ("rgb", "var", "state"):
            assert_same_bits(got[f][k], want[f][k], "frame %d: %s" % (f, k))
        for k in ("ldr", "len", "target"):
            assert np.array_equal(got[f][k], want[f][k]), "frame %d: %s" % (f, k)
    assert (want[-1]["len"] > 1).any() and (want[-1]["target"] != NO_TARGET).any()
    assert (got[-1]["len"] > 1).any() and (got[-1]["target"] != NO_TARGET).any()


def _shards_child(index, out_path):
    """In a process of its own, torch's HIP runtime first (the library then shares it, as in bench.py).  For worlds 2 and 3: one context
    per rank on the one device; the strips reach rank 0's PostExchange by device copies, laid out as its gather lays them out.  Both
    routes run on the same contexts: the orbit through set_camera on every rank, then -- the history reset -- through upload."""
    import torch
    torch.cuda.set_device(0)
    from cpuraytracer_amd import HipRenderer, scenes, distributed as D
    W, H, frames, N, M = SHARD_SHAPE
    saved = {}
    for world in (2, 3):
        ranks = [HipRenderer(0) for _ in range(world)]
        xch = [D.PostExchange(H, W, s, world, "cuda:0", with_ids=True) for s in range(world)]
        for move in ("set_camera", "upload"):
            ranks[0].temporal_reset()
            for f in range(frames):
                sc = orbit_scene(scenes, "cover", W, H, 0.5 * f)
                for s, r in enumerate(ranks):
                    if f == 0 or move == "upload":
                        r.upload(sc)
                        r.set_noise_estimate(True)
                    else:
                        r.set_camera(sc.camera)
                    rs = D.shard_rowset(H, s, world)
                    r.render(W, H, 1, 1 + N, 50, 1 + f, rowset=rs, stats=False)
                    r.render_features(W, H, 1, 1 + M, rowset=rs)
                    xch[s].buf.view(torch.int32).fill_(-1)  # NaN in the float strips' padding, 0xffffffff in the ids'
                    torch.cuda.synchronize()
                    xch[s].fill(r)
                    r.synchronize()
                    xch[0].all[s].copy_(xch[s].buf)
                x0 = xch[0]
                x0.hdr_parts.copy_(x0.all[:, :x0.cut[0]].reshape(world, x0.rows_max, W, 3))
                x0.sq_parts.copy_(x0.all[:, x0.cut[0]:x0.cut[1]].reshape(world, x0.rows_max, W, 3))
                x0.feat_parts.copy_(x0.all[:, x0.cut[1]:x0.cut[2]].reshape(world, x0.rows_max, W, 8))
                x0.ids_parts.copy_(x0.all[:, x0.cut[2]:].view(torch.int32).reshape(world, x0.rows_max, W))
                D.denoise_gathered_temporal(ranks[0], x0, N, M, sc.camera, fetch=4)
                for k, a in dict(ranks[0].download_denoised(), **ranks[0].download_temporal()).items():
                    saved["w%d_%s_%d_%s" % (world, move, f, k)] = a
        for r in ranks:
            r.close()
    np.savez(out_path, **saved)


SHARD_SHAPE = (70, 41, 3, 2, 2)  # W, H, frames, samples in hdr and sq, samples in feat


def test_shards_move_with_set_camera(built, tmp_path):
    """Worlds 2 and 3, every rank a context on the one device: all ranks move with set_camera, and denoise_gathered_temporal on rank 0
    equals the route that uploads, frame by frame."""
    import torch.multiprocessing as mp
    out = str(tmp_path / "shards.npz")
    mp.spawn(_shards_child, args=(out,), nprocs=1, join=True)
    z = np.load(out)
    W, H, frames = SHARD_SHAPE[:3]
    for world in (2, 3):
        for f in range(frames):
            got, want = ({k: z["w%d_%s_%d_%s" % (world, move, f, k)] for k in ("rgb", "var", "state", "ldr", "len", "target")} for move in ("set_camera", "upload"))
            assert got["rgb"].shape == (H, W, 3)
            for k in ("rgb", "var", "state"):
                assert_same_bits(got[k], want[k], "world %d, frame %d: %s" % (world, f, k))
            for k in ("ldr", "len", "target"):
                assert np.array_equal(got[k], want[k]), "world %d, frame %d: %s" % (world, f, k)
        assert (got["len"] > 1).any() and (got["target"] != NO_TARGET).any()


def test_a_move_costs_less_than_an_upload(ctxs, scenes):
    """A condition, not a tuned threshold: a move that costs as much as an upload has not been built.  The median host time of nine
    set_camera calls (alternating C0 and C1, each after a synchronize) against the fastest of three uploads."""
    W, H = 96, 64
    sc0 = scenes.build_scene("cover", 1, W, H)
    c1 = turned(scenes, sc0.camera)
    r = ctxs()
    uploads = []
    for _ in range(3):
        r.synchronize()
        t = time.perf_counter()
        r.upload(sc0)
        uploads.append(time.perf_counter() - t)
    moves = []
    for k in range(9):
        r.synchronize()
        cam = c1 if k % 2 == 0 else sc0.camera
        t = time.perf_counter()
        r.set_camera(cam)
        moves.append(time.perf_counter() - t)
    print("rt_scene_upload (cover): %s ms; rt_set_camera: median %.4f ms of %s"
          % (", ".join("%.3f" % (1e3 * u) for u in uploads), 1e3 * float(np.median(moves)), ", ".join("%.4f" % (1e3 * m) for m in moves)))
    assert float(np.median(moves)) < min(uploads)
