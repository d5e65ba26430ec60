"""Temporal accumulation across row shards on the device (rt_denoise_shards_temporal; csrc/rt_denoise.hip
rt_denoise_prepare_shards_temporal_kernel and its bilinear sibling): a reference context renders every frame of an orbit whole (or a band
of it contiguously) and calls rt_denoise_temporal_fetch; a second context renders the frame shard after shard into 0xff-filled parts
(whatever padding is read becomes NaN, a padding id 0xffffffff) and the sharded call over them must give the reference's bits frame by
frame -- den, den_var, ldr, the history's state, len and target -- and the host twin's; the history's lifetime and its key; that nothing
else of the context changes; the refusals; and two rank processes sharing device 0 that gather through
distributed.PostExchange(with_ids=True)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from temporal_bilinear_common import BILINEAR, NEAREST
from temporal_common import NO_TARGET, history_of, orbit_scene
from test_denoise import forms_for
from test_denoise_cpu import DEFAULTS, params_struct
from test_denoise_shards import DevMem, _free_port, hiprt  # noqa: F401  (hiprt: a fixture)
from test_noise_estimate_cpu import assert_same_bits
from test_temporal import dr, render_frame, scenes, strips  # noqa: F401  (dr, scenes: fixtures)

pytestmark = pytest.mark.gpu

RT_ERR_INVALID_ARG, RT_ERR_SEQUENCE = 2, 6
N, M = 8, 8
FRAMES, STEP = 3, 0.5  # the orbit: degrees per frame; frame f has seed 1 + f (test_temporal.render_frame)
SHARDINGS = [(1, 1), (2, 1), (3, 1), (8, 1), (3, 4)]  # world, block_rows
SHAPES = {"96x64": (96, 64, 0, 64), "70x41": (70, 41, 0, 41), "band": (70, 41, 5, 29)}  # W, H, first_row, num_rows
CASES = [(k, w, b) for k in ("96x64", "70x41") for w, b in SHARDINGS] + [("band", 3, 1)]
LEVELS = (1, 3, 5)
KEYS = ("rgb", "var", "state")


def params_of(levels):
    return None if levels == 3 else params_struct(dict(DEFAULTS, levels=levels))


def result(r):
    d, t = r.download_denoised(), r.download_temporal()
    return dict(rgb=d["rgb"], var=d["var"], ldr=d["ldr"], **t)


def same(got, want, what):
    for k in KEYS:
        assert_same_bits(got[k], want[k], "%s: %s" % (what, k))
    for k in ("ldr", "len", "target"):
        assert np.array_equal(got[k], want[k]), "%s: %s differs at %d places" % (what, k, int((got[k] != want[k]).sum()))


def contiguous_rowset(shape):
    W, H, first, rows = SHAPES[shape]
    return None if (first, rows) == (0, H) else (first, rows, rows, 0, 1)


@pytest.fixture(scope="module")
def reference(built, scenes):
    """Per shape, fetch and level count: the orbit's frames rendered contiguously in one context, rt_denoise_temporal_fetch on each with
    that fetch's defaults, and what it left (RT_DENOISE_STAGE unset) -- computed once, never changed."""
    from cpuraytracer_amd import HipRenderer
    saved = os.environ.pop("RT_DENOISE_STAGE", None)
    out = {}
    r = HipRenderer(0)
    try:
        for shape, (W, H, first, rows) in SHAPES.items():
            for fetch in (NEAREST, BILINEAR):
                for levels in LEVELS:
                    r.temporal_reset()
                    seq = []
                    for f in range(FRAMES):
                        render_frame(r, scenes, W, H, f, contiguous_rowset(shape), deg=STEP, spp=N)
                        r.denoise_temporal(params_of(levels), None, fetch=fetch)
                        seq.append(result(r))
                        for a in seq[-1].values():
                            a.setflags(write=False)
                        if f > 0:  # the orbit is not vacuous: the history was used, the move rejected some pixels and shifted others
                            acc = seq[-1]["target"] != NO_TARGET
                            own = np.arange(acc.size, dtype=np.uint32).reshape(acc.shape)
                            assert acc.any() and (~acc).any() and (seq[-1]["target"][acc] != own[acc]).any(), (shape, fetch, f)
                    out[(shape, fetch, levels)] = seq
    finally:
        r.close()
        if saved is not None:
            os.environ["RT_DENOISE_STAGE"] = saved
    return out


def render_parts(r, hiprt, scenes, shape, f, world, block_rows):
    """Frame f of the orbit rendered shard after shard in r, each shard's hdr, sq, feat and id strips copied device to device into its
    slot of 0xff-filled parts buffers."""
    from cpuraytracer_amd import _capi
    L = _capi.load()
    W, H, first, num_rows = SHAPES[shape]
    sc = orbit_scene(scenes, "cover", W, H, STEP * f)
    rows = [L.rt_rowset_local_rows(_capi.RtRowset(first, num_rows, block_rows, s, world)) for s in range(world)]
    rows_max = max(rows)
    px = rows_max * W
    bufs = [DevMem(hiprt, world * px * c * 4) for c in (3, 3, 8, 1)]
    r.upload(sc)
    r.set_noise_estimate(True)
    for s in range(world):
        rs = _capi.RtRowset(first, num_rows, block_rows, s, world)
        r.render(W, H, 1, 1 + N, 50, 1 + f, rowset=rs, stats=False)
        r.render_features(W, H, 1, 1 + M, rowset=rs)
        r.copy_to_device(bufs[0].at(s * px * 12), None)
        r.copy_moments_to_device(bufs[1].at(s * px * 12))
        r.copy_features_to_device(bufs[2].at(s * px * 32), bufs[3].at(s * px * 4))
    r.synchronize()
    return dict(bufs=bufs, rows=rows, rows_max=rows_max, cam=sc.camera, shape=shape, world=world, block_rows=block_rows)


@pytest.fixture(scope="module")
def parts_of(built, hiprt, scenes):
    """parts_of(shape, world, block_rows) -> the orbit's frames as parts on the device, rendered once per module by a context of their own."""
    from cpuraytracer_amd import HipRenderer
    cache = {}
    maker = HipRenderer(0)

    def get(shape, world, block_rows):
        key = (shape, world, block_rows)
        if key not in cache:
            cache[key] = [render_parts(maker, hiprt, scenes, shape, f, world, block_rows) for f in range(FRAMES)]
        return cache[key]

    yield get
    maker.close()
    for frames in cache.values():
        for fp in frames:
            for b in fp["bufs"]:
                b.free()


def shards_call(r, fp, params=None, tparams=None, fetch=BILINEAR, timed=False):
    W, H, first, num_rows = SHAPES[fp["shape"]]
    b = fp["bufs"]
    return r.denoise_shards_temporal(b[0].at(0), b[1].at(0), b[2].at(0), b[3].at(0), W, H, fp["world"], fp["rows_max"], N, M, fp["cam"], params=params,
                                     tparams=tparams, fetch=fetch, timed=timed, block_rows=fp["block_rows"], first_row=first, num_rows=num_rows)


def shards_step(r, fp, levels=3, fetch=BILINEAR):
    shards_call(r, fp, params_of(levels), None, fetch)
    return result(r)


def download_parts(fp):
    W = SHAPES[fp["shape"]][0]
    shape = (fp["world"], fp["rows_max"], W)
    b = fp["bufs"]
    return [b[0].download(np.float32, shape + (3,)), b[1].download(np.float32, shape + (3,)), b[2].download(np.float32, shape + (8,)),
            b[3].download(np.uint32, shape)]


def twin_step(fp, parts, hist, levels, fetch):
    from cpuraytracer_amd import _capi
    W, H, first, num_rows = SHAPES[fp["shape"]]
    frame = _capi.shard_frame(W, H, fp["world"], fp["rows_max"], N, M, fp["cam"], block_rows=fp["block_rows"], first_row=first, num_rows=num_rows)
    return _capi.unit_temporal_shards_host(parts[0], parts[1], parts[2], parts[3], frame, history=hist, params=params_of(levels), tparams=None, fetch=fetch)


@pytest.mark.parametrize("shape,world,block_rows", CASES, ids=["%s_w%d_b%d" % c for c in CASES])
def test_device_equals_reference_and_twin(dr, reference, parts_of, monkeypatch, shape, world, block_rows):
    frames = parts_of(shape, world, block_rows)
    host = [download_parts(fp) for fp in frames]
    for fp, parts in zip(frames, host):  # every padding row holds 0xff bytes
        for s in range(world):
            assert all((p[s, fp["rows"][s]:].view(np.uint32) == 0xffffffff).all() for p in parts)
        assert (min(fp["rows"]) < fp["rows_max"]) == np.isnan(parts[0]).any()
    for fetch in (NEAREST, BILINEAR):
        for knob in (None, "0", "1"):
            if knob is None:
                monkeypatch.delenv("RT_DENOISE_STAGE", raising=False)
            else:
                monkeypatch.setenv("RT_DENOISE_STAGE", knob)
            for levels in LEVELS:
                dr.temporal_reset()
                hist = None
                for f, fp in enumerate(frames):
                    what = "%s in %d shards of %d-row blocks, fetch %d, %d levels, RT_DENOISE_STAGE=%s, frame %d" % (shape, world, block_rows, fetch, levels, knob, f)
                    got = shards_step(dr, fp, levels, fetch)
                    assert dr.denoise_forms() == forms_for(levels, knob), what
                    same(got, reference[(shape, fetch, levels)][f], what)
                    if knob is None:
                        twin = twin_step(fp, host[f], hist, levels, fetch)
                        for k in KEYS:
                            assert_same_bits(got[k], twin[k], what + ": %s vs the host twin" % k)
                        assert np.array_equal(got["len"], twin["len"]) and np.array_equal(got["target"], twin["target"]), what + " vs the host twin"
                        hist = history_of(twin)


def test_history_lifetime(dr, reference, parts_of, hiprt, scenes):
    from cpuraytracer_amd import _capi
    shape = "70x41"
    W, H = SHAPES[shape][:2]
    ref = reference[(shape, BILINEAR, 3)]
    three, two = parts_of(shape, 3, 1), parts_of(shape, 2, 1)
    # rt_temporal_reset empties the history
    same(shards_step(dr, three[0]), ref[0], "frame 0")
    dr.temporal_reset()
    with pytest.raises(_capi.RtError) as e:
        dr.download_temporal()
    assert e.value.code == RT_ERR_SEQUENCE
    got = shards_step(dr, three[1])
    assert (got["len"] == 1).all() and (got["target"] == NO_TARGET).all()
    dr.denoise_shards(three[1]["bufs"][0].at(0), three[1]["bufs"][1].at(0), three[1]["bufs"][2].at(0), W, H, 3, three[1]["rows_max"], N, M)
    plain = dr.download_denoised()
    for k in ("rgb", "var"):
        assert_same_bits(got[k], plain[k], "an empty history gives rt_denoise_shards' bits: " + k)
    assert np.array_equal(got["ldr"], plain["ldr"])
    # upload keeps it
    dr.temporal_reset()
    same(shards_step(dr, three[0]), ref[0], "frame 0 again")
    dr.upload(orbit_scene(scenes, "three", 32, 16, 0.0))
    same(shards_step(dr, three[1]), ref[1], "frame 1 after an upload")
    # a different sharding of the same picture starts empty
    got = shards_step(dr, two[2])
    assert (got["len"] == 1).all() and (got["target"] == NO_TARGET).all()
    # ... and goes on from there
    assert (shards_step(dr, two[2])["len"] == 2).any()
    # the two fetches alternate on one history: the contiguous twin's chain over the strips a whole render leaves
    from temporal_bilinear_common import host_temporal_fetch
    dr.temporal_reset()
    whole = []
    for f in range(FRAMES):
        cam = render_frame(dr, scenes, W, H, f, deg=STEP, spp=N)
        whole.append((cam,) + strips(dr))
    hist = None
    for f, fetch in enumerate((BILINEAR, NEAREST, BILINEAR)):
        cam, S, Q, feat, ids = whole[f]
        want = host_temporal_fetch(S, Q, N, feat, M, ids, W, H, cam, hist, None, None, 0, fetch)
        got = shards_step(dr, three[f], fetch=fetch)
        for k in KEYS:
            assert_same_bits(got[k], want[k], "alternating, frame %d: %s" % (f, k))
        assert np.array_equal(got["len"], want["len"]) and np.array_equal(got["target"], want["target"]), f
        hist = history_of(want)
    assert got["len"].max() == 3


def test_one_shard_with_the_whole_image_key_shares_the_history_with_the_contiguous_call(dr, reference, parts_of, scenes):
    """world = 1, block_rows = H: the key of a whole-image render.  Whole, sharded, whole -- and sharded, whole, sharded -- give the bits of
    the all-whole sequence; with another block_rows the key differs and the history starts empty."""
    shape = "70x41"
    W, H = SHAPES[shape][:2]
    ref = reference[(shape, BILINEAR, 3)]
    one = parts_of(shape, 1, H)
    for start in (0, 1):
        dr.temporal_reset()
        for f in range(FRAMES):
            if (f + start) % 2 == 0:
                render_frame(dr, scenes, W, H, f, deg=STEP, spp=N)
                dr.denoise_temporal(None, None, fetch=BILINEAR)
                got = result(dr)
            else:
                got = shards_step(dr, one[f])
            same(got, ref[f], "start %d, frame %d" % (start, f))
    other = parts_of(shape, 1, 1)  # the same rows in the same order, another key
    got = shards_step(dr, other[2])
    assert (got["len"] == 1).all()


def test_independence(dr, reference, parts_of, scenes):
    """The call between two halves of an accumulation of ANOTHER picture size changes nothing of the render, its moments, features and
    LDR; rt_denoise and rt_denoise_shards leave the history alone; a context without a scene runs it."""
    from cpuraytracer_amd import HipRenderer
    shape = "70x41"
    ref = reference[(shape, BILINEAR, 3)]
    frames = parts_of(shape, 3, 1)
    W, H = 96, 64
    render_frame(dr, scenes, W, H, 0, spp=4)
    dr.resolve()
    before = (dr.download(), dr.download_moments(), dr.download_features())
    same(shards_step(dr, frames[0]), ref[0], "frame 0")
    got = shards_step(dr, frames[1])
    same(got, ref[1], "frame 1")
    after = (dr.download(), dr.download_moments(), dr.download_features())
    assert_same_bits(after[0][0], before[0][0], "hdr")
    assert np.array_equal(after[0][1], before[0][1]), "ldr"
    assert_same_bits(after[1], before[1], "sq")
    for key in ("albedo", "normal", "depth", "coverage"):
        assert_same_bits(after[2][key], before[2][key], key)
    assert np.array_equal(after[2]["id"], before[2]["id"])
    assert dr.committed_samples() == 4 and dr.feature_samples() == 4
    # the accumulation goes on as if nothing had happened
    dr.render(W, H, 5, 9, 50, 1, stats=False)
    one = HipRenderer(0)
    try:
        render_frame(one, scenes, W, H, 0, spp=8)
        assert_same_bits(dr.download(ldr=False)[0], one.download(ldr=False)[0], "the continued render vs the one-shot render")
        assert_same_bits(dr.download_moments(), one.download_moments(), "its second moments")
    finally:
        one.close()
    # rt_denoise and rt_denoise_shards leave the history alone
    dr.render_features(W, H, 5, 9)
    dr.denoise()
    b = frames[2]["bufs"]
    dr.denoise_shards(b[0].at(0), b[1].at(0), b[2].at(0), 70, 41, 3, frames[2]["rows_max"], N, M)
    t = dr.download_temporal()
    assert_same_bits(t["state"], got["state"], "the history after rt_denoise and rt_denoise_shards")
    assert np.array_equal(t["len"], got["len"]) and np.array_equal(t["target"], got["target"])
    same(shards_step(dr, frames[2]), ref[2], "frame 2")
    fresh = HipRenderer(0)  # no scene, no accumulation
    try:
        same(shards_step(fresh, frames[0], levels=5), reference[(shape, BILINEAR, 5)][0], "a context without a scene")
    finally:
        fresh.close()


def test_refusals_on_the_device_path(dr, reference, parts_of):
    from cpuraytracer_amd import _capi
    L = _capi.load()
    shape, world = "band", 3
    W, H, first, num_rows = SHAPES[shape]
    ref = reference[(shape, BILINEAR, 3)]
    frames = parts_of(shape, world, 1)
    fp = frames[1]
    b = fp["bufs"]
    ptrs = dict(hdr=b[0].at(0), sq=b[1].at(0), feat=b[2].at(0), ids=b[3].at(0))

    def call(P=None, T=None, fetch=BILINEAR, ctx=True, shape=True, camera=fp["cam"], **over):
        kw = dict(W=W, H=H, world=world, rows_max=fp["rows_max"], n=N, m=M, block_rows=1, first_row=first, num_rows=num_rows, **ptrs)
        kw.update(over)
        fr = _capi.shard_frame(camera=camera, **kw)
        return L.rt_denoise_shards_temporal(dr._h if ctx else None, C.byref(fr) if shape else None, C.byref(P) if P is not None else None,
                                            C.byref(T) if T is not None else None, fetch, None)

    def refusals():
        assert call(ctx=False) == RT_ERR_INVALID_ARG and call(shape=False) == RT_ERR_INVALID_ARG
        for null in ("hdr", "sq", "feat", "ids"):
            assert call(**{null: None}) == RT_ERR_INVALID_ARG, null
        for zero in ("W", "num_rows", "world", "block_rows"):
            assert call(**{zero: 0}) == RT_ERR_INVALID_ARG, zero
        assert call(rows_max=fp["rows_max"] - 1) == RT_ERR_INVALID_ARG
        for off in (4, 8, 12):
            assert call(feat=ptrs["feat"] + off) == RT_ERR_INVALID_ARG, off
        for off in (1, 2, 3):
            assert call(ids=ptrs["ids"] + off) == RT_ERR_INVALID_ARG, off
        assert call(H=first + num_rows - 1) == RT_ERR_INVALID_ARG and call(H=(1 << 24) + 1) == RT_ERR_INVALID_ARG
        for fetch in (0, 2, 3, 5):
            assert call(fetch=fetch) == RT_ERR_INVALID_ARG, fetch
        for bad in (dict(levels=0), dict(levels=6), dict(k_albedo=-1.0), dict(k_colour=float("nan")), dict(var_floor=0.0)):
            assert call(P=params_struct(bad)) == RT_ERR_INVALID_ARG, bad
        for bad in (dict(max_history=0), dict(max_history=65), dict(depth_tol=-1.0), dict(normal_tol=float("nan")), dict(coverage_tol=float("inf"))):
            assert call(T=_capi.temporal_params_fetch(BILINEAR, **bad)) == RT_ERR_INVALID_ARG, bad
        for field, k in (("origin", 1), ("x", 0), ("y", 2), ("origin_image_plane", 2), ("aperture", None), ("focal_length", None)):
            c = _capi.RtCamera.from_buffer_copy(bytes(fp["cam"]))
            if k is None:
                setattr(c, field, float("inf"))
            else:
                getattr(c, field)[k] = float("nan")
            assert call(camera=c) == RT_ERR_INVALID_ARG, field
        for n in (0, 1):
            assert call(n=n) == RT_ERR_SEQUENCE
        assert call(m=0) == RT_ERR_SEQUENCE

    refusals()
    for reader in (dr.download_denoised, dr.download_temporal):  # refused calls left no result and no history
        with pytest.raises(_capi.RtError) as e:
            reader()
        assert e.value.code == RT_ERR_SEQUENCE
    assert dr.denoise_forms() == [0] * 5
    same(shards_step(dr, frames[0]), ref[0], "frame 0")
    good = shards_step(dr, frames[1])
    same(good, ref[1], "frame 1")
    assert (dr.denoised_W, dr.denoised_rows, dr.temporal_W, dr.temporal_rows) == (W, num_rows, W, num_rows)
    refusals()
    same(result(dr), good, "a refused call keeps the history and the snapshot")
    same(shards_step(dr, frames[2]), ref[2], "... and the next good call uses the kept history")


def test_device_copy_and_timed_call(dr, reference, parts_of, hiprt):
    shape = "70x41"
    W, H = SHAPES[shape][:2]
    frames = parts_of(shape, 8, 1)
    assert shards_call(dr, frames[0], timed=False) is None
    ms = shards_call(dr, frames[1], timed=True)
    assert ms is not None and ms > 0.0
    want = reference[(shape, BILINEAR, 3)][1]
    same(result(dr), want, "the timed call")
    out = [DevMem(hiprt, W * H * 12, fill=0), DevMem(hiprt, W * H * 4, fill=0), DevMem(hiprt, W * H * 3, fill=0)]
    try:
        dr.copy_denoised_to_device(out[0].at(0), out[1].at(0), out[2].at(0))
        dr.synchronize()
        assert_same_bits(out[0].download(np.float32, (H, W, 3)), want["rgb"], "copy_denoised_to_device: rgb")
        assert_same_bits(out[1].download(np.float32, (H, W)), want["var"], "copy_denoised_to_device: var")
        assert np.array_equal(out[2].download(np.uint8, (H, W, 3)), want["ldr"])
    finally:
        for o in out:
            o.free()


def _rank(rank, world, port, W, H, frames, out_path):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(0)  # torch's HIP runtime first, as in bench.py: the library then shares it; both ranks share device 0
    from cpuraytracer_amd import HipRenderer, scenes, distributed as D
    dist.init_process_group("gloo", rank=rank, world_size=world)
    r = None
    try:
        r = HipRenderer(0)
        xch = D.PostExchange(H, W, rank, world, "cuda:0", with_ids=True)
        saved = {}
        for f in range(frames):
            sc = orbit_scene(scenes, "cover", W, H, STEP * f)
            r.upload(sc)  # a camera move is an upload: rank 0's history survives it
            r.set_noise_estimate(True)
            rs = D.shard_rowset(H, rank, world)
            r.render(W, H, 1, 1 + N, 50, 1 + f, rowset=rs, stats=False)
            r.render_features(W, H, 1, 1 + M, rowset=rs)
            xch.buf.view(torch.int32).fill_(-1)  # 0xff bytes: NaN in the float strips' padding, 0xffffffff in the ids'
            torch.cuda.synchronize()
            xch.fill(r)
            r.synchronize()
            parts = xch.gather(through_host=True)
            if rank == 0:
                assert len(parts) == 4 and all(p.is_cuda and p.is_contiguous() for p in parts) and parts[2].data_ptr() % 16 == 0
                assert parts[3].dtype == torch.int32 and parts[3].shape == (world, xch.rows_max, W)
                D.denoise_gathered_temporal(r, xch, N, M, sc.camera, fetch=4)
                d, t = r.download_denoised(), r.download_temporal()
                for k, a in dict(d, **t).items():
                    saved["%s%d" % (k, f)] = a
            else:
                assert parts == (None, None, None, None)
            dist.barrier()
        if rank == 0:
            np.savez(out_path, **saved)
    finally:
        if r is not None:
            r.close()
        dist.destroy_process_group()


def test_two_rank_rehearsal_on_one_device(built, reference, tmp_path, monkeypatch):
    """Two rank processes share device 0 (gloo, strips through host memory -- tests/test_denoise_shards.py's recipe): two frames of the
    orbit, each rendered in the ranks' rows with moments, features and ids, one PostExchange(with_ids=True) gather per frame and
    denoise_gathered_temporal on rank 0, whose history is kept from frame to frame.  41 rows: rank 1's part has a padding row."""
    import torch.multiprocessing as mp
    shape = "70x41"
    W, H = SHAPES[shape][:2]
    monkeypatch.setenv("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    monkeypatch.delenv("RT_DENOISE_STAGE", raising=False)
    out = str(tmp_path / "den.npz")
    mp.spawn(_rank, args=(2, _free_port(), W, H, 2, out), nprocs=2, join=True)
    z = np.load(out)
    for f in range(2):
        got = {k: z["%s%d" % (k, f)] for k in ("rgb", "var", "ldr", "state", "len", "target")}
        assert got["rgb"].shape == (H, W, 3) and got["ldr"].dtype == np.uint8 and got["len"].dtype == np.uint32
        same(got, reference[(shape, BILINEAR, 3)][f], "two ranks, frame %d" % f)
    assert (z["len1"] == 2).any()
