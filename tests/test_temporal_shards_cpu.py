"""Temporal accumulation across row shards, the part that needs no GPU (rt_unit_temporal_shards_host, csrc/host/rt_temporal_host.cpp over
csrc/rt_rowset_map.h and csrc/rt_temporal.h; distributed.PostExchange(with_ids=True)): the twin over parts cut from the
CPU oracle's strips along an orbit against the contiguous twin (rt_unit_temporal_host_fetch) on the uncut strips, bit for bit, both
fetches, each on its own history fed forward, with NaN and 0xffffffff in every padding row; the empty history; the refusals (all but the
alignment of the device pointer `ids`, which only the device entry looks at: tests/test_temporal_shards.py); the API surface; the ids
through the one-gather exchange over gloo; and the stand-alone selftest, plain and under ASan + UBSan."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from temporal_bilinear_common import BILINEAR, NEAREST, host_temporal_fetch
from temporal_common import NO_TARGET, assert_same_step, history_of, oracle_frame, orbit_scene
from test_denoise_cpu import DEFAULTS, params_struct, random_strips
from test_denoise_shards_cpu import _free_port, cut, host_denoise_shards
from test_noise_estimate_cpu import assert_same_bits

RT_ERR_INVALID_ARG, RT_ERR_SEQUENCE = 2, 6
F = np.float32
SPP = 2                       # samples per frame in the oracle's strips (n = m = SPP)
FRAMES, STEP = 3, 0.5         # the orbit: degrees per frame about the cover scene's look-at point
SIZES = [(96, 64), (70, 41)]
SHARDINGS = [(1, 1), (2, 1), (3, 1), (8, 1), (3, 4)]  # world, block_rows
BAND = dict(W=70, H=41, first_row=5, num_rows=29, world=3, block_rows=1)
KEYS = ("state", "len", "target", "rgb", "var")


@pytest.fixture(scope="module")
def scenes(built):
    from cpuraytracer_amd import scenes
    return scenes


@pytest.fixture(scope="module")
def orbit(oracle, scenes):
    """Per size: FRAMES frames (camera, hdr, sq, feat, ids) of the cover scene from the CPU oracle, SPP samples each, seed 1 + f, the
    camera turned STEP degrees per frame -- computed once, never changed.  (A band is rows of the 70 x 41 frames: a pixel's samples do
    not depend on the row set it is rendered in.)"""
    out = {}
    for W, H in SIZES:
        out[(W, H)] = []
        for f in range(FRAMES):
            sc = orbit_scene(scenes, "cover", W, H, STEP * f)
            out[(W, H)].append((sc.camera,) + oracle_frame(oracle, sc, W, H, range(H), SPP, 50, 1 + f))
    for frames in out.values():
        for fr in frames:
            for a in fr[1:]:
                a.setflags(write=False)
    return out


def band_of(frames, first_row, num_rows):
    return [(cam,) + tuple(a[first_row:first_row + num_rows] for a in strips) for cam, *strips in frames]


def cut_frame(S, Q, feat, ids, world, block_rows, extra=0):
    """The four strips as parts: NaN in every padding row, 0xffffffff in every padding id; `extra` more padding rows per part."""
    parts = [cut(np.asarray(a), world, block_rows)[0] for a in (S, Q, feat)]
    parts.append(cut(np.asarray(ids, dtype=np.uint32), world, block_rows, fill=0xffffffff)[0])
    if extra:
        parts = [np.concatenate([p, np.full((world, extra) + p.shape[2:], 0xffffffff if p.dtype == np.uint32 else np.nan, p.dtype)], axis=1) for p in parts]
    return parts


def host_temporal_shards(parts, W, H, world, block_rows, n, m, cam, hist=None, P=None, T=None, fetch=BILINEAR, first_row=0, num_rows=None):
    """The sharded twin; T replaces fields of THAT fetch's defaults (as temporal_bilinear_common.host_temporal_fetch)."""
    from cpuraytracer_amd import _capi
    frame = _capi.shard_frame(W, H, world, parts[0].shape[1], n, m, cam, block_rows=block_rows, first_row=first_row, num_rows=num_rows)
    return _capi.unit_temporal_shards_host(parts[0], parts[1], parts[2], parts[3], frame, history=hist, params=_capi.denoise_params(**dict(DEFAULTS, **(P or {}))),
                                           tparams=_capi.temporal_params_fetch(fetch, **(T or {})), fetch=fetch)


def assert_orbit_is_not_vacuous(step, W, what):
    """What the issue asks of every frame after the first, asserted on the CONTIGUOUS twin's result: the history was used, the move
    rejected some pixels and shifted others."""
    acc = step["target"] != NO_TARGET
    own = np.arange(acc.size, dtype=np.uint32).reshape(acc.shape)
    assert acc.any(), what + ": no pixel accepted"
    assert (~acc).any(), what + ": no pixel rejected"
    assert (step["target"][acc] != own[acc]).any(), what + ": every accepted pixel was blended with its own index"


def run_orbit(frames, W, H, world, block_rows, fetch, first_row=0, P=None):
    """The frames through the contiguous twin and through the sharded twin over the cut parts, each on its own history."""
    rows = frames[0][1].shape[0]
    hc = hp = None
    for f, (cam, S, Q, feat, ids) in enumerate(frames):
        what = "%d x %d rows %d..+%d in %d shards of %d-row blocks, fetch %d, frame %d" % (W, H, first_row, rows, world, block_rows, fetch, f)
        want = host_temporal_fetch(S, Q, SPP, feat, SPP, ids, W, H, cam, hc, P, None, first_row, fetch)
        parts = cut_frame(S, Q, feat, ids, world, block_rows)
        if world > 1 and rows % (world * block_rows) != 0:
            assert np.isnan(parts[0]).any() and (parts[3] == 0xffffffff).any()
        got = host_temporal_shards(parts, W, H, world, block_rows, SPP, SPP, cam, hp, P, None, fetch, first_row, rows)
        assert_same_step(got, want, what, KEYS)
        assert_same_bits(got["guides"], want["guides"], what + ": guides")
        assert np.array_equal(got["ids"], want["ids"]), what + ": ids"
        assert bytes(got["camera"]) == bytes(want["camera"])
        if f > 0:
            assert_orbit_is_not_vacuous(want, W, what)
        hc, hp = history_of(want), history_of(got)


@pytest.mark.parametrize("fetch", [NEAREST, BILINEAR], ids=["nearest", "bilinear"])
@pytest.mark.parametrize("W,H", SIZES, ids=["%dx%d" % s for s in SIZES])
@pytest.mark.parametrize("world,block_rows", SHARDINGS, ids=["w%d_b%d" % s for s in SHARDINGS])
def test_twin_over_parts_equals_contiguous_twin(built, orbit, W, H, world, block_rows, fetch):
    run_orbit(orbit[(W, H)], W, H, world, block_rows, fetch)


@pytest.mark.parametrize("fetch", [NEAREST, BILINEAR], ids=["nearest", "bilinear"])
def test_band(built, orbit, fetch):
    B = BAND
    run_orbit(band_of(orbit[(B["W"], B["H"])], B["first_row"], B["num_rows"]), B["W"], B["H"], B["world"], B["block_rows"], fetch, B["first_row"], P=dict(levels=2))


@pytest.mark.parametrize("fetch", [NEAREST, BILINEAR], ids=["nearest", "bilinear"])
def test_padding_changes_nothing(built, orbit, fetch):
    """Two more padding rows per part (NaN, ids 0xffffffff), and padding of finite garbage: the same bits."""
    W, H, world, block_rows = 70, 41, 3, 4
    (cam0, S0, Q0, feat0, ids0), (cam1, S1, Q1, feat1, ids1) = orbit[(W, H)][:2]
    hist = history_of(host_temporal_fetch(S0, Q0, SPP, feat0, SPP, ids0, W, H, cam0, None, None, None, 0, fetch))
    want = host_temporal_shards(cut_frame(S1, Q1, feat1, ids1, world, block_rows), W, H, world, block_rows, SPP, SPP, cam1, hist, fetch=fetch)
    wide = cut_frame(S1, Q1, feat1, ids1, world, block_rows, extra=2)
    assert wide[0].shape[1] == 16 + 2 and np.isnan(wide[0][:, -2:]).all() and (wide[3][:, -2:] == 0xffffffff).all()
    got = host_temporal_shards(wide, W, H, world, block_rows, SPP, SPP, cam1, hist, fetch=fetch)
    assert_same_step(got, want, "rows_max + 2", KEYS)
    from cpuraytracer_amd import distributed as D
    junk = [p.copy() for p in wide]
    for s in range(world):
        own = D.local_rows(H, s, world, block_rows)
        for p in junk[:3]:
            p[s, own:] = F(0.375)
        junk[3][s, own:] = 1
    assert [D.local_rows(H, s, world, block_rows) for s in range(world)] == [16, 13, 12] and not any(np.isnan(p).any() for p in junk[:3])
    got = host_temporal_shards(junk, W, H, world, block_rows, SPP, SPP, cam1, hist, fetch=fetch)
    assert_same_step(got, want, "padding of finite garbage", KEYS)


@pytest.mark.parametrize("fetch", [NEAREST, BILINEAR], ids=["nearest", "bilinear"])
def test_empty_history_is_the_filter_over_the_parts(built, orbit, fetch):
    W, H = 70, 41
    cam, S, Q, feat, ids = orbit[(W, H)][0]
    for world, block_rows in SHARDINGS:
        parts = cut_frame(S, Q, feat, ids, world, block_rows)
        for levels in (1, 3, 5):
            P = dict(DEFAULTS, levels=levels)
            got = host_temporal_shards(parts, W, H, world, block_rows, SPP, SPP, cam, None, P, fetch=fetch)
            want = host_denoise_shards(parts[0], parts[1], parts[2], W, H, world, block_rows, SPP, SPP, P)
            what = "%d shards of %d-row blocks, %d levels" % (world, block_rows, levels)
            assert_same_bits(got["rgb"], want[0], what + ": den")
            assert_same_bits(got["var"], want[1], what + ": den_var")
            assert (got["len"] == 1).all() and (got["target"] == NO_TARGET).all()


def test_one_shard_is_the_contiguous_twin_whatever_block_rows(built, orbit):
    W, H = 70, 41
    (cam0, S0, Q0, feat0, ids0), (cam1, S1, Q1, feat1, ids1) = orbit[(W, H)][:2]
    first = host_temporal_fetch(S0, Q0, SPP, feat0, SPP, ids0, W, H, cam0, None, None, None, 0, BILINEAR)
    want = host_temporal_fetch(S1, Q1, SPP, feat1, SPP, ids1, W, H, cam1, history_of(first), None, None, 0, BILINEAR)
    for block_rows in (1, 4, H, H + 3):
        got = host_temporal_shards([a[None] for a in (S1, Q1, feat1, ids1)], W, H, 1, block_rows, SPP, SPP, cam1, history_of(first), fetch=BILINEAR)
        assert_same_step(got, want, "block_rows %d" % block_rows, KEYS)


def test_refusals(built, scenes):
    from cpuraytracer_amd import _capi
    L = _capi.load()
    W, H, first, rows, world = 3, 7, 1, 5, 2  # rows 1..5 of 7; shard 0 owns range rows 0, 2, 4: rows_max = 3
    cam = orbit_scene(scenes, "cover", W, H, 0.0).camera
    z3, z8, zi = np.zeros((world, 3, W, 3), F), np.zeros((world, 3, W, 8), F), np.zeros((world, 3, W), np.uint32)
    hs, hg, hi, hl = np.zeros((rows, W, 4), F), np.zeros((rows, W, 8), F), np.zeros((rows, W), np.uint32), np.ones((rows, W), np.uint32)
    o3, o1 = np.zeros((rows, W, 3), F), np.zeros((rows, W), F)
    ptr = lambda a: a.ctypes.data if a is not None else None

    def call(P=None, T=None, fetch=4, hdr=z3, sq=z3, feat=z8, ids=zi, shape=True, hist_cam=cam, camera=cam, **over):
        kw = dict(W=W, H=H, world=world, rows_max=3, n=2, m=1, block_rows=1, first_row=first, num_rows=rows)
        kw.update(over)
        fr = _capi.shard_frame(camera=camera, **kw)
        hc = C.byref(_capi.RtCamera.from_buffer_copy(bytes(hist_cam))) if hist_cam is not None else None
        return L.rt_unit_temporal_shards_host(ptr(hdr), ptr(sq), ptr(feat), ptr(ids), C.byref(fr) if shape else None, hc, ptr(hs), ptr(hg), ptr(hi), ptr(hl),
                                              C.byref(P) if P is not None else None, C.byref(T) if T is not None else None, fetch, ptr(o3), ptr(o1), None, None,
                                              None, None)

    assert call() == 0 and call(fetch=1) == 0, L.rt_last_error()
    # everything rt_denoise_shards refuses
    for null in ("hdr", "sq", "feat"):
        assert call(**{null: None}) == RT_ERR_INVALID_ARG, null
    assert call(shape=False) == RT_ERR_INVALID_ARG
    for zero in ("W", "num_rows", "world", "block_rows"):
        assert call(**{zero: 0}) == RT_ERR_INVALID_ARG, zero
    assert call(rows_max=2) == RT_ERR_INVALID_ARG
    for bad in (dict(levels=0), dict(levels=6), dict(k_depth=-1.0), dict(k_colour=float("nan")), dict(var_floor=0.0)):
        assert call(P=params_struct(bad)) == RT_ERR_INVALID_ARG, bad
    # null ids (their alignment is the device entry's business)
    assert call(ids=None) == RT_ERR_INVALID_ARG
    # H < first_row + num_rows; W or H above 2^24
    assert call(H=first + rows - 1) == RT_ERR_INVALID_ARG and call(H=first + rows) == 0
    assert call(H=(1 << 24) + 1) == RT_ERR_INVALID_ARG and call(H=1 << 24) == 0
    assert call(W=(1 << 24) + 1, num_rows=1, rows_max=1) == RT_ERR_INVALID_ARG
    # fetch neither 1 nor 4
    for fetch in (0, 2, 3, 5, 0xffffffff):
        assert call(fetch=fetch) == RT_ERR_INVALID_ARG, fetch
    # tparams outside their domain; NULL means that fetch's defaults
    for bad in (dict(max_history=0), dict(max_history=65), dict(depth_tol=-1.0), dict(normal_tol=float("nan")), dict(coverage_tol=float("inf"))):
        assert call(T=_capi.temporal_params_fetch(4, **bad)) == RT_ERR_INVALID_ARG, bad
    # a camera with a non-finite field
    for field, k in (("origin", 0), ("x", 1), ("y", 2), ("origin_image_plane", 0), ("aperture", None), ("focal_length", None)):
        for bad in (float("nan"), float("inf"), float("-inf")):
            c = _capi.RtCamera.from_buffer_copy(bytes(cam))
            if k is None:
                setattr(c, field, bad)
            else:
                getattr(c, field)[k] = bad
            assert call(camera=c) == RT_ERR_INVALID_ARG, (field, bad)
    assert b"camera" in L.rt_last_error()
    # the sample counts: RT_ERR_SEQUENCE, judged after everything else
    for n in (0, 1):
        assert call(n=n) == RT_ERR_SEQUENCE
    assert call(m=0) == RT_ERR_SEQUENCE
    assert call(n=1, rows_max=2) == RT_ERR_INVALID_ARG and call(n=1, fetch=2) == RT_ERR_INVALID_ARG and call(m=0, H=first) == RT_ERR_INVALID_ARG
    # the twin's own: a history without its camera
    assert call(hist_cam=None) == RT_ERR_INVALID_ARG


def test_api_surface(built):
    import inspect
    from cpuraytracer_amd import HipRenderer, _capi, distributed
    L = _capi.load()
    assert L.rt_api_version() == 2  # additions only
    header = open(os.path.join(ROOT, "include", "rt_api.h")).read()
    for name in ("rt_denoise_shards_temporal", "rt_unit_temporal_shards_host"):
        assert hasattr(L, name) and name in _capi.EXPORTS and (" " + name + "(") in header, name
    assert "typedef struct rt_shard_frame" in header
    S = _capi.RtShardFrame  # LP64: parts 64, ids 8, H 4, camera 72, padded to the pointer's alignment
    assert (S.parts.offset, S.ids.offset, S.H.offset, S.camera.offset, C.sizeof(S)) == (0, 64, 72, 76, 152)
    # the device entry fails cleanly on a null context (no GPU is touched)
    fr = _capi.shard_frame(4, 4, 2, 2, 2, 1, _capi.RtCamera())
    assert L.rt_denoise_shards_temporal(None, C.byref(fr), None, None, 1, None) == RT_ERR_INVALID_ARG
    want = ["self", "hdr_ptr", "sq_ptr", "feat_ptr", "ids_ptr", "W", "H", "world", "rows_max", "n", "m", "camera", "params", "tparams", "fetch", "timed",
            "block_rows", "first_row", "num_rows"]
    assert list(inspect.signature(HipRenderer.denoise_shards_temporal).parameters) == want
    assert list(inspect.signature(distributed.denoise_gathered_temporal).parameters) == ["renderer", "xch", "n", "m", "camera", "params", "tparams", "fetch", "timed"]
    assert inspect.signature(distributed.PostExchange.__init__).parameters["with_ids"].default is False


GLOO_W, GLOO_H = 23, 17


def _gloo_strips():
    """hdr, sq, feat and ids whose bits a float conversion would not survive: 0xffffffff (the sky; a NaN as binary32), values above 2^31
    and above 2^24, signalling-NaN patterns, denormals, and small ids."""
    rng = np.random.default_rng(78)
    S, Q, feat = random_strips(rng, GLOO_W, GLOO_H, 4, 3)[:3]
    ids = rng.integers(0, 2 ** 32, (GLOO_H, GLOO_W), dtype=np.uint64).astype(np.uint32)
    ids[0, :6] = (0xffffffff, 0x7fa00001, 0xffa00001, 0x00000001, 0x80000000, 0x01000001)
    ids[1::3] = rng.integers(0, 200, ids[1::3].shape)
    return S, Q, feat, ids


def _worker(rank, world, port, out_path):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch
    import torch.distributed as dist
    from cpuraytracer_amd import distributed as D
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        W, H = GLOO_W, GLOO_H
        S, Q, feat, ids = _gloo_strips()
        mine = [D.global_row(lr, rank, world) for lr in range(D.local_rows(H, rank, world))]
        got = {}
        for with_ids in (True, False):
            xch = D.PostExchange(H, W, rank, world, "cpu", with_ids=with_ids)
            px = xch.rows_max * W
            assert xch.cut == (3 * px, 6 * px, 14 * px) and xch.buf.numel() == (15 if with_ids else 14) * px and xch.buf.dtype == torch.float32
            assert (xch.ids is not None) == with_ids
            xch.buf.fill_(float("nan"))  # whatever the padding holds is never read
            for view, a in zip((xch.hdr, xch.sq, xch.feat), (S, Q, feat)):
                view[:xch.rows] = torch.from_numpy(a[mine])
            if with_ids:
                assert xch.ids.dtype == torch.int32 and xch.ids.shape == (xch.rows_max, W)
                xch.ids[:xch.rows] = torch.from_numpy(ids[mine].view(np.int32))
            parts = xch.gather(through_host=True)
            dist.barrier()
            if rank != 0:
                assert parts == ((None,) * 4 if with_ids else (None,) * 3)
                continue
            assert len(parts) == (4 if with_ids else 3) and (xch.ids_parts is not None) == with_ids
            assert all(p.is_contiguous() for p in parts) and all(p.dtype == torch.float32 for p in parts[:3]) and parts[2].data_ptr() % 16 == 0
            assert parts[0].shape == (world, xch.rows_max, W, 3) and parts[2].shape == (world, xch.rows_max, W, 8)
            if with_ids:
                assert parts[3].dtype == torch.int32 and parts[3].shape == (world, xch.rows_max, W) and parts[3].data_ptr() % 4 == 0
            got[with_ids] = [p.numpy().copy() for p in parts]
        if rank == 0:
            np.savez(out_path, hdr=got[True][0], sq=got[True][1], feat=got[True][2], ids=got[True][3].view(np.uint32), hdr0=got[False][0], sq0=got[False][1],
                     feat0=got[False][2])
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_gloo_gather_brings_the_ids_bit_exact(built, tmp_path, world):
    import torch.multiprocessing as mp
    from cpuraytracer_amd import distributed as D
    out = str(tmp_path / "parts.npz")
    mp.spawn(_worker, args=(world, _free_port(), out), nprocs=world, join=True)
    z = np.load(out)
    S, Q, feat, ids = _gloo_strips()
    for s in range(world):
        mine = [D.global_row(lr, s, world) for lr in range(D.local_rows(GLOO_H, s, world))]
        assert np.array_equal(z["ids"][s, :len(mine)], ids[mine]), "ids of shard %d" % s
        for key, a in (("hdr", S), ("sq", Q), ("feat", feat)):
            assert_same_bits(z[key][s, :len(mine)], a[mine], "%s of shard %d" % (key, s))
            # with_ids=False: what it always was, and what with_ids=True gives beside the ids -- the NaN padding included
            assert np.array_equal(z[key + "0"].view(np.uint32), z[key].view(np.uint32)), key
    assert D.assemble(list(z["ids"]), GLOO_H, world).tobytes() == ids.tobytes()


def test_one_rank_exchange_keeps_its_layout(built):
    """world = 1, no process group: without ids the buffer is the 14 planes it was and gather returns three values; with ids a fifteenth."""
    import torch
    from cpuraytracer_amd import distributed as D
    W, H = 7, 5
    plain = D.PostExchange(H, W, 0, 1, "cpu")
    assert plain.buf.numel() == 14 * W * H and plain.ids is None and plain.ids_parts is None and plain.feat.shape == (H, W, 8)
    plain.buf.copy_(torch.arange(14 * W * H, dtype=torch.float32))
    parts = plain.gather()
    assert len(parts) == 3 and torch.equal(parts[2].reshape(-1), plain.buf[6 * W * H:])
    with_ids = D.PostExchange(H, W, 0, 1, "cpu", with_ids=True)
    assert with_ids.buf.numel() == 15 * W * H and with_ids.feat.shape == (H, W, 8)
    with_ids.ids.copy_(torch.arange(-17, W * H - 17, dtype=torch.int32).view(H, W))
    parts = with_ids.gather()
    assert len(parts) == 4 and torch.equal(parts[3].reshape(-1), torch.arange(-17, W * H - 17, dtype=torch.int32))
    with pytest.raises(ValueError):
        D.denoise_gathered_temporal(None, plain, 2, 1, None)


def test_standalone_selftest(built):
    """host/temporal_shards_selftest.cpp: random shardings, bands and cameras against the contiguous twin -- the shipped program, and
    the same sources built under ASan + UBSan (Makefile temporal_shards_selftest_san), where every index the mapping forms is checked."""
    exe = os.path.join(ROOT, "cpuraytracer_amd", "lib", "temporal_shards_selftest")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "temporal_shards_selftest ok: 300 cases" in p.stdout
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "cpuraytracer_amd", "csrc"), "temporal_shards_selftest_san"], stdout=subprocess.DEVNULL)
    p = subprocess.run([os.path.join(ROOT, "build", "temporal_shards_selftest_san")], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "temporal_shards_selftest ok: 300 cases" in p.stdout
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr
