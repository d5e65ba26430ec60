"""Denoise across row shards, the part that needs no GPU (csrc/rt_rowset_map.h, csrc/host/rt_denoise_host.cpp, distributed.PostExchange;
DESIGN.md "Denoise"): the mapping from an image row to its shard and local row against the two functions it inverts; the host twin over
parts cut from synthetic strips against the contiguous twin on the uncut strips, bit for bit, with NaN in every padding row; the
refusals; the API surface; and the one-gather exchange over gloo in worlds of 2 and 3."""
import ctypes as C
import os
import socket
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_denoise_cpu import DEFAULTS, host_denoise, params_struct, random_strips
from test_noise_estimate_cpu import assert_same_bits

RT_ERR_INVALID_ARG, RT_ERR_SEQUENCE = 2, 6
F = np.float32
N, M = 4, 3  # samples in the synthetic hdr / sq (random_strips relies on 4) and in feat
CASES = [(1, 1, 1, 1), (5, 3, 2, 1), (37, 19, 3, 1), (70, 41, 8, 1), (70, 41, 3, 4)]  # W, H, world, block_rows


def locate(L, rs, j):
    s, lr = C.c_uint32(0xdead), C.c_uint32(0xdead)
    assert L.rt_rowset_locate(rs, j, C.byref(s), C.byref(lr)) == 0
    return s.value, lr.value


def cut(a, world, block_rows, fill=np.nan):
    """[H, W, c] -> [world, rows_max, W, c]: shard s's rows in increasing order, every padding row filled with `fill`."""
    H = a.shape[0]
    rows = [[j for j in range(H) if (j // block_rows) % world == s] for s in range(world)]
    rows_max = max(len(r) for r in rows)
    out = np.full((world, rows_max) + a.shape[1:], fill, dtype=a.dtype)
    for s, r in enumerate(rows):
        out[s, :len(r)] = a[r]
    return out, rows_max


def host_denoise_shards(hdr_p, sq_p, feat_p, W, H, world, block_rows, n, m, P, rows_max=None):
    from cpuraytracer_amd import _capi
    L = _capi.load()
    hdr_p, sq_p, feat_p = (np.ascontiguousarray(a, dtype=F) for a in (hdr_p, sq_p, feat_p))
    shape = _capi.shard_parts(W, H, world, hdr_p.shape[1] if rows_max is None else rows_max, n, m, block_rows=block_rows)
    rgb = np.full((H, W, 3), -1.0, F)
    var = np.full((H, W), -1.0, F)
    ps = params_struct(P)
    _capi.check(L.rt_unit_denoise_shards_host(hdr_p.ctypes.data, sq_p.ctypes.data, feat_p.ctypes.data, C.byref(shape), C.byref(ps), rgb.ctypes.data,
                                              var.ctypes.data))
    return rgb, var


def test_mapping_inverts_global_row(built):
    from cpuraytracer_amd import _capi
    L = _capi.load()
    combos = 0
    for first_row in (0, 3):
        for num_rows in range(1, 51):
            for block_rows in (1, 2, 4, 7):
                for nshards in range(1, 10):
                    local = [L.rt_rowset_local_rows(_capi.RtRowset(first_row, num_rows, block_rows, s, nshards)) for s in range(nshards)]
                    assert sum(local) == num_rows
                    seen = set()
                    for j in range(num_rows):
                        # rs.shard is ignored: any value gives the same answer
                        s, lr = locate(L, _capi.RtRowset(first_row, num_rows, block_rows, (j * 7 + 1) % 11, nshards), j)
                        assert s < nshards and lr < local[s], (first_row, num_rows, block_rows, nshards, j, s, lr)
                        assert L.rt_rowset_global_row(_capi.RtRowset(first_row, num_rows, block_rows, s, nshards), lr) == first_row + j
                        seen.add((s, lr))
                    assert len(seen) == num_rows  # one to one, and by the counts above onto every shard's local rows
                    for s in range(nshards):  # the round trip from the other side
                        rs = _capi.RtRowset(first_row, num_rows, block_rows, s, nshards)
                        for lr in range(local[s]):
                            assert locate(L, rs, L.rt_rowset_global_row(rs, lr) - first_row) == (s, lr)
                    combos += 1
    assert combos == 2 * 50 * 4 * 9
    # refusals: null pointers, a degenerate row set, a row beyond the range
    s, lr = C.c_uint32(), C.c_uint32()
    ok = _capi.RtRowset(0, 8, 1, 0, 2)
    assert L.rt_rowset_locate(ok, 0, None, C.byref(lr)) == RT_ERR_INVALID_ARG and L.rt_rowset_locate(ok, 0, C.byref(s), None) == RT_ERR_INVALID_ARG
    assert L.rt_rowset_locate(ok, 8, C.byref(s), C.byref(lr)) == RT_ERR_INVALID_ARG
    assert L.rt_rowset_locate(_capi.RtRowset(0, 8, 0, 0, 2), 0, C.byref(s), C.byref(lr)) == RT_ERR_INVALID_ARG
    assert L.rt_rowset_locate(_capi.RtRowset(0, 8, 1, 0, 0), 0, C.byref(s), C.byref(lr)) == RT_ERR_INVALID_ARG


@pytest.mark.parametrize("W,H,world,block_rows", CASES, ids=["%dx%d_w%d_b%d" % c for c in CASES])
def test_host_twin_equals_contiguous_twin(built, W, H, world, block_rows):
    rng = np.random.default_rng(1000 * W + 10 * H + world)
    S, Q, feat, _, _ = random_strips(rng, W, H, N, M)
    parts = [cut(a, world, block_rows) for a in (S, Q, feat)]
    rows_max = parts[0][1]
    if world > 1 and H % (world * block_rows) != 0:
        assert any(np.isnan(p[0]).any() for p in parts)  # there IS padding, and it is NaN
    for levels in range(1, 6):
        P = dict(DEFAULTS, levels=levels)
        want = host_denoise(S, Q, N, feat, M, P)
        got = host_denoise_shards(parts[0][0], parts[1][0], parts[2][0], W, H, world, block_rows, N, M, P)
        tag = "%d x %d in %d shards of %d-row blocks, %d levels" % (W, H, world, block_rows, levels)
        assert_same_bits(got[0], want[0], tag + ": den")
        assert_same_bits(got[1], want[1], tag + ": den_var")
        assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    # more padding than the gather needs changes nothing
    wider = [np.concatenate([p[0], np.full((world, 2) + p[0].shape[2:], np.nan, F)], axis=1) for p in parts]
    got = host_denoise_shards(wider[0], wider[1], wider[2], W, H, world, block_rows, N, M, DEFAULTS)
    want = host_denoise(S, Q, N, feat, M, DEFAULTS)
    assert_same_bits(got[0], want[0], "rows_max + 2: den")
    assert_same_bits(got[1], want[1], "rows_max + 2: den_var")
    assert wider[0].shape[1] == rows_max + 2


def test_one_shard_is_the_contiguous_filter(built):
    """world = 1: the one part IS the strip, whatever block_rows."""
    rng = np.random.default_rng(5)
    W, H = 37, 19
    S, Q, feat, _, _ = random_strips(rng, W, H, N, M)
    want = host_denoise(S, Q, N, feat, M, DEFAULTS)
    for block_rows in (1, 4, H, H + 3):
        got = host_denoise_shards(S[None], Q[None], feat[None], W, H, 1, block_rows, N, M, DEFAULTS)
        assert_same_bits(got[0], want[0], "block_rows %d: den" % block_rows)
        assert_same_bits(got[1], want[1], "block_rows %d: den_var" % block_rows)


def test_refusals(built):
    from cpuraytracer_amd import _capi
    L = _capi.load()
    W, H, world = 3, 5, 2  # shard 0 owns rows 0, 2, 4: rows_max = 3
    z3, z8 = np.zeros((world, 3, W, 3), F), np.zeros((world, 3, W, 8), F)
    o3, o1 = np.zeros((H, W, 3), F), np.zeros((H, W), F)
    d = _capi.denoise_params()

    def call(P=d, hdr=z3, sq=z3, feat=z8, rgb=o3, var=o1, shape=True, **over):
        kw = dict(W=W, H=H, world=world, rows_max=3, n=2, m=1, block_rows=1)
        kw.update(over)
        sp = _capi.shard_parts(**kw)
        ptr = lambda a: a.ctypes.data if a is not None else None
        return L.rt_unit_denoise_shards_host(ptr(hdr), ptr(sq), ptr(feat), C.byref(sp) if shape else None, C.byref(P) if P is not None else None,
                                             ptr(rgb), ptr(var))

    assert call() == 0 and call(P=None) == 0  # NULL parameters are the defaults
    for null in ("hdr", "sq", "feat", "rgb", "var"):
        assert call(**{null: None}) == RT_ERR_INVALID_ARG, null
    assert call(shape=False) == RT_ERR_INVALID_ARG
    for zero in ("W", "H", "world", "block_rows"):
        assert call(**{zero: 0}) == RT_ERR_INVALID_ARG, zero
    assert call(rows_max=2) == RT_ERR_INVALID_ARG and call(rows_max=0) == RT_ERR_INVALID_ARG
    assert call(block_rows=2, rows_max=2) == RT_ERR_INVALID_ARG  # blocks {0,1} {2,3} {4}: shard 0 owns 3 rows
    assert call(block_rows=2, rows_max=3) == 0
    for bad in (dict(levels=0), dict(levels=6), dict(k_depth=-1.0), dict(k_colour=float("nan")), dict(k_normal=float("inf")), dict(var_floor=0.0)):
        assert call(P=params_struct(bad)) == RT_ERR_INVALID_ARG, bad
    assert L.rt_last_error()
    for n in (0, 1):
        assert call(n=n) == RT_ERR_SEQUENCE
    assert call(m=0) == RT_ERR_SEQUENCE
    assert call(n=1, rows_max=2) == RT_ERR_INVALID_ARG  # the shape is judged before the sample counts


def test_api_surface(built):
    from cpuraytracer_amd import HipRenderer, _capi, distributed
    L = _capi.load()
    assert L.rt_api_version() == 2  # additions only
    names = ("rt_copy_moments_to_device", "rt_rowset_locate", "rt_denoise_shards", "rt_unit_denoise_shards_host")
    header = open(os.path.join(ROOT, "include", "rt_api.h")).read()
    for name in names:
        assert hasattr(L, name) and name in _capi.EXPORTS and (" " + name + "(") in header, name
    assert "typedef struct rt_shard_parts" in header
    assert C.sizeof(_capi.RtShardParts) == 64 and _capi.RtShardParts.rs.offset == 32 and _capi.RtShardParts.n.offset == 52  # LP64
    # the device entries fail cleanly on a null context (no GPU is touched)
    assert L.rt_copy_moments_to_device(None, None) == RT_ERR_INVALID_ARG
    sp = _capi.shard_parts(4, 4, 2, 2, 2, 1)
    assert L.rt_denoise_shards(None, C.byref(sp), None, None) == RT_ERR_INVALID_ARG
    for name in ("copy_moments_to_device", "denoise_shards"):
        assert callable(getattr(HipRenderer, name))
    assert callable(distributed.PostExchange) and callable(distributed.denoise_gathered)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


GLOO_W, GLOO_H = 23, 17


def _strips():
    return random_strips(np.random.default_rng(77), GLOO_W, GLOO_H, N, M)[:3]


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
        xch = D.PostExchange(H, W, rank, world, "cpu")
        assert xch.rows == D.local_rows(H, rank, world) and xch.rows_max == D.max_local_rows(H, world)
        xch.buf.fill_(float("nan"))  # whatever the padding holds is never read
        mine = [D.global_row(lr, rank, world) for lr in range(xch.rows)]
        for view, a in zip((xch.hdr, xch.sq, xch.feat), _strips()):
            view[:xch.rows] = torch.from_numpy(a[mine])
        parts = xch.gather(through_host=True)
        dist.barrier()
        if rank != 0:
            assert parts == (None, None, None)
            return
        hp, qp, fp = (p.numpy() for p in parts)
        assert hp.shape == (world, xch.rows_max, W, 3) and fp.shape == (world, xch.rows_max, W, 8)
        assert all(p.is_contiguous() and p.dtype == torch.float32 for p in parts) and parts[2].data_ptr() % 16 == 0
        rgb, var = host_denoise_shards(hp, qp, fp, W, H, world, D.BLOCK_ROWS, N, M, DEFAULTS)
        np.savez(out_path, rgb=rgb, var=var, padded=np.isnan(hp).any())
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_gloo_gather_then_host_twin(built, tmp_path, world):
    import torch.multiprocessing as mp
    out = str(tmp_path / "den.npz")
    mp.spawn(_worker, args=(world, _free_port(), out), nprocs=world, join=True)
    z = np.load(out)
    S, Q, feat = _strips()
    want = host_denoise(S, Q, N, feat, M, DEFAULTS)
    assert_same_bits(z["rgb"], want[0], "world %d: den" % world)
    assert_same_bits(z["var"], want[1], "world %d: den_var" % world)
    assert bool(z["padded"]) == (GLOO_H % world != 0)
