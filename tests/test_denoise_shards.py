"""Denoise across row shards on the device (rt_denoise_shards, rt_copy_moments_to_device; csrc/rt_denoise.hip
rt_denoise_prepare_shards_kernel): one context renders the picture shard after shard, copies every shard's strips device to device into
its slot of parts buffers that were filled with 0xff bytes (whatever padding is read becomes NaN), and the filter over the parts must
give the bits of rt_denoise in a context that rendered the whole image -- and the host twin's; that nothing else of the context
changes; the refusals; and two rank processes sharing device 0 that gather through distributed.PostExchange."""
import ctypes as C
import os
import socket
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_denoise import OTHER, forms_for, prepare, strips
from test_denoise_cpu import DEFAULTS, params_struct
from test_denoise_shards_cpu import host_denoise_shards
from test_noise_estimate_cpu import assert_same_bits

pytestmark = pytest.mark.gpu

RT_ERR_INVALID_ARG, RT_ERR_SEQUENCE = 2, 6
N, M = 8, 8
SHARDINGS = [(1, 1), (2, 1), (3, 1), (8, 1), (3, 4)]  # world, block_rows
SIZES = [(96, 64), (70, 41)]


@pytest.fixture(scope="module")
def hiprt(built):
    """The HIP runtime librt_hip.so is linked against: the caller-owned device memory of these tests."""
    from cpuraytracer_amd import _capi
    _capi.load()
    maps = open("/proc/self/maps").read()
    return C.CDLL(next(l.split()[-1] for l in maps.splitlines() if "libamdhip64.so" in l))


class DevMem:
    def __init__(self, hiprt, nbytes, fill=0xff):
        self.hiprt, self.nbytes, self.ptr = hiprt, nbytes, C.c_void_p()
        assert hiprt.hipMalloc(C.byref(self.ptr), C.c_size_t(nbytes)) == 0
        assert hiprt.hipMemset(self.ptr, C.c_int(fill), C.c_size_t(nbytes)) == 0
        assert hiprt.hipDeviceSynchronize() == 0

    def at(self, byte_offset):
        assert 0 <= byte_offset < self.nbytes
        return self.ptr.value + byte_offset

    def download(self, dtype, shape):
        out = np.zeros(shape, dtype)
        assert out.nbytes == self.nbytes
        assert self.hiprt.hipMemcpy(C.c_void_p(out.ctypes.data), self.ptr, C.c_size_t(self.nbytes), 2) == 0  # device to host
        return out

    def free(self):
        if self.ptr:
            self.hiprt.hipFree(self.ptr)
            self.ptr = C.c_void_p()


@pytest.fixture()
def dr(built):
    from cpuraytracer_amd import HipRenderer
    r = HipRenderer(0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def whole(built):
    """Per size: the cover scene rendered whole in one context (samples 1..8, features 1..8), its strips, and rt_denoise's rgb, var and
    ldr for the defaults and OTHER at levels 1..5 (RT_DENOISE_STAGE unset) -- computed once, never changed."""
    from cpuraytracer_amd import HipRenderer, scenes
    saved = os.environ.pop("RT_DENOISE_STAGE", None)
    out = {}
    r = HipRenderer(0)
    try:
        for W, H in SIZES:
            sc = scenes.build_scene("cover", 1, W, H)
            prepare(r, sc, W, H, N, M)
            S = strips(r)
            wants = {}
            for name, over in (("defaults", {}), ("other", OTHER)):
                for levels in range(1, 6):
                    P = dict(DEFAULTS, levels=levels, **over)
                    r.denoise(params_struct(P))
                    wants[(name, levels)] = (P, r.download_denoised())
            for a in S + tuple(a for _, d in wants.values() for a in d.values()):
                a.setflags(write=False)
            out[(W, H)] = (sc, S, wants)
    finally:
        r.close()
        if saved is not None:
            os.environ["RT_DENOISE_STAGE"] = saved
    return out


def render_into_parts(r, hiprt, sc, W, H, world, block_rows):
    """Render shard after shard in r, copying each shard's hdr, sq and feat strips into its slot of 0xff-filled parts buffers."""
    from cpuraytracer_amd import _capi
    L = _capi.load()
    rows = [L.rt_rowset_local_rows(_capi.RtRowset(0, H, block_rows, s, world)) for s in range(world)]
    rows_max = max(rows)
    px = rows_max * W
    bufs = [DevMem(hiprt, world * px * c * 4) for c in (3, 3, 8)]
    r.upload(sc)
    r.set_noise_estimate(True)
    for s in range(world):
        rs = _capi.RtRowset(0, H, block_rows, s, world)
        r.render(W, H, 1, 1 + N, 50, 1, rowset=rs, stats=False)
        r.render_features(W, H, 1, 1 + M, rowset=rs)
        r.copy_to_device(bufs[0].at(s * px * 12), None)
        r.copy_moments_to_device(bufs[1].at(s * px * 12))
        r.copy_features_to_device(bufs[2].at(s * px * 32), None)
    r.synchronize()
    return bufs, rows, rows_max


def check(r, want, what):
    d = r.download_denoised()
    assert_same_bits(d["rgb"], want["rgb"], what + ": rgb")
    assert_same_bits(d["var"], want["var"], what + ": var")
    assert np.array_equal(d["ldr"], want["ldr"]), what + ": ldr"
    return d


@pytest.mark.parametrize("W,H", SIZES, ids=["%dx%d" % s for s in SIZES])
@pytest.mark.parametrize("world,block_rows", SHARDINGS, ids=["w%d_b%d" % s for s in SHARDINGS])
def test_shards_equal_the_contiguous_filter(dr, hiprt, whole, monkeypatch, W, H, world, block_rows):
    sc, S, wants = whole[(W, H)]
    bufs, rows, rows_max = render_into_parts(dr, hiprt, sc, W, H, world, block_rows)
    try:
        hp, qp = (b.download(np.float32, (world, rows_max, W, 3)) for b in bufs[:2])
        fp = bufs[2].download(np.float32, (world, rows_max, W, 8))
        # the parts hold the whole-image strips' rows, and NaN (0xff bytes) in every padding row
        for s in range(world):
            own = [j for j in range(H) if (j // block_rows) % world == s]
            assert len(own) == rows[s]
            for part, full, what in ((hp, S[0], "hdr"), (qp, S[1], "sq"), (fp, S[2], "feat")):
                assert_same_bits(part[s, :rows[s]], full[own], "%s of shard %d" % (what, s))
                assert (part[s, rows[s]:].view(np.uint32) == 0xffffffff).all()
        assert (min(rows) < rows_max) == any(np.isnan(p).any() for p in (hp, qp, fp))
        for knob in (None, "0", "1"):
            if knob is None:
                monkeypatch.delenv("RT_DENOISE_STAGE", raising=False)
            else:
                monkeypatch.setenv("RT_DENOISE_STAGE", knob)
            for (name, levels), (P, want) in wants.items():
                default_call = (name, levels) == ("defaults", 3)
                ms = dr.denoise_shards(bufs[0].at(0), bufs[1].at(0), bufs[2].at(0), W, H, world, rows_max, N, M,
                                       params=None if default_call else params_struct(P), timed=(levels == 2), block_rows=block_rows)
                assert (ms is not None and ms > 0.0) if levels == 2 else ms is None
                what = "%d x %d in %d shards of %d-row blocks, %s, %d levels, RT_DENOISE_STAGE=%s" % (W, H, world, block_rows, name, levels, knob)
                assert dr.denoise_forms() == forms_for(levels, knob), what
                d = check(dr, want, what)
                if knob is None:
                    twin = host_denoise_shards(hp, qp, fp, W, H, world, block_rows, N, M, P)
                    assert_same_bits(d["rgb"], twin[0], what + ": rgb vs the host twin")
                    assert_same_bits(d["var"], twin[1], what + ": var vs the host twin")
        # the device copy serves the result as after rt_denoise
        out = DevMem(hiprt, W * H * 4, fill=0)
        try:
            dr.copy_denoised_to_device(None, out.at(0), None)
            dr.synchronize()
            assert_same_bits(out.download(np.float32, (H, W)), dr.download_denoised()["var"], "copy_denoised_to_device")
        finally:
            out.free()
    finally:
        for b in bufs:
            b.free()


def test_copy_moments_to_device(dr, hiprt, whole):
    from cpuraytracer_amd import _capi
    W, H = 70, 41
    sc, S, wants = whole[(W, H)]
    n = W * H * 3 + 256
    dev = DevMem(hiprt, n * 4)
    try:
        dr.upload(sc)
        dr.render(W, H, 1, 3, 50, 1)
        with pytest.raises(_capi.RtError) as e:   # the switch is off
            dr.copy_moments_to_device(dev.at(0))
        assert e.value.code == RT_ERR_SEQUENCE
        dr.set_noise_estimate(True)
        with pytest.raises(_capi.RtError) as e:   # nothing accumulated
            dr.copy_moments_to_device(dev.at(0))
        assert e.value.code == RT_ERR_SEQUENCE
        dr.render(W, H, 1, 1 + N, 50, 1)
        with pytest.raises(_capi.RtError) as e:
            dr.copy_moments_to_device(None)
        assert e.value.code == RT_ERR_INVALID_ARG
        dr.copy_moments_to_device(dev.at(0))
        dr.synchronize()
        got = dev.download(np.float32, n)
        assert_same_bits(got[:W * H * 3].reshape(H, W, 3), dr.download_moments(), "rt_copy_moments_to_device vs rt_download_moments")
        assert_same_bits(got[:W * H * 3].reshape(H, W, 3), S[1], "... and the fixture's")
        assert (got[W * H * 3:].view(np.uint32) == 0xffffffff).all()  # and not a byte beyond the strip
    finally:
        dev.free()


def test_independence(dr, hiprt, whole):
    """rt_denoise_shards between two halves of an accumulation of ANOTHER picture size: hdr, sq, feat and ldr end on the one-shot bits.
    And a context without a scene runs it."""
    from cpuraytracer_amd import HipRenderer
    W, H = 96, 64
    sc, S, wants = whole[(W, H)]
    sc2, S2, wants2 = whole[(70, 41)]
    maker = HipRenderer(0)
    try:
        bufs, rows, rows_max = render_into_parts(maker, hiprt, sc2, 70, 41, 3, 1)
    finally:
        maker.close()
    try:
        dr.upload(sc)
        dr.set_noise_estimate(True)
        dr.render(W, H, 1, 5, 50, 1, stats=False)
        dr.render_features(W, H, 1, 5)
        dr.denoise_shards(bufs[0].at(0), bufs[1].at(0), bufs[2].at(0), 70, 41, 3, rows_max, N, M)
        check(dr, wants2[("defaults", 3)][1], "between the halves")
        assert dr.committed_samples() == 4 and dr.feature_samples() == 4
        dr.render(W, H, 5, 9, 50, 1, stats=False)
        dr.render_features(W, H, 5, 9)
        dr.denoise_shards(bufs[0].at(0), bufs[1].at(0), bufs[2].at(0), 70, 41, 3, rows_max, N, M, timed=True)
        dr.resolve()
        got = strips(dr)
        for a, b, what in zip(got, S, ("hdr", "sq", "feat")):
            assert_same_bits(a, b, what + " after a render with rt_denoise_shards in between")
        one = HipRenderer(0)
        try:
            prepare(one, sc, W, H, N, M)
            one.resolve()
            assert np.array_equal(dr.download(hdr=False)[1], one.download(hdr=False)[1]), "ldr"
        finally:
            one.close()
        dr.denoise()  # the context's own picture is still what rt_denoise filters
        check(dr, wants[("defaults", 3)][1], "rt_denoise afterwards")
        fresh = HipRenderer(0)  # no scene, no accumulation
        try:
            fresh.denoise_shards(bufs[0].at(0), bufs[1].at(0), bufs[2].at(0), 70, 41, 3, rows_max, N, M, params=params_struct(wants2[("other", 5)][0]))
            check(fresh, wants2[("other", 5)][1], "a context without a scene")
        finally:
            fresh.close()
    finally:
        for b in bufs:
            b.free()


def test_refusals_on_the_device_path(dr, hiprt, whole):
    from cpuraytracer_amd import _capi
    L = _capi.load()
    W, H, world = 70, 41, 3
    sc, S, wants = whole[(W, H)]
    bufs, rows, rows_max = render_into_parts(dr, hiprt, sc, W, H, world, 1)
    try:
        ptrs = dict(hdr=bufs[0].at(0), sq=bufs[1].at(0), feat=bufs[2].at(0))

        def call(P=None, ctx=True, shape=True, **over):
            kw = dict(W=W, H=H, world=world, rows_max=rows_max, n=N, m=M, block_rows=1, **ptrs)
            kw.update(over)
            sp = _capi.shard_parts(**kw)
            return L.rt_denoise_shards(dr._h if ctx else None, C.byref(sp) if shape else None, C.byref(P) if P is not None else None, None)

        with pytest.raises(_capi.RtError) as e:
            dr.download_denoised()  # nothing denoised yet in this context
        assert e.value.code == RT_ERR_SEQUENCE
        assert call(ctx=False) == RT_ERR_INVALID_ARG and call(shape=False) == RT_ERR_INVALID_ARG
        for null in ("hdr", "sq", "feat"):
            assert call(**{null: None}) == RT_ERR_INVALID_ARG, null
        for zero in ("W", "H", "world", "block_rows"):
            assert call(**{zero: 0}) == RT_ERR_INVALID_ARG, zero
        assert call(rows_max=rows_max - 1) == RT_ERR_INVALID_ARG
        for off in (4, 8, 12):
            assert call(feat=ptrs["feat"] + off) == RT_ERR_INVALID_ARG, off
        for bad in (dict(levels=0), dict(levels=6), dict(k_albedo=-1.0), dict(k_colour=float("nan")), dict(var_floor=0.0)):
            assert call(P=params_struct(bad)) == RT_ERR_INVALID_ARG, bad
        for n in (0, 1):
            assert call(n=n) == RT_ERR_SEQUENCE
        assert call(m=0) == RT_ERR_SEQUENCE
        with pytest.raises(_capi.RtError):
            dr.download_denoised()  # a refused call leaves no result
        assert dr.denoise_forms() == [0] * 5
        # (through the Python view, which records the result's size for download_denoised; `call` goes to the library directly)
        dr.denoise_shards(ptrs["hdr"], ptrs["sq"], ptrs["feat"], W, H, world, rows_max, N, M)
        assert (dr.denoised_W, dr.denoised_rows) == (W, H)
        check(dr, wants[("defaults", 3)][1], "after the refusals")
        assert call(n=1) == RT_ERR_SEQUENCE
        check(dr, wants[("defaults", 3)][1], "a refused call keeps the snapshot")
    finally:
        for b in bufs:
            b.free()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank(rank, world, port, W, H, out_path):
    sys.path.insert(0, ROOT)
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
        r.upload(scenes.build_scene("cover", 1, W, H))
        r.set_noise_estimate(True)
        rs = D.shard_rowset(H, rank, world)
        r.render(W, H, 1, 1 + N, 50, 1, rowset=rs, stats=False)
        r.render_features(W, H, 1, 1 + M, rowset=rs)
        xch = D.PostExchange(H, W, rank, world, "cuda:0")
        xch.buf.fill_(float("nan"))
        torch.cuda.synchronize()
        xch.fill(r)
        r.synchronize()
        parts = xch.gather(through_host=True)
        if rank == 0:
            assert all(p.is_cuda and p.is_contiguous() for p in parts) and parts[2].data_ptr() % 16 == 0
            D.denoise_gathered(r, xch, N, M)
            np.savez(out_path, **r.download_denoised())
        else:
            assert parts == (None, None, None)
        dist.barrier()
    finally:
        if r is not None:
            r.close()
        dist.destroy_process_group()


def test_two_rank_rehearsal_on_one_device(built, whole, tmp_path, monkeypatch):
    """Two rank processes share device 0 (gloo, strips through host memory -- the recipe of bench.py's rehearsal): each renders its rows
    with moments and features, one PostExchange gather, denoise_gathered on rank 0.  41 rows: rank 1's part has a padding row."""
    import torch.multiprocessing as mp
    W, H = 70, 41
    sc, S, wants = whole[(W, H)]
    monkeypatch.setenv("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    monkeypatch.delenv("RT_DENOISE_STAGE", raising=False)
    out = str(tmp_path / "den.npz")
    mp.spawn(_rank, args=(2, _free_port(), W, H, out), nprocs=2, join=True)
    z = np.load(out)
    want = wants[("defaults", 3)][1]
    assert z["rgb"].shape == (H, W, 3) and z["ldr"].dtype == np.uint8
    assert_same_bits(z["rgb"], want["rgb"], "two ranks: rgb")
    assert_same_bits(z["var"], want["var"], "two ranks: var")
    assert np.array_equal(z["ldr"], want["ldr"])
