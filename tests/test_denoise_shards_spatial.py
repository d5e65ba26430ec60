"""The spatial variance source across row shards on the device (rt_denoise_shards_variance, rt_denoise_shards_temporal_variance;
csrc/rt_denoise.hip rt_denoise_prepare_spatial_shards_kernel and rt_denoise_prepared_shards_temporal_kernel with its bilinear sibling): a
reference context renders every frame of an orbit whole (or a band of it contiguously) at ONE sample per pixel with the noise estimate
off and calls rt_denoise_variance and rt_denoise_temporal_variance; a second context renders the frame shard after shard into 0xff-filled
parts -- whatever padding is read becomes NaN -- with no buffer of second moments at all, and the sharded calls over them must give the
reference's bits frame by frame -- den, den_var, ldr, the history's state, len and target -- and the host twins'; alternation of sources
and forms over one history; the moments source through the new entries; that nothing else of the context changes; the refusals; and two
rank processes sharing device 0 that gather through distributed.PostExchange(with_moments=False, with_ids=True)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from denoise_spatial_common import BILINEAR, MOMENTS, NEAREST, SPATIAL, variance_struct
from temporal_common import NO_TARGET, history_of, orbit_scene
from test_denoise import forms_for
from test_denoise_cpu import DEFAULTS, params_struct
from test_denoise_shards import DevMem, _free_port, hiprt  # noqa: F401  (hiprt: a fixture)
from test_denoise_spatial import dr, render_frame, scenes, strips  # noqa: F401  (dr, scenes: fixtures)
from test_noise_estimate_cpu import assert_same_bits

pytestmark = pytest.mark.gpu

RT_ERR_INVALID_ARG, RT_ERR_SEQUENCE = 2, 6
N, M = 1, 2            # ONE sample in hdr, the features after two (m != n)
FRAMES, STEP = 3, 0.5  # the orbit: degrees per frame; frame f has seed 1 + f (test_denoise_spatial.render_frame)
SHARDINGS = [(1, 1), (2, 1), (3, 1), (8, 1), (3, 4)]  # world, block_rows
SHAPES = {"96x64": (96, 64, 0, 64), "70x41": (70, 41, 0, 41), "band": (70, 41, 5, 29), "5x3": (5, 3, 0, 3)}  # W, H, first_row, num_rows
KEYS = ("rgb", "var", "state")
# shape, world, block_rows -> the (R, levels, knobs) it runs: every sharding at R = 1 with 1, 3 and 5 levels under every RT_DENOISE_STAGE;
# R = 2 and 3 where halos cross shard (3, 1) and block (3, 4) boundaries; the band and the picture smaller than a tile at R = 1 and 3
ALL_KNOBS = (None, "0", "1")
CASES = {}
for _k in ("96x64", "70x41"):
    for _w, _b in SHARDINGS:
        CASES[(_k, _w, _b)] = [(1, lv, ALL_KNOBS) for lv in (1, 3, 5)] + ([(2, 3, (None,)), (3, 3, (None,))] if _w == 3 else [])
for _c in (("band", 3, 1), ("5x3", 2, 1), ("5x3", 3, 1)):
    CASES[_c] = [(1, 3, (None,)), (3, 3, (None,))]
VARIANTS = sorted({(k, R, lv) for (k, _, _), v in CASES.items() for R, lv, _ in v})


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


def same_plain(got, want, what):
    assert_same_bits(got["rgb"], want["rgb"], what + ": den")
    assert_same_bits(got["var"], want["var"], what + ": den_var")
    assert np.array_equal(got["ldr"], want["ldr"]), what + ": ldr"


def contiguous_rowset(shape):
    W, H, first, rows = SHAPES[shape]
    return None if (first, rows) == (0, H) else (first, rows, rows, 0, 1)


@pytest.fixture(scope="module")
def reference(built, scenes):
    """Per shape, radius, level count and fetch: the orbit's frames rendered contiguously in one context at n = 1, m = 2 with the noise
    estimate off, rt_denoise_variance and then rt_denoise_temporal_variance (that fetch's defaults) on each, and what they left
    (RT_DENOISE_STAGE unset) -- computed once, never changed.  [(shape, R, levels, fetch)][f] = the temporal result, "plain": the filter's."""
    from cpuraytracer_amd import HipRenderer
    saved = os.environ.pop("RT_DENOISE_STAGE", None)
    out = {}
    r = HipRenderer(0)
    try:
        for shape, R, levels in VARIANTS:
            W, H, first, rows = SHAPES[shape]
            V = variance_struct(SPATIAL, R)
            for fetch in (NEAREST, BILINEAR):
                r.temporal_reset()
                seq = []
                for f in range(FRAMES):
                    render_frame(r, scenes, W, H, f, contiguous_rowset(shape), deg=STEP, n=N, m=M)
                    r.denoise(params_of(levels), variance=V)
                    plain = r.download_denoised()
                    r.denoise_temporal(params_of(levels), None, fetch=fetch, variance=V)
                    seq.append(dict(result(r), plain=plain))
                    for a in list(seq[-1].values())[:-1] + list(plain.values()):
                        a.setflags(write=False)
                    if f > 0 and W * rows > 100:  # the orbit is not vacuous: the history was used, the move rejected some pixels and shifted others
                        acc = seq[-1]["target"] != NO_TARGET
                        own = np.arange(acc.size, dtype=np.uint32).reshape(acc.shape)
                        assert acc.any() and (~acc).any() and (seq[-1]["target"][acc] != own[acc]).any(), (shape, R, fetch, f)
                out[(shape, R, levels, fetch)] = seq
    finally:
        r.close()
        if saved is not None:
            os.environ["RT_DENOISE_STAGE"] = saved
    return out


def render_parts(r, hiprt, scenes, shape, f, world, block_rows, n=N, noise=False):
    """Frame f of the orbit rendered shard after shard in r at n samples, each shard's hdr, feat and id strips copied device to device
    into its slot of 0xff-filled parts buffers.  bufs[1], the second moments, exists only with the noise estimate on."""
    from cpuraytracer_amd import _capi
    L = _capi.load()
    W, H, first, num_rows = SHAPES[shape]
    sc = orbit_scene(scenes, "cover", W, H, STEP * f)
    rows = [L.rt_rowset_local_rows(_capi.RtRowset(first, num_rows, block_rows, s, world)) for s in range(world)]
    rows_max = max(rows)
    px = rows_max * W
    bufs = [DevMem(hiprt, world * px * c * 4) if c else None for c in (3, 3 if noise else 0, 8, 1)]
    r.upload(sc)
    r.set_noise_estimate(noise)
    for s in range(world):
        rs = _capi.RtRowset(first, num_rows, block_rows, s, world)
        if rows[s] == 0:
            continue
        r.render(W, H, 1, 1 + n, 50, 1 + f, rowset=rs, stats=False)
        r.render_features(W, H, 1, 1 + M, rowset=rs)
        r.copy_to_device(bufs[0].at(s * px * 12), None)
        if noise:
            r.copy_moments_to_device(bufs[1].at(s * px * 12))
        r.copy_features_to_device(bufs[2].at(s * px * 32), bufs[3].at(s * px * 4))
    r.synchronize()
    return dict(bufs=bufs, rows=rows, rows_max=rows_max, cam=sc.camera, shape=shape, world=world, block_rows=block_rows, n=n)


@pytest.fixture(scope="module")
def parts_of(built, hiprt, scenes):
    """parts_of(shape, world, block_rows, n=1, noise=False) -> the orbit's frames as parts on the device, rendered once per module by a
    context of their own."""
    from cpuraytracer_amd import HipRenderer
    cache = {}
    maker = HipRenderer(0)

    def get(shape, world, block_rows, n=N, noise=False):
        key = (shape, world, block_rows, n, noise)
        if key not in cache:
            cache[key] = [render_parts(maker, hiprt, scenes, shape, f, world, block_rows, n, noise) for f in range(FRAMES)]
        return cache[key]

    yield get
    maker.close()
    for frames in cache.values():
        for fp in frames:
            for b in fp["bufs"]:
                if b is not None:
                    b.free()


def sq_of(fp):
    return fp["bufs"][1].at(0) if fp["bufs"][1] is not None else None


def plain_call(r, fp, V, params=None, timed=False):
    W, H, first, num_rows = SHAPES[fp["shape"]]
    assert first == 0 and num_rows == H
    b = fp["bufs"]
    return r.denoise_shards(b[0].at(0), sq_of(fp), b[2].at(0), W, H, fp["world"], fp["rows_max"], fp["n"], M, params=params, timed=timed,
                            block_rows=fp["block_rows"], variance=V)


def shards_call(r, fp, V, params=None, tparams=None, fetch=BILINEAR, timed=False):
    W, H, first, num_rows = SHAPES[fp["shape"]]
    b = fp["bufs"]
    return r.denoise_shards_temporal_variance(b[0].at(0), sq_of(fp), b[2].at(0), b[3].at(0), W, H, fp["world"], fp["rows_max"], fp["n"], M, fp["cam"],
                                              params=params, tparams=tparams, fetch=fetch, timed=timed, block_rows=fp["block_rows"], first_row=first,
                                              num_rows=num_rows, variance=V)


def shards_step(r, fp, R=1, levels=3, fetch=BILINEAR):
    shards_call(r, fp, variance_struct(SPATIAL, R), params_of(levels), None, fetch)
    return result(r)


def download_parts(fp):
    W = SHAPES[fp["shape"]][0]
    shape = (fp["world"], fp["rows_max"], W)
    b = fp["bufs"]
    return [b[0].download(np.float32, shape + (3,)), b[2].download(np.float32, shape + (8,)), b[3].download(np.uint32, shape)]


def twin_step(fp, parts, hist, R, levels, fetch):
    from cpuraytracer_amd import _capi
    W, H, first, num_rows = SHAPES[fp["shape"]]
    frame = _capi.shard_frame(W, H, fp["world"], fp["rows_max"], N, M, fp["cam"], block_rows=fp["block_rows"], first_row=first, num_rows=num_rows)
    return _capi.unit_temporal_shards_variance_host(parts[0], None, parts[1], parts[2], frame, history=hist, params=params_of(levels), tparams=None,
                                                    fetch=fetch, variance=variance_struct(SPATIAL, R))


@pytest.mark.parametrize("shape,world,block_rows", list(CASES), ids=["%s_w%d_b%d" % c for c in CASES])
def test_device_equals_reference_and_twin(dr, reference, parts_of, monkeypatch, shape, world, block_rows):
    frames = parts_of(shape, world, block_rows)
    assert all(fp["bufs"][1] is None for fp in frames)  # no buffer of second moments exists
    host = [download_parts(fp) for fp in frames]
    for fp, parts in zip(frames, host):  # every padding row holds 0xff bytes
        for s in range(world):
            assert all((p[s, fp["rows"][s]:].view(np.uint32) == 0xffffffff).all() for p in parts)
        assert (min(fp["rows"]) < fp["rows_max"]) == np.isnan(parts[0]).any()
    whole = SHAPES[shape][2:] == (0, SHAPES[shape][1])
    for R, levels, knobs in CASES[(shape, world, block_rows)]:
        V = variance_struct(SPATIAL, R)
        for fetch in (NEAREST, BILINEAR):
            for knob in knobs:
                if knob is None:
                    monkeypatch.delenv("RT_DENOISE_STAGE", raising=False)
                else:
                    monkeypatch.setenv("RT_DENOISE_STAGE", knob)
                dr.temporal_reset()
                hist = None
                for f, fp in enumerate(frames):
                    what = "%s in %d shards of %d-row blocks, R %d, fetch %d, %d levels, RT_DENOISE_STAGE=%s, frame %d" % (shape, world, block_rows, R, fetch,
                                                                                                                      levels, knob, f)
                    want = reference[(shape, R, levels, fetch)][f]
                    if whole and fetch == NEAREST:  # the plain entry (it leaves the history alone)
                        plain_call(dr, fp, V, params_of(levels))
                        assert dr.denoise_forms() == forms_for(levels, knob), what
                        same_plain(dr.download_denoised(), want["plain"], what + ", rt_denoise_shards_variance")
                    got = shards_step(dr, fp, R, levels, fetch)
                    assert dr.denoise_forms() == forms_for(levels, knob), what
                    same(got, want, what)
                    if knob is None:
                        twin = twin_step(fp, host[f], hist, R, levels, fetch)
                        for k in KEYS:
                            assert_same_bits(got[k], twin[k], what + ": %s vs the host twin" % k)
                        assert np.array_equal(got["len"], twin["len"]) and np.array_equal(got["target"], twin["target"]), what + " vs the host twin"
                        hist = history_of(twin)


def test_alternation_over_one_history(dr, parts_of, scenes):
    """One shard with the whole image's key: a shards-spatial frame, a shards-moments frame and a contiguous spatial frame over one
    history give the bits of the same sequence of contiguous calls."""
    from cpuraytracer_amd import HipRenderer
    shape = "70x41"
    W, H = SHAPES[shape][:2]
    V = variance_struct(SPATIAL, 2)
    one = parts_of(shape, 1, H)                    # n = 1, no sq
    two = parts_of(shape, 1, H, n=2, noise=True)   # the moments frame needs n = 2 and sq
    ref = HipRenderer(0)
    try:
        want = []
        render_frame(ref, scenes, W, H, 0, deg=STEP, n=1, m=M)
        ref.denoise_temporal(None, None, fetch=BILINEAR, variance=V)
        want.append(result(ref))
        render_frame(ref, scenes, W, H, 1, deg=STEP, n=2, m=M, noise=True)
        ref.denoise_temporal(None, None, fetch=NEAREST)
        want.append(result(ref))
        render_frame(ref, scenes, W, H, 2, deg=STEP, n=1, m=M)
        ref.denoise_temporal(None, None, fetch=BILINEAR, variance=V)
        want.append(result(ref))
    finally:
        ref.close()
    assert want[2]["len"].max() == 3 and (want[1]["target"] != NO_TARGET).any()
    dr.temporal_reset()
    shards_call(dr, one[0], V, fetch=BILINEAR)
    same(result(dr), want[0], "frame 0, shards, spatial")
    shards_call(dr, two[1], variance_struct(MOMENTS, 1), fetch=NEAREST)
    same(result(dr), want[1], "frame 1, shards, moments")
    render_frame(dr, scenes, W, H, 2, deg=STEP, n=1, m=M)
    dr.denoise_temporal(None, None, fetch=BILINEAR, variance=V)
    same(result(dr), want[2], "frame 2, contiguous, spatial")
    # ... and the reverse: a contiguous call's history continued by the sharded entry
    dr.temporal_reset()
    render_frame(dr, scenes, W, H, 0, deg=STEP, n=1, m=M)
    dr.denoise_temporal(None, None, fetch=BILINEAR, variance=V)
    same(result(dr), want[0], "frame 0, contiguous, spatial")
    shards_call(dr, two[1], None, fetch=NEAREST)
    same(result(dr), want[1], "frame 1, shards, variance=None")
    shards_call(dr, one[2], V, fetch=BILINEAR)
    same(result(dr), want[2], "frame 2, shards, spatial")


def test_moments_source_through_the_new_entries(dr, parts_of):
    """vparams == NULL or RT_VARIANCE_MOMENTS: rt_denoise_shards' and rt_denoise_shards_temporal's bits, history and refusals."""
    from cpuraytracer_amd import _capi
    shape = "70x41"
    W, H = SHAPES[shape][:2]
    frames = parts_of(shape, 3, 1, n=2, noise=True)
    Mo = variance_struct(MOMENTS, 3)
    b = frames[0]["bufs"]
    dr.denoise_shards(b[0].at(0), b[1].at(0), b[2].at(0), W, H, 3, frames[0]["rows_max"], 2, M)
    want = dr.download_denoised()
    plain_call(dr, frames[0], Mo)
    same_plain(dr.download_denoised(), want, "moments through rt_denoise_shards_variance")
    for fetch in (NEAREST, BILINEAR):
        seqs = []
        for V in (None, Mo):
            dr.temporal_reset()
            seq = []
            for fp in frames[:2]:
                if V is None:
                    b = fp["bufs"]
                    dr.denoise_shards_temporal(b[0].at(0), b[1].at(0), b[2].at(0), b[3].at(0), W, H, 3, fp["rows_max"], 2, M, fp["cam"], fetch=fetch)
                else:
                    shards_call(dr, fp, V, fetch=fetch)
                seq.append(result(dr))
            seqs.append(seq)
        for f in range(2):
            same(seqs[1][f], seqs[0][f], "moments through rt_denoise_shards_temporal_variance, fetch %d, frame %d" % (fetch, f))
        assert (seqs[0][1]["len"] == 2).any()
    # its refusals are the existing entries': one sample is too few, and sq is needed
    one = parts_of(shape, 3, 1)[0]
    for V in (None, Mo):
        with pytest.raises(_capi.RtError) as e:
            shards_call(dr, dict(frames[0], n=1), V)
        assert e.value.code == RT_ERR_SEQUENCE and "rt_denoise_shards_temporal:" in str(e.value)
        with pytest.raises(_capi.RtError) as e:
            shards_call(dr, dict(one, n=2), V)
        assert e.value.code == RT_ERR_INVALID_ARG


def test_independence(dr, reference, parts_of, scenes):
    """The calls between two halves of an accumulation of ANOTHER picture size change nothing of the render, its features and LDR, and
    the render that continues ends on its one-shot bits; a context without a scene runs them."""
    from cpuraytracer_amd import HipRenderer
    shape = "70x41"
    ref = reference[(shape, 1, 3, BILINEAR)]
    frames = parts_of(shape, 3, 1)
    W, H = 96, 64
    render_frame(dr, scenes, W, H, 0, n=4, m=4)
    dr.resolve()
    before = (dr.download(), dr.download_features())
    plain_call(dr, frames[0], variance_struct(SPATIAL, 1))
    same_plain(dr.download_denoised(), ref[0]["plain"], "the plain call")
    same(shards_step(dr, frames[0]), ref[0], "frame 0")
    same(shards_step(dr, frames[1]), ref[1], "frame 1")
    after = (dr.download(), dr.download_features())
    assert_same_bits(after[0][0], before[0][0], "hdr")
    assert np.array_equal(after[0][1], before[0][1]), "ldr"
    for key in ("albedo", "normal", "depth", "coverage"):
        assert_same_bits(after[1][key], before[1][key], key)
    assert np.array_equal(after[1]["id"], before[1]["id"])
    assert dr.committed_samples() == 4 and dr.feature_samples() == 4
    dr.render(W, H, 5, 9, 50, 1, stats=False)  # the accumulation goes on as if nothing had happened
    one = HipRenderer(0)
    try:
        render_frame(one, scenes, W, H, 0, n=8, m=1)
        assert_same_bits(dr.download(ldr=False)[0], one.download(ldr=False)[0], "the continued render vs the one-shot render")
    finally:
        one.close()
    same(shards_step(dr, frames[2]), ref[2], "frame 2")
    fresh = HipRenderer(0)  # no scene, no accumulation
    try:
        same(shards_step(fresh, frames[0], levels=5), reference[(shape, 1, 5, BILINEAR)][0], "a context without a scene")
    finally:
        fresh.close()


def test_refusals_on_the_device_path(dr, reference, parts_of):
    from cpuraytracer_amd import _capi
    L = _capi.load()
    shape, world = "band", 3
    W, H, first, num_rows = SHAPES[shape]
    ref = reference[(shape, 1, 3, BILINEAR)]
    frames = parts_of(shape, world, 1)
    fp = frames[1]
    b = fp["bufs"]
    ptrs = dict(hdr=b[0].at(0), sq=None, feat=b[2].at(0), ids=b[3].at(0))
    SP = variance_struct(SPATIAL, 1)

    def temporal(V=SP, P=None, T=None, fetch=BILINEAR, ctx=True, shape=True, **over):
        kw = dict(W=W, H=H, world=world, rows_max=fp["rows_max"], n=N, m=M, block_rows=1, first_row=first, num_rows=num_rows, **ptrs)
        kw.update(over)
        fr = _capi.shard_frame(camera=fp["cam"], **kw)
        return L.rt_denoise_shards_temporal_variance(dr._h if ctx else None, C.byref(fr) if shape else None, C.byref(P) if P is not None else None,
                                                     C.byref(T) if T is not None else None, fetch, C.byref(V) if V is not None else None, None)

    def plain(V=SP, P=None, ctx=True, shape=True, **over):
        kw = dict(W=W, H=num_rows, world=world, rows_max=fp["rows_max"], n=N, m=M, block_rows=1, first_row=first, hdr=ptrs["hdr"], sq=None, feat=ptrs["feat"])
        kw.update(over)
        sh = _capi.shard_parts(**kw)
        return L.rt_denoise_shards_variance(dr._h if ctx else None, C.byref(sh) if shape else None, C.byref(P) if P is not None else None,
                                            C.byref(V) if V is not None else None, None)

    def refusals():
        for call in (plain, temporal):
            assert call(ctx=False) == RT_ERR_INVALID_ARG and call(shape=False) == RT_ERR_INVALID_ARG
            for radius in (0, 4):
                assert call(V=variance_struct(SPATIAL, radius)) == RT_ERR_INVALID_ARG, radius
            assert call(V=variance_struct(2, 1)) == RT_ERR_INVALID_ARG
            assert call(n=0) == RT_ERR_SEQUENCE and call(m=0) == RT_ERR_SEQUENCE
            for null in ("hdr", "feat"):
                assert call(**{null: None}) == RT_ERR_INVALID_ARG, null
            for zero in ("W", "world", "block_rows"):
                assert call(**{zero: 0}) == RT_ERR_INVALID_ARG, zero
            assert call(rows_max=fp["rows_max"] - 1) == RT_ERR_INVALID_ARG
            for off in (4, 8, 12):
                assert call(feat=ptrs["feat"] + off) == RT_ERR_INVALID_ARG, off
            for bad in (dict(levels=0), dict(levels=6), dict(k_albedo=-1.0), dict(var_floor=0.0)):
                assert call(P=params_struct(bad)) == RT_ERR_INVALID_ARG, bad
            # sq = NULL under the moments source is still refused, whatever n
            for V in (None, variance_struct(MOMENTS, 1)):
                assert call(V=V, n=2) == RT_ERR_INVALID_ARG
        assert temporal(ids=None) == RT_ERR_INVALID_ARG and temporal(ids=ptrs["ids"] + 2) == RT_ERR_INVALID_ARG
        assert temporal(H=first + num_rows - 1) == RT_ERR_INVALID_ARG and temporal(num_rows=0) == RT_ERR_INVALID_ARG
        for fetch in (0, 2, 5):
            assert temporal(fetch=fetch) == RT_ERR_INVALID_ARG, fetch
        for bad in (dict(max_history=0), dict(max_history=65), dict(depth_tol=-1.0)):
            assert temporal(T=_capi.temporal_params_fetch(BILINEAR, **bad)) == RT_ERR_INVALID_ARG, bad
        c = _capi.RtCamera.from_buffer_copy(bytes(fp["cam"]))
        c.origin[1] = float("nan")
        fr = _capi.shard_frame(W, H, world, fp["rows_max"], N, M, c, ptrs["hdr"], None, ptrs["feat"], ptrs["ids"], block_rows=1, first_row=first, num_rows=num_rows)
        assert L.rt_denoise_shards_temporal_variance(dr._h, C.byref(fr), None, None, BILINEAR, C.byref(SP), None) == RT_ERR_INVALID_ARG

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
    V = variance_struct(SPATIAL, 1)
    assert shards_call(dr, frames[0], V, timed=False) is None
    ms = shards_call(dr, frames[1], V, timed=True)
    assert ms is not None and ms > 0.0
    want = reference[(shape, 1, 3, BILINEAR)][1]
    same(result(dr), want, "the timed call")
    assert plain_call(dr, frames[1], V, timed=False) is None
    ms = plain_call(dr, frames[1], V, timed=True)
    assert ms is not None and ms > 0.0
    out = [DevMem(hiprt, W * H * 12, fill=0), DevMem(hiprt, W * H * 4, fill=0), DevMem(hiprt, W * H * 3, fill=0)]
    try:
        dr.copy_denoised_to_device(out[0].at(0), out[1].at(0), out[2].at(0))
        dr.synchronize()
        assert_same_bits(out[0].download(np.float32, (H, W, 3)), want["plain"]["rgb"], "copy_denoised_to_device: rgb")
        assert_same_bits(out[1].download(np.float32, (H, W)), want["plain"]["var"], "copy_denoised_to_device: var")
        assert np.array_equal(out[2].download(np.uint8, (H, W, 3)), want["plain"]["ldr"])
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
        xch = D.PostExchange(H, W, rank, world, "cuda:0", with_ids=True, with_moments=False)
        assert xch.buf.numel() == 12 * xch.rows_max * W
        V = variance_struct(SPATIAL, 1)
        saved = {}
        for f in range(frames):
            sc = orbit_scene(scenes, "cover", W, H, STEP * f)
            r.upload(sc)  # a camera move is an upload: rank 0's history survives it
            r.set_noise_estimate(False)
            rs = D.shard_rowset(H, rank, world)
            r.render(W, H, 1, 1 + N, 50, 1 + f, rowset=rs, stats=False)
            r.render_features(W, H, 1, 1 + M, rowset=rs)
            xch.buf.view(torch.int32).fill_(-1)  # 0xff bytes: NaN in the float strips' padding, 0xffffffff in the ids'
            torch.cuda.synchronize()
            xch.fill(r)  # no moments: the noise estimate is off
            r.synchronize()
            parts = xch.gather(through_host=True)
            if rank == 0:
                assert len(parts) == 4 and parts[1] is None and all(p.is_cuda and p.is_contiguous() for p in parts if p is not None)
                assert parts[2].data_ptr() % 16 == 0 and parts[3].dtype == torch.int32 and parts[3].shape == (world, xch.rows_max, W)
                D.denoise_gathered_temporal_variance(r, xch, N, M, sc.camera, fetch=4, variance=V)
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
    """Two rank processes share device 0 (gloo, strips through host memory -- tests/test_denoise_shards.py's recipe): three frames of the
    orbit, each rendered in the ranks' rows at ONE sample with the noise estimate off, one PostExchange(with_moments=False,
    with_ids=True) gather of 12 words per pixel per frame and the spatial source on rank 0, whose history is kept from frame to frame.
    41 rows: rank 1's part has a padding row."""
    import torch.multiprocessing as mp
    shape = "70x41"
    W, H = SHAPES[shape][:2]
    monkeypatch.setenv("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    monkeypatch.delenv("RT_DENOISE_STAGE", raising=False)
    out = str(tmp_path / "den.npz")
    mp.spawn(_rank, args=(2, _free_port(), W, H, FRAMES, out), nprocs=2, join=True)
    z = np.load(out)
    for f in range(FRAMES):
        got = {k: z["%s%d" % (k, f)] for k in ("rgb", "var", "ldr", "state", "len", "target")}
        assert got["rgb"].shape == (H, W, 3) and got["ldr"].dtype == np.uint8 and got["len"].dtype == np.uint32
        same(got, reference[(shape, 1, 3, BILINEAR)][f], "two ranks, frame %d" % f)
    assert (z["len2"] == 3).any()
