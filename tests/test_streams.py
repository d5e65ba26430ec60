"""The stream contract on the device: everything the library enqueues lands on the caller's stream, every entry that returns data to
the host waits for a busy stream, and rt_set_stream orders the new stream behind the old one.

The instrument is a delay: torch.cuda._sleep(cycles) queues a spin kernel on a torch stream S.  With the delay sitting on S, work that is
wrongly launched on another stream, or read back without a wait for S, sees the buffers as they were before the calls under test --
plainly wrong bits, never a fault: every buffer is allocated on the host side of a call, and a context keeps one picture size, so
nothing is reallocated under work in flight.  Two conditions keep a test from passing vacuously, and both are asserted:
  * the delay was still running when the asynchronous calls had returned (an event behind the sleep, queried before the first call that
    waits: upload, resolve -- it reads its timer --, the first frame of a frame pipeline, rt_synchronize and the readers);
  * for the two-stream tests, a delay on A does not hold up B (streams may share a hardware queue; a torch-only control picks the pair).
The reference of every case is the same calls on a fresh context that runs on its own idle stream with synchronize() after every call:
the route the rest of the suite ties to the oracle.  Every comparison is bit for bit.

torch is imported before the library is loaded, as in bench.py: the two then share one HIP runtime, so a torch stream's handle is a
stream of the library's runtime."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BAND = (8, 24, 24, 0, 1)  # rows 8..31 of the 96 x 64 picture as one contiguous row set
COVER_PIVOT = (0.0, 1.0, 0.0)  # the cover scene's look-at point
TURN = 20.0
SPP, DEPTH, SEED = 3, 8, 1
TARGET_MS = 40.0  # not tuned: it only has to outlast a few host-side enqueues, and the query() assertions decide
MODES = ["plain", "batch", "lookahead", "pipelining"]


# ------------------------------------------------------------------------------------------------------------------ the instrument
@pytest.fixture(scope="module")
def gpu(built):
    torch.cuda.init()
    torch.cuda.set_device(0)
    # torch loads a kernel at its first use, tens of ms on the host: the ops the tests queue behind a delay, once beforehand
    for dtype, fill in ((torch.float32, float("nan")), (torch.int32, 7), (torch.uint8, 7)):
        t = torch.full((2, 6, 4), fill, dtype=dtype, device="cuda:0")
        t.clone().copy_(t).fill_(5)
        torch.empty((2, 3, 4), dtype=dtype, device="cuda:0").copy_(t[:, :3].reshape(2, 3, 4))
    torch.cuda.synchronize()
    import cpuraytracer_amd
    return cpuraytracer_amd


@pytest.fixture(scope="module")
def delay_cycles(gpu):
    """Cycles of torch.cuda._sleep for TARGET_MS, from one timed _sleep(10**6)."""
    s = torch.cuda.Stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(s):
        torch.cuda._sleep(1000)  # (the first launch loads the kernel)
        e0.record(s)
        torch.cuda._sleep(10**6)
        e1.record(s)
    e1.synchronize()
    ms = e0.elapsed_time(e1)
    assert ms > 0.0
    per_ms = 1e6 / ms
    cycles = int(per_ms * TARGET_MS)
    print("torch.cuda._sleep: %.0f cycles per ms (10^6 cycles took %.3f ms); a delay of %.0f ms is %d cycles" % (per_ms, ms, TARGET_MS, cycles))
    return cycles


class Delays:
    """The delays of one test: at most 1 s in all."""

    def __init__(self, cycles):
        self.cycles, self.queued_ms = cycles, 0.0

    def queue(self, stream):
        """The delay on `stream`, and an event right behind it."""
        self.queued_ms += TARGET_MS
        assert self.queued_ms <= 1000.0, "a test queues at most 1 s of delay"
        ev = torch.cuda.Event()
        with torch.cuda.stream(stream):
            torch.cuda._sleep(self.cycles)
            ev.record(stream)
        return ev

    def independent(self, a, b):
        """The torch-only control: with a delay on a, a one-element fill on b completes while a's event is still pending."""
        ea, eb = self.queue(a), torch.cuda.Event()
        with torch.cuda.stream(b):
            x = torch.empty(1, dtype=torch.float32, device="cuda:0")
            x.fill_(1.0)
            eb.record(b)
        eb.synchronize()
        ok = not ea.query()
        a.synchronize()
        return ok

    def assert_independent(self, a, b):
        assert self.independent(a, b), "the delay on stream A held up stream B: the pair is serialised, a missing order would not show"


def still_running(ev, what):
    assert not ev.query(), "the delay had ended when %s had returned: nothing was shown to be asynchronous" % what


@pytest.fixture()
def delays(delay_cycles):
    return Delays(delay_cycles)


@pytest.fixture(scope="module")
def stream_pair(gpu, delay_cycles):
    """(A, B): the first pair of up to four torch streams on which a delay on A does not hold up B.  Distinct HIP streams can share a
    hardware queue and are then serialised, which would hide the race the two-stream tests look for."""
    streams = [torch.cuda.Stream() for _ in range(4)]
    control = Delays(delay_cycles)
    for i in range(4):
        for j in range(4):
            if i != j and control.independent(streams[i], streams[j]):
                print("stream pair: torch streams %d and %d of 4 run independently (handles %#x, %#x)" % (i, j, streams[i].cuda_stream, streams[j].cuda_stream))
                return streams[i], streams[j]
    pytest.fail("no pair of four torch streams ran independently: a delay on one held up the other every time, so a missing order "
                "between two streams cannot be observed here")


# ------------------------------------------------------------------------------------------------------------------ helpers
@pytest.fixture()
def ctxs(gpu):
    """Contexts of the test's own, closed afterwards."""
    made = []

    def make():
        made.append(gpu.HipRenderer(0))
        return made[-1]
    yield make
    for r in made:
        r.close()


def rowset_of(rs):
    from cpuraytracer_amd import _capi
    return _capi.RtRowset(*rs) if rs else None


def cover(W, H):
    from cpuraytracer_amd import scenes
    return scenes.build_scene("cover", 1, W, H)


def turned(camera, degrees=TURN):
    from cpuraytracer_amd import scenes
    return scenes.orbit_camera(camera, degrees, COVER_PIVOT)


def with_camera(sc, camera):
    import copy
    out = copy.copy(sc)
    out.camera = camera
    return out


def same(got, want, what):
    """Dicts of arrays, bit for bit."""
    assert sorted(got) == sorted(want), what
    for k in sorted(want):
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert g.shape == w.shape and g.dtype.itemsize == w.dtype.itemsize, "%s: %s: %s %s against %s %s" % (what, k, g.shape, g.dtype, w.shape, w.dtype)
        gb, wb = g.reshape(-1).view(np.uint8), w.reshape(-1).view(np.uint8)
        if not np.array_equal(gb, wb):
            bad = np.flatnonzero(gb != wb)
            raise AssertionError("%s: %s differs in %d of %d bytes (first at byte %d)" % (what, k, bad.size, gb.size, int(bad[0])))


def setting(r, mode):
    if mode == "batch":
        r.set_frame_batch(4)
    elif mode == "lookahead":
        r.set_frame_lookahead(4)
    elif mode == "pipelining":
        r.set_frame_pipelining(2)


def settle_without_waiting(r, mode):
    """Render the pending batch, finish the frames in flight: the two settings settle on being stored, and wait for nothing."""
    if mode == "batch":
        r.set_frame_batch(4)
    elif mode == "pipelining":
        r.set_frame_pipelining(2)


def raw_features(r):
    feat = np.zeros((r.feature_rows, r.feature_W, 8), dtype=np.float32)
    ids = np.zeros((r.feature_rows, r.feature_W), dtype=np.uint32)
    from cpuraytracer_amd import _capi
    _capi.check(r._L.rt_download_features(r._h, feat.ctypes.data, ids.ctypes.data))
    return feat, ids


class Settled:
    """The reference route: the context's own idle stream, synchronize() after every call, results by download."""

    def __init__(self, r):
        self.r, self.out = r, {}

    def after(self):
        self.r.synchronize()

    def delay(self):
        pass

    def still_running(self, what):
        pass

    def picture(self, key):
        self.out[key + "_hdr"], self.out[key + "_ldr"] = self.r.download()

    def moments(self, key):
        self.out[key + "_sq"] = self.r.download_moments()

    def features(self, key):
        self.out[key + "_feat"], self.out[key + "_ids"] = raw_features(self.r)

    def denoised(self, key):
        for k, a in self.r.download_denoised().items():
            self.out[key + "_" + k] = a

    def finish(self):
        return self.out


class OnStream:
    """The route under test: the caller's stream S with a delay ahead, results by device copies into torch tensors, each cloned by a
    torch op queued on S behind the copy."""

    def __init__(self, r, stream, delays):
        self.r, self.S, self.delays, self.ev, self.clones, self.keep = r, stream, delays, None, {}, []

    def after(self):
        pass

    def delay(self):
        self.ev = self.delays.queue(self.S)

    def still_running(self, what):
        still_running(self.ev, what)

    def _dst(self, shape, dtype):
        with torch.cuda.stream(self.S):
            t = torch.full(shape, 7 if dtype != torch.float32 else float("nan"), dtype=dtype, device="cuda:0")
        self.keep.append(t)
        return t

    def _clone(self, **tensors):
        with torch.cuda.stream(self.S):
            for k, t in tensors.items():
                self.clones[k] = t.clone()

    def picture(self, key):
        r = self.r
        h, l = self._dst((r.rows, r.W, 3), torch.float32), self._dst((r.rows, r.W, 3), torch.uint8)
        r.copy_to_device(h.data_ptr(), l.data_ptr())
        self._clone(**{key + "_hdr": h, key + "_ldr": l})

    def moments(self, key):
        r = self.r
        q = self._dst((r.rows, r.W, 3), torch.float32)
        r.copy_moments_to_device(q.data_ptr())
        self._clone(**{key + "_sq": q})

    def features(self, key):
        r = self.r
        f, i = self._dst((r.feature_rows, r.feature_W, 8), torch.float32), self._dst((r.feature_rows, r.feature_W), torch.int32)
        r.copy_features_to_device(f.data_ptr(), i.data_ptr())
        self._clone(**{key + "_feat": f, key + "_ids": i})

    def denoised(self, key):
        r = self.r
        rows, W = r.denoised_rows, r.denoised_W
        rgb, var, ldr = self._dst((rows, W, 3), torch.float32), self._dst((rows, W), torch.float32), self._dst((rows, W, 3), torch.uint8)
        r.copy_denoised_to_device(rgb.data_ptr(), var.data_ptr(), ldr.data_ptr())
        self._clone(**{key + "_rgb": rgb, key + "_var": var, key + "_ldr": ldr})

    def finish(self):
        self.S.synchronize()
        return {k: t.cpu().numpy() for k, t in self.clones.items()}


def accumulate(r, io, W, H, rs, mode, noise, delay=True, settle=True, seed=SEED, first=1, count=SPP):
    """`count` one-sample frames from sample `first` without statistics, then (settle) settled without a wait.  The first frame of a
    frame pipeline waits for the stream once (its control block is copied from the stack); the delay is queued behind that frame."""
    starts_with_wait = mode == "pipelining" and not noise
    if delay and not starts_with_wait:
        io.delay()
    for f in range(first, first + count):
        r.render(W, H, f, f + 1, DEPTH, seed, rowset=rowset_of(rs), stats=False)
        io.after()
        if delay and starts_with_wait and f == first:
            io.delay()
    if settle:
        settle_without_waiting(r, mode)
        io.after()


# ------------------------------------------------------------------------------------------------------------------ test 1
def all_asynchronous_calls(r, io, sc, W, H, rs, mode):
    """Every entry that only enqueues, in an order a caller would use them; io is the route."""
    from cpuraytracer_amd import _capi
    rowset = rowset_of(rs)
    # an accumulation without the second moments: here the frame pipeline carries paths across calls
    accumulate(r, io, W, H, rs, mode, False)
    io.still_running("rt_render without statistics")
    r.resolve()  # (waits: it reads its timer)
    io.after()
    io.delay()
    io.picture("plain")
    io.still_running("rt_copy_to_device")
    # with the second moments: the feature pass, the denoise family, a camera move
    r.set_noise_estimate(True)
    accumulate(r, io, W, H, rs, mode, True)
    r.render_features(W, H, 1, 1 + SPP, rowset=rowset)
    io.after()
    io.still_running("rt_render with the noise estimate, rt_render_features")
    r.resolve()
    io.after()
    io.delay()
    io.picture("first")
    io.moments("first")
    io.features("first")
    r.denoise()
    io.after()
    io.denoised("den")
    r.denoise_temporal(fetch=4)
    io.after()
    io.denoised("tmp0")
    r.denoise(variance=_capi.variance_params(source=1))
    io.after()
    io.denoised("spatial")
    r.set_camera(turned(sc.camera))
    io.after()
    accumulate(r, io, W, H, rs, mode, True, delay=False)
    r.render_features(W, H, 1, 1 + SPP, rowset=rowset)
    io.after()
    io.moments("moved")
    io.features("moved")
    r.denoise_temporal(fetch=4)  # (the history of the first camera is reprojected)
    io.after()
    io.denoised("tmp1")
    io.still_running("the device copies, the denoise family, rt_set_camera and the second accumulation")
    r.resolve()
    io.after()
    io.delay()
    io.picture("moved")
    io.still_running("rt_copy_to_device after the move")
    return io.finish()


@pytest.fixture(scope="module")
def want_all(gpu):
    """The reference of test 1 per (scene, shape): computed once, shared by the modes."""
    cache = {}

    def get(key, sc, W, H, rs):
        if key not in cache:
            r = gpu.HipRenderer(0)
            try:
                r.upload(sc)
                cache[key] = all_asynchronous_calls(r, Settled(r), sc, W, H, rs, "plain")
            finally:
                r.close()
        return cache[key]
    return get


CASES_1 = [("cover", "96x64", m) for m in MODES] + [("cover", "70x41", "plain"), ("cover", "band", "plain"), ("grid10k", "96x64", "plain")]


@pytest.mark.parametrize("scene,shape,mode", CASES_1, ids=["%s-%s-%s" % c for c in CASES_1])
def test_everything_asynchronous_lands_on_the_callers_stream(ctxs, want_all, delays, monkeypatch, scene, shape, mode):
    W, H, rs = {"96x64": (96, 64, None), "70x41": (70, 41, None), "band": (96, 64, BAND)}[shape]
    if scene == "grid10k":  # the bounds hierarchy's scan and its launches
        import trace_variant_cases as tvc
        monkeypatch.setenv("RT_GRID", "0")
        sc = tvc.build_scene("grid10k", W, H)
    else:
        monkeypatch.delenv("RT_GRID", raising=False)
        sc = cover(W, H)
    want = want_all((scene, shape), sc, W, H, rs)
    S = torch.cuda.Stream()
    r = ctxs()
    r.set_stream(S.cuda_stream)
    r.upload(sc)  # (waits for the stream: the tables are copied by blocking copies)
    setting(r, mode)
    got = all_asynchronous_calls(r, OnStream(r, S, delays), sc, W, H, rs, mode)
    if scene == "grid10k":
        assert r.last_trace_launch().kScan == 2
    same(got, want, "%s %s %s on a caller's stream against settled calls" % (scene, shape, mode))


# ------------------------------------------------------------------------------------------------------------------ test 2
SHARD_W, SHARD_H = 70, 41


@pytest.fixture(scope="module")
def shard_strips(gpu):
    """Per world and frame (two cameras), the gathered parts as numpy arrays [world, rows_max, W, c], from strips that one context per
    rank rendered with synchronize() after every call; the padding rows hold NaN and 0xffffffff."""
    from cpuraytracer_amd import distributed as D
    W, H = SHARD_W, SHARD_H
    sc0 = cover(W, H)
    cams = [sc0.camera, turned(sc0.camera)]
    out = {}
    r = gpu.HipRenderer(0)
    try:
        r.upload(sc0)
        r.set_noise_estimate(True)
        for world in (2, 3):
            rows_max = D.max_local_rows(H, world)
            for f, cam in enumerate(cams):
                hdr = np.full((world, rows_max, W, 3), np.nan, dtype=np.float32)
                sq = np.full((world, rows_max, W, 3), np.nan, dtype=np.float32)
                feat = np.full((world, rows_max, W, 8), np.nan, dtype=np.float32)
                ids = np.full((world, rows_max, W), 0xffffffff, dtype=np.uint32)
                for s in range(world):
                    rs = D.shard_rowset(H, s, world)
                    r.set_camera(cam)
                    r.render(W, H, 1, 1 + SPP, DEPTH, SEED + f, rowset=rs, stats=False)
                    r.synchronize()
                    r.render_features(W, H, 1, 1 + SPP, rowset=rs)
                    r.synchronize()
                    rows = r.rows
                    hdr[s, :rows] = r.download(ldr=False)[0]
                    sq[s, :rows] = r.download_moments()
                    feat[s, :rows], ids[s, :rows] = raw_features(r)
                out[(world, f)] = {"hdr": hdr, "sq": sq, "feat": feat, "ids": ids.view(np.int32), "camera": cam, "rows_max": rows_max}
    finally:
        r.close()
    return out


def shard_entries(r, io_inputs, world, strips, settle):
    """The three entries over gathered parts, each on inputs that io_inputs(frame) has just produced; settle(what) stands between the
    call and the downloads.  The temporal entry runs two frames: the second reprojects the first's history."""
    from cpuraytracer_amd import _capi
    W, H = SHARD_W, SHARD_H
    out = {}

    def ptrs(t):
        return t["hdr"].data_ptr(), t["sq"].data_ptr(), t["feat"].data_ptr()
    rows_max = strips[(world, 0)]["rows_max"]
    t = io_inputs(0)
    r.denoise_shards(*ptrs(t), W, H, world, rows_max, SPP, SPP)
    settle("rt_denoise_shards")
    for k, a in r.download_denoised().items():
        out["shards_" + k] = a
    t = io_inputs(0)
    r.denoise_shards(*ptrs(t), W, H, world, rows_max, SPP, SPP, variance=_capi.variance_params(source=1))
    settle("rt_denoise_shards_variance")
    for k, a in r.download_denoised().items():
        out["spatial_" + k] = a
    for f in (0, 1):
        t = io_inputs(f)
        r.denoise_shards_temporal(*ptrs(t), t["ids"].data_ptr(), W, H, world, rows_max, SPP, SPP, strips[(world, f)]["camera"], fetch=4)
        settle("rt_denoise_shards_temporal")
        for k, a in dict(r.download_denoised(), **r.download_temporal()).items():
            out["temporal%d_%s" % (f, k)] = a
    return out


@pytest.mark.parametrize("world", [2, 3])
def test_caller_produced_inputs_are_read_on_the_stream(ctxs, shard_strips, delays, world):
    """The gathered parts reach the device tensors by torch copies queued on S behind the delay; the entries are called directly (the
    distributed.denoise_gathered* wrappers synchronise torch's stream first).  Before the copies the tensors hold other data."""
    S = torch.cuda.Stream()
    names = ("hdr", "sq", "feat", "ids")
    src = {f: {k: torch.from_numpy(shard_strips[(world, f)][k]).to("cuda:0") for k in names} for f in (0, 1)}
    dst = {k: torch.zeros_like(src[0][k]) for k in names}
    torch.cuda.synchronize()
    # the reference: settled inputs, the context's own stream
    ref = ctxs()
    want = shard_entries(ref, lambda f: src[f], world, shard_strips, lambda what: ref.synchronize())
    assert (want["temporal1_len"] > 1).any()  # the second frame met a history
    r = ctxs()
    r.set_stream(S.cuda_stream)
    state = {}

    def produce(f):
        with torch.cuda.stream(S):
            for k in names:  # what a wrong stream would read: not the frame's parts
                dst[k].fill_(5)
        S.synchronize()
        state["ev"] = delays.queue(S)
        with torch.cuda.stream(S):
            for k in names:
                dst[k].copy_(src[f][k])
        return dst
    got = shard_entries(r, produce, world, shard_strips, lambda what: still_running(state["ev"], what))
    same(got, want, "world %d: gathered parts written on the stream behind a delay" % world)


# ------------------------------------------------------------------------------------------------------------------ test 3
READ_W, READ_H, READ_RS = 96, 64, BAND


def unit_pixels():
    rows, first = READ_RS[1], READ_RS[0]
    return np.array([[i, first + j, s] for s in (1, 2) for j in (0, rows // 2, rows - 1) for i in (0, READ_W // 3, READ_W - 1)], dtype=np.uint32)


def tile_masks(r):
    from cpuraytracer_amd import _capi
    rs = rowset_of(READ_RS)
    cap = (READ_W * r._L.rt_rowset_local_rows(rs)) >> 6
    words = np.zeros((cap, 8), dtype=np.uint32)
    gos = np.zeros(20000, dtype=np.uint32)
    n = C.c_uint32(0)
    _capi.check(r._L.rt_unit_tile_masks(r._h, READ_W, READ_H, rs, cap, C.byref(n), words.ctypes.data, gos.shape[0], gos.ctypes.data, None))
    assert n.value == cap
    return {"tiles": np.array([n.value]), "masks": words, "groups": gos}


def tile_spheres(r):
    from cpuraytracer_amd import _capi
    rs = rowset_of(READ_RS)
    cap = (READ_W * r._L.rt_rowset_local_rows(rs)) >> 6
    lists = np.zeros((cap, 64), dtype=np.uint16)
    n = C.c_uint32(0)
    _capi.check(r._L.rt_unit_tile_spheres(r._h, READ_W, READ_H, rs, cap, C.byref(n), lists.ctypes.data, None))
    assert n.value == cap
    for t in range(cap):  # (the slots behind a count are unspecified)
        cnt = int(lists[t, 0])
        lists[t, 1 + (0 if cnt == 0xffff else cnt):] = 0
    return {"tiles": np.array([n.value]), "lists": lists}


def sky_planes(r):
    from cpuraytracer_amd import _capi
    n = C.c_uint64(0)
    _capi.check(r._L.rt_unit_sky_planes(r._h, C.byref(n)))
    return {"planes": np.array([n.value], dtype=np.uint64)}


def sky_excluded(r):
    from cpuraytracer_amd import _capi
    n = C.c_uint32(0)
    _capi.check(r._L.rt_unit_sky_excluded(r._h, C.byref(n)))
    return {"tiles": np.array([n.value])}


def render_with_statistics(r):
    st = r.render(READ_W, READ_H, 1, 1 + SPP, DEPTH, SEED, rowset=rowset_of(READ_RS))
    return {"stats": np.array([st.samples, st.traversals, st.segments, st.local_rows, st.passes], dtype=np.uint64)}


def kernel_fields(r):
    launch = r.last_trace_launch()
    return {"kernel": np.array([int(getattr(launch, f)) for f in launch._fields if f in ("row", "lights") or f.startswith("k")], dtype=np.int64)}


def noise_summary(r):
    counts, mx = r.noise_summary([0.05, 0.2, 1.0])
    return {"counts": counts, "max": np.array([mx], dtype=np.float32)}


def unit_trace(r):
    rgb, trav = r.unit_trace(READ_W, READ_H, unit_pixels(), DEPTH, SEED)
    return {"rgb": rgb, "trav": trav}


# name -> (the reader, what has to be produced under the delay, whether the entry reads device memory and so has to wait for the stream)
READERS = {
    "committed_samples": (lambda r: {"n": np.array([r.committed_samples()])}, "all", True),
    "download": (lambda r: {"hdr": r.download(ldr=False)[0]}, "all", True),
    "download_moments": (lambda r: {"sq": r.download_moments()}, "all", True),
    "noise_map": (lambda r: {"map": r.noise_map()}, "all", True),
    "noise_summary": (noise_summary, "all", True),
    "feature_samples": (lambda r: {"m": np.array([r.feature_samples()])}, "all", False),
    "download_features": (lambda r: dict(zip(("feat", "ids"), raw_features(r))), "all", True),
    "download_denoised": (lambda r: r.download_denoised(), "all", True),
    "download_temporal": (lambda r: r.download_temporal(), "all", True),
    "render_with_statistics": (render_with_statistics, "camera", True),
    "last_trace_launch": (kernel_fields, "all", False),
    "unit_trace": (unit_trace, "camera", True),
    "unit_primary_rays": (lambda r: {"rays": r.unit_primary_rays(READ_W, READ_H, unit_pixels())}, "camera", True),
    "unit_tile_masks": (tile_masks, "all", True),
    "unit_tile_spheres": (tile_spheres, "all", True),
    "unit_sky_planes": (sky_planes, "all", True),
    "unit_sky_excluded": (sky_excluded, "all", False),
}


def produce(r, camera, seed, what, after):
    """What the readers read, all of it enqueued only: another camera (the tile tables are rebuilt), an accumulation with the second
    moments, the feature strips, the denoised picture and a history of one frame."""
    W, H, rowset = READ_W, READ_H, rowset_of(READ_RS)
    r.set_camera(camera)
    after()
    if what == "camera":
        return
    r.temporal_reset()
    for f in range(1, 1 + SPP):
        r.render(W, H, f, f + 1, DEPTH, seed, rowset=rowset, stats=False)
        after()
    r.render_features(W, H, 1, 1 + SPP, rowset=rowset)
    after()
    r.denoise_temporal(fetch=4)
    after()


def primed(r, sc, reader, what, after):
    """A context whose buffers already hold results -- of another camera and another seed: what a reader that does not wait hands out."""
    r.upload(sc)
    r.set_noise_estimate(True)
    produce(r, turned(sc.camera, -TURN), SEED + 6, "all", after)
    r.synchronize()
    return reader(r)


@pytest.mark.parametrize("entry", sorted(READERS))
def test_every_entry_that_returns_to_the_host_waits_for_a_busy_stream(ctxs, delays, entry):
    reader, what, reads_device = READERS[entry]
    sc = cover(READ_W, READ_H)
    c1 = turned(sc.camera)
    ref = ctxs()
    stale = primed(ref, sc, reader, what, ref.synchronize)
    produce(ref, c1, SEED, what, ref.synchronize)
    want = reader(ref)
    # the primed context holds something else, so a reader that did not wait would show (the two counts may well coincide)
    if reads_device and entry not in ("committed_samples", "unit_sky_planes"):
        assert any(not np.array_equal(np.asarray(stale[k]), np.asarray(want[k])) for k in want), entry
    S = torch.cuda.Stream()
    r = ctxs()
    r.set_stream(S.cuda_stream)
    same(primed(r, sc, reader, what, lambda: None), stale, "%s on the primed context" % entry)
    ev = delays.queue(S)
    produce(r, c1, SEED, what, lambda: None)
    still_running(ev, "the calls that produce what %s reads" % entry)
    got = reader(r)
    if reads_device:
        assert ev.query(), "%s returned while the stream was still busy" % entry
    same(got, want, "%s behind a delay against settled calls" % entry)


# ------------------------------------------------------------------------------------------------------------------ test 4
@pytest.fixture(scope="module")
def one_shot(gpu):
    """render(1 .. 5) in one call with statistics on a fresh context: strip, moments and LDR, per shape."""
    cache = {}

    def get(shape):
        if shape not in cache:
            W, H = shape
            r = gpu.HipRenderer(0)
            try:
                r.upload(cover(W, H))
                r.set_noise_estimate(True)
                r.render(W, H, 1, 5, DEPTH, SEED)
                r.resolve()
                hdr, ldr = r.download()
                cache[shape] = {"hdr": hdr, "ldr": ldr, "sq": r.download_moments()}
            finally:
                r.close()
        return cache[shape]
    return get


def handle(stream):
    return 0 if stream is None else stream.cuda_stream


class DelayOn:
    """accumulate()'s route for a stream that may be the context's own (None), which a caller cannot delay."""

    def __init__(self, stream, delays):
        self.stream, self.delays, self.ev = stream, delays, None

    def after(self):
        pass

    def delay(self):
        if self.stream is not None:
            self.ev = self.delays.queue(self.stream)

    def still_running(self, what):
        if self.ev is not None:
            still_running(self.ev, what)


def switched_accumulation(r, old, new, delays, W, H, mode, noise):
    """Samples 1 and 2 on `old` with the delay ahead, rt_set_stream(new), samples 3 and 4 on `new`; None is the context's own stream.
    What is pending or in flight at the switch is rt_set_stream's to settle.  Returns the strip, the LDR and, with the noise estimate,
    the moments."""
    io = DelayOn(old, delays)
    r.set_stream(handle(old))
    r.upload(cover(W, H))
    setting(r, mode)
    r.set_noise_estimate(noise)
    accumulate(r, io, W, H, None, mode, noise, settle=False, first=1, count=2)
    r.set_stream(handle(new))
    if mode == "pipelining" and not noise:  # (the next frame starts a new pipeline, and that waits for the stream)
        io.still_running("rt_render on the old stream and rt_set_stream")
        io.ev = None
    accumulate(r, io, W, H, None, mode, noise, delay=False, settle=False, first=3, count=2)
    io.still_running("rt_render on the old stream, rt_set_stream and rt_render on the new one")
    r.synchronize()
    assert r.committed_samples() == 4
    r.resolve()
    hdr, ldr = r.download()
    out = {"hdr": hdr, "ldr": ldr}
    if noise:
        out["sq"] = r.download_moments()
    return out


DIRECTIONS = ["A_to_B", "A_to_own", "own_to_A", "A_to_A"]
CASES_4 = [(d, m, n, "96x64") for d in DIRECTIONS for m in MODES for n in (False, True)] + [("A_to_B", m, True, "70x41") for m in MODES]


@pytest.mark.parametrize("direction,mode,noise,shape", CASES_4, ids=["%s-%s-%s-%s" % (d, m, "noise" if n else "strip", s) for d, m, n, s in CASES_4])
def test_replacing_the_stream_in_the_middle_of_an_accumulation(ctxs, one_shot, stream_pair, delays, direction, mode, noise, shape):
    """A stats-less rt_render(1 .. 3) on one stream, rt_set_stream, rt_render(3 .. 5) on the other is a legal continuation: the result
    is the one-shot render's.  A_to_A: the handle already in force changes nothing.  (own_to_A cannot be delayed and is kept for the
    bits; in A_to_own only the first vacuity condition can be asserted: nothing of the caller's runs on the context's own stream.)"""
    A, B = stream_pair
    W, H = {"96x64": (96, 64), "70x41": (70, 41)}[shape]
    if direction == "A_to_B":
        delays.assert_independent(A, B)
    old, new = {"A_to_B": (A, B), "A_to_own": (A, None), "own_to_A": (None, A), "A_to_A": (A, A)}[direction]
    got = switched_accumulation(ctxs(), old, new, delays, W, H, mode, noise)
    want = {k: a for k, a in one_shot((W, H)).items() if k in got}
    same(got, want, "%s, %s: the accumulation continued across rt_set_stream against the one-shot render" % (direction, mode))


def test_the_feature_strips_continue_across_the_switch(ctxs, stream_pair, delays):
    A, B = stream_pair
    delays.assert_independent(A, B)
    W, H = 70, 41
    sc = cover(W, H)
    ref = ctxs()
    ref.upload(sc)
    ref.render_features(W, H, 1, 5)
    ref.synchronize()
    want = dict(zip(("feat", "ids"), raw_features(ref)))
    r = ctxs()
    r.set_stream(A.cuda_stream)
    r.upload(sc)
    ev = delays.queue(A)
    r.render_features(W, H, 1, 3)
    r.set_stream(B.cuda_stream)
    r.render_features(W, H, 3, 5)
    still_running(ev, "rt_render_features on A, rt_set_stream and rt_render_features on B")
    assert r.feature_samples() == 4
    same(dict(zip(("feat", "ids"), raw_features(r))), want, "the feature strips continued across rt_set_stream")


def temporal_frames(r, sc, W, H, before_frame, after):
    """Three frames of an orbit through rt_set_camera, two samples each, each denoised with the history; the last frame's results."""
    for f in range(3):
        before_frame(f)
        if f:
            r.set_camera(turned(sc.camera, 0.5 * f))
            after()
        r.render(W, H, 1, 3, DEPTH, SEED + f, stats=False)
        after()
        r.render_features(W, H, 1, 3)
        after()
        r.denoise_temporal(fetch=4)
        after()


def test_the_temporal_history_continues_across_the_switch(ctxs, stream_pair, delays):
    """Two frames on A with the delay ahead, the third on B: it reprojects a history that A's kernels are still to write."""
    A, B = stream_pair
    delays.assert_independent(A, B)
    W, H = 96, 64
    sc = cover(W, H)
    ref = ctxs()
    ref.upload(sc)
    ref.set_noise_estimate(True)
    temporal_frames(ref, sc, W, H, lambda f: None, ref.synchronize)
    want = dict(ref.download_denoised(), **ref.download_temporal())
    assert (want["len"] > 2).any()
    r = ctxs()
    r.set_stream(A.cuda_stream)
    r.upload(sc)
    r.set_noise_estimate(True)
    state = {}

    def before_frame(f):
        if f == 0:
            state["ev"] = delays.queue(A)
        elif f == 2:
            r.set_stream(B.cuda_stream)
    temporal_frames(r, sc, W, H, before_frame, lambda: None)
    still_running(state["ev"], "two frames on A, rt_set_stream and the third frame on B")
    same(dict(r.download_denoised(), **r.download_temporal()), want, "the history continued across rt_set_stream")


# ------------------------------------------------------------------------------------------------------------------ test 5
def context_calls(r, W, H, after):
    r.set_noise_estimate(True)
    yield
    for f in range(1, 1 + SPP):
        r.render(W, H, f, f + 1, DEPTH, SEED, stats=False)
        after()
        yield
    r.render_features(W, H, 1, 1 + SPP)
    after()
    yield
    r.denoise()
    after()
    yield


def context_results(r):
    r.resolve()
    hdr, ldr = r.download()
    out = {"hdr": hdr, "ldr": ldr, "sq": r.download_moments()}
    out["feat"], out["ids"] = raw_features(r)
    for k, a in r.download_denoised().items():
        out["den_" + k] = a
    return out


def test_two_contexts_two_streams_one_device(ctxs, stream_pair, delays):
    """X on A and Y on B, different cameras, their calls interleaved, the delay on A only: each equals its own reference -- nothing of
    the stream, the tables or the strips is shared between contexts."""
    A, B = stream_pair
    delays.assert_independent(A, B)
    W, H = 96, 64
    sc = cover(W, H)
    scs = [sc, with_camera(sc, turned(sc.camera))]
    wants = []
    for s in scs:
        ref = ctxs()
        ref.upload(s)
        for _ in context_calls(ref, W, H, ref.synchronize):
            pass
        wants.append(context_results(ref))
    assert not np.array_equal(wants[0]["hdr"], wants[1]["hdr"])
    x, y = ctxs(), ctxs()
    x.set_stream(A.cuda_stream)
    y.set_stream(B.cuda_stream)
    x.upload(scs[0])
    y.upload(scs[1])
    ev = delays.queue(A)
    for _ in zip(context_calls(x, W, H, lambda: None), context_calls(y, W, H, lambda: None)):
        pass
    still_running(ev, "the interleaved calls of the two contexts")
    same(context_results(y), wants[1], "context Y on stream B")
    same(context_results(x), wants[0], "context X on stream A, behind the delay")


# ------------------------------------------------------------------------------------------------------------------ test 6
def test_the_documented_recipe_as_bench_runs_it(ctxs, delays):
    """INTEGRATION.md section 4 on one device: a real torch stream made current, rt_set_stream with its handle, ranks 0 and 1 of world 2
    as two contexts, PostExchange.fill, a regroup by torch on the same stream in the gather's place, rt_denoise_shards -- and no
    synchronize() before the final download.  The result is rt_denoise's on a one-context render."""
    from cpuraytracer_amd import distributed as D
    W, H, world = SHARD_W, SHARD_H, 2
    sc = cover(W, H)
    ref = ctxs()
    ref.upload(sc)
    ref.set_noise_estimate(True)
    ref.render(W, H, 1, 1 + SPP, DEPTH, SEED)
    ref.render_features(W, H, 1, 1 + SPP)
    ref.denoise()
    want = ref.download_denoised()
    S = torch.cuda.Stream()
    assert S.cuda_stream != 0
    with torch.cuda.stream(S):  # (made current, as torch.cuda.set_stream does in bench.py)
        ranks = [ctxs() for _ in range(world)]
        for r in ranks:
            r.set_stream(torch.cuda.current_stream().cuda_stream)
            r.upload(sc)
            r.set_noise_estimate(True)
        xch = [D.PostExchange(H, W, s, world, "cuda:0") for s in range(world)]
        x0 = xch[0]

        def gather_and_regroup():  # the gather's stand-in, then what PostExchange.gather does behind it
            for s in range(world):
                x0.all[s].copy_(xch[s].buf)
            x0.hdr_parts.copy_(x0.all[:, :x0.cut[0]].reshape(world, x0.rows_max, W, 3))
            x0.sq_parts.copy_(x0.all[:, x0.cut[0]:x0.cut[1]].reshape(world, x0.rows_max, W, 3))
            x0.feat_parts.copy_(x0.all[:, x0.cut[1]:x0.cut[2]].reshape(world, x0.rows_max, W, 8))
        gather_and_regroup()  # (over the empty buffers: torch loads a kernel at its first use, tens of ms on the host)
        ev = delays.queue(S)
        for s, r in enumerate(ranks):
            rs = D.shard_rowset(H, s, world)
            r.render(W, H, 1, 1 + SPP, DEPTH, SEED, rowset=rs, stats=False)
            r.render_features(W, H, 1, 1 + SPP, rowset=rs)
            xch[s].fill(r)
        gather_and_regroup()
        ranks[0].denoise_shards(x0.hdr_parts.data_ptr(), x0.sq_parts.data_ptr(), x0.feat_parts.data_ptr(), W, H, world, x0.rows_max, SPP, SPP)
        still_running(ev, "the two ranks' renders, the fills, the regroup and rt_denoise_shards")
        got = ranks[0].download_denoised()
    assert got["rgb"].shape == (H, W, 3)
    same(got, want, "the recipe on a caller's stream against rt_denoise on one context")
