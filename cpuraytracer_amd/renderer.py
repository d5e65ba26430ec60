"""Python-side handle over the C ABI: scene upload, render, resolve, download.

Plumbing for tests, bench.py and the torch.distributed launcher — the host mirror of the
reference's class API is C++ (cpuraytracer_amd/csrc/host/).
"""
import collections
import ctypes as C

import numpy as np

from . import _capi
from ._capi import RtRowset, RtStats, check, whole_image


# Default `floor` of the relative noise estimate: added to the pixel's mean (r + g + b, HDR units after exposure, where 1.0 per
# channel is about display white) so that black pixels have a finite relative error.
NOISE_FLOOR = 0.01


# What the launcher reports of a trace-kernel launch (rt_unit_last_trace_launch): `row` of csrc/rt_trace_variants.h (-1: not in the
# list), `lights` = the _lights twin ran, the ten template arguments of rt_trace_kernel in their order, the grid (`blocks` workgroups
# of kThreads), the queue cut of rt_params.h (all 0 for the frame-pipelining launch, whose caller cuts the queue), the calls'
# `launches` since rt_create, and the raw words of rt_unit_launch_plan: `kernel_word` is plan_words[25].
TraceLaunch = collections.namedtuple("TraceLaunch", [
    "row", "lights", "kLds", "kThreads", "kScan", "kCache", "kHitLds", "kCarry", "kStash", "kMatsL2", "kSgLds", "kGridQ",
    "blocks", "queue_block", "static_blocks", "dyn_begin", "dyn_blocks", "launches", "kernel_word", "case_words", "plan_words"])


def trace_variants():
    """rt_unit_trace_variants: word [25] of every instantiated trace-kernel row, single-light form, in list order.  Needs no GPU."""
    L = _capi.load()
    n = C.c_uint32(0)
    check(L.rt_unit_trace_variants(None, 0, C.byref(n)))
    words = np.zeros(n.value, dtype=np.uint32)
    check(L.rt_unit_trace_variants(words.ctypes.data, n.value, C.byref(n)))
    return [int(w) for w in words]


def trace_lean_variants():
    """rt_unit_trace_lean_variants: the words of the rows that exist a second time without far-hit state (a subset of trace_variants())."""
    L = _capi.load()
    n = C.c_uint32(0)
    check(L.rt_unit_trace_lean_variants(None, 0, C.byref(n)))
    words = np.zeros(n.value, dtype=np.uint32)
    check(L.rt_unit_trace_lean_variants(words.ctypes.data, n.value, C.byref(n)))
    return [int(w) for w in words]


def far_state_plan(case_words, path_list=False, trav_out=False, shadow_grid=True, force_full=False):
    """rt_unit_far_state_plan: True when the launch these 28 case words describe takes its row's lean kernel.  Needs no GPU."""
    case = np.ascontiguousarray(case_words, dtype=np.uint32)
    assert case.shape == (28,)
    lean = C.c_uint32(7)
    check(_capi.load().rt_unit_far_state_plan(case.ctypes.data, int(path_list), int(trav_out), int(shadow_grid), int(force_full), C.byref(lean)))
    return bool(lean.value)


def decode_kernel_word(word):
    """Word [25] of rt_unit_launch_plan as a dict: lights, the ten template arguments, instantiated (bit 31)."""
    w = int(word)
    return {"lights": bool(w & 1), "kLds": bool(w & 2), "kThreads": (256, 512, 1024, 0)[(w >> 2) & 3], "kScan": (w >> 4) & 3,
            "kCache": bool(w >> 6 & 1), "kHitLds": bool(w >> 7 & 1), "kCarry": bool(w >> 8 & 1), "kStash": bool(w >> 9 & 1),
            "kMatsL2": bool(w >> 10 & 1), "kSgLds": bool(w >> 11 & 1), "kGridQ": bool(w >> 12 & 1), "instantiated": bool(w >> 31 & 1)}


class HipRenderer:
    """One context per device ordinal (rt_create).  Raises when no GPU is present."""

    def __init__(self, device=0):
        self._L = _capi.load()
        self._h = C.c_void_p()
        check(self._L.rt_create(int(device), C.byref(self._h)))
        self.W = self.rows = 0
        self.feature_W = self.feature_rows = 0
        self.denoised_W = self.denoised_rows = 0
        self.temporal_W = self.temporal_rows = 0

    def close(self):
        if getattr(self, "_h", None):
            self._L.rt_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, hip_stream_ptr):
        """rt_set_stream: enqueue on the caller's hipStream_t (torch.cuda.Stream().cuda_stream) from here on, ordered behind what was
        queued on the previous stream.  0 -- also the handle of torch's default stream -- selects the context's own stream."""
        check(self._L.rt_set_stream(self._h, C.c_void_p(hip_stream_ptr)))

    def set_workspace_limit(self, nbytes):
        check(self._L.rt_set_workspace_limit(self._h, int(nbytes)))

    def set_sampler(self, flags):
        """RT_SAMPLER_* flags (0 = the reference's uniform hemisphere and linear-r disk)."""
        check(self._L.rt_set_sampler(self._h, int(flags)))

    def set_frame_pipelining(self, depth):
        """rt_set_frame_pipelining: up to `depth` stats-less render calls may stay in flight (0 = off)."""
        check(self._L.rt_set_frame_pipelining(self._h, int(depth)))

    def set_frame_batch(self, frames):
        """rt_set_frame_batch: stats-less render calls that continue each other are rendered `frames` sample planes per launch (1 = off)."""
        check(self._L.rt_set_frame_batch(self._h, int(frames)))

    def set_frame_lookahead(self, frames):
        """rt_set_frame_lookahead: a stats-less render call traces the next `frames` sample planes with its one launch and adds only its own (1 = off)."""
        check(self._L.rt_set_frame_lookahead(self._h, int(frames)))

    def committed_samples(self):
        n = C.c_uint32(0)
        check(self._L.rt_committed_samples(self._h, C.byref(n)))
        return n.value

    def upload(self, scene):
        """scene: object with .spheres/.materials (numpy structured arrays in the rt_api.h layouts), .camera, .sun,
        .sky (ctypes structs of identical layout), .exposure_scale."""
        sph = np.ascontiguousarray(scene.spheres)
        mat = np.ascontiguousarray(scene.materials)
        assert sph.dtype.itemsize == 16 and mat.dtype.itemsize == 48
        cam = _capi.RtCamera.from_buffer_copy(bytes(scene.camera))
        # m_lights (spheres-app.h:38): scene.lights when the scene carries a list (it may be empty), else the generators' single sun
        ls = getattr(scene, "lights", None)
        ls = [scene.sun] if ls is None else list(ls)
        lights = (_capi.RtLight * max(1, len(ls)))()
        for k, l in enumerate(ls):
            lights[k] = _capi.RtLight.from_buffer_copy(bytes(l))
        sky = _capi.RtMaterial.from_buffer_copy(bytes(scene.sky))
        check(self._L.rt_scene_upload(self._h, sph.ctypes.data, mat.ctypes.data, sph.shape[0], C.byref(cam), lights, len(ls),
                                      C.byref(sky), float(scene.exposure_scale)))
        self._materials = mat.copy()  # (set_materials compares against them: which spheres to forget)
        self._sky = bytes(sky)

    def set_camera(self, camera):
        """rt_set_camera: move the camera of the uploaded scene without an upload -- no scene preparation, no table copied, no host
        wait.  camera: an rt_camera record (scene.camera, scenes.orbit_camera(...)).  Everything computed afterwards equals, bit
        for bit, what an upload() of the same scene with this camera computes; the accumulation, the feature strips and the denoise
        snapshot are void as after an upload, the sampler, the noise switch, the progressive settings and the temporal history
        stay.  The same record again changes nothing and voids nothing.  A NaN or an infinity in the record is refused."""
        cam = _capi.RtCamera.from_buffer_copy(bytes(camera))
        check(self._L.rt_set_camera(self._h, C.byref(cam)))

    def get_camera(self):
        """rt_get_camera: the RtCamera record of the last upload() or set_camera()."""
        cam = _capi.RtCamera()
        check(self._L.rt_get_camera(self._h, C.byref(cam)))
        return cam

    def set_materials(self, materials, sky=None, forget=True):
        """rt_set_materials: new material records (the structured array of scene.materials, one per sphere) and sky (an rt_material
        record; None keeps the current one) for the uploaded scene without an upload -- no scene preparation, no host wait of its
        own.  Everything computed afterwards equals, bit for bit, what an upload() of the same spheres, camera and lights with these
        records computes; voids and keeps what set_camera() does.  The same records again change nothing.
        forget=True: the temporal history's validation never looks at colour, so the spheres whose 48-byte record changed -- and the
        sky, 0xffffffff, when its record did -- are handed to temporal_forget(): their pixels start over.  Returns the ids forgotten.
        forget=False is the bare C call and returns []."""
        mat = np.ascontiguousarray(materials)
        assert mat.dtype.itemsize == 48 and mat.ndim == 1
        sky_bytes = self._sky if sky is None else bytes(sky)
        sky_rec = _capi.RtMaterial.from_buffer_copy(sky_bytes)
        check(self._L.rt_set_materials(self._h, mat.ctypes.data, mat.shape[0], C.byref(sky_rec)))
        old = self._materials
        changed = []
        if forget:
            a = mat.view(np.uint8).reshape(mat.shape[0], 48)
            b = old.view(np.uint8).reshape(old.shape[0], 48)
            changed = [int(k) for k in np.nonzero(np.any(a != b, axis=1))[0]]
            if sky_bytes != self._sky:
                changed.append(_capi.FORGET_SKY)
        self._materials = mat.copy()
        self._sky = sky_bytes
        if changed:
            self.temporal_forget(changed)
        return changed

    def set_lights(self, lights):
        """rt_set_lights: new colours and luminances for the uploaded lights (a list of rt_light records, as many as uploaded, each
        with the current direction bit for bit -- the uploaded one, or the one turn_lights() set last; a direction change goes through
        turn_lights()).  Equivalence, voids and keeps as set_materials(); never waits."""
        ls = list(lights)
        arr = (_capi.RtLight * max(1, len(ls)))()
        for k, l in enumerate(ls):
            arr[k] = _capi.RtLight.from_buffer_copy(bytes(l))
        check(self._L.rt_set_lights(self._h, arr, len(ls)))

    def turn_lights(self, lights, forget=True):
        """rt_turn_lights: whole new records -- direction, colour and luminance -- for the uploaded lights (a list of rt_light records,
        as many as uploaded; scenes.turn_light(...) turns one) without an upload: the shadow indices are rebuilt on the host over the
        layout kept from the upload and copied on the stream; no layout is built, nothing allocated, no host wait of its own.
        Everything computed afterwards equals, bit for bit, what an upload() of the same scene with these lights computes; voids
        and keeps what set_camera() does.  The same records again change nothing.
        forget=True: the temporal history's validation never looks at colour, and after a turn every shadow in it is stale, so
        temporal_reset() is called when a direction changed.  forget=False is the bare C call.  Returns whether a direction changed."""
        ls = list(lights)
        arr = (_capi.RtLight * max(1, len(ls)))()
        for k, l in enumerate(ls):
            arr[k] = _capi.RtLight.from_buffer_copy(bytes(l))
        old = self.get_lights() if forget else []
        check(self._L.rt_turn_lights(self._h, arr, len(ls)))
        turned = any(bytes(a)[:12] != bytes(b)[:12] for a, b in zip(arr, old))  # (direction: the record's first three floats)
        if turned:
            self.temporal_reset()
        return turned

    def get_lights(self):
        """rt_get_lights: the RtLight records the context renders with now (the last upload(), set_lights() or turn_lights())."""
        n = C.c_uint32(0)
        check(self._L.rt_get_lights(self._h, None, 0, C.byref(n)))
        arr = (_capi.RtLight * max(1, n.value))()
        check(self._L.rt_get_lights(self._h, arr, n.value, C.byref(n)))
        return [_capi.RtLight.from_buffer_copy(bytes(arr[k])) for k in range(n.value)]

    def set_exposure(self, exposure_scale):
        """rt_set_exposure: a new exposure for the uploaded scene.  Equivalence, voids and keeps as set_materials(); never waits."""
        check(self._L.rt_set_exposure(self._h, float(exposure_scale)))

    def temporal_forget(self, ids):
        """rt_temporal_forget: every pixel of the current history whose id is in ids (sphere indices; 0xffffffff, _capi.FORGET_SKY, is
        the sky) gets len = 0, so the next temporal call treats it as a pixel with no history.  Stream-ordered, no host wait; an empty
        list or an empty history does nothing."""
        f = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
        check(self._L.rt_temporal_forget(self._h, f.ctypes.data if f.size else None, f.size))

    def render(self, W, H, s0, s1, max_depth, seed, rowset=None, stats=True):
        """rt_render; stats=False passes out_stats = NULL: the call only enqueues work on the context's stream (no host
        wait; progressive 1-spp frames are launch bound) and returns None."""
        rs = rowset if rowset is not None else whole_image(H)
        rs = RtRowset.from_buffer_copy(bytes(rs))
        if not stats:
            check(self._L.rt_render(self._h, W, H, rs, s0, s1, max_depth, seed, None))
            self.W, self.rows = W, self._L.rt_rowset_local_rows(rs)
            return None
        st = RtStats()
        check(self._L.rt_render(self._h, W, H, rs, s0, s1, max_depth, seed, C.byref(st)))
        self.W, self.rows = W, st.local_rows
        return st

    def clear(self):
        check(self._L.rt_clear(self._h))

    def resolve(self, n=0):
        check(self._L.rt_resolve(self._h, n))
        return self._L.rt_last_resolve_ms(self._h)

    def download(self, hdr=True, ldr=True):
        h = np.zeros((self.rows, self.W, 3), dtype=np.float32) if hdr else None
        l = np.zeros((self.rows, self.W, 3), dtype=np.uint8) if ldr else None
        check(self._L.rt_download(self._h, h.ctypes.data if hdr else None, l.ctypes.data if ldr else None))
        return h, l

    def copy_to_device(self, dev_hdr_ptr=None, dev_ldr_ptr=None):
        check(self._L.rt_copy_to_device(self._h, C.c_void_p(dev_hdr_ptr or 0), C.c_void_p(dev_ldr_ptr or 0)))

    def synchronize(self):
        check(self._L.rt_synchronize(self._h))

    # ---- noise estimate (rt_api.h "noise estimate")
    def set_noise_estimate(self, on):
        """rt_set_noise_estimate: the next accumulation keeps the strip of second moments (changing it voids a running one)."""
        check(self._L.rt_set_noise_estimate(self._h, 1 if on else 0))

    def download_moments(self):
        """The sums of squared samples, (rows, W, 3) float32."""
        q = np.zeros((self.rows, self.W, 3), dtype=np.float32)
        check(self._L.rt_download_moments(self._h, q.ctypes.data))
        return q

    def copy_moments_to_device(self, dev_sq_ptr):
        """rt_copy_moments_to_device: the sums of squared samples ((rows, W, 3) float32) into caller-owned device memory,
        asynchronously on the context's stream."""
        check(self._L.rt_copy_moments_to_device(self._h, C.c_void_p(dev_sq_ptr or 0)))

    def noise_map(self, floor=NOISE_FLOOR):
        """(rows, W, 2) float32: absolute and relative standard error of every pixel's mean."""
        out = np.zeros((self.rows, self.W, 2), dtype=np.float32)
        check(self._L.rt_noise_map(self._h, float(floor), out.ctypes.data))
        return out

    def noise_summary(self, thresholds, floor=NOISE_FLOOR):
        """(counts, max_rel): counts[k] = pixels whose relative error is above thresholds[k] (at most 8; a non-finite error counts
        for every threshold), max_rel = the largest finite relative error."""
        thr = np.ascontiguousarray(thresholds, dtype=np.float32).reshape(-1)
        counts = np.zeros(thr.shape[0], dtype=np.uint32)
        mx = C.c_float(0.0)
        check(self._L.rt_noise_summary(self._h, float(floor), thr.ctypes.data, thr.shape[0], counts.ctypes.data, C.byref(mx)))
        return counts, mx.value

    def render_until(self, W, H, max_depth, seed, rel_error, fraction=0.0, step_spp=8, max_spp=1024, floor=NOISE_FLOOR, rowset=None):
        """Render `step_spp` sample planes at a time, from sample 1, until at most `fraction` of the pixels have a relative error
        above `rel_error`, or the next step would pass `max_spp`.  Turns the noise estimate on; returns the spp reached."""
        if step_spp < 1 or max_spp < max(step_spp, 2):
            raise ValueError("render_until: step_spp must be 1..max_spp and max_spp at least 2 (the estimate needs two samples)")
        self.set_noise_estimate(True)
        spp = 0
        while True:
            self.render(W, H, spp + 1, spp + 1 + step_spp, max_depth, seed, rowset=rowset, stats=False)
            spp += step_spp
            if spp >= 2:
                counts, _ = self.noise_summary([rel_error], floor=floor)
                if int(counts[0]) / (self.W * self.rows) <= fraction:
                    return spp
            if spp + step_spp > max_spp:
                return spp

    # ---- feature buffers (rt_api.h "feature buffers")
    def render_features(self, W, H, s0, s1, rowset=None, timed=False):
        """rt_render_features: first-hit albedo, normal, depth, coverage and object id of the samples [s0, s1), added to strips of
        their own (sequenced like render, independently of it).  timed=True waits and returns the HIP-event time in ms; else the
        call only enqueues work and returns None."""
        rs = rowset if rowset is not None else whole_image(H)
        rs = RtRowset.from_buffer_copy(bytes(rs))
        ms = C.c_double(0.0)
        check(self._L.rt_render_features(self._h, W, H, rs, s0, s1, C.byref(ms) if timed else None))
        self.feature_W, self.feature_rows = W, self._L.rt_rowset_local_rows(rs)
        return ms.value if timed else None

    def feature_samples(self):
        """Samples per pixel in the feature strips (0: nothing accumulated)."""
        n = C.c_uint32(0)
        check(self._L.rt_feature_samples(self._h, C.byref(n)))
        return n.value

    def download_features(self, normalize=False):
        """The strips as a dict of arrays shaped like the strip: albedo and normal (rows, W, 3) float32, depth and coverage (rows, W)
        float32 -- the raw sums, or with normalize=True each sum divided by the sample count in binary32 -- and id (rows, W) uint32, the
        object id of the sample added last (0xffffffff: it hit nothing)."""
        rows, W = self.feature_rows, self.feature_W
        feat = np.zeros((rows, W, 8), dtype=np.float32)
        ids = np.zeros((rows, W), dtype=np.uint32)
        check(self._L.rt_download_features(self._h, feat.ctypes.data, ids.ctypes.data))
        if normalize:
            feat = feat / np.float32(self.feature_samples())
            assert feat.dtype == np.float32
        return {"albedo": np.ascontiguousarray(feat[..., 0:3]), "normal": np.ascontiguousarray(feat[..., 3:6]),
                "depth": np.ascontiguousarray(feat[..., 6]), "coverage": np.ascontiguousarray(feat[..., 7]), "id": ids}

    def copy_features_to_device(self, feat_ptr=None, id_ptr=None):
        """rt_copy_features_to_device: the raw sums ((rows, W, 8) float32) and ids ((rows, W) uint32) into caller-owned device memory,
        asynchronously on the context's stream."""
        check(self._L.rt_copy_features_to_device(self._h, C.c_void_p(feat_ptr or 0), C.c_void_p(id_ptr or 0)))

    def clear_features(self):
        check(self._L.rt_clear_features(self._h))

    # ---- denoise (rt_api.h "denoise")
    def denoise(self, params=None, timed=False, variance=None):
        """rt_denoise: the feature-guided a-trous filter over the picture, its noise estimate and the feature strips as they are now
        (noise estimate on, at least 2 samples; feature strips of the same image and row set).  params: an RtDenoiseParams
        (_capi.denoise_params(levels=..., ...)) or None for the defaults.  timed=True waits and returns the HIP-event time in ms; else
        the call only enqueues work and returns None.  variance (rt_denoise_variance): an RtVarianceParams
        (_capi.variance_params(source=..., radius=...)) or None for this call as it always was; with source RT_VARIANCE_SPATIAL the
        variance comes from the picture's own neighbourhoods, so one sample suffices, the noise estimate may be off and pipelined
        frames stay in flight."""
        ms = C.c_double(0.0)
        if variance is None:
            check(self._L.rt_denoise(self._h, C.byref(params) if params is not None else None, C.byref(ms) if timed else None))
        else:
            check(self._L.rt_denoise_variance(self._h, C.byref(params) if params is not None else None, C.byref(variance), C.byref(ms) if timed else None))
        self.denoised_W, self.denoised_rows = self.W, self.rows
        return ms.value if timed else None

    def denoise_shards(self, hdr_ptr, sq_ptr, feat_ptr, W, H, world, rows_max, n, m, params=None, timed=False, block_rows=_capi.BLOCK_ROWS, variance=None):
        """rt_denoise_shards: the same filter over a W x H picture that `world` shards rendered (cyclic blocks of block_rows rows) and a
        gather brought to this device: hdr_ptr, sq_ptr ([world][rows_max * W * 3] float32) and feat_ptr ([world][rows_max * W * 8] float32,
        16-byte aligned) are device memory holding the shards' sums after n and m samples.  Needs no scene and no accumulation in this
        context; download_denoised() then returns the H x W result.  params and timed as in denoise().  variance
        (rt_denoise_shards_variance): as in denoise(); with source RT_VARIANCE_SPATIAL the shards may have rendered ONE sample with the
        noise estimate off, and sq_ptr may be None: the second moments are not read."""
        parts = _capi.shard_parts(W, H, world, rows_max, n, m, hdr_ptr, sq_ptr, feat_ptr, block_rows=block_rows)
        ms = C.c_double(0.0)
        if variance is None:
            check(self._L.rt_denoise_shards(self._h, C.byref(parts), C.byref(params) if params is not None else None, C.byref(ms) if timed else None))
        else:
            check(self._L.rt_denoise_shards_variance(self._h, C.byref(parts), C.byref(params) if params is not None else None, C.byref(variance),
                                                     C.byref(ms) if timed else None))
        self.denoised_W, self.denoised_rows = W, H
        return ms.value if timed else None

    # ---- temporal accumulation (rt_api.h "temporal accumulation")
    def denoise_temporal(self, params=None, tparams=None, timed=False, fetch=1, variance=None):
        """rt_denoise_temporal: denoise() with the previous call's pre-filter state reprojected into the current camera,
        validated against the guides and blended in before the levels.  The history survives set_camera() -- a camera move -- and
        upload(), and starts empty after temporal_reset() or when the picture's size or row set changes; on an empty history the result is
        denoise()'s.  tparams: an RtTemporalParams (_capi.temporal_params(max_history=..., ...)) or None for the defaults; params and
        timed as in denoise().  download_denoised() serves the result.  fetch (rt_denoise_temporal_fetch): 1, nearest, is
        rt_denoise_temporal's bits; 4, bilinear, interpolates the history from the four pixels around the reprojected point.  tparams
        None means that fetch's defaults (_capi.temporal_params_fetch).  variance (rt_denoise_temporal_variance): as in denoise()."""
        ms = C.c_double(0.0)
        if variance is None:
            check(self._L.rt_denoise_temporal_fetch(self._h, C.byref(params) if params is not None else None,
                                                    C.byref(tparams) if tparams is not None else None, int(fetch), C.byref(ms) if timed else None))
        else:
            check(self._L.rt_denoise_temporal_variance(self._h, C.byref(params) if params is not None else None,
                                                       C.byref(tparams) if tparams is not None else None, int(fetch), C.byref(variance),
                                                       C.byref(ms) if timed else None))
        self.denoised_W, self.denoised_rows = self.W, self.rows
        self.temporal_W, self.temporal_rows = self.W, self.rows
        return ms.value if timed else None

    def denoise_shards_temporal(self, hdr_ptr, sq_ptr, feat_ptr, ids_ptr, W, H, world, rows_max, n, m, camera, params=None, tparams=None, fetch=1,
                                timed=False, block_rows=_capi.BLOCK_ROWS, first_row=0, num_rows=None):
        """rt_denoise_shards_temporal: denoise_temporal() over the gathered parts of denoise_shards() -- plus ids_ptr ([world][rows_max * W]
        uint32, the shards' feature ids) and `camera`, the rt_camera record the shards were rendered with (scene.camera).  The parts hold
        rows [first_row, first_row + num_rows) of the W x H image (default: all of it).  The history is this context's one history, kept
        across calls and uploads and keyed with the image's size and the sharding: another sharding starts from an empty one, and world = 1
        with the rows and block_rows of a denoise_temporal() picture continues that picture's history.  Needs no scene and no accumulation
        in this context; download_denoised() and download_temporal() then return the num_rows x W results in image order.  params,
        tparams, fetch and timed as in denoise_temporal()."""
        return self.denoise_shards_temporal_variance(hdr_ptr, sq_ptr, feat_ptr, ids_ptr, W, H, world, rows_max, n, m, camera, params, tparams, fetch, timed,
                                                     block_rows, first_row, num_rows)

    def denoise_shards_temporal_variance(self, hdr_ptr, sq_ptr, feat_ptr, ids_ptr, W, H, world, rows_max, n, m, camera, params=None, tparams=None, fetch=1,
                                         timed=False, block_rows=_capi.BLOCK_ROWS, first_row=0, num_rows=None, variance=None):
        """rt_denoise_shards_temporal_variance: denoise_shards_temporal() with the variance source chosen, over the same one history.
        variance as in denoise_shards(): None is denoise_shards_temporal() as it always was; under RT_VARIANCE_SPATIAL n = 1 suffices and
        sq_ptr may be None."""
        frame = _capi.shard_frame(W, H, world, rows_max, n, m, camera, hdr_ptr, sq_ptr, feat_ptr, ids_ptr, block_rows=block_rows, first_row=first_row,
                                  num_rows=num_rows)
        ms = C.c_double(0.0)
        if variance is None:
            check(self._L.rt_denoise_shards_temporal(self._h, C.byref(frame), C.byref(params) if params is not None else None,
                                                     C.byref(tparams) if tparams is not None else None, int(fetch), C.byref(ms) if timed else None))
        else:
            check(self._L.rt_denoise_shards_temporal_variance(self._h, C.byref(frame), C.byref(params) if params is not None else None,
                                                              C.byref(tparams) if tparams is not None else None, int(fetch), C.byref(variance),
                                                              C.byref(ms) if timed else None))
        self.denoised_W, self.denoised_rows = W, frame.parts.rs.num_rows
        self.temporal_W, self.temporal_rows = W, frame.parts.rs.num_rows
        return ms.value if timed else None

    def temporal_reset(self):
        """rt_temporal_reset: drop the history; the next denoise_temporal() starts from an empty one."""
        check(self._L.rt_temporal_reset(self._h))

    def download_temporal(self):
        """The history as the last denoise_temporal() left it: state (rows, W, 4) float32, the blended (c.rgb, v) that went into level 0;
        len (rows, W) uint32, the frames blended into it; target (rows, W) uint32, the history pixel each pixel was blended with
        (local row * W + column; 0xffffffff: rejected)."""
        rows, W = self.temporal_rows, self.temporal_W
        state = np.zeros((rows, W, 4), dtype=np.float32)
        ln = np.zeros((rows, W), dtype=np.uint32)
        target = np.zeros((rows, W), dtype=np.uint32)
        check(self._L.rt_download_temporal(self._h, state.ctypes.data, ln.ctypes.data, target.ctypes.data))
        return {"state": state, "len": ln, "target": target}

    def download_denoised(self):
        """The last denoise()'s result: rgb (rows, W, 3) float32, the filtered MEAN colour; var (rows, W) float32, the variance left in
        it; ldr (rows, W, 3) uint8, its tonemap."""
        rows, W = self.denoised_rows, self.denoised_W
        rgb = np.zeros((rows, W, 3), dtype=np.float32)
        var = np.zeros((rows, W), dtype=np.float32)
        ldr = np.zeros((rows, W, 3), dtype=np.uint8)
        check(self._L.rt_download_denoised(self._h, rgb.ctypes.data, var.ctypes.data, ldr.ctypes.data))
        return {"rgb": rgb, "var": var, "ldr": ldr}

    def copy_denoised_to_device(self, rgb_ptr=None, var_ptr=None, ldr_ptr=None):
        """rt_copy_denoised_to_device: rgb ((rows, W, 3) float32), var ((rows, W) float32) and ldr ((rows, W, 3) uint8) into caller-owned
        device memory, asynchronously on the context's stream."""
        check(self._L.rt_copy_denoised_to_device(self._h, C.c_void_p(rgb_ptr or 0), C.c_void_p(var_ptr or 0), C.c_void_p(ldr_ptr or 0)))

    def denoise_forms(self):
        """Per level of the last denoise(): 0 not run, 1 taps read from global memory, 2 from a tile staged in LDS."""
        out = (C.c_uint32 * 5)()
        check(self._L.rt_unit_denoise_forms(self._h, out))
        return list(out)

    # ---- unit entries
    def last_trace_launch(self):
        """rt_unit_last_trace_launch as a TraceLaunch: which kernel variant the most recent trace launch of this context ran, its grid
        and queue cut, and the launcher's packed inputs and plan.  RtError (RT_ERR_SEQUENCE) before the first launch."""
        case = np.zeros(28, dtype=np.uint32)
        plan = np.zeros(28, dtype=np.uint32)
        n = C.c_uint32(0)
        check(self._L.rt_unit_last_trace_launch(self._h, case.ctypes.data, plan.ctypes.data, C.byref(n)))
        word = int(plan[25])
        k = decode_kernel_word(word)
        rows = trace_variants()
        single = (word & ~1) | (1 << 31)
        return TraceLaunch(row=rows.index(single) if (k["instantiated"] and single in rows) else -1, lights=k["lights"], kLds=k["kLds"],
                           kThreads=k["kThreads"], kScan=k["kScan"], kCache=k["kCache"], kHitLds=k["kHitLds"], kCarry=k["kCarry"],
                           kStash=k["kStash"], kMatsL2=k["kMatsL2"], kSgLds=k["kSgLds"], kGridQ=k["kGridQ"], blocks=int(plan[2]),
                           queue_block=int(plan[21]), static_blocks=int(plan[22]), dyn_begin=int(plan[23]), dyn_blocks=int(plan[24]),
                           launches=n.value, kernel_word=word, case_words=case, plan_words=plan)

    def last_trace_far_state(self):
        """rt_unit_last_trace_far_state: "lean" when the most recent trace launch ran its row's kernel without far-hit state, "full"
        when it ran the one with it.  RtError (RT_ERR_SEQUENCE) before the first launch."""
        lean = C.c_uint32(7)
        check(self._L.rt_unit_last_trace_far_state(self._h, C.byref(lean)))
        return "lean" if lean.value else "full"

    def trace_launches(self):
        """Trace-kernel launches of this context since rt_create (0 before the first: no error)."""
        n = C.c_uint32(0)
        rc = self._L.rt_unit_last_trace_launch(self._h, None, None, C.byref(n))
        if rc not in (_capi.RT_OK, _capi.RT_ERR_SEQUENCE):
            check(rc)
        return n.value

    def unit_tile_order(self, W, H, rowset=None, source=0):
        """rt_unit_tile_order: the work order of the strip's full tiles -- source 0 built afresh into buffers of the call's own (any tile
        count), source 1 what the context keeps for its running accumulation of this picture.  Returns None where there is none
        (*n_tiles = 0), else a dict: pilot_rays (n, 3, 6) float32, classes and flags (n,) uint8, order (n,) uint32, info (4,) uint32
        ([0] flagged tiles, [1..3] the bits of their constant sample)."""
        rs = rowset if rowset is not None else whole_image(H)
        rs = RtRowset.from_buffer_copy(bytes(rs))
        cap = max((W * self._L.rt_rowset_local_rows(rs)) >> 6, 1)
        out = {"pilot_rays": np.zeros((cap, 3, 6), dtype=np.float32), "classes": np.full(cap, 0xEE, dtype=np.uint8),
               "flags": np.full(cap, 0xEE, dtype=np.uint8), "order": np.full(cap, 0xEEEEEEEE, dtype=np.uint32),
               "info": np.full(4, 0xEEEEEEEE, dtype=np.uint32)}
        n = C.c_uint32(0)
        check(self._L.rt_unit_tile_order(self._h, W, H, rs, int(source), cap, C.byref(n), out["pilot_rays"].ctypes.data, out["classes"].ctypes.data,
                                         out["flags"].ctypes.data, out["order"].ctypes.data, out["info"].ctypes.data))
        if n.value == 0:
            return None
        return {k: (v if k == "info" else v[:n.value]) for k, v in out.items()}

    def unit_tile_order_sort(self, classes):
        """rt_unit_tile_order_sort: the production sort kernel over the given stored classes (uint8, each below 5).  Returns (order,
        guards): the n words of the order and the 64 guard words behind them (0xffffffff when intact)."""
        cls = np.ascontiguousarray(classes, dtype=np.uint8).reshape(-1)
        out = np.zeros(cls.shape[0] + 64, dtype=np.uint32)
        check(self._L.rt_unit_tile_order_sort(self._h, cls.ctypes.data if cls.size else None, cls.shape[0], out.ctypes.data))
        return out[:cls.shape[0]], out[cls.shape[0]:]

    def unit_halton(self, index, base):
        index = np.ascontiguousarray(index, dtype=np.uint32)
        out = np.zeros(index.shape[0], dtype=np.float32)
        check(self._L.rt_unit_halton(self._h, index.ctypes.data, base, index.shape[0], out.ctypes.data))
        return out

    def unit_math(self, op, x, y=None):
        x = np.ascontiguousarray(x, dtype=np.float32)
        y = np.ascontiguousarray(y if y is not None else np.zeros_like(x), dtype=np.float32)
        out = np.zeros_like(x)
        check(self._L.rt_unit_math(self._h, op, x.ctypes.data, y.ctypes.data, x.shape[0], out.ctypes.data))
        return out

    def unit_primary_rays(self, W, H, ijs):
        ijs = np.ascontiguousarray(ijs, dtype=np.uint32).reshape(-1, 3)
        out = np.zeros((ijs.shape[0], 6), dtype=np.float32)
        check(self._L.rt_unit_primary_rays(self._h, W, H, ijs.ctypes.data, ijs.shape[0], out.ctypes.data))
        return out

    def unit_closest_hit(self, rays):
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
        out = np.zeros((rays.shape[0], 10), dtype=np.float32)
        check(self._L.rt_unit_closest_hit(self._h, rays.ctypes.data, rays.shape[0], out.ctypes.data))
        return out

    def unit_shadow(self, light, points, glob_in_lds=False):
        """One byte per point (3 floats each) for light `light` of the uploaded scene: bit 0 = the light is occluded there, bit 1 = the
        answer came from the any-hit over every scan entry, not from the light's shadow index.  glob_in_lds: the index's global list
        is walked from its copy in LDS, as the trace kernel stages it."""
        points = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        out = np.zeros(points.shape[0], dtype=np.uint8)
        check(self._L.rt_unit_shadow(self._h, int(light), points.ctypes.data, points.shape[0], 1 if glob_in_lds else 0, out.ctypes.data))
        return out

    def unit_shadow_tier(self, tier, points, light=0, glob_in_lds=False):
        """unit_shadow with the index chosen (rt_unit_shadow_tier): tier 2 answers as the kernels without far-hit state ask -- bit 2 =
        the answer came from light 0's second index."""
        points = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        out = np.zeros(points.shape[0], dtype=np.uint8)
        check(self._L.rt_unit_shadow_tier(self._h, int(light), int(tier), points.ctypes.data, points.shape[0], 1 if glob_in_lds else 0, out.ctypes.data))
        return out

    def unit_trace(self, W, H, ijs, max_depth, seed):
        ijs = np.ascontiguousarray(ijs, dtype=np.uint32).reshape(-1, 3)
        rgb = np.zeros((ijs.shape[0], 3), dtype=np.float32)
        trav = np.zeros(ijs.shape[0], dtype=np.uint32)
        check(self._L.rt_unit_trace(self._h, W, H, ijs.ctypes.data, ijs.shape[0], max_depth, seed, rgb.ctypes.data,
                                    trav.ctypes.data))
        return rgb, trav
