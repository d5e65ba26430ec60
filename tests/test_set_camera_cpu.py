"""rt_set_camera / rt_get_camera without a GPU: the library exports them, _capi declares them with the header's signatures, and the
two event functions (rtseq::CameraChanged, rttile::CameraChanged) void what a scene upload voids -- csrc/host/camera_events_selftest.cpp,
run as a program of its own."""
import ctypes as C
import os
import re
import subprocess

from conftest import ROOT

RT_ERR_INVALID_ARG = 2


def test_library_exports_and_capi_declares_the_two_entries(built):
    from cpuraytracer_amd import _capi
    L = _capi.load()
    src = open(os.path.join(ROOT, "include", "rt_api.h")).read()
    for name, second in (("rt_set_camera", r"const\s+rt_camera\s*\*\s*camera"), ("rt_get_camera", r"rt_camera\s*\*\s*out")):
        assert re.search(r"\bint\s+%s\s*\(\s*rt_ctx\s*\*\s*ctx\s*,\s*%s\s*\)\s*;" % (name, second), src), "%s: not declared as the issue states it" % name
        assert name in _capi.EXPORTS and hasattr(L, name), name
        fn = getattr(L, name)
        assert fn.argtypes == [C.c_void_p, C.POINTER(_capi.RtCamera)], name
        assert fn.restype is C.c_int, name
    assert C.sizeof(_capi.RtCamera) == 72
    assert re.search(r"#define\s+RT_API_VERSION\s+2\b", src) and L.rt_api_version() == 2  # the change only adds entries
    # without a context both refuse a null argument before anything else
    cam = _capi.RtCamera()
    assert L.rt_set_camera(None, C.byref(cam)) == RT_ERR_INVALID_ARG and b"rt_set_camera" in L.rt_last_error()
    assert L.rt_get_camera(None, C.byref(cam)) == RT_ERR_INVALID_ARG and b"rt_get_camera" in L.rt_last_error()


def test_renderer_has_the_two_methods(built):
    from cpuraytracer_amd import HipRenderer
    assert callable(HipRenderer.set_camera) and callable(HipRenderer.get_camera)


def test_camera_events_void_what_a_scene_upload_voids(built):
    """host/camera_events_selftest.cpp: from every state that 100,000 seeded random scripts of render calls, settings, uploads, camera
    moves and other events reach, the camera event leaves rtseq::State and rttile::State field by field equal to what SceneReplaced
    leaves, with the same void mask; a move without a scene is refused and moves nothing.  Scenarios: a pending batch is settled
    first (rendered under the camera it was asked of), planes traced ahead become invalid and a restart traces anew, frames in flight
    are dropped, the flagged tiles' count is neither pending nor known afterwards and a stale copy still on its way is never taken
    for the new camera's, the same record is no event.  The program fails by itself when a kind of state was never reached."""
    exe = os.path.join(ROOT, "cpuraytracer_amd", "lib", "camera_events_selftest")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "6 scenarios, 100000 scripts of 60 steps" in p.stdout and "camera_events_selftest: ok" in p.stdout
    for name in ("pending-batch", "planes-ahead", "frames-in-flight", "masks-valid", "order-valid", "count-pending", "count-known", "no-scene",
                 "stale-copy-in-flight", "same-record", "states compared", "camera moves"):
        assert int(re.search(r"\b%s (\d+)" % name, p.stdout).group(1)) > 0, name
