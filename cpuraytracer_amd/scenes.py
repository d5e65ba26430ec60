"""Scene tables from the product's own host mirror (csrc/host/spheres-app.cpp: InitScene/InitCamera).

Returns the rt_api.h records as numpy structured arrays + ctypes structs, ready for HipRenderer.upload.
"""
import ctypes as C
import math
import os

import numpy as np

from . import _capi

_HOST_LIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "librt_host.so")
_host = None


def _load_host():
    global _host
    if _host is None:
        if not os.path.exists(_HOST_LIB):
            raise RuntimeError("librt_host.so is missing (%s): run __graft_entry__.build()" % _HOST_LIB)
        H = C.CDLL(_HOST_LIB)
        H.rth_build_scene.argtypes = [C.c_char_p, C.c_uint64, C.c_int, C.c_int, C.c_float, C.c_float, C.c_uint32, C.c_void_p,
                                      C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(_capi.RtCamera), C.POINTER(_capi.RtLight),
                                      C.POINTER(_capi.RtMaterial), C.POINTER(C.c_float)]
        _host = H
    return _host


class Scene:
    def __init__(self, spheres, materials, camera, sun, sky, exposure_scale, name, seed):
        self.spheres, self.materials = spheres, materials
        self.camera, self.sun, self.sky = camera, sun, sky
        self.exposure_scale = float(exposure_scale)
        self.name, self.seed = name, seed

    @property
    def n(self):
        return int(self.spheres.shape[0])


def build_scene(name="cover", seed=1, width=1200, height=800, vfov=-1.0, aperture=-1.0):
    """name: 'cover' (InitScene, 488 spheres), 'three' (C1), 'grid10k' (C5).  vfov/aperture < 0: scene default."""
    H = _load_host()
    cap = 10100
    sph = np.zeros(cap, dtype=_capi.SPHERE_DTYPE)
    mat = np.zeros(cap, dtype=_capi.MATERIAL_DTYPE)
    n = C.c_uint32(0)
    cam, sun, sky, exp = _capi.RtCamera(), _capi.RtLight(), _capi.RtMaterial(), C.c_float(0)
    rc = H.rth_build_scene(name.encode(), seed, width, height, vfov, aperture, cap, sph.ctypes.data, mat.ctypes.data, C.byref(n),
                           C.byref(cam), C.byref(sun), C.byref(sky), C.byref(exp))
    if rc != 0:
        raise RuntimeError("rth_build_scene(%r) failed with %d" % (name, rc))
    return Scene(sph[:n.value].copy(), mat[:n.value].copy(), cam, sun, sky, exp.value, name, seed)


def turn_light(light, degrees, axis=(0.0, 1.0, 0.0)):
    """The light record with its direction turned by `degrees` about `axis` (any non-zero vector; right-handed, Rodrigues' formula);
    colour and luminance stay.  A pure function of the record: evaluated in binary64 and rounded once to binary32, so the
    direction keeps its length up to that rounding.  Returns a new RtLight (HipRenderer.turn_lights takes a list of them)."""
    a = float(degrees) * (math.pi / 180.0)
    c, s = math.cos(a), math.sin(a)
    k = np.asarray(axis, dtype=np.float64)
    norm = float(np.sqrt(np.dot(k, k)))
    if not (norm > 0.0 and math.isfinite(norm)):
        raise ValueError("turn_light: the axis must be a finite non-zero vector")
    k = k / norm
    v = np.array([light.direction[0], light.direction[1], light.direction[2]], dtype=np.float64)
    r = v * c + np.cross(k, v) * s + k * (np.dot(k, v) * (1.0 - c))
    out = _capi.RtLight.from_buffer_copy(bytes(light))
    for j in range(3):
        out.direction[j] = np.float32(r[j])
    return out


def orbit_camera(camera, degrees, pivot=(0.0, 0.0, 0.0)):
    """The camera record turned by `degrees` about the vertical (y) axis through `pivot`: origin and origin_image_plane rotate about the
    pivot, x and y rotate as vectors; aperture and focal length stay.  A pure function of the record: evaluated in binary64 and rounded
    once to binary32.  Returns a new RtCamera."""
    a = float(degrees) * (math.pi / 180.0)
    c, s = math.cos(a), math.sin(a)  # libm's, as the spheres CLI's OrbitCamera takes them
    piv = np.asarray(pivot, dtype=np.float64)

    def turn(v):
        return np.array([c * v[0] + s * v[2], v[1], -s * v[0] + c * v[2]], dtype=np.float64)

    out = _capi.RtCamera.from_buffer_copy(bytes(camera))
    for name, point in (("origin", True), ("origin_image_plane", True), ("x", False), ("y", False)):
        src = getattr(camera, name)
        v = np.array([src[0], src[1], src[2]], dtype=np.float64)
        r = turn(v - piv) + piv if point else turn(v)
        dst = getattr(out, name)
        for k in range(3):
            dst[k] = np.float32(r[k])
    return out
