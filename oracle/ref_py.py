"""ORACLE — TEST INFRASTRUCTURE ONLY.

ctypes binding of oracle/_ref/libref.so: the reference's own translation units, compiled unmodified over the stand-in headers
of oracle/ref_shim/ (oracle/Makefile, target _ref/libref.so; C ABI in ref_api.h).  Used by tests/test_reference_code_cpu.py and
tests/golden/make_reference_code_answers.py only.  The library exists only where the reference's sources do; nothing under
oracle/_ref/ is committed.
"""
import ctypes as C
import os

import numpy as np

from .oracle_py import RtCamera, RtLight, RtMaterial, RtSphere

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "_ref", "libref.so")


def _entry():
    """__graft_entry__ (repository root): it owns the build of libref.so, with files and make only"""
    import sys
    root = os.path.dirname(_HERE)
    if root not in sys.path:
        sys.path.insert(0, root)
    import __graft_entry__
    return __graft_entry__


def reference_present():
    return os.path.exists(os.path.join(_entry().reference_root(), "src", "common-lib", "ray-tracing.cpp"))


def build(force=False):
    """make _ref/libref.so when the recipe or the reference's sources changed (__graft_entry__.build_reference_library).  Returns
    the library's path, or None where the reference is absent; raises where the compile fails."""
    return _entry().build_reference_library(force=force, quiet=False)


_lib = None


def lib():
    """The loaded library.  Raises where it is missing or does not load."""
    global _lib
    if _lib is None:
        build()
        L = C.CDLL(LIB_PATH)
        V, U32, F = C.c_void_p, C.c_uint32, C.c_float
        for name, args in (("ref_halton", [V, U32, U32, V]), ("ref_halton_2d", [V, U32, U32, U32, V]), ("ref_halton_ring", [V, U32, U32, V]),
                           ("ref_halton_disk", [V, U32, U32, U32, V]), ("ref_halton_hemisphere", [V, U32, U32, U32, V]),
                           ("ref_sphere_intersect", [C.POINTER(RtSphere), V, U32, V]), ("ref_scene_free", [V]),
                           ("ref_list_closest", [V, V, U32, V]), ("ref_bvh_closest", [V, V, U32, V]),
                           ("ref_camera_make", [V, V, F, F, F, F, C.POINTER(RtCamera)]), ("ref_camera_ray", [C.POINTER(RtCamera), V, U32, V]),
                           ("ref_texture_eval", [C.POINTER(RtMaterial), V, U32, V]), ("ref_material_free", [V]),
                           ("ref_material_counters", [V, V]), ("ref_scatter", [V, V, U32, V, V]), ("ref_emit", [V, V, U32, V]),
                           ("ref_shade", [V, V, U32, V, U32, V, V, V, V]), ("ref_light_shade", [V, V, U32, V, V, V, V]),
                           ("ref_light_make", [V, F, F, F, F, C.POINTER(RtLight)])):
            fn = getattr(L, name)
            fn.argtypes, fn.restype = args, None
        L.ref_libm.argtypes, L.ref_libm.restype = [U32, V, V, U32, V], C.c_int
        L.ref_scene_new.argtypes, L.ref_scene_new.restype = [V, U32, U32], V
        L.ref_material_new.argtypes, L.ref_material_new.restype = [C.POINTER(RtMaterial)], V
        _lib = L
    return _lib


def _f32(a, cols):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1, cols)


def _halton(fn, index, bases, cols):
    index = np.ascontiguousarray(index, dtype=np.uint64)
    out = np.zeros((index.shape[0], cols), dtype=np.float32)
    getattr(lib(), fn)(index.ctypes.data, index.shape[0], *bases, out.ctypes.data)
    return out


def halton(index, base):
    return _halton("ref_halton", index, (base,), 1)[:, 0]


def halton_2d(index, b1, b2):
    return _halton("ref_halton_2d", index, (b1, b2), 2)


def halton_ring(index, base):
    return _halton("ref_halton_ring", index, (base,), 2)


def halton_disk(index, b1, b2):
    return _halton("ref_halton_disk", index, (b1, b2), 2)


def halton_hemisphere(index, b1, b2):
    return _halton("ref_halton_hemisphere", index, (b1, b2), 3)


SIN, COS, POW, TAN, SQRT = 0, 1, 2, 3, 4


def libm(op, x, y=None):
    x = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    y = np.ascontiguousarray(y if y is not None else np.zeros_like(x), dtype=np.float32).reshape(-1)
    out = np.zeros_like(x)
    assert lib().ref_libm(op, x.ctypes.data, y.ctypes.data, x.shape[0], out.ctypes.data) == 0
    return out


def sphere_intersect(sphere, rays):
    """sphere: (cx, cy, cz, r); rays [n, 6] -> hits [n, 10]"""
    rays = _f32(rays, 6)
    out = np.zeros((rays.shape[0], 10), dtype=np.float32)
    s = RtSphere(*[float(np.float32(v)) for v in sphere])
    lib().ref_sphere_intersect(C.byref(s), rays.ctypes.data, rays.shape[0], out.ctypes.data)
    return out


class Scene:
    def __init__(self, spheres, bvh_srand=1):
        sph = np.ascontiguousarray(spheres)
        assert sph.dtype.itemsize == 16
        self.n = sph.shape[0]
        self._h = lib().ref_scene_new(sph.ctypes.data, self.n, bvh_srand)

    def _closest(self, fn, rays):
        rays = _f32(rays, 6)
        out = np.zeros((rays.shape[0], 10), dtype=np.float32)
        fn(self._h, rays.ctypes.data, rays.shape[0], out.ctypes.data)
        return out

    def list_closest(self, rays):
        return self._closest(lib().ref_list_closest, rays)

    def bvh_closest(self, rays):
        return self._closest(lib().ref_bvh_closest, rays)

    def close(self):
        if self._h:
            lib().ref_scene_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def camera_make(origin, look_at, vfov, aspect, focal, aperture):
    o, l = _f32(origin, 3), _f32(look_at, 3)
    cam = RtCamera()
    lib().ref_camera_make(o.ctypes.data, l.ctypes.data, vfov, aspect, focal, aperture, C.byref(cam))
    return cam


def camera_ray(camera, uv_offset):
    q = _f32(uv_offset, 4)
    out = np.zeros((q.shape[0], 6), dtype=np.float32)
    cam = RtCamera.from_buffer_copy(bytes(camera))
    lib().ref_camera_ray(C.byref(cam), q.ctypes.data, q.shape[0], out.ctypes.data)
    return out


def texture_eval(material, uv):
    uv = _f32(uv, 2)
    out = np.zeros((uv.shape[0], 4), dtype=np.float32)
    m = RtMaterial.from_buffer_copy(bytes(material))
    lib().ref_texture_eval(C.byref(m), uv.ctypes.data, uv.shape[0], out.ctypes.data)
    return out


def light_make(direction, r, g, b, luminance):
    d = _f32(direction, 3)
    out = RtLight()
    lib().ref_light_make(d.ctypes.data, r, g, b, luminance, C.byref(out))
    return out


def _lights(lights):
    arr = (RtLight * max(1, len(lights)))()
    for k, l in enumerate(lights):
        arr[k] = RtLight.from_buffer_copy(bytes(l))
    return arr


class Material:
    def __init__(self, record):
        m = RtMaterial.from_buffer_copy(bytes(record))
        self._h = lib().ref_material_new(C.byref(m))

    def counters(self):
        out = np.zeros(2, dtype=np.uint64)
        lib().ref_material_counters(self._h, out.ctypes.data)
        return out

    def scatter(self, in14):
        """[n, 14] (ray origin, ray direction, pos, normal, uv) -> ([n, 10] flag, attenuation, origin, direction; [n, 4] counters)"""
        q = _f32(in14, 14)
        out = np.zeros((q.shape[0], 10), dtype=np.float32)
        cnt = np.zeros((q.shape[0], 4), dtype=np.uint64)
        lib().ref_scatter(self._h, q.ctypes.data, q.shape[0], out.ctypes.data, cnt.ctypes.data)
        return out, cnt

    def emit(self, hits8):
        q = _f32(hits8, 8)
        out = np.zeros((q.shape[0], 3), dtype=np.float32)
        lib().ref_emit(self._h, q.ctypes.data, q.shape[0], out.ctypes.data)
        return out

    def shade(self, hits8, lights, view_origin, occluders=None):
        """-> ([n, 3] Shade, [n, n_lights] occluded flags)"""
        q = _f32(hits8, 8)
        vo = _f32(view_origin, 3)
        out = np.zeros((q.shape[0], 3), dtype=np.float32)
        occ = np.zeros((q.shape[0], max(1, len(lights))), dtype=np.uint8)
        lib().ref_shade(self._h, q.ctypes.data, q.shape[0], _lights(lights), len(lights), vo.ctypes.data,
                        occluders._h if occluders is not None else None, out.ctypes.data, occ.ctypes.data)
        return out, occ[:, :len(lights)]

    def light_shade(self, hits8, light, view_origin, occluders=None):
        q = _f32(hits8, 8)
        vo = _f32(view_origin, 3)
        out = np.zeros((q.shape[0], 3), dtype=np.float32)
        lib().ref_light_shade(self._h, q.ctypes.data, q.shape[0], _lights([light]), vo.ctypes.data,
                              occluders._h if occluders is not None else None, out.ctypes.data)
        return out

    def close(self):
        if self._h:
            lib().ref_material_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
