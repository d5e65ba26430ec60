"""rt_turn_lights without a GPU: the two entries are exported and declared with the header's signatures and refuse what needs no device;
the one writer of the shadow tables gives a turn the upload's tables inside the reservation's bounds (csrc/host/light_turn_selftest.cpp,
run as a program of its own); scenes.turn_light is a pure function of the record.

Which of the index builder's rules the selftest REQUIRES: the halving rule and the give-up rule are both reached on the CPU by directed
scenes (16,500 spheres of two sizes: 65,535 entries and more at 256 and at 128 cells per axis; 70 far larger spheres around a cluster:
a global list beyond 64) and both are required.  "Only huge spheres" is required to stay at ZERO: the median radius is the radius of
some sphere of the scene, that sphere is not huge (r <= 4 median), so no scene reaches the branch; the selftest's kind-5 scenes try."""
import ctypes as C
import inspect
import math
import os
import re
import subprocess

import numpy as np

from conftest import ROOT

RT_OK, RT_ERR_INVALID_ARG = 0, 2


def test_library_exports_and_capi_declares_the_entries(built):
    from cpuraytracer_amd import _capi
    L = _capi.load()
    src = open(os.path.join(ROOT, "include", "rt_api.h")).read()
    decls = {
        "rt_turn_lights": r"rt_ctx\s*\*\s*ctx\s*,\s*const\s+rt_light\s*\*\s*lights\s*,\s*uint32_t\s+n_lights",
        "rt_get_lights": r"rt_ctx\s*\*\s*ctx\s*,\s*rt_light\s*\*\s*out\s*,\s*uint32_t\s+capacity\s*,\s*uint32_t\s*\*\s*n_lights",
    }
    for name, args in decls.items():
        assert re.search(r"\bint\s+%s\s*\(\s*%s\s*\)\s*;" % (name, args), src), "%s: not declared as the issue states it" % name
        assert name in _capi.EXPORTS and hasattr(L, name), name
        assert getattr(L, name).restype is C.c_int, name
    assert L.rt_turn_lights.argtypes == [C.c_void_p, C.POINTER(_capi.RtLight), C.c_uint32]
    assert L.rt_get_lights.argtypes == [C.c_void_p, C.POINTER(_capi.RtLight), C.c_uint32, C.POINTER(C.c_uint32)]
    assert C.sizeof(_capi.RtLight) == 28
    assert re.search(r"#define\s+RT_API_VERSION\s+2\b", src) and L.rt_api_version() == 2  # the change only adds entries
    # rt_set_lights keeps its refusal and its words, and points at the new entry
    assert "a direction change goes through rt_turn_lights" in src and "the direction set last" in src
    # without a context both refuse the null argument before anything else
    light, n = _capi.RtLight(), C.c_uint32(5)
    assert L.rt_turn_lights(None, C.byref(light), 1) == RT_ERR_INVALID_ARG and b"rt_turn_lights" in L.rt_last_error()
    assert L.rt_turn_lights(None, None, 0) == RT_ERR_INVALID_ARG
    assert L.rt_get_lights(None, C.byref(light), 1, C.byref(n)) == RT_ERR_INVALID_ARG and b"rt_get_lights" in L.rt_last_error()
    assert n.value == 5  # a refused call writes nothing


def test_renderer_has_the_methods(built):
    from cpuraytracer_amd import HipRenderer, scenes
    p = inspect.signature(HipRenderer.turn_lights).parameters
    assert list(p) == ["self", "lights", "forget"] and p["forget"].default is True
    assert list(inspect.signature(HipRenderer.get_lights).parameters) == ["self"]
    p = inspect.signature(scenes.turn_light).parameters
    assert list(p) == ["light", "degrees", "axis"] and tuple(p["axis"].default) == (0, 1, 0)


def test_turn_light_is_a_pure_function_of_the_record(built):
    from cpuraytracer_amd import _capi, scenes
    l = _capi.RtLight()
    l.direction[0], l.direction[1], l.direction[2] = 0.6, 0.8, 0.0
    l.color[0], l.color[1], l.color[2], l.luminance = 0.25, 0.5, 0.75, 123.0
    before = bytes(l)
    t = scenes.turn_light(l, 90.0)  # about +y, right-handed: +x goes to -z
    assert bytes(l) == before and bytes(t)[12:] == before[12:]  # the argument is untouched; colour and luminance stay
    assert np.allclose([t.direction[0], t.direction[1], t.direction[2]], [0.0, 0.8, -0.6], atol=1e-7)
    assert bytes(scenes.turn_light(l, 90.0)) == bytes(t)
    assert bytes(scenes.turn_light(l, 0.0)) == before
    t = scenes.turn_light(l, 30.0, axis=(0.0, 0.0, 2.0))  # any non-zero axis; about +z: the angle to +x grows by 30 degrees
    a0, a1 = math.atan2(0.8, 0.6), math.atan2(t.direction[1], t.direction[0])
    assert abs(a1 - a0 - math.radians(30.0)) < 1e-6 and t.direction[2] == 0.0
    n = math.sqrt(sum(float(t.direction[c]) ** 2 for c in range(3)))
    assert abs(n - 1.0) < 1e-6  # the length stays, up to one rounding to binary32
    full = l
    for _ in range(720):  # 720 half-degree steps: back where it started, to the roundings' sum
        full = scenes.turn_light(full, 0.5)
    assert np.allclose([full.direction[c] for c in range(3)], [0.6, 0.8, 0.0], atol=1e-4)
    for axis in ((0.0, 0.0, 0.0), (float("nan"), 0.0, 1.0)):
        try:
            scenes.turn_light(l, 1.0, axis=axis)
        except ValueError:
            continue
        raise AssertionError("turn_light accepted the axis %r" % (axis,))


def test_a_turn_builds_the_shadow_tables_an_upload_builds(built):
    """host/light_turn_selftest.cpp: over 800 seeded random scenes of the three layout kinds (negative radii included), 0 to 3 lights
    and three consecutive turns each -- 2,400 scene x direction comparisons -- PrepareShadows over the part of the layout kept from
    PrepareScene(spheres, lights A) equals the shadow members of a fresh PrepareScene(spheres, lights B) byte for byte, and every table
    of an enabled index lies inside the bounds the upload reserves.  The program fails by itself where a layout kind, a light count or
    a reachable branch of the builder never occurred; the counts are checked again here."""
    exe = os.path.join(ROOT, "cpuraytracer_amd", "lib", "light_turn_selftest")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "light_turn_selftest ok" in p.stdout
    m = re.search(r"light turns: (\d+) scenes \(flat (\d+), hierarchy (\d+), cell grid (\d+); 0/1/2/3 lights (\d+)/(\d+)/(\d+)/(\d+)\), (\d+) turns, "
                  r"(\d+) indices built", p.stdout)
    assert m and all(int(g) > 0 for g in m.groups()), p.stdout
    assert int(m.group(9)) >= 2000 and sum(int(g) for g in m.groups()[1:4]) == int(m.group(1))
    m = re.search(r"branches: basis switch (\d+), spilled (\d+), wide (\d+), only huge (\d+), tier 2 on (\d+), tier 2 off (\d+) \(by its radius (\d+)\), "
                  r"no direction (\d+), on-off-on (\d+), off-on-off (\d+), enabled (\d+)", p.stdout)
    assert m, p.stdout
    b = [int(g) for g in m.groups()]
    assert all(v > 0 for v in b[:3] + b[4:]) and b[3] == 0, p.stdout  # "only huge": unreachable (this file's docstring)
    m = re.search(r"rules: halved (\d+), gave up (\d+); 1 x 1 grids (\d+), sgSph tables (\d+), turns that changed nx or ny (\d+), "
                  r"turns that grew a table (\d+)", p.stdout)
    assert m and all(int(g) > 0 for g in m.groups()), p.stdout
