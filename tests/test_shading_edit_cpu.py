"""The shading edits without a GPU: rt_set_materials, rt_set_lights, rt_set_exposure and rt_temporal_forget are exported and declared
with the header's signatures; the one writer of the material tables gives an edit the upload's tables (csrc/host/shading_edit_selftest.cpp,
run as a program of its own); rt_unit_temporal_forget_host, the forget kernel's twin from the same membership rule, equals a numpy
restatement bit for bit and refuses what its contract refuses."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from conftest import ROOT

RT_OK, RT_ERR_INVALID_ARG = 0, 2
SKY = 0xFFFFFFFF


def test_library_exports_and_capi_declares_the_entries(built):
    from cpuraytracer_amd import _capi
    L = _capi.load()
    src = open(os.path.join(ROOT, "include", "rt_api.h")).read()
    decls = {
        "rt_set_materials": r"rt_ctx\s*\*\s*ctx\s*,\s*const\s+rt_material\s*\*\s*materials\s*,\s*uint32_t\s+n\s*,\s*const\s+rt_material\s*\*\s*sky",
        "rt_set_lights": r"rt_ctx\s*\*\s*ctx\s*,\s*const\s+rt_light\s*\*\s*lights\s*,\s*uint32_t\s+n_lights",
        "rt_set_exposure": r"rt_ctx\s*\*\s*ctx\s*,\s*float\s+exposure_scale",
        "rt_temporal_forget": r"rt_ctx\s*\*\s*ctx\s*,\s*const\s+uint32_t\s*\*\s*ids\s*,\s*uint32_t\s+n_ids",
        "rt_unit_temporal_forget_host": r"uint32_t\s*\*\s*len\s*,\s*const\s+uint32_t\s*\*\s*ids\s*,\s*uint32_t\s+npix\s*,\s*uint32_t\s+n_spheres\s*,"
                                        r"\s*const\s+uint32_t\s*\*\s*forget_ids\s*,\s*uint32_t\s+n_ids",
    }
    for name, args in decls.items():
        assert re.search(r"\bint\s+%s\s*\(\s*%s\s*\)\s*;" % (name, args), src), "%s: not declared as the issue states it" % name
        assert name in _capi.EXPORTS and hasattr(L, name), name
        assert getattr(L, name).restype is C.c_int, name
    assert L.rt_set_materials.argtypes == [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(_capi.RtMaterial)]
    assert L.rt_set_lights.argtypes == [C.c_void_p, C.POINTER(_capi.RtLight), C.c_uint32]
    assert L.rt_set_exposure.argtypes == [C.c_void_p, C.c_float]
    assert L.rt_temporal_forget.argtypes == [C.c_void_p, C.c_void_p, C.c_uint32]
    assert C.sizeof(_capi.RtMaterial) == 48 and C.sizeof(_capi.RtLight) == 28
    assert re.search(r"#define\s+RT_API_VERSION\s+2\b", src) and L.rt_api_version() == 2  # the change only adds entries
    # without a context every one refuses the null argument before anything else
    mat, light, one = _capi.RtMaterial(), _capi.RtLight(), (C.c_uint32 * 1)(0)
    assert L.rt_set_materials(None, C.byref(mat), 1, C.byref(mat)) == RT_ERR_INVALID_ARG and b"rt_set_materials" in L.rt_last_error()
    assert L.rt_set_lights(None, C.byref(light), 1) == RT_ERR_INVALID_ARG and b"rt_set_lights" in L.rt_last_error()
    assert L.rt_set_exposure(None, 1.0) == RT_ERR_INVALID_ARG and b"rt_set_exposure" in L.rt_last_error()
    assert L.rt_temporal_forget(None, one, 1) == RT_ERR_INVALID_ARG and b"rt_temporal_forget" in L.rt_last_error()


def test_renderer_has_the_methods(built):
    import inspect
    from cpuraytracer_amd import HipRenderer
    for name in ("set_materials", "set_lights", "set_exposure", "temporal_forget"):
        assert callable(getattr(HipRenderer, name)), name
    p = inspect.signature(HipRenderer.set_materials).parameters
    assert list(p) == ["self", "materials", "sky", "forget"] and p["sky"].default is None and p["forget"].default is True


def test_an_edit_builds_the_tables_an_upload_builds_and_the_forget_twin_is_the_naive_loop(built):
    """host/shading_edit_selftest.cpp: over 2,000 seeded random scenes of the three layout kinds (negative radii included) and material
    tables A and B, packable or not in every combination, PrepareMaterials(B) over the orig table of PrepareScene(spheres, A) equals
    PrepareScene(spheres, B)'s mats, mats16, mats16Ok and matType byte for byte; and rt_unit_temporal_forget_host equals a naive
    double loop over 3,000 cases: inline and table sets, the sky id, ids out of range, empty sets.  The program fails by itself when
    a layout kind, a packable combination or a form of the set never occurred."""
    exe = os.path.join(ROOT, "cpuraytracer_amd", "lib", "shading_edit_selftest")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "shading_edit_selftest ok" in p.stdout
    m = re.search(r"material tables: 2000 scenes \(flat (\d+), hierarchy (\d+), cell grid (\d+)\); packable A->B: no->no (\d+), no->yes (\d+), "
                  r"yes->no (\d+), yes->yes (\d+)", p.stdout)
    assert m and all(int(g) > 0 for g in m.groups()) and sum(int(g) for g in m.groups()[:3]) == 2000, p.stdout
    m = re.search(r"forget twin: 3000 cases \(inline sets (\d+), table sets (\d+), empty (\d+), with the sky (\d+), with ids out of range (\d+)\)", p.stdout)
    assert m and all(int(g) > 0 for g in m.groups()), p.stdout


def np_forget(length, ids, n_spheres, forget_ids):
    """The contract restated: len = 0 where the pixel's id is in the list; the sky is 0xffffffff; ids at or above the count match nothing."""
    f = np.asarray(forget_ids, dtype=np.uint32).reshape(-1)
    f = f[(f == SKY) | (f < np.uint32(min(n_spheres, SKY)))]
    out = np.array(length, dtype=np.uint32, copy=True)
    out[np.isin(np.asarray(ids, dtype=np.uint32), f)] = 0
    return out


def test_forget_twin_equals_a_numpy_restatement(built):
    from cpuraytracer_amd import _capi
    rng = np.random.default_rng(5)
    seen = {"inline": 0, "table": 0, "sky": 0, "beyond": 0, "empty": 0, "nothing matched": 0, "some matched": 0}
    for case in range(300):
        n = int(rng.integers(1, 40 if case % 2 else 3000))
        shape = (int(rng.integers(1, 9)), int(rng.integers(1, 71)))
        ids = rng.integers(0, n, shape).astype(np.uint32)
        ids[rng.random(shape) < 0.2] = SKY
        length = rng.integers(0, 65, shape).astype(np.uint32)
        k = int(rng.choice([0, 1, 5, 16, 17, 40, 300]))
        forget = rng.integers(0, n, k).astype(np.uint32)
        if k and rng.random() < 0.4:
            forget[rng.integers(0, k)] = SKY
            seen["sky"] += 1
        if k and rng.random() < 0.4:
            forget[rng.integers(0, k)] = n + int(rng.integers(0, 100))
            seen["beyond"] += 1
        kept = np.unique(forget[(forget != SKY) & (forget < n)]).size  # (the twin counts repeats too: only a lower bound on "table")
        seen["table" if kept > 16 else "inline"] += 1
        seen["empty"] += k == 0
        got = _capi.unit_temporal_forget_host(length, ids, n, forget)
        want = np_forget(length, ids, n, forget)
        assert got.dtype == np.uint32 and got.shape == length.shape and np.array_equal(got, want), case
        assert np.array_equal(got[got != 0], length[got != 0])  # every other word is untouched
        seen["some matched" if (got != length).any() else "nothing matched"] += 1
    assert all(v > 0 for v in seen.values()), seen


def test_forget_twin_refusals_and_edges(built):
    from cpuraytracer_amd import _capi
    L = _capi.load()
    length = np.array([3, 4, 5], dtype=np.uint32)
    ids = np.array([0, 1, SKY], dtype=np.uint32)
    f = np.array([1], dtype=np.uint32)
    keep = length.copy()
    assert L.rt_unit_temporal_forget_host(None, ids.ctypes.data, 3, 2, f.ctypes.data, 1) == RT_ERR_INVALID_ARG and b"rt_unit_temporal_forget_host" in L.rt_last_error()
    assert L.rt_unit_temporal_forget_host(length.ctypes.data, None, 3, 2, f.ctypes.data, 1) == RT_ERR_INVALID_ARG
    assert L.rt_unit_temporal_forget_host(length.ctypes.data, ids.ctypes.data, 3, 2, None, 1) == RT_ERR_INVALID_ARG
    assert np.array_equal(length, keep)  # a refused call changes nothing
    assert L.rt_unit_temporal_forget_host(None, None, 0, 2, f.ctypes.data, 1) == RT_OK  # no pixels
    assert L.rt_unit_temporal_forget_host(length.ctypes.data, ids.ctypes.data, 3, 2, None, 0) == RT_OK and np.array_equal(length, keep)  # no ids
    # the sky is named by 0xffffffff alone; 0xfffffffe is an id beyond every count
    assert np.array_equal(_capi.unit_temporal_forget_host(length, ids, 2, [0xFFFFFFFE]), keep)
    assert np.array_equal(_capi.unit_temporal_forget_host(length, ids, 2, [SKY]), [3, 4, 0])
    # an id at the count matches nothing even where a pixel holds it
    assert np.array_equal(_capi.unit_temporal_forget_host(length, np.array([0, 2, 1], np.uint32), 2, [2]), keep)
    assert np.array_equal(_capi.unit_temporal_forget_host(length, ids, 2, [1, 1, 0]), [0, 0, 5])
