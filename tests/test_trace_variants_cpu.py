"""The trace-kernel census without a GPU: the recipes of tests/trace_variant_cases.py, together with its NOT_RUN list, name every one
of the 110 kernels librt_hip.so instantiates (rt_unit_trace_variants x {one light, light list}) -- tests/test_trace_variants.py then
makes each recipe land on its kernel on the device.  Also the two unit entries as far as they need no context."""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT

import trace_variant_cases as T


def _variants(built):
    from cpuraytracer_amd import renderer
    return renderer.trace_variants()


def test_variant_list_is_the_header_list(built):
    """rt_unit_trace_variants: 55 distinct words in the order of csrc/rt_trace_variants.h, single-light form, bit 31 set -- the recipes'
    template arguments, written out by hand, pack to exactly these words row by row; and the entry's argument checks."""
    from cpuraytracer_amd import _capi, renderer
    L = _capi.load()
    words = _variants(built)
    assert len(words) == 55 and len(set(words)) == 55
    assert all(w >> 31 == 1 and w & 1 == 0 for w in words)
    assert [row for row, _, _, _ in T._ROWS] == list(range(55))
    for row, _, _, args in T._ROWS:
        assert T.kernel_word(*args) == words[row], "row %d of the recipes is not row %d of rt_trace_variants.h" % (row, row)
        k = renderer.decode_kernel_word(words[row])
        assert (k["kLds"], k["kThreads"], k["kScan"], k["kCache"], k["kHitLds"], k["kCarry"], k["kStash"], k["kMatsL2"], k["kSgLds"], k["kGridQ"]) == args
    # the header's macro list expands to as many rows: 19 written out, 3 sizes x (4 + 4 + 2 + 2) from the families
    src = open(os.path.join(ROOT, "cpuraytracer_amd", "csrc", "rt_trace_variants.h")).read()
    body = src[src.index("#define RT_TRACE_VARIANTS(X)"):src.index("// The scans of the unit kernels")]
    assert len(re.findall(r"^\s+X\(", body, flags=re.M)) + 3 * (4 * len(re.findall(r"RT_TRACE_PLAIN4, X", body)) + 2 * len(re.findall(r"RT_TRACE_PLAIN2, X", body))) == 55
    n = C.c_uint32(0)
    assert L.rt_unit_trace_variants(None, 0, C.byref(n)) == 0 and n.value == 55
    buf = np.zeros(55, dtype=np.uint32)
    assert L.rt_unit_trace_variants(buf.ctypes.data, 54, C.byref(n)) == 2 and b"rt_unit_trace_variants" in L.rt_last_error()
    assert not buf.any()
    assert L.rt_unit_trace_variants(None, 55, C.byref(n)) == 2 and L.rt_unit_trace_variants(buf.ctypes.data, 55, None) == 2


def test_recipes_and_not_run_are_exactly_the_110_kernels(built):
    words = _variants(built)
    every = {T.twin(w, lights) for w in words for lights in (False, True)}
    assert len(every) == 110
    expected = [r.kernel for r in T.RECIPES]
    not_run = {T.twin(words[row], lights) for row, _ in T.NOT_RUN for lights in (False, True)}
    assert all(w in every for w in expected), "a recipe expects a kernel the library does not instantiate"
    assert not (set(expected) & not_run), "a row is both reached by a recipe and listed in NOT_RUN"
    assert set(expected) | not_run == every, "kernels neither reached nor listed: %s" % sorted(hex(w) for w in every - set(expected) - not_run)
    # a word expected twice needs a reason (the empty-list recipes); exactly one recipe per word has none
    for w in set(expected):
        same = [r for r in T.RECIPES if r.kernel == w]
        assert sum(1 for r in same if r.why_again is None) == 1, [r.name for r in same]
        assert all(r.why_again is None or len(r.why_again) > 20 for r in same)
    assert len({r.name for r in T.RECIPES}) == len(T.RECIPES)
    # every row x {sun alone, two lights}; the empty list once per scan family (kScan 0..3); the carrying row pipelined, nothing else
    for r in T.RECIPES:
        assert r.n_lights in (0, 1, 2) and (r.kernel & 1) == (r.n_lights != 1) and r.kernel == T.twin(words[r.row], r.n_lights != 1)
        assert (r.mode != "ordinary") == bool(r.kernel >> 8 & 1)
    assert sorted((r.kernel >> 4) & 3 for r in T.RECIPES if r.n_lights == 0) == [0, 1, 2, 3]


def test_not_run_respects_its_cap():
    """A condition, not a measurement: at most three rows, each once (both twins go together by construction: an entry is a row), each
    with a one-line reason that names the plan comparison no buildable scene satisfies."""
    assert T.MAX_NOT_RUN == 3 and len(T.NOT_RUN) <= T.MAX_NOT_RUN
    assert len({row for row, _ in T.NOT_RUN}) == len(T.NOT_RUN)
    for row, reason in T.NOT_RUN:
        assert 0 <= row < 55 and isinstance(reason, str) and len(reason) > 40 and "\n" not in reason
    if T.NOT_RUN:
        design = open(os.path.join(ROOT, "DESIGN.md")).read()
        assert all("row %d" % row in design for row, _ in T.NOT_RUN)


def test_every_scene_has_every_material_class_and_the_floor(built):
    for name in T.SCENES:
        sc = T.build_scene(name, 131, 61)
        m, s = sc.materials, sc.spheres
        assert set(np.unique(m["type"])) == {0, 1, 2, 3}, name  # diffuse, metal, glass, emissive
        assert (m["luminance"][m["type"] == 3] > 0).all() and (m["tex_type"] == 1).any(), name  # lamps that shine; a checker
        assert s["r"].max() == 1000.0 and (s["r"] < 10.0).sum() == sc.n - 1, name  # the floor, and nothing else that large
        two = T.build_scene(name, 131, 61, 2)
        assert len(two.lights) == 2 and bytes(two.lights[0]) == bytes(sc.sun) and bytes(two.lights[1]) != bytes(sc.sun)
        assert T.build_scene(name, 131, 61, 0).lights == [] and not hasattr(sc, "lights")
        again = T.build_scene(name, 131, 61)
        assert again.spheres.tobytes() == s.tobytes() and again.materials.tobytes() == m.tobytes(), "%s is not reproducible" % name
    assert {r.scene for r in T.RECIPES} == set(T.SCENES)


def test_last_trace_launch_refuses_a_null_context(built):
    """(The refusal before the first launch needs a context: tests/test_trace_variants.py checks it on the device.)"""
    from cpuraytracer_amd import _capi
    L = _capi.load()
    words = np.full(56, 0xA5A5A5A5, dtype=np.uint32)
    n = C.c_uint32(77)
    assert L.rt_unit_last_trace_launch(None, words[:28].ctypes.data, words[28:].ctypes.data, C.byref(n)) == 2
    assert b"rt_unit_last_trace_launch" in L.rt_last_error()
    assert (words == 0xA5A5A5A5).all() and n.value == 77
