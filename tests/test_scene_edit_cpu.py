"""The scene record and its edits without a GPU (csrc/host/rt_scene_edit.{h,cpp}) through the stand-alone
`scene_edit_selftest`: every refusal of rt_scene_upload, the five edits and the two getters with its code and its exact words from a
record filled by hand, the same-record rule, decide-then-commit over seeded random scripts against a model that stores the last
accepted arguments, and the staging plans' layout and bound.  (The bound against the plans of generated scenes and light lists is
checked by `light_turn_selftest` and `shading_edit_selftest`, where those are generated.)"""
import os
import re
import subprocess

from conftest import ROOT


def test_the_record_the_decisions_and_the_staging_plans(built):
    exe = os.path.join(ROOT, "cpuraytracer_amd", "lib", "scene_edit_selftest")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "scene_edit_selftest ok" in p.stdout
    m = re.search(r"refusals: (\d+), each with its code, its words and the record unchanged", p.stdout)
    assert m and int(m.group(1)) >= 100, p.stdout
    m = re.search(r"scripts: (\d+) steps \(uploads (\d+); refused / same / changed: camera (\d+)/(\d+)/(\d+), materials (\d+)/(\d+)/(\d+), "
                  r"set_lights (\d+)/(\d+)/(\d+), turn_lights (\d+)/(\d+)/(\d+), exposure (\d+)/(\d+)/(\d+)\), (\d+) edits before the first scene", p.stdout)
    assert m and int(m.group(1)) >= 3000 and all(int(g) > 0 for g in m.groups()), p.stdout
    assert "same record:" in p.stdout and "plans:" in p.stdout


def test_the_unit_is_plain_host_code(built):
    """No HIP header reaches the unit, and the library has no second copy of what moved into it."""
    host = os.path.join(ROOT, "cpuraytracer_amd", "csrc", "host")
    for name in ("rt_scene_edit.h", "rt_scene_edit.cpp"):
        src = open(os.path.join(host, name)).read()
        assert "hip/" not in src and "hip_runtime" not in src, name
    capi = open(os.path.join(ROOT, "cpuraytracer_amd", "csrc", "rt_capi.hip")).read()
    for moved in ("kCameraFields", "CameraFieldNotFinite", "SameCameraBits", "MaterialStageBytes", "StageAlign", "ShadowStageBytesMax"):
        assert moved not in capi, moved
