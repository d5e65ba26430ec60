"""The bookkeeping of the per-tile tables (csrc/host/rt_tile_tables.cpp), with no GPU and no library."""
import os
import re
import subprocess

from conftest import ROOT


def test_tile_tables_pass_their_standalone_scenarios_and_model_check(built):
    """host/tile_tables_selftest.cpp: the scenarios written from the comments of rt_tile_tables.h and DESIGN.md 5.1 and 10 (the call
    that builds the flags never sees their count, the knobs and fallbacks, a unit entry that rebuilds the masks for another picture
    inside an accumulation, a new scene, a new stream, a rebuild that fails at each of its points), and 100,000 seeded random
    scripts of scene uploads, accumulation starts with random knobs and pictures, continuing calls, unit entries, polls, stream
    replacements and injected build failures against a model of the device whose buffers remember what they were built from --
    after every step whatever a call may use was built from the current scene, the call's picture and the limits in force, tiles
    are left out of the queue only under all seven rules, the tile-aware accumulation only runs with flags of the accumulation's
    picture, and a count is never known before the model's event has completed.  The program fails by itself when one of the
    outcomes below was never reached."""
    exe = os.path.join(ROOT, "cpuraytracer_amd", "lib", "tile_tables_selftest")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "12 scenarios, 100000 scripts of 60 steps" in p.stdout and "tile_tables_selftest: ok" in p.stdout
    for name in ("keep", "not-wanted", "mask-build", "flag-build", "order-build", "count-arrived", "excluded-launch",
                 "other-picture-then-continue", "injected-failure"):
        assert int(re.search(r" %s (\d+)" % name, p.stdout).group(1)) > 0, name
