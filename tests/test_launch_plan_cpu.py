"""The launch plan (csrc/host/rt_launch_plan.cpp) without a GPU: `rt_unit_launch_plan` must answer every case of
tests/launch_plan_cases.py as the launcher did BEFORE the plan was moved out of rt_capi.hip.  tests/golden/launch_plans.npz holds those
answers, recorded from that launcher (docs/EXPERIMENTS.md "Launch plan": how) and never from the function under test: whole plans for
the directed cases and every sixth random one, a 64-bit hash of the plan for all, and the status, refusal, kernel and flag columns
the coverage conditions below are asserted on."""
import os
import subprocess

import numpy as np
import pytest

import launch_plan_cases as G
from conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_plans.npz")
N_FUNCTIONS = 110  # 55 variants of rt_trace_kernel (csrc/rt_trace_variants.h), each with its _lights twin
MIN_CASES = 20
REFUSALS = {1: "too many scan entries", 2: "no pipelining for this scene", 4: "shadow index in LDS without the hit stash",
            5: "quantised bounds without the hit stash"}
# Refusal 3, "internal: materials through L2 without the stash variant", is the one answer the recorded launcher can provably never
# give: materials go through L2 only where `cap2 >= cap + 8u && cap2 >= 16u` held for the stash kernel (rt_capi.hip:395 at 240f992;
# rt_launch_plan.cpp keeps the line), after which `cap` is cap2, or cap3 >= 48 -- so `stashKernel && cap >= 16u` two lines on holds.
NEVER_REFUSED_WITH = 3


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def cases():
    return G.all_cases()


@pytest.fixture(scope="module")
def plans(built, cases):
    from cpuraytracer_amd import _capi
    L = _capi.load()
    packed = np.ascontiguousarray(cases[0])
    out = np.full((len(packed), G.PLAN_WORDS), 0xdeadbeef, dtype=np.uint32)
    _capi.check(L.rt_unit_launch_plan(packed.ctypes.data, len(packed), out.ctypes.data))
    return out


def _kernel_name(w):
    return "rt_trace_kernel%s<%s, %d, %d, %s>" % ("_lights" if w & 1 else "", bool(w >> 1 & 1), (256, 512, 1024)[w >> 2 & 3], w >> 4 & 3,
                                                   ", ".join(str(bool(w >> b & 1)) for b in range(6, 13)))


def test_the_generator_still_makes_the_recorded_cases(golden, cases):
    packed, n_directed = cases
    assert len(packed) - n_directed >= 20000
    assert n_directed == int(golden["n_directed"]) and G.digest(packed) == str(golden["cases_digest"]), \
        "tests/launch_plan_cases.py no longer generates the cases launch_plans.npz was recorded for"


def test_every_plan_equals_the_recorded_launcher(golden, plans):
    idx = golden["full_idx"]
    diff = np.nonzero((plans[idx] != golden["full"]).any(axis=1))[0]
    assert len(diff) == 0, "case %d: words %s differ: got %s, recorded %s" % (
        idx[diff[0]], np.nonzero(plans[idx[diff[0]]] != golden["full"][diff[0]])[0].tolist(), plans[idx[diff[0]]].tolist(), golden["full"][diff[0]].tolist())
    bad = np.nonzero(G.row_hashes(plans) != golden["row_hash"])[0]
    assert len(bad) == 0, "%d plans differ from the recorded ones, first case %d: %s" % (len(bad), bad[0], plans[bad[0]].tolist())
    assert np.array_equal(plans[:, 25], golden["kernel"]) and np.array_equal(plans[:, 1], golden["refusal"])


def test_the_recorded_cases_reach_every_kernel_refusal_and_flag(golden):
    ok = golden["status"] == 0
    kernels, counts = np.unique(golden["kernel"][ok], return_counts=True)
    assert len(kernels) == N_FUNCTIONS, "%d of the %d instantiated functions are chosen" % (len(kernels), N_FUNCTIONS)
    assert np.all(kernels >> 31 == 1), "a chosen variant is not in the list of instantiated ones"
    few = [(_kernel_name(int(k)), int(c)) for k, c in zip(kernels, counts) if c < MIN_CASES]
    assert not few, "chosen in fewer than %d cases: %s" % (MIN_CASES, few)
    for code, what in REFUSALS.items():
        assert np.count_nonzero(golden["refusal"] == code) >= MIN_CASES, "refusal %d (%s) is reached too rarely" % (code, what)
    assert np.count_nonzero(golden["refusal"] == NEVER_REFUSED_WITH) == 0
    assert np.array_equal(golden["refusal"] != 0, ~ok)
    f = golden["flags"][ok]
    for name, values in (("mats_in_lds", f & 1), ("mats16_mode", f >> 1 & 3), ("sg_in_lds", f >> 3 & 1), ("tree_in_lds", f >> 4 & 1),
                         ("grid_in_lds", f >> 5 & 1), ("sg_glob16 != 0", f >> 6 & 1)):
        want = {0, 1, 2} if name == "mats16_mode" else {0, 1}
        assert set(np.unique(values).tolist()) == want, "%s takes only %s" % (name, np.unique(values).tolist())
    k = golden["kernel"][ok]
    for bit, name in ((0, "lights"), (1, "kLds"), (6, "kCache"), (7, "kHitLds"), (8, "kCarry"), (9, "kStash"), (10, "kMatsL2"), (11, "kSgLds"), (12, "kGridQ")):
        assert set(np.unique(k >> bit & 1).tolist()) == {0, 1}, name


def test_the_recorded_plans_keep_the_image_invariants(golden, cases):
    """What the kernels rely on, checked on the RECORDED launcher's answers (host/launch_plan_selftest.cpp checks the same on 200,000
    cases of the new function).  Two that one might expect do not hold and are not asserted (docs/EXPERIMENTS.md): the printed
    parts add up to the image only outside the cell-grid and materials-through-L2 variants, and the image stays within the BLOCK's
    share of the CU only where a stash or cache is placed (with several blocks per CU the tables alone may exceed it)."""
    idx = golden["full_idx"]
    p, c = golden["full"].astype(np.int64), cases[0][idx].astype(np.int64)
    keep = p[:, 0] == 0
    p, c = p[keep], c[keep]
    lds, k = p[:, 3], p[:, 25]
    waves, budget = c[:, G.W["block_threads"]] // 64, 160 * 1024 // c[:, G.W["blocks_per_cu"]]
    region = waves * p[:, 18] * 16
    placed = p[:, 17] != 0
    assert np.all(lds % 16 == 0)
    real_top = (c[:, G.W["n_levels"]] == 1) | (c[:, G.W["top_cnt"]] <= 128)  # (a hierarchy's top level has at most 128 nodes: RT_TREE_TOP)
    assert np.all(lds[real_top] <= 160 * 1024)
    assert np.all(lds[placed] <= budget[placed])
    assert np.all((p[:, 17] * 16 + region)[placed] == lds[placed]), "the stash or cache region ends where the image ends"
    assert np.all(p[~placed, 18] == 0) and np.all(p[~placed, 19] == 0)
    summed = (p[:, 10] >> 2 & 1 == 0) & (k >> 10 & 1 == 0)
    parts = (p[:, 4:10].sum(axis=1) + 15) // 16 * 16 + np.where(placed, region, 0)
    assert np.all(parts[summed] == lds[summed]), "the printed parts sum to ldsBytes"
    stash = k >> 9 & 1 == 1
    assert np.all((p[stash, 19] >= 16) & (p[stash, 19] <= 63) & (p[stash, 20] <= p[stash, 19]))
    assert np.all(stash[k >> 10 & 1 == 1]), "kMatsL2 => kStash"
    assert np.all(k >> 31 == 1), "the chosen tuple is in the shared list"
    ordinary = c[:, G.W["mode"]] == 0
    assert np.all(p[ordinary, 23] <= c[ordinary, G.W["total_paths"]]), "dyn_begin <= total_paths"
    assert np.all(p[~ordinary, 21:25] == 0) and np.all((k >> 8 & 1 == 1) == ~ordinary)
    assert np.all(p[:, 26] >> 4 & 1 == 1)


def test_cases_no_context_can_be_are_rejected(built):
    from cpuraytracer_amd import _capi
    L = _capi.load()
    out = np.zeros(G.PLAN_WORDS, dtype=np.uint32)
    for field, value in (("blocks_per_cu", 0), ("block_threads", 0), ("block_threads", 1000), ("block_threads", 2048), ("n_levels", 0), ("n_levels", 7),
                         ("cu_count", 0), ("mode", 2), ("reserved", 1), ("shape_flags", 16), ("setting_flags", 64), ("grid_nu", 65536)):
        packed = G.pack([G.base_case(**{field: value})])
        assert L.rt_unit_launch_plan(packed.ctypes.data, 1, out.ctypes.data) == 2, field
        assert b"rt_unit_launch_plan" in L.rt_last_error()
    assert L.rt_unit_launch_plan(None, 1, out.ctypes.data) == 2 and L.rt_unit_launch_plan(None, 0, None) == 0


def test_launch_plan_passes_its_standalone_invariant_sweep(built):
    """host/launch_plan_selftest.cpp: PlanTrace and PlanScanOnly alone, with no device and no library, over 200,000 generated launches;
    it exits 0 only when every plan keeps the invariants its header lists and every instantiated function was chosen."""
    exe = os.path.join(ROOT, "cpuraytracer_amd", "lib", "launch_plan_selftest")
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    assert "200000 cases" in p.stdout and "110 of 110 kernel functions chosen" in p.stdout and "launch_plan_selftest: ok" in p.stdout
