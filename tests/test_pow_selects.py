"""rt_powf at its early returns: the device (rt_unit_math op 2) and the host twin (rt_unit_math_host op 2: the same source compiled for
the host) against the oracle's own restatement, bit for bit, on every input at which one of the five returns decides -- y == 0, an x
that is not positive, x == 1, y log2 x below -160 and above 160 -- on their neighbours, and on the material domain of
tests/test_hit_processing.py (x in [0, 1], y a smoothness of the material space).  No tolerance.  The CPU test runs the host twin
alone.  (Written for the select form of those returns, which lost on the cell-grid config and was dropped -- docs/EXPERIMENTS.md;
whichever form the function has must pass it.)"""
import numpy as np
import pytest

import test_hit_processing_cpu as G

F = np.float32


def _f(bits):
    return np.array([bits], dtype=np.uint32).view(F)[0]


XS = np.array([0.0, -0.0, _f(0x00000001), 2.0 ** -126, 1.0 - 2.0 ** -24, 1.0, 1.0 + 2.0 ** -23, 0.5, _f(0x7F7FFFFF)], dtype=F)
YS = np.array([0.0, 5.0, 2.0 ** -20, 0.5, 1.0, 64.0, 1e4], dtype=F)


def inputs():
    """Every (x, y) of the two lists, then 4096 random pairs of the material domain."""
    x, y = np.meshgrid(XS, YS, indexing="ij")
    rng = np.random.default_rng(20261)
    smooth = np.array(sorted({float(m["smoothness"][0]) for m in G.material_records()}), dtype=F)
    xr = rng.uniform(0.0, 1.0, 4096).astype(F)
    yr = smooth[rng.integers(0, len(smooth), 4096)]
    return np.concatenate([x.ravel(), xr]).astype(F), np.concatenate([y.ravel(), yr]).astype(F)


def host_pow(x, y):
    from cpuraytracer_amd import _capi
    out = np.zeros_like(x)
    _capi.check(_capi.load().rt_unit_math_host(2, x.ctypes.data, y.ctypes.data, x.shape[0], out.ctypes.data))
    return out


def _assert_bits(got, want, x, y, what):
    bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
    assert bad.size == 0, "%s: %d of %d differ; first pow(%r, %r): %r, oracle %r" % (
        what, bad.size, len(want), float(x[bad[0]]), float(y[bad[0]]), float(got[bad[0]]), float(want[bad[0]]))


def _check_cases_are_there(x, y, want):
    """The lists reach every select: results 1 from y == 0 and from x == 1, 0 from x <= 0, 0 and inf from the range cuts."""
    assert np.all(want[y == 0] == 1) and np.all(want[(x == 1) & (y != 0)] == 1) and np.all(want[(x <= 0) & (y != 0)] == 0)
    big, tiny = (x == XS[-1]) & (y >= 64), (x == XS[2]) & (y >= 64)
    assert big.any() and np.all(np.isinf(want[big])) and tiny.any() and np.all(want[tiny] == 0)
    assert not np.isnan(want).any()


def test_host_twin_pow_equals_the_oracle(built, oracle):
    x, y = inputs()
    want = oracle.math_array(2, x, y)
    _check_cases_are_there(x, y, want)
    _assert_bits(host_pow(x, y), want, x, y, "host twin")


@pytest.mark.gpu
def test_device_pow_equals_the_oracle_and_the_host_twin(hip, oracle):
    x, y = inputs()
    want = oracle.math_array(2, x, y)
    _check_cases_are_there(x, y, want)
    _assert_bits(hip.unit_math(2, x, y), want, x, y, "device")
    _assert_bits(host_pow(x, y), want, x, y, "host twin")
