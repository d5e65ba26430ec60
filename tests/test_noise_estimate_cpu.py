"""Noise estimate, the part that needs no GPU (csrc/rt_noise.h, DESIGN.md "Noise estimate"): the per-pixel estimate compiled for the
host (rt_unit_noise_estimate_host, the same source the kernels compile) against a numpy restatement of its contract, bit for bit; the
quality of a variance taken from binary32 sums against an analytic bound; the API surface."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

RT_ERR_SEQUENCE = 6


def np_estimate(hdr, sq, n, floor, want_var=False):
    """The contract, restated: binary64 + - * / in the order of rt_api.h, one rounding to binary32, the IEEE binary32 square root.
    hdr, sq: [..., 3] float32.  Returns [..., 2] float32 (absolute, relative); with want_var the three var_c as well."""
    S = np.asarray(hdr, dtype=np.float32).astype(np.float64)
    Q = np.asarray(sq, dtype=np.float32).astype(np.float64)
    N, N1 = np.float64(n), np.float64(n - 1)
    with np.errstate(all="ignore"):
        mean = S / N
        var = (Q - S * mean) / N1
        var = np.where(var > 0.0, var, 0.0)
        V = (var[..., 0] + var[..., 1]) + var[..., 2]
        M = (mean[..., 0] + mean[..., 1]) + mean[..., 2]
        abs2 = V / N
        d = M + np.float64(np.float32(floor))
        out = np.stack([np.sqrt(abs2.astype(np.float32)), np.sqrt((abs2 / (d * d)).astype(np.float32))], axis=-1)
    assert out.dtype == np.float32
    return (out, var) if want_var else out


def host_estimate(hdr, sq, n, floor):
    from cpuraytracer_amd import _capi
    L = _capi.load()
    hdr = np.ascontiguousarray(hdr, dtype=np.float32).reshape(-1, 3)
    sq = np.ascontiguousarray(sq, dtype=np.float32).reshape(-1, 3)
    out = np.full((hdr.shape[0], 2), -1.0, dtype=np.float32)
    _capi.check(L.rt_unit_noise_estimate_host(hdr.ctypes.data, sq.ctypes.data, hdr.shape[0], n, float(floor), out.ctypes.data))
    return out


def assert_same_bits(a, b, what):
    """Bit for bit, except that a NaN only has to meet a NaN (its sign and payload are outside the contract)."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    assert a.shape == b.shape, what
    na, nb = np.isnan(a), np.isnan(b)
    assert np.array_equal(na, nb), "%s: NaNs in different places" % what
    bad = (a.view(np.uint32) != b.view(np.uint32)) & ~na
    assert not bad.any(), "%s: %d of %d values differ, first at %s: %r vs %r" % (what, int(bad.sum()), bad.size, np.argwhere(bad)[0], a[bad][0], b[bad][0])


def sequential_sums(samples):
    """samples [n, npix, 3] float32 -> (S, Q) as the accumulate kernels build them: q = q + (v * v), two roundings, increasing s."""
    S = np.zeros(samples.shape[1:], dtype=np.float32)
    Q = np.zeros(samples.shape[1:], dtype=np.float32)
    for v in samples:
        S = S + v
        Q = Q + (v * v)
    assert S.dtype == np.float32 and Q.dtype == np.float32
    return S, Q


@pytest.mark.parametrize("n", [2, 3, 16, 128, 4097])
@pytest.mark.parametrize("floor", [0.0, 0.01, 1.5])
def test_host_twin_equals_numpy_on_random_strips(built, n, floor):
    rng = np.random.default_rng(1000 * n + int(100 * floor))
    npix = 20000
    # strips of real sums: n samples of a skewed distribution per channel, at a brightness of 1e-3 .. 1e3 per pixel
    scale = (10.0 ** rng.uniform(-3, 3, (1, npix, 1))).astype(np.float32)
    k = min(n, 24)  # (the sums of k draws stand in for n samples: Q and S stay consistent enough, and n is only a divisor)
    v = (rng.gamma(0.7, 1.0, (k, npix, 3)).astype(np.float32) * scale).astype(np.float32)
    S, Q = sequential_sums(v)
    assert_same_bits(host_estimate(S, Q, n, floor), np_estimate(S, Q, n, floor), "sums of samples, n = %d" % n)
    # ... and unrelated S and Q over the whole exponent range, both signs of S: the formula is total
    S = (rng.standard_normal((npix, 3)) * 10.0 ** rng.uniform(-30, 30, (npix, 3))).astype(np.float32)
    Q = (10.0 ** rng.uniform(-40, 38, (npix, 3))).astype(np.float32)
    assert_same_bits(host_estimate(S, Q, n, floor), np_estimate(S, Q, n, floor), "unrelated strips, n = %d" % n)


def test_host_twin_edge_cases(built):
    inf, big, tiny = np.float32(np.inf), np.float32(3.0e38), np.float32(1e-40)
    cases = [
        # (hdr, sq, n, floor, what)
        ([3, 3, 3], [1, 1, 1], 4, 0.01, "Q < S^2/n clamps to no variance"),
        ([3, 3, 3], [2.25, 2.25, 2.25], 4, 0.01, "Q == S^2/n"),
        ([0, 0, 0], [0, 0, 0], 7, 0.01, "all-zero pixel"),
        ([0, 0, 0], [0, 0, 0], 7, 0.0, "all-zero pixel without a floor: 0/0"),
        ([1, -1, 0], [1, 1, 0], 2, 0.0, "M == 0 with variance, floor 0: x/0"),
        ([1, 2, 3], [1, 2, 9], 2, 0.01, "n == 2"),
        ([1, 0, 0], [1, 0, 0], 2, 0.0, "n == 2, one sample of 1 and one of 0"),
        ([big, big, big], [inf, inf, inf], 2, 0.01, "squares overflowed binary32"),
        ([big, big, big], [big, big, big], 3, 0.01, "huge sums"),
        ([big, 0, 0], [inf, 0, 0], 16, 1.0, "one overflowed channel"),
        ([tiny, tiny, tiny], [1e-45, 1e-45, 1e-45], 2, 0.0, "denormal sums"),
        ([tiny, 0, tiny], [0, 0, 0], 5, 1e-38, "denormal sums whose squares flushed to zero"),
        ([1e-20, 1e-20, 1e-20], [1e-38, 1e-38, 1e-38], 2, 0.0, "tiny normal values"),
        ([inf, 1, 1], [inf, 1, 1], 9, 0.01, "an infinite sum: inf - inf is no variance"),
        ([np.nan, 1, 1], [1, 1, 1], 9, 0.01, "a NaN in hdr"),
        ([5, 5, 5], [100, 100, 100], 0xFFFFFFFF, 0.01, "largest n"),
    ]
    for hdr, sq, n, floor, what in cases:
        h = np.array([hdr], dtype=np.float32)
        q = np.array([sq], dtype=np.float32)
        got, want = host_estimate(h, q, n, floor), np_estimate(h, q, n, floor)
        assert_same_bits(got, want, what)
    # the values the contract spells out
    assert np.array_equal(host_estimate([[3, 3, 3]], [[1, 1, 1]], 4, 0.01), np.zeros((1, 2), np.float32))
    assert np.array_equal(host_estimate([[0, 0, 0]], [[0, 0, 0]], 7, 0.01), np.zeros((1, 2), np.float32))
    e = host_estimate([[0, 0, 0]], [[0, 0, 0]], 7, 0.0)
    assert e[0, 0] == 0.0 and not np.isfinite(e[0, 1]), "floor == 0 on a black pixel: the relative error is reported as non-finite"
    e = host_estimate([[1, -1, 0]], [[1, 1, 0]], 2, 0.0)
    assert e[0, 0] > 0.0 and np.isposinf(e[0, 1])
    # n == 2, samples 1 and 0 in one channel: mean 1/2, var 1/2, abs = sqrt(1/4), rel = abs / mean
    assert np.array_equal(host_estimate([[1, 0, 0]], [[1, 0, 0]], 2, 0.0), np.array([[0.5, 1.0]], np.float32))


def test_host_twin_refuses_fewer_than_two_samples(built):
    from cpuraytracer_amd import _capi
    L = _capi.load()
    z = np.zeros(3, dtype=np.float32)
    out = np.zeros(2, dtype=np.float32)
    for n in (0, 1):
        assert L.rt_unit_noise_estimate_host(z.ctypes.data, z.ctypes.data, 1, n, 0.01, out.ctypes.data) == RT_ERR_SEQUENCE
    assert L.rt_unit_noise_estimate_host(None, z.ctypes.data, 1, 2, 0.01, out.ctypes.data) == 2  # RT_ERR_INVALID_ARG
    assert L.rt_unit_noise_estimate_host(z.ctypes.data, z.ctypes.data, 0, 2, 0.01, out.ctypes.data) == 0


@pytest.mark.parametrize("n", [2, 4, 16, 50, 150, 500])
def test_variance_from_binary32_sums_is_within_the_analytic_bound(n):
    """var_c from S and Q accumulated sequentially in binary32 against the binary64 two-pass variance of the same samples (recorded
    per-sample radiances of the headline configuration, golden/c2_cover_1200x800_samples.npz, cut into runs of n).

    The bound, per channel, to first order in u = 2^-24:  Q32 is n roundings of squares and n - 1 of adds, each relative u on a partial
    sum <= Q:  |Q32 - Q| <= n u Q.  |S32 - S| <= (n - 1) u sum|v|, so |S32^2 - S^2| / n <= 2 (n - 1) u (sum|v|)^2 / n <= 2 (n - 1) u Q
    (Cauchy-Schwarz).  The binary64 steps add ~2^-53.  Together |var32 - var64| <= 3 n 2^-24 Q64 / (n - 1); the clamp at 0 only moves
    var32 towards var64 >= 0."""
    g = np.load(os.path.join(GOLDEN, "c2_cover_1200x800_samples.npz"))
    rgb = np.ascontiguousarray(g["rgb"], dtype=np.float32)
    npix = rgb.shape[0] // n
    assert npix >= 3
    v = rgb[:npix * n].reshape(npix, n, 3).transpose(1, 0, 2)  # [n, npix, 3]
    S, Q = sequential_sums(v)
    _, var32 = np_estimate(S, Q, n, 0.01, want_var=True)
    v64 = v.astype(np.float64)
    m64 = v64.sum(axis=0) / n
    var64 = ((v64 - m64) ** 2).sum(axis=0) / (n - 1)
    Q64 = (v64 * v64).sum(axis=0)
    bound = 3.0 * n * 2.0 ** -24 * Q64 / (n - 1)
    err = np.abs(var32 - var64)
    print("n = %d: max |var32 - var64| / bound = %.3g over %d pixels" % (n, float((err / np.maximum(bound, 1e-300)).max()), npix))
    assert (Q64 > 0).any()
    assert (err <= bound).all(), "worst: err %r, bound %r" % (err.max(), bound[np.unravel_index(err.argmax(), err.shape)])


def test_api_surface(built):
    from cpuraytracer_amd import _capi
    L = _capi.load()
    assert L.rt_api_version() == 2  # additions only: no caller breaks
    for name in ("rt_set_noise_estimate", "rt_download_moments", "rt_noise_map", "rt_noise_summary", "rt_unit_noise_estimate_host"):
        assert hasattr(L, name), name
        assert name in _capi.EXPORTS
    # the device entries fail cleanly on a null context (no GPU is touched)
    assert L.rt_set_noise_estimate(None, 1) == 2
    assert L.rt_download_moments(None, None) == 2
    assert L.rt_noise_map(None, 0.01, None) == 2
    assert L.rt_noise_summary(None, 0.01, None, 0, None, None) == 2
    from cpuraytracer_amd import HipRenderer
    for name in ("set_noise_estimate", "download_moments", "noise_map", "noise_summary", "render_until"):
        assert callable(getattr(HipRenderer, name))
