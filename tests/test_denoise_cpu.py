"""Denoise, the part that needs no GPU (csrc/rt_denoise.h, DESIGN.md "Denoise"): the filter compiled for the host
(rt_unit_denoise_host, the same source the kernels compile) against a numpy binary32 restatement of its contract, bit for bit; what the
filter does to a plain picture and at an edge of the guides, against closed forms; the refusals and the API surface."""
import ctypes as C

import numpy as np
import pytest

from test_noise_estimate_cpu import assert_same_bits, np_estimate

RT_ERR_INVALID_ARG, RT_ERR_SEQUENCE = 2, 6
F = np.float32
H5 = [F(1) / F(16), F(1) / F(4), F(3) / F(8), F(1) / F(4), F(1) / F(16)]
DEFAULTS = dict(levels=3, k_normal=16.0, k_depth=400.0, k_albedo=64.0, k_coverage=16.0, k_colour=1.0, var_floor=1e-6)
ZERO_K = dict(k_normal=0.0, k_depth=0.0, k_albedo=0.0, k_coverage=0.0, k_colour=0.0)


def np_denoise(hdr, sq, n, feat, m, P, count=None):
    """The contract of include/rt_api.h "denoise", restated: binary32 + - * / one operation at a time, in its order.
    hdr, sq [rows, W, 3], feat [rows, W, 8] float32; P a dict of the seven parameters.  Returns den [rows, W, 3], den_var [rows, W].
    count (a dict): taps skipped at the strip's edge and taps whose weight fell below h / 100 are counted into it."""
    hdr, sq, feat = (np.asarray(a, dtype=F) for a in (hdr, sq, feat))
    rows, W = hdr.shape[:2]
    kn, kz, ka, kc, kl, vf = (F(P[k]) for k in ("k_normal", "k_depth", "k_albedo", "k_coverage", "k_colour", "var_floor"))
    with np.errstate(all="ignore"):
        c = hdr / F(n)
        sigma = np_estimate(hdr, sq, n, 0.0)[..., 0]
        v = sigma * sigma
        g = feat / F(m)
        assert c.dtype == F and v.dtype == F and g.dtype == F
        yy, xx = np.mgrid[0:rows, 0:W]
        for l in range(P["levels"]):
            step = 1 << l
            sc = np.zeros((rows, W, 3), F)
            sv = np.zeros((rows, W), F)
            sw = np.zeros((rows, W), F)
            for a in range(5):
                for b in range(5):
                    qy, qx = yy + (a - 2) * step, xx + (b - 2) * step
                    ok = (qy >= 0) & (qy < rows) & (qx >= 0) & (qx < W)
                    qy, qx = np.where(ok, qy, 0), np.where(ok, qx, 0)
                    gq, cq, vq = g[qy, qx], c[qy, qx], v[qy, qx]
                    dn = g[..., 3:6] - gq[..., 3:6]
                    xn = kn * ((dn[..., 0] * dn[..., 0] + dn[..., 1] * dn[..., 1]) + dn[..., 2] * dn[..., 2])
                    da = g[..., 0:3] - gq[..., 0:3]
                    xa = ka * ((da[..., 0] * da[..., 0] + da[..., 1] * da[..., 1]) + da[..., 2] * da[..., 2])
                    dz = g[..., 6] - gq[..., 6]
                    zm = np.where(g[..., 6] > gq[..., 6], g[..., 6], gq[..., 6])
                    xz = kz * ((dz * dz) / (zm * zm + F(1e-12)))
                    dc = g[..., 7] - gq[..., 7]
                    xc = kc * (dc * dc)
                    dl = c - cq
                    xl = kl * (((dl[..., 0] * dl[..., 0] + dl[..., 1] * dl[..., 1]) + dl[..., 2] * dl[..., 2]) / ((v + vq) + vf))
                    x = (((xn + xz) + xa) + xc) + xl
                    hab = H5[a] * H5[b]
                    ww = hab / (F(1) + x)
                    assert ww.dtype == F and x.dtype == F
                    # a tap outside the strip adds nothing and takes no slot: the sums keep their bits
                    sc = np.where(ok[..., None], sc + ww[..., None] * cq, sc)
                    sv = np.where(ok, sv + (ww * ww) * vq, sv)
                    sw = np.where(ok, sw + ww, sw)
                    if count is not None:
                        count["skipped"] = count.get("skipped", 0) + int((~ok).sum())
                        count["small"] = count.get("small", 0) + int((ok & (ww < hab / F(100))).sum())
                        count["taps"] = count.get("taps", 0) + int(ok.sum())
            assert (sw > 0).all()
            c = sc / sw[..., None]
            v = sv / (sw * sw)
            assert c.dtype == F and v.dtype == F
    return c, v


def params_struct(P):
    from cpuraytracer_amd import _capi
    return _capi.denoise_params(**P)


def host_denoise(hdr, sq, n, feat, m, P):
    from cpuraytracer_amd import _capi
    L = _capi.load()
    hdr, sq, feat = (np.ascontiguousarray(a, dtype=F) for a in (hdr, sq, feat))
    rows, W = hdr.shape[:2]
    rgb = np.full((rows, W, 3), -1.0, F)
    var = np.full((rows, W), -1.0, F)
    ps = params_struct(P)
    _capi.check(L.rt_unit_denoise_host(hdr.ctypes.data, sq.ctypes.data, n, feat.ctypes.data, m, W, rows, C.byref(ps), rgb.ctypes.data, var.ctypes.data))
    return rgb, var


def random_strips(rng, W, rows, n, m):
    """Sums of n samples per pixel and of m feature vectors, with the pixels a picture has: noisy ones, pixels without variance, pixels
    whose binary32 sums left Q < S^2 / n, black pixels, and sky pixels (all-zero guides but the albedo) beside covered ones."""
    kind = rng.integers(0, 8, (rows, W))  # 0 black, 1 no variance, 2 Q < S^2 / n, else noisy
    v = (4.0 * rng.random((n, rows, W, 3)) * rng.random((n, rows, W, 3))).astype(F)
    v = np.where((kind == 1)[None, ..., None], F(0.5), v)
    v = np.where((kind == 0)[None, ..., None], F(0.0), v)
    S, Q = np.zeros((rows, W, 3), F), np.zeros((rows, W, 3), F)
    for s in v:
        S = S + s
        Q = Q + (s * s)
    Q = np.where((kind == 2)[..., None], Q * F(0.2), Q)  # S^2 >= Q for samples >= 0, so S^2 / 4 > Q / 5
    sky = rng.integers(0, 4, (rows, W)) == 0
    # objects as vertical bands, so that neighbours often share guides and often do not
    band = (np.arange(W)[None, :] // 3 + np.arange(rows)[:, None] // 5) % 4
    feat = np.zeros((rows, W, 8), F)
    feat[..., 0:3] = (rng.random((rows, W, 3)) * 0.1 + band[..., None] * 0.25).astype(F) * F(m)
    nrm = rng.standard_normal((4, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    feat[..., 3:6] = (nrm[band] + 0.02 * rng.standard_normal((rows, W, 3))).astype(F) * F(m)
    feat[..., 6] = (5.0 + 3.0 * band + 0.05 * rng.random((rows, W))).astype(F) * F(m)
    feat[..., 7] = rng.integers(1, m + 1, (rows, W)).astype(F)
    feat[sky, 3:] = 0
    assert S.dtype == F and Q.dtype == F and feat.dtype == F
    return S, Q, feat, kind, sky


SHAPES = [(1, 1), (5, 3), (37, 19), (70, 41)]  # the last: interior 32 x 8 tiles and ragged edges in both directions


@pytest.mark.parametrize("W,rows", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_host_twin_equals_numpy(built, W, rows):
    rng = np.random.default_rng(100 * W + rows)
    n, m = 4, 3  # (random_strips' Q < S^2 / n pixels rely on n == 4)
    S, Q, feat, kind, sky = random_strips(rng, W, rows, n, m)
    if W * rows > 100:
        assert all((kind == k).any() for k in range(4)) and sky.any() and not sky.all()
        est, var = np_estimate(S, Q, n, 0.0, want_var=True)
        assert (est[..., 0][kind == 1] == 0).all() and (var[kind == 2] == 0).all() and (est[..., 0][kind > 2] > 0).all()
    count = {}
    sets = [("defaults", {}), ("all k = 0", ZERO_K),
            ("random k", dict(k_normal=float(rng.random() * 100), k_depth=float(rng.random() * 1000), k_albedo=float(rng.random() * 100),
                              k_coverage=float(rng.random() * 100), k_colour=float(rng.random() * 10), var_floor=float(1e-8 + rng.random() * 1e-3)))]
    for levels in range(1, 6):  # steps 8 and 16 exceed the small shapes
        for what, over in sets:
            P = dict(DEFAULTS, levels=levels, **over)
            want = np_denoise(S, Q, n, feat, m, P, count if what == "defaults" else None)
            got = host_denoise(S, Q, n, feat, m, P)
            tag = "%d x %d, %d levels, %s" % (W, rows, levels, what)
            assert_same_bits(got[0], want[0], tag + ": den")
            assert_same_bits(got[1], want[1], tag + ": den_var")
            assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all() and (got[1] >= 0).all()
    # not vacuous: taps fell outside the strip, and (beyond one pixel) the guides stopped some taps
    assert count["skipped"] > 0
    if W * rows > 100:
        assert 0 < count["small"] < count["taps"] - W * rows * 5, count  # (every centre tap weighs its full h)


def test_plain_filter(built):
    """All k = 0, one level: every tap weighs h[a] h[b], so an interior pixel's colour is the B3-spline convolution and its variance
    (sum h^2)^2 / (sum h)^4 = (70/256)^2 of the uniform v0.  Bound: 25 taps of two roundings each, then two divisions -- under 64 ulp."""
    rng = np.random.default_rng(7)
    W, rows, n = 23, 17, 2
    # samples c + 1/4 and c - 1/4 with c on a grid of 1/64: S = 2c, Q = 2c^2 + 1/8 and the variance 1/8 per channel are exact
    c = rng.integers(16, 128, (rows, W, 3)).astype(F) / F(64)
    S, Q = F(2) * c, F(2) * c * c + F(0.125)
    feat = rng.random((rows, W, 8)).astype(F)
    est, var = np_estimate(S, Q, n, 0.0, want_var=True)
    assert (var == 0.125).all()
    v0 = est[..., 0].astype(np.float64) ** 2
    assert np.unique(v0).size == 1
    rgb, dvar = host_denoise(S, Q, n, feat, 1, dict(DEFAULTS, levels=1, **ZERO_K))
    h = np.array([1, 4, 6, 4, 1], np.float64) / 16
    c64 = c.astype(np.float64)
    bound = 64 * 2.0 ** -24
    for y in range(2, rows - 2):
        for x in range(2, W - 2):
            conv = sum(h[a] * h[b] * c64[y + a - 2, x + b - 2] for a in range(5) for b in range(5))
            assert (np.abs(rgb[y, x] - conv) <= bound * conv).all(), (y, x)
            want = (70.0 / 256.0) ** 2 * v0[y, x]
            assert abs(dvar[y, x] - want) <= bound * want, (y, x, dvar[y, x], want)
    assert dvar[0, 0] > dvar[8, 11]  # a corner keeps 9 of the 25 taps


def test_edge_stop(built):
    """Two half-planes that differ in normal (|dn|^2 = 2) and in a constant colour, no variance, k_colour = 0.  For every pixel the taps
    on its own side have x = 0 and hold at least 11/16 of the kernel's weight (columns -2..0 or 0..2 of the five, every row alike);
    the taps across hold at most 5/16 and are divided by 1 + 2 k_normal.  So one level moves a pixel from its side's colour by at most
    |dc| (5/16) / (1 + 2 k_normal) / (11/16), plus rounding (64 ulp of the larger colour)."""
    W, rows, n = 16, 9, 4
    left = np.arange(W)[None, :, None] < W // 2
    cl, cr = F(0.5), F(0.25)
    c = np.broadcast_to(np.where(left, cl, cr), (rows, W, 3)).astype(F)
    S, Q = F(n) * c, F(n) * c * c  # exact: no variance
    assert (np_estimate(S, Q, n, 0.0)[..., 0] == 0).all()
    feat = np.zeros((rows, W, 8), F)
    feat[..., 0:3] = 0.5
    feat[..., 3:6] = np.where(left, np.array([1, 0, 0], F), np.array([0, 1, 0], F))
    feat[..., 6] = 7.0
    feat[..., 7] = 1.0
    dc = float(abs(cl - cr))
    rounding = 64 * 2.0 ** -24 * float(max(cl, cr))
    moved = {}
    for kn in (16.0, 0.0):
        P = dict(DEFAULTS, levels=1, k_colour=0.0, k_normal=kn)
        rgb, var = host_denoise(S, Q, n, feat, 1, P)
        moved[kn] = np.abs(rgb.astype(np.float64) - c.astype(np.float64)).max(axis=-1)
        assert (var == 0).all()
    bound = dc * (5.0 / 11.0) / (1.0 + 2.0 * 16.0)
    assert (moved[16.0] <= bound + rounding).all(), moved[16.0].max()
    assert moved[16.0][4, W // 2] > 0  # the stop is soft: the pixel at the edge does move
    # without the normal term the same pixel blurs across: 5/16 of the difference, far beyond that bound
    assert moved[0.0][4, W // 2] > bound + rounding and abs(moved[0.0][4, W // 2] - dc * 5.0 / 16.0) < 1e-6
    assert (moved[0.0][:, :W // 2 - 2] == 0).all()  # pixels whose taps all lie on their side keep their colour exactly


def test_refusals_and_defaults(built):
    from cpuraytracer_amd import _capi
    L = _capi.load()
    d = _capi.RtDenoiseParams()
    assert L.rt_denoise_default_params(C.byref(d)) == 0
    assert (d.levels, d.k_normal, d.k_depth, d.k_albedo, d.k_coverage, d.k_colour) == (3, 16.0, 400.0, 64.0, 16.0, 1.0)
    assert F(d.var_floor) == F(1e-6)
    assert L.rt_denoise_default_params(None) == RT_ERR_INVALID_ARG
    z = np.zeros(8, F)
    o3, o1 = np.zeros(3, F), np.zeros(1, F)

    def call(P=None, hdr=z, sq=z, n=2, feat=z, m=1, W=1, rows=1, rgb=o3, var=o1):
        ptr = lambda a: a.ctypes.data if a is not None else None
        return L.rt_unit_denoise_host(ptr(hdr), ptr(sq), n, ptr(feat), m, W, rows, C.byref(P) if P is not None else None, ptr(rgb), ptr(var))

    assert call() == 0 and call(d) == 0  # NULL parameters are the defaults
    for levels in (0, 6):
        assert call(params_struct(dict(levels=levels))) == RT_ERR_INVALID_ARG
    for name in ("k_normal", "k_depth", "k_albedo", "k_coverage", "k_colour", "var_floor"):
        for bad in (-1.0, float("nan"), float("inf"), -float("inf")):
            assert call(params_struct({name: bad})) == RT_ERR_INVALID_ARG, (name, bad)
        assert call(params_struct({name: 0.0})) == (RT_ERR_INVALID_ARG if name == "var_floor" else 0), name
    for null in ("hdr", "sq", "feat", "rgb", "var"):
        assert call(d, **{null: None}) == RT_ERR_INVALID_ARG, null
    assert L.rt_last_error()
    for n in (0, 1):
        assert call(d, n=n) == RT_ERR_SEQUENCE
    assert call(d, m=0) == RT_ERR_SEQUENCE


def test_api_surface(built):
    from cpuraytracer_amd import HipRenderer, _capi
    L = _capi.load()
    assert L.rt_api_version() == 2  # additions only
    for name in ("rt_denoise_default_params", "rt_denoise", "rt_download_denoised", "rt_copy_denoised_to_device", "rt_unit_denoise_host",
                 "rt_unit_denoise_forms"):
        assert hasattr(L, name) and name in _capi.EXPORTS, name
    assert C.sizeof(_capi.RtDenoiseParams) == 28
    # the device entries fail cleanly on a null context (no GPU is touched)
    assert L.rt_denoise(None, None, None) == RT_ERR_INVALID_ARG
    assert L.rt_download_denoised(None, None, None, None) == RT_ERR_INVALID_ARG
    assert L.rt_copy_denoised_to_device(None, None, None, None) == RT_ERR_INVALID_ARG
    assert L.rt_unit_denoise_forms(None, None) == RT_ERR_INVALID_ARG
    for name in ("denoise", "download_denoised", "copy_denoised_to_device", "denoise_forms"):
        assert callable(getattr(HipRenderer, name))
