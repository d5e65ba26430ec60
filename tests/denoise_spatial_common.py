"""Shared by tests/test_denoise_spatial_cpu.py and tests/test_denoise_spatial.py: a numpy binary32 restatement of the spatial variance
source of include/rt_api.h ("spatial variance estimate"; csrc/rt_denoise.h) -- one operation at a time, in its order -- on top of the
restatements of the levels and of the temporal step that tests/temporal_common.py and tests/temporal_bilinear_common.py hold, and the
host twins' wrappers."""
import contextlib

import numpy as np

import temporal_bilinear_common
import temporal_common
from temporal_common import DEFAULTS, F, np_levels

MOMENTS, SPATIAL = 0, 1
NEAREST, BILINEAR = 1, 4


def np_spatial_prepare(hdr, n, feat, m, P, R, count=None):
    """c0 [rows, W, 3], v0 [rows, W], g [rows, W, 8]: the prepared state under RT_VARIANCE_SPATIAL.  sq does not exist here.
    count (a dict): taps skipped at the strip's edge are counted into it."""
    hdr, feat = np.asarray(hdr, dtype=F), np.asarray(feat, dtype=F)
    rows, W = hdr.shape[:2]
    kn, kz, ka, kc = (F(P[k]) for k in ("k_normal", "k_depth", "k_albedo", "k_coverage"))
    with np.errstate(all="ignore"):
        c = hdr / F(n)
        g = feat / F(m)
        yy, xx = np.mgrid[0:rows, 0:W]
        s1, s2, sw = np.zeros((rows, W, 3), F), np.zeros((rows, W, 3), F), np.zeros((rows, W), F)
        for a in range(2 * R + 1):
            for b in range(2 * R + 1):
                qy, qx = yy + (a - R), xx + (b - R)
                ok = (qy >= 0) & (qy < rows) & (qx >= 0) & (qx < W)
                qy, qx = np.where(ok, qy, 0), np.where(ok, qx, 0)
                gq, cq = g[qy, qx], c[qy, qx]
                dn = g[..., 3:6] - gq[..., 3:6]
                xn = kn * ((dn[..., 0] * dn[..., 0] + dn[..., 1] * dn[..., 1]) + dn[..., 2] * dn[..., 2])
                da = g[..., 0:3] - gq[..., 0:3]
                xa = ka * ((da[..., 0] * da[..., 0] + da[..., 1] * da[..., 1]) + da[..., 2] * da[..., 2])
                dz = g[..., 6] - gq[..., 6]
                zm = np.where(g[..., 6] > gq[..., 6], g[..., 6], gq[..., 6])
                xz = kz * ((dz * dz) / (zm * zm + F(1e-12)))
                dc = g[..., 7] - gq[..., 7]
                xc = kc * (dc * dc)
                x = ((xn + xz) + xa) + xc
                w = F(1) / (F(1) + x)
                assert w.dtype == F and x.dtype == F
                # a tap outside the strip adds nothing: the sums keep their bits
                s1 = np.where(ok[..., None], s1 + w[..., None] * cq, s1)
                s2 = np.where(ok[..., None], s2 + w[..., None] * (cq * cq), s2)
                sw = np.where(ok, sw + w, sw)
                if count is not None:
                    count["skipped"] = count.get("skipped", 0) + int((~ok).sum())
                    count["stopped"] = count.get("stopped", 0) + int((ok & (w < F(0.01))).sum())
        assert (sw >= 1).all()  # the centre tap
        mu = s1 / sw[..., None]
        e = s2 / sw[..., None]
        d = e - mu * mu
        d = np.where(d > 0, d, F(0))
        v = (d[..., 0] + d[..., 1]) + d[..., 2]
        assert c.dtype == F and v.dtype == F and g.dtype == F
    return c, v, g


def np_denoise_spatial(hdr, n, feat, m, P, R):
    """den [rows, W, 3], den_var [rows, W] and the prepared state [rows, W, 4] under RT_VARIANCE_SPATIAL."""
    c, v, g = np_spatial_prepare(hdr, n, feat, m, P, R)
    rgb, var = np_levels(c, v, g, P)
    return {"rgb": rgb, "var": var, "state": np.concatenate([c, v[..., None]], axis=-1)}


@contextlib.contextmanager
def _prepared_by(fn):
    """The temporal restatements with their prepare step replaced: everything after it is the contract's unchanged temporal step."""
    keep = (temporal_common.np_prepare, temporal_bilinear_common.np_prepare)
    temporal_common.np_prepare = temporal_bilinear_common.np_prepare = fn
    try:
        yield
    finally:
        temporal_common.np_prepare, temporal_bilinear_common.np_prepare = keep


def np_temporal_spatial(hdr, n, feat, m, ids, W, H, cam, R, hist=None, P=None, T=None, first_row=0, fetch=NEAREST, levels=True):
    """One frame step plus the levels under RT_VARIANCE_SPATIAL, for either fetch (T replaces fields of that fetch's defaults)."""
    Pf = dict(DEFAULTS, **(P or {}))
    step = temporal_common.np_temporal if fetch == NEAREST else temporal_bilinear_common.np_temporal_bilinear
    with _prepared_by(lambda hdr_, sq_, n_, feat_, m_: np_spatial_prepare(hdr_, n_, feat_, m_, Pf, R)):
        return step(hdr, None, n, feat, m, ids, W, H, cam, hist=hist, P=P, T=T, first_row=first_row, levels=levels)


def variance_struct(source=SPATIAL, radius=1):
    from cpuraytracer_amd import _capi
    return _capi.variance_params(source=source, radius=radius)


def host_denoise_spatial(hdr, n, feat, m, P, R, sq=None, source=SPATIAL):
    from cpuraytracer_amd import _capi
    return _capi.unit_denoise_variance_host(hdr, sq, n, feat, m, params=_capi.denoise_params(**P), variance=variance_struct(source, R))


def host_temporal_spatial(hdr, n, feat, m, ids, W, H, cam, R, hist=None, P=None, T=None, first_row=0, fetch=NEAREST, sq=None, source=SPATIAL):
    from cpuraytracer_amd import _capi
    return _capi.unit_temporal_host(hdr, sq, n, feat, m, ids, W, H, cam, history=hist, params=_capi.denoise_params(**dict(DEFAULTS, **(P or {}))),
                                    tparams=_capi.temporal_params_fetch(fetch, **(T or {})), first_row=first_row, fetch=fetch,
                                    variance=variance_struct(source, R))


def mse(x, ref):
    return float(np.mean((x.astype(np.float64) - ref.astype(np.float64)) ** 2))


def rel_mse(x, ref):  # tests/test_denoise.py's definition
    x, ref = x.astype(np.float64), ref.astype(np.float64)
    return float(np.mean((x - ref) ** 2 / (ref ** 2 + 0.01)))


# The quality protocol (docs/EXPERIMENTS.md "Spatial variance estimate"): cover scene, 240 x 160, depth 50; frame f of 8 is rendered with
# seed 1 + f from a camera turned 0.5 f degrees about the look-at point, ONE sample; the reference is samples 1..1024 of the last camera
# with the last frame's seed.
QUALITY = dict(W=240, H=160, frames=8, deg=0.5, depth=50, ref_spp=1024)
