"""Shared by tests/test_temporal_bilinear_cpu.py and tests/test_temporal_bilinear.py: a numpy binary32 restatement of the bilinear
history fetch of include/rt_api.h ("temporal accumulation", RT_TEMPORAL_FETCH_BILINEAR; csrc/rt_temporal.h) -- one operation at a time,
in its order -- over the helpers of tests/temporal_common.py, and the host twin's wrapper with the fetch chosen."""
import numpy as np

from temporal_common import F, NO_TARGET, TDEFAULTS, dot3, np_levels, np_prepare, np_reproject
from test_denoise_cpu import DEFAULTS

NEAREST, BILINEAR = 1, 4
TDEFAULTS4 = dict(TDEFAULTS, max_history=3)   # rt_temporal_default_params_fetch(4)


def np_validate(T, g, ids, dist, hg, hid, hl):
    """temporal_validate of the current pixels against the gathered history pixels (the rule of temporal_common.np_temporal)."""
    with np.errstate(all="ignore"):
        ok = hl >= 1
        if T["use_id"]:
            ok = ok & (ids == hid)
        cov = g[..., 7]
        dc = cov - hg[..., 7]
        ok = ok & (np.where(dc < 0, -dc, dc) <= F(T["coverage_tol"]))
        dn = g[..., 3:6] - hg[..., 3:6]
        ok = ok & (dot3(dn, dn) <= F(T["normal_tol"]))
        zh = hg[..., 6] / hg[..., 7]
        dz = dist - zh
        zm = np.where(dist > zh, dist, zh)
        depth_ok = (hg[..., 7] > 0) & (dz * dz <= (F(T["depth_tol"]) * F(T["depth_tol"])) * (zm * zm))
        ok = ok & np.where(cov > 0, depth_ok, (cov == 0) & (hg[..., 7] == 0))
    return ok


def np_taps(g, W, H, first_row, rows, cam, hist_cam):
    """ok, dist of np_reproject and, per tap k = 0..3 in the order (0,0) (1,0) (0,1) (1,1): inside [4, rows, W] bool, the local row and
    column (0 where not inside) and the weight w (float32)."""
    ok, xi, yi, dist, why = np_reproject(g, W, H, first_row, rows, cam, hist_cam)
    with np.errstate(all="ignore"):
        fx = np.where(ok, why["fx"], F(0))
        fy = np.where(ok, why["fy"], F(first_row))
        rx = fx - xi.astype(F)
        ry = fy - yi.astype(F)
        hx, hy = rx >= F(0.5), ry >= F(0.5)
        x0 = np.where(hx, xi, xi - 1)
        y0 = np.where(hy, yi, yi - 1)
        tx = np.where(hx, rx - F(0.5), rx + F(0.5))
        ty = np.where(hy, ry - F(0.5), ry + F(0.5))
        assert rx.dtype == F and tx.dtype == F and ty.dtype == F
        inside, ql, qx_, w = [], [], [], []
        for k in range(4):
            i, j = k & 1, k >> 1
            qx, qy = x0 + i, y0 + j
            ins = ok & (qx >= 0) & (qx < W) & (qy >= first_row) & (qy < first_row + rows)
            wk = (tx if i else F(1) - tx) * (ty if j else F(1) - ty)
            assert wk.dtype == F
            inside.append(ins)
            qx_.append(np.where(ins, qx, 0))
            ql.append(np.where(ins, qy - first_row, 0))
            w.append(wk)
    return ok, dist, np.stack(inside), np.stack(ql), np.stack(qx_), np.stack(w)


def np_temporal_bilinear(hdr, sq, n, feat, m, ids, W, H, cam, hist=None, P=None, T=None, first_row=0, levels=True):
    """temporal_common.np_temporal with the bilinear fetch.  Also returns taps [rows, W] (how many taps took part), take [4, rows, W]
    and q [4, rows, W] (each tap's index, 0 where outside) and sw."""
    P = dict(DEFAULTS, **(P or {}))
    T = dict(TDEFAULTS4, **(T or {}))
    c, v, g = np_prepare(hdr, sq, n, feat, m)
    rows = v.shape[0]
    ids = np.asarray(ids, dtype=np.uint32).reshape(rows, W)
    ln = np.ones((rows, W), np.uint32)
    target = np.full((rows, W), NO_TARGET, np.uint32)
    taps = np.zeros((rows, W), np.int64)
    take_all, q_all, sw = np.zeros((4, rows, W), bool), np.zeros((4, rows, W), np.int64), np.zeros((rows, W), F)
    if hist is not None:
        ok, dist, inside, ql, qx, w = np_taps(g, W, H, first_row, rows, cam, hist["camera"])
        hS, hG = np.asarray(hist["state"], F).reshape(rows, W, 4), np.asarray(hist["guides"], F).reshape(rows, W, 8)
        hI, hL = np.asarray(hist["ids"], np.uint32).reshape(rows, W), np.asarray(hist["len"], np.uint32).reshape(rows, W)
        sc, sv = np.zeros((rows, W, 3), F), np.zeros((rows, W), F)
        wbest = np.zeros((rows, W), F)
        lmin = np.full((rows, W), 0xFFFFFFFF, np.uint32)
        tgt = np.full((rows, W), NO_TARGET, np.int64)
        with np.errstate(all="ignore"):
            for k in range(4):
                hs, hg, hid, hl = hS[ql[k], qx[k]], hG[ql[k], qx[k]], hI[ql[k], qx[k]], hL[ql[k], qx[k]]
                take = inside[k] & (w[k] > F(0)) & np_validate(T, g, ids, dist, hg, hid, hl)
                wk = w[k]
                sc = np.where(take[..., None], sc + wk[..., None] * hs[..., 0:3], sc)
                sv = np.where(take, sv + (wk * wk) * hs[..., 3], sv)
                sw = np.where(take, sw + wk, sw)
                lmin = np.where(take, np.minimum(lmin, hl), lmin)
                upd = take & (wk > wbest)
                wbest = np.where(upd, wk, wbest)
                tgt = np.where(upd, ql[k] * W + qx[k], tgt)
                taps += take
                take_all[k], q_all[k] = take, ql[k] * W + qx[k]
            assert sc.dtype == F and sv.dtype == F and sw.dtype == F and lmin.dtype == np.uint32
            acc = sw > F(0)
            ch = sc / sw[..., None]
            vh = sv / (sw * sw)
            cap = np.uint32(T["max_history"] - 1)
            l = np.minimum(lmin, cap)
            a = F(1) / (l.astype(F) + F(1))
            b = F(1) - a
            cb = a[..., None] * c + b[..., None] * ch
            vb = (a * a) * v + (b * b) * vh
            assert ch.dtype == F and vh.dtype == F and cb.dtype == F and vb.dtype == F
        c = np.where(acc[..., None], cb, c)
        v = np.where(acc, vb, v)
        ln = np.where(acc, l + np.uint32(1), np.uint32(1)).astype(np.uint32)
        target = np.where(acc, tgt, NO_TARGET).astype(np.uint32)
    out = {"state": np.concatenate([c, v[..., None]], axis=-1), "guides": g, "len": ln, "target": target, "ids": ids.copy(), "camera": cam,
           "taps": taps, "take": take_all, "q": q_all, "sw": sw}
    if levels:
        out["rgb"], out["var"] = np_levels(c, v, g, P)
    return out


def host_temporal_fetch(hdr, sq, n, feat, m, ids, W, H, cam, hist=None, P=None, T=None, first_row=0, fetch=BILINEAR):
    """The twin with the fetch chosen; T replaces fields of THAT fetch's defaults."""
    from cpuraytracer_amd import _capi
    return _capi.unit_temporal_host(hdr, sq, n, feat, m, ids, W, H, cam, history=hist, params=_capi.denoise_params(**dict(DEFAULTS, **(P or {}))),
                                    tparams=_capi.temporal_params_fetch(fetch, **(T or {})), first_row=first_row, fetch=fetch)
