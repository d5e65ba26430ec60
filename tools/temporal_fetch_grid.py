"""What the bilinear history fetch buys, without a GPU (docs/EXPERIMENTS.md "Temporal accumulation: bilinear history taps"): the host
twin (rt_unit_temporal_host_fetch) over the CPU oracle's strips, DESIGN.md 5.8's protocol -- cover scene, 240 x 160, depth 50, eight
frames of 2 spp (seeds 1..8) from a camera that turns --deg degrees per frame about the look-at point; the last frame's result
against rt_unit_denoise_host on that frame alone, both measured against the oracle's samples 1..1024 at the last camera: MSE and
relative MSE mean((x - ref)^2 / (ref^2 + 0.01)).  One row per fetch and max_history, the other parameters at their defaults; also the
MSE of the blended pre-filter state, the share of accepted pixels and the mean history length of the last frame.

usage: python tools/temporal_fetch_grid.py [--deg 0.5 1.0] [--threads 8] [--ref-spp 1024]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))  # the oracle's strips are made by the tests' helper (temporal_common.oracle_frame)

PIVOT = (0.0, 1.0, 0.0)  # the cover scene's look-at point


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--deg", type=float, nargs="+", default=[0.5, 1.0])
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--ref-spp", type=int, default=1024)
    ap.add_argument("--history", type=int, nargs="+", default=[2, 3, 4, 6, 8])
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    import numpy as np
    from cpuraytracer_amd import _capi, scenes
    from oracle import oracle_py as oracle
    from temporal_common import oracle_frame
    W, H, frames, spp, depth = 240, 160, 8, 2, 50
    mse = lambda x, ref: float(np.mean((x.astype(np.float64) - ref.astype(np.float64)) ** 2))
    rel = lambda x, ref: float(np.mean((x.astype(np.float64) - ref.astype(np.float64)) ** 2 / (ref.astype(np.float64) ** 2 + 0.01)))
    for deg in args.deg:
        seq = []
        for f in range(frames):
            sc = scenes.build_scene("cover", 1, W, H)
            sc.camera = scenes.orbit_camera(sc.camera, deg * f, PIVOT)
            seq.append((sc.camera,) + oracle_frame(oracle, sc, W, H, range(H), spp, depth, 1 + f))
        orc = oracle.Oracle()
        orc.upload(sc)
        orc.render(W, H, 1, 1 + args.ref_spp, depth, frames, threads=args.threads)
        ref = (orc.download()[0] / np.float32(args.ref_spp)).reshape(H, W, 3)
        orc.close()
        cam, S, Q, feat, ids = seq[-1]
        single = _capi.unit_temporal_host(S, Q, spp, feat, spp, ids, W, H, cam)["rgb"]
        m0, r0 = mse(single, ref), rel(single, ref)
        raw = mse(S / np.float32(spp), ref)
        print("\n%.2f degrees per frame: rt_denoise on the last frame alone MSE %.5f, relative MSE %.5f; the raw %d spp MSE %.5f" % (deg, m0, r0, spp, raw))
        print("  fetch     max_history   MSE x   relMSE x   state MSE   accepted   mean len")
        for fetch, name in ((1, "nearest"), (4, "bilinear")):
            for mh in args.history:
                hist = None
                for cam, S, Q, feat, ids in seq:
                    out = _capi.unit_temporal_host(S, Q, spp, feat, spp, ids, W, H, cam, history=hist, tparams=_capi.temporal_params_fetch(fetch, max_history=mh),
                                                   fetch=fetch)
                    hist = {k: out[k] for k in ("camera", "state", "guides", "ids", "len")}
                acc = out["target"] != 0xFFFFFFFF
                print("  %-8s  %11d  %6.3f  %9.3f  %10.5f  %9.3f  %9.2f" % (name, mh, mse(out["rgb"], ref) / m0, rel(out["rgb"], ref) / r0,
                                                                           mse(out["state"][..., 0:3], ref), float(acc.mean()), float(out["len"].mean())))


if __name__ == "__main__":
    main()
