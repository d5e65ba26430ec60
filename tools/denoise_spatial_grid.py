"""What the spatial variance source buys at one sample per pixel, without a GPU (docs/EXPERIMENTS.md "Spatial variance estimate"): the
numpy restatement (tests/denoise_spatial_common.py; the host twin has its bits and is checked against it here) over the CPU oracle's
strips.  Cover scene, 240 x 160, depth 50; frame f of 8 has seed 1 + f and a camera turned 0.5 f degrees about the look-at point and
ONE sample; rt_denoise_temporal_variance's chain with the bilinear fetch and its defaults, radius 1, 2, 3; at equal budget the moments
source at 2 spp x 4 frames (the cameras of frames 1, 3, 5, 7).  The last frame's result against the oracle's samples 1..1024 at the
last camera (seed 8): MSE and relative MSE mean((x - ref)^2 / (ref^2 + 0.01)), as ratios to the unfiltered one-sample last frame.

usage: python tools/denoise_spatial_grid.py [--threads 8] [--ref-spp 1024]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PIVOT = (0.0, 1.0, 0.0)  # the cover scene's look-at point


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--ref-spp", type=int, default=1024)
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    import numpy as np
    from cpuraytracer_amd import _capi, scenes
    from oracle import oracle_py as oracle
    import denoise_spatial_common as D
    from temporal_common import history_of, oracle_frame
    Q = D.QUALITY
    W, H, frames, depth = Q["W"], Q["H"], Q["frames"], Q["depth"]

    def scene(f):
        sc = scenes.build_scene("cover", 1, W, H)
        sc.camera = scenes.orbit_camera(sc.camera, Q["deg"] * f, PIVOT)
        return sc

    one = [(scene(f).camera,) + oracle_frame(oracle, scene(f), W, H, range(H), 1, depth, 1 + f) for f in range(frames)]
    two = [(scene(f).camera,) + oracle_frame(oracle, scene(f), W, H, range(H), 2, depth, 1 + f) for f in (1, 3, 5, 7)]
    orc = oracle.Oracle()
    orc.upload(scene(frames - 1))
    orc.render(W, H, 1, 1 + args.ref_spp, depth, frames, threads=args.threads)
    ref = (orc.download()[0] / np.float32(args.ref_spp)).reshape(H, W, 3)
    orc.close()
    raw = one[-1][1]
    m0, r0 = D.mse(raw, ref), D.rel_mse(raw, ref)
    print("cover %d x %d, %d frames, %.1f degrees per frame; the unfiltered 1-spp last frame: MSE %.5f, relative MSE %.5f" % (W, H, frames, Q["deg"], m0, r0))
    print("  source   radius  spp x frames  chain                 MSE x   relMSE x")
    for R in (1, 2, 3):
        hist = None
        for cam, S, _, feat, ids in one:
            out = D.host_temporal_spatial(S, 1, feat, 1, ids, W, H, cam, R, hist=hist, fetch=D.BILINEAR)
            hist = history_of(out)
        print("  spatial  %6d  1 x 8         temporal, bilinear  %6.4f  %9.4f" % (R, D.mse(out["rgb"], ref) / m0, D.rel_mse(out["rgb"], ref) / r0))
        if R == 3:  # the asserted configuration a second time, through the numpy restatement: the same bits
            hist = None
            for cam, S, _, feat, ids in one:
                want = D.np_temporal_spatial(S, 1, feat, 1, ids, W, H, cam, R, hist=hist, fetch=D.BILINEAR)
                hist = history_of(want)
            same = np.array_equal(want["rgb"].view(np.uint32), out["rgb"].view(np.uint32))
            print("           (numpy restatement: MSE x %.4f, relMSE x %.4f; bits equal to the twin's: %s)"
                  % (D.mse(want["rgb"], ref) / m0, D.rel_mse(want["rgb"], ref) / r0, same))
        cam, S, _, feat, ids = one[-1]
        single = D.host_denoise_spatial(S, 1, feat, 1, D.DEFAULTS, R)
        print("  spatial  %6d  1 x 1         last frame alone    %6.4f  %9.4f" % (R, D.mse(single["rgb"], ref) / m0, D.rel_mse(single["rgb"], ref) / r0))
    hist = None
    for cam, S, Sq, feat, ids in two:
        out = _capi.unit_temporal_host(S, Sq, 2, feat, 2, ids, W, H, cam, history=hist, fetch=D.BILINEAR)
        hist = history_of(out)
    print("  moments       -  2 x 4         temporal, bilinear  %6.4f  %9.4f" % (D.mse(out["rgb"], ref) / m0, D.rel_mse(out["rgb"], ref) / r0))
    cam, S, Sq, feat, ids = two[-1]
    print("  (the unfiltered 2-spp last frame of that run: MSE x %.4f, relMSE x %.4f)" % (D.mse(S / np.float32(2), ref) / m0, D.rel_mse(S / np.float32(2), ref) / r0))


if __name__ == "__main__":
    main()
