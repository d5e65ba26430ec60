"""rt_denoise_temporal against rt_denoise at 1200 x 800 (profiles/temporal_timing.txt): a record, no threshold.

One process on one MI355X, cover scene, samples 1..4 per frame (features after the same four).  For levels 1, 3, 5: rt_denoise, then
rt_denoise_temporal over a history taken from the same camera (static: every pixel finds itself), then over a history taken 0.5
degrees earlier on the orbit about the look-at point (the history is re-made before every timed call: a call replaces it) --
interleaved, --rounds rounds, best of --best HIP-event times each.  The sha256 of den | den_var is printed for each side, and for the
temporal sides the share of accepted pixels and the mean history length: the gather and the blend were done.  The difference is the
temporal prepare pass against the plain one; the levels and the tonemap are the same launches.

usage: python tools/temporal_timing.py [--rounds 3] [--best 5] > profiles/temporal_timing.txt"""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

PIVOT = (0.0, 1.0, 0.0)  # the cover scene's look-at point


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--best", type=int, default=5)
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    import numpy as np
    from cpuraytracer_amd import HipRenderer, _capi, scenes
    W, H, n = 1200, 800, 4
    os.environ.pop("RT_DENOISE_STAGE", None)
    print("rt_denoise_temporal against rt_denoise at %d x %d, cover scene, samples 1..%d per frame; kernel sources %s"
          % (W, H, n, bench.kernel_sources_hash()[:16]))
    base = scenes.build_scene("cover", bench.SCENE_SEED, W, H)
    a = HipRenderer(0)

    def frame(deg):
        sc = scenes.build_scene("cover", bench.SCENE_SEED, W, H)
        sc.camera = scenes.orbit_camera(base.camera, deg, PIVOT)
        a.upload(sc)
        a.set_noise_estimate(True)
        a.render(W, H, 1, 1 + n, bench.DEPTH, bench.RENDER_SEED, stats=False)
        a.render_features(W, H, 1, 1 + n)

    def digest():
        d = a.download_denoised()
        return hashlib.sha256(d["rgb"].tobytes() + d["var"].tobytes()).hexdigest()[:16]

    def used():
        t = a.download_temporal()
        return "%.3f / %.2f" % (float((t["target"] != 0xFFFFFFFF).mean()), float(t["len"].mean()))

    def plain(levels, best):
        p = _capi.denoise_params(levels=levels)
        return min(a.denoise(p, timed=True) for _ in range(best))

    def static(levels, best):
        p = _capi.denoise_params(levels=levels)
        return min(a.denoise_temporal(p, timed=True) for _ in range(best))

    def orbit(levels, best):
        p = _capi.denoise_params(levels=levels)
        out = []
        for _ in range(best):
            a.temporal_reset()
            frame(0.0)
            a.denoise_temporal(p)
            frame(0.5)
            out.append(a.denoise_temporal(p, timed=True))
        return min(out)

    frame(0.0)
    for L in (1, 3, 5):  # warm-up: buffers, code objects
        plain(L, 1), static(L, 1)
    print("\nHIP-event time of the whole call (prepare pass, levels, tonemap), %d rounds interleaved, best of %d per cell, ms:" % (args.rounds, args.best))
    print("  levels  round  rt_denoise  temporal static  temporal orbit  static - plain  orbit - plain  sha256 plain / static / orbit"
          "                        accepted / mean len: static, orbit")
    T = {}
    for rnd in range(args.rounds):
        for L in (1, 3, 5):
            a.temporal_reset()
            frame(0.0)
            a.denoise_temporal(_capi.denoise_params(levels=L))
            t0 = plain(L, args.best)
            h0 = digest()
            t1 = static(L, args.best)
            h1, u1 = digest(), used()
            t2 = orbit(L, args.best)
            h2, u2 = digest(), used()
            T.setdefault(L, []).append((t0, t1, t2))
            print("  %6d  %5d  %10.4f  %15.4f  %14.4f  %+14.4f  %+13.4f  %s / %s / %s  %s, %s" % (L, rnd + 1, t0, t1, t2, t1 - t0, t2 - t0, h0, h1, h2, u1, u2))
    print("\nbest over the rounds, ms:")
    best = {}
    for L in (1, 3, 5):
        best[L] = tuple(min(t[k] for t in T[L]) for k in range(3))
        t0, t1, t2 = best[L]
        print("  levels %d: rt_denoise %.4f  temporal static %.4f (%+.4f)  temporal orbit %.4f (%+.4f)" % (L, t0, t1, t1 - t0, t2, t2 - t0))
    per_level = (best[5][0] - best[1][0]) / 4.0
    print("\none a-trous level in this run, (5 levels - 1 level) / 4 of rt_denoise: %.4f ms" % per_level)
    npix = W * H
    print("the plain prepare pass reads %d pixels x 56 B (hdr 12, sq 12, feat 32) and writes 48 B each: %.1f MB; the temporal pass reads 60 B"
          "\n(the ids too), gathers 56 B of history (state 16, guides 32, id 4, len 4) and writes 60 B (state 16, guides 32, id, len, target): %.1f MB."
          % (npix, npix * 104 / 1e6, npix * 176 / 1e6))
    a.close()


if __name__ == "__main__":
    main()
