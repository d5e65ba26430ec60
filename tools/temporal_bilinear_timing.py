"""The bilinear history fetch against rt_denoise_temporal and rt_denoise at 1200 x 800 (profiles/temporal_bilinear_timing.txt): a
record, no threshold.  tools/temporal_timing.py's protocol with two more columns.

One process on one MI355X, cover scene, samples 1..4 per frame (features after the same four).  For levels 1, 3, 5: rt_denoise;
rt_denoise_temporal over a history taken from the same camera (static: every pixel finds itself) and over a history taken 0.5 degrees
earlier on the orbit about the look-at point (the history is re-made before every timed call: a call replaces it); then
rt_denoise_temporal_fetch with RT_TEMPORAL_FETCH_BILINEAR and that fetch's defaults, static and orbit, on a history of its own made
the same way -- interleaved, --rounds rounds, best of --best HIP-event times each.  The nearest sides run exactly the calls of
tools/temporal_timing.py in its order, so their sha256 of den | den_var are those of profiles/temporal_timing.txt.  For the temporal
sides the share of accepted pixels and the mean history length are printed: the gather and the blend were done.

usage: python tools/temporal_bilinear_timing.py [--rounds 3] [--best 5] > profiles/temporal_bilinear_timing.txt"""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

PIVOT = (0.0, 1.0, 0.0)  # the cover scene's look-at point
NEAREST, BILINEAR = 1, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--best", type=int, default=5)
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    from cpuraytracer_amd import HipRenderer, _capi, scenes
    W, H, n = 1200, 800, 4
    os.environ.pop("RT_DENOISE_STAGE", None)
    print("rt_denoise_temporal_fetch (bilinear) against rt_denoise_temporal and rt_denoise at %d x %d, cover scene, samples 1..%d per frame; kernel sources %s"
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

    def static(levels, best, fetch):
        p = _capi.denoise_params(levels=levels)
        return min(a.denoise_temporal(p, timed=True, fetch=fetch) for _ in range(best))

    def orbit(levels, best, fetch):
        p = _capi.denoise_params(levels=levels)
        out = []
        for _ in range(best):
            a.temporal_reset()
            frame(0.0)
            a.denoise_temporal(p, fetch=fetch)
            frame(0.5)
            out.append(a.denoise_temporal(p, timed=True, fetch=fetch))
        return min(out)

    frame(0.0)
    for L in (1, 3, 5):  # warm-up: buffers, code objects
        plain(L, 1), static(L, 1, NEAREST), static(L, 1, BILINEAR)
    print("\nHIP-event time of the whole call (prepare pass, levels, tonemap), %d rounds interleaved, best of %d per cell, ms:" % (args.rounds, args.best))
    print("  levels  round  rt_denoise  nearest static  nearest orbit  bilinear static  bilinear orbit  bilinear - nearest: static, orbit"
          "  sha256 plain / nearest static / nearest orbit / bilinear static / bilinear orbit"
          "                    accepted / mean len: nearest static, orbit; bilinear static, orbit")
    T = {}
    for rnd in range(args.rounds):
        for L in (1, 3, 5):
            a.temporal_reset()
            frame(0.0)
            a.denoise_temporal(_capi.denoise_params(levels=L))
            t0 = plain(L, args.best)
            h0 = digest()
            t1 = static(L, args.best, NEAREST)
            h1, u1 = digest(), used()
            t2 = orbit(L, args.best, NEAREST)
            h2, u2 = digest(), used()
            a.temporal_reset()
            frame(0.0)
            a.denoise_temporal(_capi.denoise_params(levels=L), fetch=BILINEAR)
            t3 = static(L, args.best, BILINEAR)
            h3, u3 = digest(), used()
            t4 = orbit(L, args.best, BILINEAR)
            h4, u4 = digest(), used()
            T.setdefault(L, []).append((t0, t1, t2, t3, t4))
            print("  %6d  %5d  %10.4f  %14.4f  %13.4f  %15.4f  %14.4f  %+25.4f, %+.4f  %s / %s / %s / %s / %s  %s, %s; %s, %s"
                  % (L, rnd + 1, t0, t1, t2, t3, t4, t3 - t1, t4 - t2, h0, h1, h2, h3, h4, u1, u2, u3, u4))
    print("\nbest over the rounds, ms:")
    best = {}
    for L in (1, 3, 5):
        best[L] = tuple(min(t[k] for t in T[L]) for k in range(5))
        t0, t1, t2, t3, t4 = best[L]
        print("  levels %d: rt_denoise %.4f  nearest static %.4f (%+.4f)  nearest orbit %.4f (%+.4f)  bilinear static %.4f (%+.4f, %+.4f over nearest)"
              "  bilinear orbit %.4f (%+.4f, %+.4f over nearest)" % (L, t0, t1, t1 - t0, t2, t2 - t0, t3, t3 - t0, t3 - t1, t4, t4 - t0, t4 - t2))
    per_level = (best[5][0] - best[1][0]) / 4.0
    print("\none a-trous level in this run, (5 levels - 1 level) / 4 of rt_denoise: %.4f ms" % per_level)
    npix = W * H
    print("the nearest pass reads %d pixels x 60 B, gathers 56 B of history (state 16, guides 32, id 4, len 4) and writes 60 B: %.1f MB; the bilinear pass"
          "\ngathers four taps of 44 B each (state 16, normal x 4, second guide plane 16, id 4, len 4; the albedo is not read): %.1f MB asked for, of which"
          "\nneighbouring pixels share all but the first read of a line." % (npix, npix * 176 / 1e6, npix * (120 + 4 * 44) / 1e6))
    a.close()


if __name__ == "__main__":
    main()
