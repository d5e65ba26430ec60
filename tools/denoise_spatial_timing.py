"""The spatial variance source against rt_denoise at 1200 x 800 (profiles/denoise_spatial_timing.txt): a record, no threshold.

One process on one MI355X, cover scene.  Side A: rt_denoise over samples 1..4 with the noise estimate on (its precondition).  Side B:
rt_denoise_variance with RT_VARIANCE_SPATIAL, radius 1, 2, 3, over the SAME strips -- the spatial pass reads hdr and feat only, so the
two sides differ in their prepare pass alone and the levels do the same work.  Interleaved A B1 B2 B3, --rounds rounds, best of --best
HIP-event times of the whole call (prepare pass, levels, tonemap) per cell, for 1, 3 and 5 levels; the difference B - A is the cost of
the (2R+1)^2 window over the plain prepare pass.  Then the temporal entry, bilinear fetch, on a history from the same camera: moments
against spatial.  Last, the headline mode: one sample per pixel, noise estimate off, rt_denoise_variance alone (rt_denoise refuses it).
Every cell's sha256 of den | den_var is printed: the work was done, and a radius changes the result.

usage: python tools/denoise_spatial_timing.py [--rounds 3] [--best 5] > profiles/denoise_spatial_timing.txt"""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

BILINEAR = 4


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
    print("rt_denoise_variance (spatial) against rt_denoise at %d x %d, cover scene, samples 1..%d; kernel sources %s" % (W, H, n, bench.kernel_sources_hash()[:16]))
    sc = scenes.build_scene("cover", bench.SCENE_SEED, W, H)
    a = HipRenderer(0)
    a.upload(sc)
    a.set_noise_estimate(True)
    a.render(W, H, 1, 1 + n, bench.DEPTH, bench.RENDER_SEED, stats=False)
    a.render_features(W, H, 1, 1 + n)
    V = {R: _capi.variance_params(source=_capi.RT_VARIANCE_SPATIAL, radius=R) for R in (1, 2, 3)}

    def digest():
        d = a.download_denoised()
        return hashlib.sha256(d["rgb"].tobytes() + d["var"].tobytes()).hexdigest()[:12]

    def plain(levels, best, variance=None):
        p = _capi.denoise_params(levels=levels)
        return min(a.denoise(p, timed=True, variance=variance) for _ in range(best))

    def temporal(levels, best, variance=None):
        p = _capi.denoise_params(levels=levels)
        return min(a.denoise_temporal(p, timed=True, fetch=BILINEAR, variance=variance) for _ in range(best))

    for L in (1, 3, 5):  # warm-up: buffers, code objects
        plain(L, 1)
        for R in (1, 2, 3):
            plain(L, 1, V[R]), temporal(L, 1, V[R])
        temporal(L, 1)
    print("\nHIP-event time of the whole call, %d rounds interleaved, best of %d per cell, ms:" % (args.rounds, args.best))
    print("  levels  round  rt_denoise  spatial R=1  R=2  R=3    R - rt_denoise: 1, 2, 3    temporal: moments  spatial R=1  R=2  R=3    sha256 rt_denoise / R=1 / R=2 / R=3")
    cells = {}
    for rnd in range(args.rounds):
        for L in (1, 3, 5):
            t0 = plain(L, args.best)
            h = [digest()]
            ts = []
            for R in (1, 2, 3):
                ts.append(plain(L, args.best, V[R]))
                h.append(digest())
            a.temporal_reset()
            temporal(L, 1)
            m0 = temporal(L, args.best)
            ms = []
            for R in (1, 2, 3):
                ms.append(temporal(L, args.best, V[R]))
            cells.setdefault(L, []).append((t0,) + tuple(ts) + (m0,) + tuple(ms))
            print("  %6d  %5d  %10.4f  %11.4f  %.4f  %.4f    %+.4f, %+.4f, %+.4f    %17.4f  %11.4f  %.4f  %.4f    %s"
                  % (L, rnd + 1, t0, ts[0], ts[1], ts[2], ts[0] - t0, ts[1] - t0, ts[2] - t0, m0, ms[0], ms[1], ms[2], " / ".join(h)))
    print("\nbest over the rounds, ms:")
    best = {L: tuple(min(c[k] for c in cells[L]) for k in range(8)) for L in (1, 3, 5)}
    for L in (1, 3, 5):
        b = best[L]
        print("  levels %d: rt_denoise %.4f  spatial R=1 %.4f (%+.4f)  R=2 %.4f (%+.4f)  R=3 %.4f (%+.4f)   temporal bilinear: moments %.4f  spatial R=1 %.4f (%+.4f)"
              "  R=2 %.4f (%+.4f)  R=3 %.4f (%+.4f)" % (L, b[0], b[1], b[1] - b[0], b[2], b[2] - b[0], b[3], b[3] - b[0], b[4], b[5], b[5] - b[4], b[6], b[6] - b[4],
                                                      b[7], b[7] - b[4]))
    per_level = (best[5][0] - best[1][0]) / 4.0
    print("\none a-trous level in this run, (5 levels - 1 level) / 4 of rt_denoise: %.4f ms" % per_level)
    print("the spatial pass over the plain prepare pass, in levels: R=1 %.2f, R=2 %.2f, R=3 %.2f (levels 3)"
          % tuple((best[3][k] - best[3][0]) / per_level for k in (1, 2, 3)))
    # the headline mode: one sample, the noise estimate off
    a.set_noise_estimate(False)
    a.render(W, H, 1, 2, bench.DEPTH, bench.RENDER_SEED, stats=False)
    a.render_features(W, H, 1, 2)
    print("\none sample per pixel, noise estimate off (rt_denoise refuses this picture), 3 levels, best of %d, ms:" % args.best)
    for R in (1, 2, 3):
        print("  rt_denoise_variance spatial R=%d: %.4f  sha256 %s" % (R, plain(3, args.best, V[R]), digest()))
    a.close()


if __name__ == "__main__":
    main()
