"""rt_denoise at 1200 x 800 (profiles/denoise_timing.txt): a record, no threshold.

One process on one MI355X, cover scene, strips after samples 1..4 (features after the same four):
  * HIP-event time of rt_denoise (prepare pass, one a-trous launch per level, tonemap) for levels 1, 3 and 5 under the shipped cut;
  * the staged / direct A/B per step: rt_denoise with L = 1..5 levels under RT_DENOISE_STAGE=0 and =1, interleaved, --rounds rounds,
    best of --best calls each.  T1(L) - T0(L) is the sum of (staged - direct) over the levels below L that fit LDS, so the difference at
    step 2^(L-1) is [T1(L) - T0(L)] - [T1(L-1) - T0(L-1)]; T(L) - T(L-1) is about what the level costs.  The two forms must give the same
    den (sha256 printed);
  * for scale: the trace kernel of the C2 step (spp 128) and the wall time of a 1-spp frame under render-ahead 8;
  * bytes each level reads and writes at least once (48 B of state and guides in, 16 B out, per pixel) against its time;
  * with --quality: the 240 x 160 quality figures of tests/test_denoise.py.

usage: python tools/denoise_timing.py [--rounds 3] [--best 5] [--quality] > profiles/denoise_timing.txt"""
import argparse
import hashlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--best", type=int, default=5)
    ap.add_argument("--quality", action="store_true")
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    import numpy as np
    from cpuraytracer_amd import HipRenderer, _capi, scenes
    W, H, n = 1200, 800, 4
    npix = W * H
    print("rt_denoise at %d x %d, cover scene, strips after samples 1..%d; kernel sources %s" % (W, H, n, bench.kernel_sources_hash()[:16]))
    r = HipRenderer(0)
    r.upload(scenes.build_scene("cover", bench.SCENE_SEED, W, H))
    r.set_noise_estimate(True)
    r.render(W, H, 1, 1 + n, bench.DEPTH, bench.RENDER_SEED)
    r.render_features(W, H, 1, 1 + n)

    def timed(levels, knob, best):
        if knob is None:
            os.environ.pop("RT_DENOISE_STAGE", None)
        else:
            os.environ["RT_DENOISE_STAGE"] = knob
        p = _capi.denoise_params(levels=levels)
        return min(r.denoise(p, timed=True) for _ in range(best))

    def digest():
        d = r.download_denoised()
        return hashlib.sha256(d["rgb"].tobytes() + d["var"].tobytes()).hexdigest()[:16]

    for L in (1, 3, 5):  # warm-up: buffers, code objects
        timed(L, "0", 1), timed(L, "1", 1)
    print("\nshipped cut (RT_DENOISE_STAGE unset), HIP-event time of the whole call, best of %d:" % args.best)
    for L in (1, 3, 5):
        ms = timed(L, None, args.best)
        print("  levels %d: %.4f ms  forms %s (1 direct, 2 staged)  den sha256 %s" % (L, ms, r.denoise_forms()[:L], digest()))
    print("\nstaged / direct A/B, %d rounds interleaved, best of %d per cell, ms:" % (args.rounds, args.best))
    print("  levels  round  T0 (never staged)  T1 (staged where it fits)  T1 - T0   forms under 1      same den")
    T = {}
    for rnd in range(args.rounds):
        for L in range(1, 6):
            t0 = timed(L, "0", args.best)
            h0 = digest()
            t1 = timed(L, "1", args.best)
            h1, forms = digest(), r.denoise_forms()[:L]
            T.setdefault(L, []).append((t0, t1))
            print("  %6d  %5d  %17.4f  %25.4f  %+8.4f  %-16s  %s" % (L, rnd + 1, t0, t1, t1 - t0, forms, "yes" if h0 == h1 else "NO (%s vs %s)" % (h0, h1)))
    print("\nper step, from the best T0 and T1 over the rounds (ms); bytes = %d pixels x (48 read + 16 written):" % npix)
    print("  step  direct level  staged level  staged - direct  GB/s of the direct level")
    b0 = {L: min(t[0] for t in T[L]) for L in T}
    b1 = {L: min(t[1] for t in T[L]) for L in T}
    prev0 = prev1 = None
    for L in range(1, 6):
        step = 1 << (L - 1)
        if L == 1:
            print("  %4d  %12s  %12s  %+15.4f  (levels 1 holds the prepare pass and the tonemap too: T0 %.4f, T1 %.4f)" % (step, "-", "-", b1[1] - b0[1], b0[1], b1[1]))
        else:
            d0, d1 = b0[L] - prev0, b1[L] - prev1
            fits = step in (1, 2, 4)
            print("  %4d  %12.4f  %12s  %15s  %8.1f" % (step, d0, "%.4f" % d1 if fits else "(no fit)",
                                                   "%+.4f" % ((b1[L] - b0[L]) - (b1[L - 1] - b0[L - 1])) if fits else "-", npix * 64 / (d0 * 1e-3) / 1e9))
        prev0, prev1 = b0[L], b1[L]
    os.environ.pop("RT_DENOISE_STAGE", None)
    # for scale
    cfg = bench.CONFIGS["c2"]
    st = r.render(W, H, 1, 1 + cfg["spp"], bench.DEPTH, bench.RENDER_SEED)
    st = r.render(W, H, 1, 1 + cfg["spp"], bench.DEPTH, bench.RENDER_SEED)
    print("\nfor scale: C2 step (spp %d) trace kernel %.3f ms, accumulate %.3f ms" % (cfg["spp"], st.ms_render, st.ms_accumulate))
    r.set_frame_lookahead(8)
    N = 256
    best = None
    for rep in range(3):
        r.clear()
        t0 = time.perf_counter()
        for s in range(1, N + 1):
            r.render(W, H, s, s + 1, bench.DEPTH, bench.RENDER_SEED, stats=False)
        r.synchronize()
        dt = time.perf_counter() - t0
        best = dt if best is None or dt < best else best
    print("for scale: 1-spp frame under render-ahead 8: %.3f ms per frame (wall, %d frames, best of 3)" % (best / N * 1e3, N))
    r.set_frame_lookahead(1)
    if args.quality:
        w, h = 240, 160
        r.upload(scenes.build_scene("cover", 1, w, h))
        r.render(w, h, 1, 5, 50, 1)
        r.render_features(w, h, 1, 5)
        raw = r.download(ldr=False)[0].astype(np.float64) / 4
        r.denoise()
        den = r.download_denoised()["rgb"].astype(np.float64)
        r.render(w, h, 5, 1025, 50, 1)
        ref = r.download(ldr=False)[0].astype(np.float64) / 1024
        mse = lambda x: float(np.mean((x - ref) ** 2))
        rel = lambda x: float(np.mean((x - ref) ** 2 / (ref ** 2 + 0.01)))
        print("\nquality, cover %d x %d, seed 1, depth 50, samples 1..4, defaults, against samples 1..1024:" % (w, h))
        print("  MSE %.5f -> %.5f (x %.3f); relative MSE %.5f -> %.5f (x %.3f)" % (mse(raw), mse(den), mse(den) / mse(raw), rel(raw), rel(den), rel(den) / rel(raw)))
    r.close()


if __name__ == "__main__":
    main()
