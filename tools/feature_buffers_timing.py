"""Feature pass against the trace kernel's own closest-hit rate (profiles/feature_buffers_timing.txt).

One process on one MI355X.  For the C2 workload (cover scene, 1200x800, spp 128) and the C5 workload (grid10k, 4096^2, spp 64):
  * rt_render with statistics: ms_render, samples and segments (closest-hit scans) of the trace kernel;
  * rt_render_features for the same sample range with out_ms: the HIP-event time of the feature pass (its ray-generation tables and
    its one kernel);
  * the bar ms_render x samples / segments: what the existing trace kernel spends per closest-hit scan, times one scan per sample.
The two are interleaved, one warm-up round and --rounds timed rounds; the medians are compared.  The feature pass is to be no slower
than 1.0 x the bar on both workloads; the script says by how much it is faster or slower and exits 0 either way (it measures).

usage: python tools/feature_buffers_timing.py [--rounds 5] [--only c2|c5] > profiles/feature_buffers_timing.txt"""
import argparse
import hashlib
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (the workloads' definitions: CONFIGS, DEPTH, the seeds)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", choices=["c2", "c5"], default=None)
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    import numpy as np
    from cpuraytracer_amd import HipRenderer, scenes
    print("feature pass vs. the trace kernel's time per closest-hit scan; kernel sources %s" % bench.kernel_sources_hash()[:16])
    print("one process, one GPU; per workload 1 warm-up round + %d timed rounds of (rt_render with statistics, rt_render_features with out_ms)" % args.rounds)
    verdicts = []
    for name in ("c2", "c5"):
        if args.only and args.only != name:
            continue
        cfg = bench.CONFIGS[name]
        W, H, spp = cfg["W"], cfg["H"], cfg["spp"]
        r = HipRenderer(0)
        r.upload(scenes.build_scene(cfg["scene"], bench.SCENE_SEED, W, H, aperture=cfg["aperture"]))
        rows = []
        for k in range(args.rounds + 1):
            st = r.render(W, H, 1, 1 + spp, bench.DEPTH, bench.RENDER_SEED)
            ms_feat = r.render_features(W, H, 1, 1 + spp, timed=True)
            if k:
                rows.append((st.ms_render, int(st.samples), int(st.segments), ms_feat))
        d = r.download_features()
        digest = hashlib.sha256(b"".join(np.ascontiguousarray(d[key]).tobytes() for key in ("albedo", "normal", "depth", "coverage", "id"))).hexdigest()[:16]
        coverage = float(d["coverage"].sum()) / (W * H * spp)
        r.close()
        print("\n%s: %s, %d x %d, spp %d, depth %d" % (name.upper(), cfg["scene"], W, H, spp, bench.DEPTH))
        print("  round  ms_render   segments/sample  bar = ms_render*samples/segments  ms_features  features/bar")
        for k, (ms_r, n, seg, ms_f) in enumerate(rows):
            bar = ms_r * n / seg
            print("  %5d  %9.3f   %15.4f  %32.3f  %11.3f  %12.3f" % (k + 1, ms_r, seg / n, bar, ms_f, ms_f / bar))
        ms_r = statistics.median(x[0] for x in rows)
        n, seg = rows[0][1], rows[0][2]
        ms_f = statistics.median(x[3] for x in rows)
        bar = ms_r * n / seg
        lo, hi = min(x[3] for x in rows), max(x[3] for x in rows)
        print("  median: trace %.3f ms for %d samples and %d closest-hit scans = %.3f ns per 64 scans; bar %.3f ms" % (ms_r, n, seg, ms_r * 1e6 / seg * 64, bar))
        print("  median: feature pass %.3f ms (min %.3f, max %.3f) = %.1f Msamples/s; mean coverage %.4f; strips sha256 %s" % (ms_f, lo, hi, n / ms_f / 1e3, coverage, digest))
        ratio = ms_f / bar
        verdict = "%s: feature pass = %.3f x the bar (%s by %.1f %%)" % (name.upper(), ratio, "FASTER" if ratio <= 1.0 else "SLOWER", abs(1.0 - ratio) * 100.0)
        print("  " + verdict)
        verdicts.append(verdict)
    print("\nresult: " + "; ".join(verdicts))


if __name__ == "__main__":
    main()
