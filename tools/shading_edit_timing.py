"""What a material edit costs the host (profiles/shading_edit_timing.txt): rt_scene_upload per frame against rt_set_materials per frame.
A record, no threshold.  The protocol of tools/camera_move_timing.py.

One process on one MI355X, cover scene, 1200 x 800, a fixed camera.  Each frame recolours one sphere (another one every frame, a byte
colour that depends on the frame), then renders one sample per pixel, runs the feature pass and rt_denoise_temporal_variance (spatial
source, bilinear fetch), then rt_synchronize.  Two routes on two contexts, each with a history of its own, interleaved frame by frame:
(a) the frame's materials arrive with an upload of the whole scene, (b) with rt_set_materials.  Both then call rt_temporal_forget for
the recoloured sphere, so that the histories stay comparable.  --rounds rounds of --frames frames; per route the host wall time of
the edit call alone (upload, or set_materials; the forget is timed with the frame) and of the whole frame up to the end of
rt_synchronize, best and median over every frame after the first of every round (the first uploads on both routes).  The sha256 of
the last frame's den | den_var | history is printed for each route: the two are equal, or the run says so and exits 1.

usage: python tools/shading_edit_timing.py [--rounds 3] [--frames 24] > profiles/shading_edit_timing.txt"""
import argparse
import hashlib
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, BILINEAR = 1200, 800, 4


def recolour(materials, picks, f):
    """Frame f's table: sphere picks[f % len(picks)] of the table before gets a byte colour of its own."""
    m = materials.copy()
    k = int(picks[f % len(picks)])
    m["rgb0"][k] = [np.float32((37 * f + 11) % 256) * np.float32(1.0 / 255.0), np.float32((91 * f + 5) % 256) * np.float32(1.0 / 255.0),
                    np.float32((53 * f + 200) % 256) * np.float32(1.0 / 255.0)]
    return m, k


def frame(r, sc, mats, sphere, f, route, V, bench):
    """One frame on r; returns (seconds in the edit call, seconds for the whole frame up to the end of rt_synchronize)."""
    t0 = time.perf_counter()
    if route == "upload":
        sc.materials = mats
        r.upload(sc)
    else:
        r.set_materials(mats, forget=False)
    t1 = time.perf_counter()
    r.temporal_forget([sphere])
    r.render(W, H, 1, 2, bench.DEPTH, bench.RENDER_SEED + f, stats=False)
    r.render_features(W, H, 1, 2)
    r.denoise_temporal(fetch=BILINEAR, variance=V)
    r.synchronize()
    return t1 - t0, time.perf_counter() - t0


def digest(r):
    d, t = r.download_denoised(), r.download_temporal()
    return hashlib.sha256(d["rgb"].tobytes() + d["var"].tobytes() + t["state"].tobytes() + t["len"].tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--frames", type=int, default=24)
    args = ap.parse_args()
    import bench
    import __graft_entry__ as g
    from cpuraytracer_amd import _capi
    if os.environ.get("RT_HIP_LIB"):  # A/B runs against another build of the library (tool only, as tools/bench_scene.py)
        _capi.LIB_PATH = os.path.abspath(os.environ["RT_HIP_LIB"])
    g.build()
    from cpuraytracer_amd import HipRenderer, scenes
    V =_capi.variance_params(source=_capi.RT_VARIANCE_SPATIAL)
    routes = ("upload", "set_materials")
    ctx = {m: HipRenderer(0) for m in routes}
    scs = {m: scenes.build_scene("cover", bench.SCENE_SEED, W, H) for m in routes}
    base = scs[routes[0]].materials.copy()
    picks = np.nonzero((base["type"] <= 1) & (scs[routes[0]].spheres["r"] < 100.0))[0]
    tables, m = [], base
    for f in range(args.frames):
        m, k = recolour(m, picks, f)
        tables.append((m, k))
    times = {m: [] for m in routes}
    first = {m: [] for m in routes}
    shas = {}
    for rnd in range(args.rounds):
        for m in routes:
            ctx[m].temporal_reset()
        for f in range(args.frames):
            for m in routes:
                t = frame(ctx[m], scs[m], tables[f][0], tables[f][1], f, "upload" if f == 0 else m, V, bench)
                (first if f == 0 else times)[m].append(t)
        for m in routes:
            shas.setdefault(m, []).append(digest(ctx[m]))
    print("material edit at %d x %d, cover scene, one sphere recoloured per frame, %d frames x %d rounds interleaved; one sample, feature pass, "
          "rt_temporal_forget, rt_denoise_temporal_variance (spatial, bilinear); kernel sources %s" % (W, H, args.frames, args.rounds, bench.kernel_sources_hash()[:16]))
    print("host wall time, ms, over the %d frames after the first of every round (frame 0 uploads on both routes: %s ms):"
          % (len(times[routes[0]]), ", ".join("%.3f" % (1e3 * t[0]) for t in first["set_materials"])))
    print("  route                            edit call: best  median      whole frame up to rt_synchronize: best  median")
    for m, label in (("upload", "(a) rt_scene_upload per frame  "), ("set_materials", "(b) rt_set_materials per frame ")):
        mv, fr = [1e3 * t[0] for t in times[m]], [1e3 * t[1] for t in times[m]]
        print("  %s  %15.4f  %6.4f  %38.4f  %6.4f" % (label, min(mv), statistics.median(mv), min(fr), statistics.median(fr)))
    a, b = times["upload"], times["set_materials"]
    print("  (a) / (b), best: edit call %.0f x, whole frame %.1f x; median: edit call %.0f x, whole frame %.1f x"
          % (min(t[0] for t in a) / min(t[0] for t in b), min(t[1] for t in a) / min(t[1] for t in b),
             statistics.median(t[0] for t in a) / statistics.median(t[0] for t in b), statistics.median(t[1] for t in a) / statistics.median(t[1] for t in b)))
    print("sha256 of the last frame's den | den_var | history (state, len), per round:")
    for m in routes:
        print("  %-13s %s" % (m, " ".join(s[:16] for s in shas[m])))
    same = shas["upload"] == shas["set_materials"]
    print("the two routes' pictures and histories are %s" % ("equal" if same else "NOT EQUAL"))
    for r in ctx.values():
        r.close()
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
