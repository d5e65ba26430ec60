"""What turning the sun costs the host (profiles/light_turn_timing.txt): rt_scene_upload per frame against rt_turn_lights per frame.
A record, no threshold.  The protocol of tools/shading_edit_timing.py.

One process on one MI355X, a fixed camera; the cover scene at 1200 x 800 (488 spheres: the index staged into LDS, plus the far tier),
then grid10k at 1024 x 1024 (10,004 spheres: two indices of up to 256 x 256 cells in global memory).  The sun turns 0.5 degrees about
the vertical per frame.  A frame is: the edit, rt_temporal_reset (every shadow in the history is stale), one sample per pixel, the
feature pass, rt_denoise_temporal_variance (spatial source, bilinear fetch), rt_synchronize.  Two routes on two contexts, interleaved
frame by frame: (a) the frame's sun arrives with an upload of the whole scene, (b) with rt_turn_lights.  --rounds rounds of --frames
frames; per route the host wall time of the edit call alone and of the whole frame up to the end of rt_synchronize, best and median
over every frame after the first of every round (the first uploads on both routes).  The sha256 of the last frame's den | den_var is
printed for each route: the two are equal, or the run says so and exits 1.
A third context, created under RT_SHADOW_GRID=0, takes the same turns and is timed for the call alone: it builds no index and copies
no table, so (b) - (c) is what the host spends building the indices and staging them.

usage: python tools/light_turn_timing.py [--rounds 3] [--frames 24] > profiles/light_turn_timing.txt"""
import argparse
import copy
import hashlib
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BILINEAR, STEP_DEGREES = 4, 0.5
SCENES = (("cover", 1200, 800), ("grid10k", 1024, 1024))


def frame(r, sc, W, H, f, route, V, bench):
    """One frame on r; returns (seconds in the edit call, seconds for the whole frame up to the end of rt_synchronize)."""
    t0 = time.perf_counter()
    if route == "upload":
        r.upload(sc)
    else:
        r.turn_lights([sc.sun], forget=False)
    t1 = time.perf_counter()
    r.temporal_reset()
    r.render(W, H, 1, 2, bench.DEPTH, bench.RENDER_SEED + f, stats=False)
    r.render_features(W, H, 1, 2)
    r.denoise_temporal(fetch=BILINEAR, variance=V)
    r.synchronize()
    return t1 - t0, time.perf_counter() - t0


def digest(r):
    d = r.download_denoised()
    return hashlib.sha256(d["rgb"].tobytes() + d["var"].tobytes()).hexdigest()


def measure(name, W, H, args, bench, HipRenderer, _capi, scenes):
    V = _capi.variance_params(source=_capi.RT_VARIANCE_SPATIAL)
    routes = ("upload", "turn_lights")
    ctx = {m: HipRenderer(0) for m in routes}
    os.environ["RT_SHADOW_GRID"] = "0"  # (read at rt_create)
    bare = HipRenderer(0)
    del os.environ["RT_SHADOW_GRID"]
    base = scenes.build_scene(name, bench.SCENE_SEED, W, H)
    suns, sun = [], base.sun
    for f in range(args.frames):
        suns.append(sun)
        sun = scenes.turn_light(sun, STEP_DEGREES)

    def scene_of(f):
        sc = copy.copy(base)
        sc.sun = suns[f]
        return sc
    times, first, shas, bare_ms = {m: [] for m in routes}, {m: [] for m in routes}, {}, []
    for rnd in range(args.rounds):
        for f in range(args.frames):
            for m in routes:
                t = frame(ctx[m], scene_of(f), W, H, f, "upload" if f == 0 else m, V, bench)
                (first if f == 0 else times)[m].append(t)
            if f == 0:
                bare.upload(scene_of(0))
            else:
                t0 = time.perf_counter()
                bare.turn_lights([suns[f]], forget=False)
                bare_ms.append(1e3 * (time.perf_counter() - t0))
        for m in routes:
            shas.setdefault(m, []).append(digest(ctx[m]))
    print("%s at %d x %d, %d spheres, the sun turned %.1f degrees per frame, %d frames x %d rounds interleaved; rt_temporal_reset, one sample, "
          "feature pass, rt_denoise_temporal_variance (spatial, bilinear)" % (name, W, H, base.spheres.shape[0], STEP_DEGREES, args.frames, args.rounds))
    print("host wall time, ms, over the %d frames after the first of every round (frame 0 uploads on both routes: %s ms):"
          % (len(times[routes[0]]), ", ".join("%.3f" % (1e3 * t[0]) for t in first["turn_lights"])))
    print("  route                            edit call: best  median      whole frame up to rt_synchronize: best  median")
    for m, label in (("upload", "(a) rt_scene_upload per frame  "), ("turn_lights", "(b) rt_turn_lights per frame   ")):
        mv, fr = [1e3 * t[0] for t in times[m]], [1e3 * t[1] for t in times[m]]
        print("  %s  %15.4f  %6.4f  %38.4f  %6.4f" % (label, min(mv), statistics.median(mv), min(fr), statistics.median(fr)))
    print("  (c) rt_turn_lights, no indices   %15.4f  %6.4f    (RT_SHADOW_GRID=0 at rt_create: the call without index building and table copies)"
          % (min(bare_ms), statistics.median(bare_ms)))
    a, b = times["upload"], times["turn_lights"]
    print("  (a) / (b), best: edit call %.1f x, whole frame %.1f x; median: edit call %.1f x, whole frame %.1f x"
          % (min(t[0] for t in a) / min(t[0] for t in b), min(t[1] for t in a) / min(t[1] for t in b),
             statistics.median(t[0] for t in a) / statistics.median(t[0] for t in b), statistics.median(t[1] for t in a) / statistics.median(t[1] for t in b)))
    print("sha256 of the last frame's den | den_var, per round:")
    for m in routes:
        print("  %-13s %s" % (m, " ".join(s[:16] for s in shas[m])))
    same = shas["upload"] == shas["turn_lights"]
    print("the two routes' pictures are %s\n" % ("equal" if same else "NOT EQUAL"))
    for r in list(ctx.values()) + [bare]:
        r.close()
    return same


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
    print("turning the sun: rt_scene_upload against rt_turn_lights; kernel sources %s\n" % bench.kernel_sources_hash()[:16])
    ok = True
    for name, W, H in SCENES:
        ok = measure(name, W, H, args, bench, HipRenderer, _capi, scenes) and ok
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
