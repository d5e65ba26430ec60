"""What a camera move costs the host (profiles/camera_move_timing.txt): rt_scene_upload per frame against rt_set_camera per frame.  A
record, no threshold.

One process on one MI355X, cover scene, 1200 x 800, an orbit of 0.5 degrees per frame.  Each frame is one sample per pixel, the feature
pass and rt_denoise_temporal_variance (spatial source, bilinear fetch), then rt_synchronize.  Two routes on two contexts, each with a
history of its own, interleaved frame by frame: (a) the frame's camera arrives with an upload of the whole scene, (b) with
rt_set_camera.  --rounds rounds of the orbit; per route the host wall time of the move call alone and of the whole frame up to the end
of rt_synchronize, best and median over every frame after the first of every round (the first uploads on both routes).  The sha256 of
the last frame's den | den_var | history is printed for each route: the two are equal, or the run says so and exits 1.

--profile: a separate run.  Starts `rocprofv3 --kernel-trace --stats` (no counters) over route (b) alone in a child process of its
own and reports, from the child's kernel statistics, the device time per frame that route (b) spends rebuilding the per-tile tables
(masks and lists, sky flags, pilot rays and their scan, tile classes, work order) next to the trace kernel's.  Report only.

usage: python tools/camera_move_timing.py [--rounds 3] [--frames 24] > profiles/camera_move_timing.txt
       python tools/camera_move_timing.py --profile [--frames 24] >> profiles/camera_move_timing.txt"""
import argparse
import csv
import glob
import hashlib
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, DEG, BILINEAR = 1200, 800, 0.5, 4
PIVOT = (0.0, 1.0, 0.0)  # the cover scene's look-at point (csrc/host/spheres-app.cpp InitCamera)
TABLE_KERNELS = ("tile_mask", "sky_tiles", "pilot_rays", "closest", "tile_class", "tile_order")


def frame(r, sc, cam, f, move, V, bench):
    """One frame on r; returns (seconds in the move call, seconds for the whole frame up to the end of rt_synchronize)."""
    t0 = time.perf_counter()
    if move == "upload":
        sc.camera = cam
        r.upload(sc)
    else:
        r.set_camera(cam)
    t1 = time.perf_counter()
    r.render(W, H, 1, 2, bench.DEPTH, bench.RENDER_SEED + f, stats=False)
    r.render_features(W, H, 1, 2)
    r.denoise_temporal(fetch=BILINEAR, variance=V)
    r.synchronize()
    return t1 - t0, time.perf_counter() - t0


def digest(r):
    d, t = r.download_denoised(), r.download_temporal()
    return hashlib.sha256(d["rgb"].tobytes() + d["var"].tobytes() + t["state"].tobytes() + t["len"].tobytes()).hexdigest()


def run_routes(args):
    import bench
    import __graft_entry__ as g
    g.build()
    from cpuraytracer_amd import HipRenderer, _capi, scenes
    V = _capi.variance_params(source=_capi.RT_VARIANCE_SPATIAL)
    routes = ("upload", "set_camera") if not args.route_b_only else ("set_camera",)
    ctx = {m: HipRenderer(0) for m in routes}
    scs = {m: scenes.build_scene("cover", bench.SCENE_SEED, W, H) for m in routes}
    cams = [scenes.orbit_camera(scs[routes[0]].camera, DEG * f, PIVOT) for f in range(args.frames)]
    times = {m: [] for m in routes}
    first = {m: [] for m in routes}
    shas = {}
    for rnd in range(args.rounds):
        for m in routes:
            ctx[m].temporal_reset()
        for f in range(args.frames):
            for m in routes:
                t = frame(ctx[m], scs[m], cams[f], f, "upload" if f == 0 else m, V, bench)
                (first if f == 0 else times)[m].append(t)
        for m in routes:
            shas.setdefault(m, []).append(digest(ctx[m]))
    if args.route_b_only:
        return 0
    print("camera move at %d x %d, cover scene, %.1f degrees per frame, %d frames x %d rounds interleaved; one sample, feature pass, "
          "rt_denoise_temporal_variance (spatial, bilinear); kernel sources %s" % (W, H, DEG, args.frames, args.rounds, bench.kernel_sources_hash()[:16]))
    print("host wall time, ms, over the %d frames after the first of every round (frame 0 uploads on both routes: %s ms):"
          % (len(times[routes[0]]), ", ".join("%.3f" % (1e3 * t[0]) for t in first["set_camera"])))
    print("  route                          move call: best  median      whole frame up to rt_synchronize: best  median")
    for m, label in (("upload", "(a) rt_scene_upload per frame"), ("set_camera", "(b) rt_set_camera per frame  ")):
        mv, fr = [1e3 * t[0] for t in times[m]], [1e3 * t[1] for t in times[m]]
        print("  %s  %15.4f  %6.4f  %38.4f  %6.4f" % (label, min(mv), statistics.median(mv), min(fr), statistics.median(fr)))
    a, b = times["upload"], times["set_camera"]
    print("  (a) / (b), best: move call %.0f x, whole frame %.1f x" % (min(t[0] for t in a) / min(t[0] for t in b), min(t[1] for t in a) / min(t[1] for t in b)))
    print("sha256 of the last frame's den | den_var | history (state, len), per round:")
    for m in routes:
        print("  %-10s %s" % (m, " ".join(s[:16] for s in shas[m])))
    same = shas["upload"] == shas["set_camera"]
    print("the two routes' pictures and histories are %s" % ("equal" if same else "NOT EQUAL"))
    for r in ctx.values():
        r.close()
    return 0 if same else 1


def run_profile(args):
    """The parent never touches the GPU: rocprofv3 runs this file again, route (b) alone, as the program after `--`."""
    out = tempfile.mkdtemp(prefix="camera_move_kt_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", sys.executable, os.path.abspath(__file__), "--route-b-only",
           "--rounds", "1", "--frames", str(args.frames)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if p.returncode != 0:
        print("rocprofv3 failed (%d): %s" % (p.returncode, p.stderr[-2000:]))
        return 1
    stats = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
    if not stats:
        print("rocprofv3 wrote no kernel statistics under %s" % out)
        return 1
    groups = {}
    for row in csv.DictReader(open(stats[0])):
        name, calls, total = row["Name"], int(row["Calls"]), float(row["TotalDurationNs"])
        if "rt_trace_kernel" in name:
            key = "trace kernel"
        elif any(k in name for k in TABLE_KERNELS):
            key = "per-tile tables"
        elif "features" in name:
            key = "feature pass"
        elif "denoise" in name or "atrous" in name:
            key = "denoise"
        else:
            key = "other (ray tables, accumulate, resolve, memset, camera patch)"
        g = groups.setdefault(key, {"calls": 0, "ns": 0.0, "names": []})
        g["calls"] += calls
        g["ns"] += total
        g["names"].append("%s x%d %.1f us" % (name.split("(")[0][:60], calls, total / calls * 1e-3))
    n = args.frames
    print("\nrocprofv3 --kernel-trace --stats over route (b) alone, %d frames (frame 0 uploads), a run of its own; device time per frame:" % n)
    for key in sorted(groups, key=lambda k: -groups[k]["ns"]):
        g = groups[key]
        print("  %-62s %8.4f ms per frame  (%d dispatches)" % (key, g["ns"] * 1e-6 / n, g["calls"]))
    for name in groups.get("per-tile tables", {"names": []})["names"]:
        print("      %s" % name)
    if "per-tile tables" in groups and "trace kernel" in groups:
        print("  rebuilding the per-tile tables is %.2f x the trace kernel's device time at one sample per pixel"
              % (groups["per-tile tables"]["ns"] / groups["trace kernel"]["ns"]))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--route-b-only", action="store_true", help="route (b) alone, nothing printed: what --profile runs under rocprofv3")
    args = ap.parse_args()
    sys.exit(run_profile(args) if args.profile else run_routes(args))


if __name__ == "__main__":
    main()
